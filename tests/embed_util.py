"""What the CPU and the GPU tests of rollout_embedding / evaluate_embedding share: the weights of every case (numpy, so that both
tests see the same floats), a numpy float32 restatement of csrc/bsx_embed.h with one rounding per operation, the cases of the
GPU test, and the closed loop of the contract on the C oracle (oracle/coracle.py) — which is how the weight seeds were chosen
and how the CPU test checks, without a GPU, that the GPU test's twin sees every action and both signs of pre-activation."""
import numpy as np

from oracle import coracle

MAX_HIDDEN = 64
LDS_BYTES = 15360                               # BSX_EMBED_LDS_BYTES
ENV_SEED = 11                                   # tests.test_gpu_policy_eval.SEED: the seed of every environment of the GPU test
LANE0 = (1 << 32) - 17                          # tests.test_gpu_policy_eval.OFFSET

# (name, family, constructor arguments, H): deep_sea size 8 with H = 64 is the smallest shared pair that misses the LDS budget
# (size 7 fits: 51 rows), so it is read from global memory; every other shared pair here is staged in LDS.
CASES = [('deep_sea_4_h1', 'deep_sea', dict(size=4, mapping_seed=42), 1),
         ('deep_sea_4_h5', 'deep_sea', dict(size=4, mapping_seed=42), 5),
         ('deep_sea_4_h64', 'deep_sea', dict(size=4, mapping_seed=42), 64),
         ('deep_sea_stochastic_h5', 'deep_sea', dict(size=6, deterministic=False, mapping_seed=1), 5),
         ('deep_sea_8_h64_global', 'deep_sea', dict(size=8, mapping_seed=3), 64),
         ('catch_h1', 'catch', dict(), 1),
         ('catch_h5', 'catch', dict(), 5),
         ('catch_h64', 'catch', dict(), 64)]
# The weight seed of each case's shared pair: the first seed from 0 on with which the contract's loop on the C oracle — 257
# lanes from LANE0, a fresh call of 11 steps and 11 more — takes every action on live steps and sees pre-activations of both
# signs (first_good_seed below; test_embed_host.py repeats the check).
PAIR_SEED = {'deep_sea_4_h1': 0, 'deep_sea_4_h5': 2, 'deep_sea_4_h64': 2, 'deep_sea_stochastic_h5': 0, 'deep_sea_8_h64_global': 0,
             'catch_h1': 22, 'catch_h5': 0, 'catch_h64': 0}


def geometry(fam, kwargs):
  """(C, K, A) of a family."""
  if fam == 'deep_sea':
    return kwargs['size'] ** 2, 1, 2
  return kwargs.get('rows', 10) * kwargs.get('columns', 5), 2, 3


def stride(H):
  return ((H + 3) & ~3) + 4


def staged_bytes(C, H):
  return 4 * ((C + 2) * stride(H) + 4 * (H + 1))


def pair(C, A, H, seed, P=None):
  """w1 [(P,) C + 2, H], w2 [(P,) A, H + 1] float32: unit normal embeddings, smaller biases."""
  rng = np.random.RandomState(1000 + seed)
  lead = () if P is None else (P,)
  w1 = rng.standard_normal(lead + (C + 2, H)).astype(np.float32)
  w1[..., C + 1, :] *= np.float32(0.5)
  w2 = rng.standard_normal(lead + (A, H + 1)).astype(np.float32)
  w2[..., H] *= np.float32(0.25)
  return w1, w2


def np_logits(w1, w2, cells):
  """The rule of csrc/bsx_embed.h in numpy float32, one rounding per operation: cells [B, K] (any int32), one pair or a pair
  per lane -> (logits [B, A], pre-activations [B, H])."""
  cells = np.asarray(cells, np.int64)
  B, K = cells.shape
  w1 = np.broadcast_to(w1, (B,) + w1.shape[-2:]) if w1.ndim == 2 else w1
  w2 = np.broadcast_to(w2, (B,) + w2.shape[-2:]) if w2.ndim == 2 else w2
  C, H = w1.shape[1] - 2, w1.shape[2]
  rows = np.clip(cells, -1, C - 1) + 1
  lane = np.arange(B)
  s = w1[:, C + 1, :].astype(np.float32).copy()
  with np.errstate(invalid='ignore'):
    for k in range(K):
      s = (s + w1[lane, rows[:, k], :]).astype(np.float32)
    h = np.where(s > 0, s, np.float32(0.0)).astype(np.float32)
    l = w2[:, :, H].astype(np.float32).copy()
    for j in range(H):
      prod = (w2[:, :, j] * h[:, j:j + 1]).astype(np.float32)
      l = (l + prod).astype(np.float32)
  return l, s


def np_argmax(l):
  best = np.zeros(l.shape[0], np.int32)
  l_best = l[:, 0].copy()
  with np.errstate(invalid='ignore'):
    for a in range(1, l.shape[1]):
      better = l[:, a] > l_best
      best = np.where(better, np.int32(a), best)
      l_best = np.where(better, l[:, a], l_best)
  return best


def np_select(w1, w2, cells):
  return np_argmax(np_logits(w1, w2, cells)[0])


def oracle_cells(orc):
  """The index rows [B, K] of the C oracle's lanes, from its state (what deep_sea_hot / catch_hot decode from the state word)."""
  if orc.family == 'deep_sea':
    N = orc.kw['size']
    row, col = orc.s['row'], orc.s['col']
    return np.where(row < N, row * N + col, -1).astype(np.int32)[:, None]
  rows, cols = orc.obs_shape
  return np.stack([orc.s['ball_y'] * cols + orc.s['ball_x'], (rows - 1) * cols + orc.s['paddle_x']], axis=1).astype(np.int32)


def oracle_loop(fam, kwargs, w1, w2, B=257, T=22, lane0=LANE0):
  """The contract's greedy loop on the C oracle: (actions on live steps, pre-activations on live steps)."""
  orc = coracle.OracleEnv(fam, dict(kwargs), np.uint64(lane0) + np.arange(B, dtype=np.uint64), seed=ENV_SEED)
  acts, pre = [], []
  for t in range(T):
    resets = orc.reset_next.astype(bool).copy()
    l, s = np_logits(w1, w2, oracle_cells(orc))
    a = np.where(resets, 0, np_argmax(l)).astype(np.int32)
    orc.call(a, t)
    acts.append(a[~resets])
    pre.append(s[~resets])
  return np.concatenate(acts), np.concatenate(pre)


def diverse(fam, kwargs, w1, w2):
  A = geometry(fam, kwargs)[2]
  acts, pre = oracle_loop(fam, kwargs, w1, w2)
  return sorted(set(acts.tolist())) == list(range(A)) and bool((pre > 0).any()) and bool((pre < 0).any())


def first_good_seed(name, limit=200):
  _, fam, kwargs, H = next(c for c in CASES if c[0] == name)
  C, _, A = geometry(fam, kwargs)
  return next(seed for seed in range(limit) if diverse(fam, kwargs, *pair(C, A, H, seed)))
