"""What the CPU and the GPU tests of sample_embedding / evaluate_sampled_embedding share: the composed rule of
csrc/bsx_embed_sample.h restated in numpy (tests.embed_util.np_logits, then tests.tab_sample_util.np_select: one rounding per
operation in both), and the contract's SAMPLED closed loop on the C oracle (oracle/coracle.py) — which is how the weight seeds
were chosen and how the CPU test checks, without a GPU, that the GPU test's twin sees every action and both signs of
pre-activation.  The cases, the weights' scheme, the lanes and the environment seed are tests/embed_util.py's."""
import numpy as np

from oracle import coracle
from oracle import stream
from tests import embed_util as mu
from tests import tab_sample_util as tu

CASES = mu.CASES
# The first two calls of the GPU test — a fresh batch and a running one — draw with the defaults.
TEMPERATURE, SAMPLE_SEED = 1.0, 0
# The weight seed of each case's shared pair: the first seed from 0 on (embed_util.pair's scheme) with which the contract's
# sampled loop on the C oracle — 257 lanes from LANE0, a fresh call of 11 steps and 11 more, the defaults above — takes every
# action on live steps and sees pre-activations of both signs (first_good_seed below; test_embed_sample_host.py re-derives them).
PAIR_SEED = {'deep_sea_4_h1': 0, 'deep_sea_4_h5': 0, 'deep_sea_4_h64': 0, 'deep_sea_stochastic_h5': 0, 'deep_sea_8_h64_global': 0,
             'catch_h1': 0, 'catch_h5': 0, 'catch_h64': 0}


def np_sample(w1, w2, cells, words, beta):
  """The rule of csrc/bsx_embed_sample.h in numpy: cells [B, K], words uint32 [B, A], beta a float64 or [B] -> (action [B],
  logits [B, A], pre-activations [B, H])."""
  l, s = mu.np_logits(w1, w2, cells)
  return tu.np_select(l, words, beta), l, s


def oracle_loop(fam, kwargs, w1, w2, B=257, T=22, lane0=mu.LANE0, temperature=TEMPERATURE, sample_seed=SAMPLE_SEED):
  """The contract's sampled loop on the C oracle: (actions on live steps, pre-activations on live steps)."""
  lanes = np.uint64(lane0) + np.arange(B, dtype=np.uint64)
  orc = coracle.OracleEnv(fam, dict(kwargs), lanes, seed=mu.ENV_SEED)
  A = mu.geometry(fam, kwargs)[2]
  acts, pre = [], []
  for t in range(T):
    resets = orc.reset_next.astype(bool).copy()
    a, _, s = np_sample(w1, w2, mu.oracle_cells(orc), stream.words(sample_seed, lanes, t, tu.STREAM_SAMPLE, A), 1.0 / temperature)
    a = np.where(resets, 0, a).astype(np.int32)
    orc.call(a, t)
    acts.append(a[~resets])
    pre.append(s[~resets])
  return np.concatenate(acts), np.concatenate(pre)


def diverse(fam, kwargs, w1, w2):
  A = mu.geometry(fam, kwargs)[2]
  acts, pre = oracle_loop(fam, kwargs, w1, w2)
  return sorted(set(acts.tolist())) == list(range(A)) and bool((pre > 0).any()) and bool((pre < 0).any())


def first_good_seed(name, limit=200):
  _, fam, kwargs, H = next(c for c in CASES if c[0] == name)
  C, _, A = mu.geometry(fam, kwargs)
  return next(seed for seed in range(limit) if diverse(fam, kwargs, *mu.pair(C, A, H, seed)))
