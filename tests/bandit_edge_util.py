"""The mixed-phase edge grid of the two-call families (bandit, mnist) and its reference side, for
tests/test_bandit_edges_host.py (CPU) and tests/test_gpu_bandit_edges.py (GPU).

An episode of both families is two calls (FIRST, LAST), so from a fresh reset every lane of a batch is in the same phase on
every call: a wave of bandit_env::core / ::step or of mnist_advance_body never diverges between the reset branch and the step
branch, bandit's fused rollout adds to its register-resident regret on the same loop iterations for all lanes, and every
16-byte chunk of mnist_observe_chunks sees all lanes showing or none.  The grid puts the lanes of one batch in both phases:
a deterministic product of state words, actions on both sides of every comparison and info columns no natural run reaches,
padded with seeded random rows of the same product to m * 256 + 1 lanes.  The reference side is oracle/coracle.OracleEnv with
its numpy state written in place; the engine side is loaded through the public state_dict() / load_state_dict().

Only words the kernels themselves write: bandit 0 (running) and 1 (reset pending); mnist idx | label << 24 | 1 << 29 (showing)
and idx | label << 24 | 1 << 28 (reset pending, as a LAST step leaves it), always with label = labels[idx].

Out-of-spec actions: bandit's (outside 0..num_actions-1) are in the grid — the engine clamps and counts them, the reference
raises, so the oracle gets the clamped action (`oracle_actions`).  mnist's are in the grid as they are: the reference
compares action == label without a range check and so does the kernel; nothing is counted.
"""
import functools

import numpy as np

from oracle import coracle
from tests import golden_util as gu
from tests.chain_edge_util import BIG, BLOCK, LANE_OFFSET, MIN_LANES, MT_STRIDE, SEED, STEP0      # (the chain grids' constants)
from tests.grid_edge_util import _padded, _product

BD, MN = 'bandit', 'mnist'
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
MN_RESET_BIT, MN_SHOW_BIT = 1 << 28, 1 << 29          # csrc/mnist_fam.h
MN_MAX_DATA = 1 << 24                                  # the index field of the mnist word: 24 bits
MAX_ARMS = 32                                          # BSX_BANDIT_MAX_ACTIONS
OBS_BLOCK = 4096                                       # floats per workgroup of the mnist observation stream (4 x 4 KiB runs)
CELL_ROWS = 96                                         # product rows per (phase, action) cell at least: a wave, with room for
                                                       # the masked third of the reset_mask test
SMALL_REGRET = 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1  # 0.1 summed 7 times in f64, left to right: a column with low bits set
assert float(np.float32(SMALL_REGRET)) != SMALL_REGRET

# (family, arguments) — what each case is there for.  mnist's argument names a dataset (`dataset()`), not a constructor
# argument: `ctor_kwargs` turns it into images= / labels=.
CASES = [
    (BD, dict(mapping_seed=0)),                        # 11 arms
    (BD, dict(mapping_seed=3)),                        # 11 arms, the sweep's bandit/3
    (BD, dict(mapping_seed=0, num_actions=1)),         # the clamp target is arm 0 on both sides
    (BD, dict(mapping_seed=0, num_actions=MAX_ARMS)),  # the widest table; linspace rewards inexact in binary, so 1 - reward is
    (MN, dict(dataset='28x28')),                       # golden_util.mnist_dataset() as it is
    (MN, dict(dataset='2x2_one')),                     # num_data = 1: randint(1), one 16-byte row
    (MN, dict(dataset='10x10')),                       # 400-byte rows: the 4096-float blocks cut rows at every offset; labels 10..15
    (MN, dict(dataset='64x64')),                       # num_pixels = 4096, the maximum: one lane per block
    (MN, dict(dataset='2x2_2p24')),                    # 64 MiB table: non-temporal stores; the index field full to its top
]
GROUPED_BANDIT, GROUPED_MNIST = CASES[1], CASES[4]     # the grid rows of the grouped test's bandit/3 and mnist/0 segments


def case_id(family, kwargs):
  if family == BD:
    return f'bandit_seed{kwargs["mapping_seed"]}_arms{kwargs.get("num_actions", 11)}'
  return f'edge_mnist_{kwargs["dataset"]}'


CASE_IDS = [case_id(*c) for c in CASES]


@functools.lru_cache(maxsize=None)
def dataset(name):
  """(int8 images [n, rows, cols], uint8 labels [n]), read-only: seeded synthetic tables with bytes over the full
  -128..127 range and pairwise distinct rows (tests/test_bandit_edges_host.py asserts both)."""
  if name == '28x28':
    images, labels = gu.mnist_dataset()
    images, labels = np.ascontiguousarray(images), np.ascontiguousarray(labels)
  elif name == '2x2_2p24':
    # 2^24 independent 4-byte rows cannot be pairwise distinct (about 2^15 coincide), and the index a reset draws is read off
    # the observation: row i is the 32-bit word (i * odd + offset) mod 2^32, a bijection of the index, with the seeded
    # multiplier and offset taken from default_rng's int8 stream like the other tables
    rng = np.random.default_rng(1204)
    mult, off = (int(v) for v in rng.integers(-128, 128, size=(2, 4), dtype=np.int8).view(np.uint32).reshape(2))
    words = (np.arange(MN_MAX_DATA, dtype=np.uint64) * np.uint64(mult | 1) + np.uint64(off)).astype(np.uint32)
    images = words.view(np.int8).reshape(MN_MAX_DATA, 2, 2)
    labels = rng.integers(0, 10, size=MN_MAX_DATA, dtype=np.uint8)
  else:
    n, side, seed = {'2x2_one': (1, 2, 1201), '10x10': (300, 10, 1202), '64x64': (64, 64, 1203)}[name]
    rng = np.random.default_rng(seed)
    images = rng.integers(-128, 128, size=(n, side, side), dtype=np.int8)
    labels = rng.integers(0, 10, size=n, dtype=np.uint8)
    if name == '10x10':      # labels the reference accepts although no action of the spec equals them; 15 fills the 4-bit field
      over = rng.random(n) < 0.1
      labels[over] = rng.integers(10, 16, size=int(over.sum()), dtype=np.uint8)
      labels[[1, n // 2, n - 1]] = [10, 15, 12]
      labels[[0, n - 2]] = [0, 9]
  images.setflags(write=False)
  labels.setflags(write=False)
  return images, labels


def ctor_kwargs(family, kwargs):
  """The constructor arguments of the case, for bsuite_amd (engine_util.make_env) and for coracle.OracleEnv alike."""
  if family == BD:
    return dict(kwargs)
  images, labels = dataset(kwargs['dataset'])
  return dict(images=images, labels=labels)


def num_actions_of(kwargs):
  return kwargs.get('num_actions', 11)


def numel_of(family, kwargs):
  return 1 if family == BD else int(np.prod(dataset(kwargs['dataset'])[0].shape[1:]))


def rewards_of(kwargs):
  return coracle.bandit_rewards(kwargs.get('mapping_seed'), num_actions_of(kwargs))


BD_PREDICATES = ('resets', 'steps', 'clamped_low', 'clamped_high', 'best_arm', 'worst_arm', 'big_regret')
MN_PREDICATES = ('resets', 'hit', 'miss', 'miss_out_of_spec', 'top_index', 'big_regret', 'label_over_9')


def predicate_names(family, kwargs):
  """The predicates that can occur in the case."""
  if family == BD:      # one arm: its reward is linspace(0, 1, 1) = 0, no arm pays 1
    return BD_PREDICATES if num_actions_of(kwargs) > 1 else tuple(p for p in BD_PREDICATES if p != 'best_arm')
  return MN_PREDICATES if (dataset(kwargs['dataset'])[1] > 9).any() else MN_PREDICATES[:-1]


def _edge_set(values, lo, hi):
  return np.asarray(sorted({int(v) for v in values if lo <= v <= hi}), np.int64)


def bandit_grid(kwargs):
  na, rewards = num_actions_of(kwargs), rewards_of(kwargs)
  # the issue's edge actions, and the arms that pay most and least (whichever the mapping puts them on)
  acts = [INT_MIN, -1, 0, na, na + 1, INT_MAX] + [a for a in (1, na // 2, na - 2, na - 1, int(np.argmax(rewards)), int(np.argmin(rewards)))
                                                   if 0 <= a < na]
  acts = np.asarray(sorted(set(acts)), np.int64)
  regrets = np.asarray([0.0, SMALL_REGRET, BIG])
  reps = -(-CELL_ROWS // len(regrets))
  st, a, h, _ = _product(np.asarray([0, 1]), acts, regrets, np.arange(reps))
  (st, a, h), n = _padded([st, a, h], 1010, 1, False)
  return dict(family=BD, kwargs=dict(kwargs), n_product=n, lanes=len(st), na=na, rewards=rewards, reset=st.astype(bool),
              action=a.astype(np.int32), state=st.astype(np.int32), info=h[None].astype(np.float64))


def mnist_words(idx, label, reset):
  return (np.asarray(idx, np.int64) | (np.asarray(label, np.int64) << 24)
          | np.where(np.asarray(reset, bool), MN_RESET_BIT, MN_SHOW_BIT)).astype(np.int32)


# the action axis of the mnist grid: values, or offsets from the row's own label
_MN_ACTIONS = (('abs', INT_MIN), ('abs', -1), ('abs', 0), ('rel', -1), ('rel', 0), ('rel', 1), ('abs', 9), ('abs', 10), ('abs', 15),
               ('abs', INT_MAX))


def mnist_grid(kwargs):
  images, labels = dataset(kwargs['dataset'])
  nd = len(labels)
  idxs = _edge_set((0, 1, nd // 2, nd - 2, nd - 1), 0, nd - 1)
  reps = -(-CELL_ROWS // (2 * len(idxs)))
  ph, idx, ac, h, _ = _product(np.asarray([0, 1]), idxs, np.arange(len(_MN_ACTIONS)), np.asarray([0.0, BIG]), np.arange(reps))
  (ph, idx, ac, h), n = _padded([ph, idx, ac, h], 1111, 1, False)
  label = labels[idx].astype(np.int64)
  kind = np.asarray([k == 'rel' for k, _ in _MN_ACTIONS])[ac]
  value = np.asarray([v for _, v in _MN_ACTIONS], np.int64)[ac]
  action = np.where(kind, label + value, value)
  reset = ph.astype(bool)
  return dict(family=MN, kwargs=dict(kwargs), n_product=n, lanes=len(ph), num_data=nd, num_pixels=int(np.prod(images.shape[1:])),
              idx=idx, label=label, reset=reset, action=action.astype(np.int32), state=mnist_words(idx, label, reset),
              info=h[None].astype(np.float64))


_BUILDERS = {BD: bandit_grid, MN: mnist_grid}
_GRIDS = {}


def _frozen(g):
  g['numel'] = numel_of(g['family'], g['kwargs'])
  for v in g.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return g


def _key(family, kwargs):
  return (family, tuple(sorted(kwargs.items())))


def grid(family, kwargs):
  """The (cached, read-only) grid of a case."""
  key = _key(family, kwargs)
  if key not in _GRIDS:
    _GRIDS[key] = _frozen(_BUILDERS[family](kwargs))
  return _GRIDS[key]


def invalid_rows(g):
  """bool [B]: the running rows whose action the engine clamps and counts (bandit, action outside 0..num_actions-1)."""
  if g['family'] != BD:
    return np.zeros(g['lanes'], bool)
  return ~g['reset'] & ((g['action'] < 0) | (g['action'] >= g['na']))


def oracle_actions(g, a):
  """The actions as the oracle gets them: bandit's clamped by the documented rule (below 0: arm 0, above: the last arm) — the
  reference raises IndexError there and the oracle does not model it; mnist's as they are."""
  a = np.asarray(a, np.int32)
  return np.clip(a, 0, g['na'] - 1).astype(np.int32) if g['family'] == BD else a


def random_actions(g, shape, seed=31):
  """Seeded in-spec actions."""
  return np.random.default_rng(seed).integers(0, g['na'] if g['family'] == BD else 10, size=shape).astype(np.int32)


def episode_actions(g, T):
  """int32 [T, B]: the grid's action first, seeded random ones after it."""
  return np.concatenate([g['action'][None], random_actions(g, (T - 1, g['lanes']), seed=78)])


def mt_rows(g):
  return np.arange(0, g['lanes'], MT_STRIDE)


def reset_mask(g):
  """The seeded third of the lanes that test_reset_mask_and_mark_reset_on_the_grid marks."""
  return np.random.default_rng(41).random(g['lanes']) < 1.0 / 3.0


def make_oracle(g, rows=None, lane_ids=None):
  """The reference at the grid's states (rows: an index array — those rows of the grid on lanes LANE_OFFSET + rows, or on
  `lane_ids` if given)."""
  rows = np.arange(g['lanes']) if rows is None else np.asarray(rows)
  ids = np.uint64(LANE_OFFSET) + rows.astype(np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
  orc = coracle.OracleEnv(g['family'], ctor_kwargs(g['family'], g['kwargs']), ids, seed=SEED)
  if g['family'] == MN:
    orc.s['correct_label'][:] = g['label'][rows]
  orc.info['total_regret'][:] = g['info'][0, rows]
  orc.reset_next[:] = g['reset'][rows]
  return orc


def _copies(out):
  return tuple(v.copy() for v in out)


def oracle_step(g, rows=None, lane_ids=None, reset_mask=None):      # pylint: disable=redefined-outer-name
  """One step of the reference from the grid: (orc, (step_type, reward, discount, obs) copies)."""
  orc = make_oracle(g, rows, lane_ids)
  if reset_mask is not None:
    orc.reset_next[np.asarray(reset_mask)] = 1
  a = g['action'] if rows is None else g['action'][np.asarray(rows)]
  return orc, _copies(orc.call(oracle_actions(g, a), STEP0))


def oracle_run(g, actions, step0=STEP0):
  """The reference from the grid through actions [T, B]: (orc, step_type [T, B], float64 reward [T, B], obs [T, B, ...])."""
  orc = make_oracle(g)
  st, r, obs = [], [], []
  for t, a in enumerate(np.asarray(actions)):
    s, rew, _, o = orc.call(oracle_actions(g, a), step0 + t)
    st.append(s.copy())
    r.append(rew.copy())
    obs.append(o.copy())
  return orc, np.stack(st), np.stack(r), np.stack(obs)


@functools.lru_cache(maxsize=None)
def _row_index(name):
  """(sorted row keys, the indices in that order) of a dataset: its rows as one integer each."""
  images = dataset(name)[0]
  flat = images.reshape(len(images), -1)
  if flat.shape[1] == 4:
    keys = flat.view(np.uint32).reshape(-1)
  else:
    weights = np.random.default_rng(5).integers(1, 1 << 62, size=flat.shape[1], dtype=np.uint64) | np.uint64(1)
    keys = (flat.view(np.uint8).astype(np.uint64) * weights[None]).sum(axis=1, dtype=np.uint64)
  order = np.argsort(keys, kind='stable')
  return keys[order], order, (None if flat.shape[1] == 4 else weights)


def rows_are_distinct(name):
  keys = _row_index(name)[0]
  return bool((keys[1:] != keys[:-1]).all())


def drawn_index(g, obs):
  """int64 [n]: the index whose image is the observation (FIRST rows of the reference's float32 [n, ...] observations), found
  by the rows' bytes and confirmed by the reference's own arithmetic, int8 -> float32 / 255, bit for bit."""
  name = g['kwargs']['dataset']
  images = dataset(name)[0]
  flat = images.reshape(len(images), -1)
  obs = np.asarray(obs, np.float32).reshape(len(obs), -1)
  pix = np.rint(obs.astype(np.float64) * 255.0).astype(np.int8)
  keys, order, weights = _row_index(name)
  if weights is None:
    k = np.ascontiguousarray(pix).view(np.uint32).reshape(-1)
  else:
    k = (pix.view(np.uint8).astype(np.uint64) * weights[None]).sum(axis=1, dtype=np.uint64)
  pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
  drawn = order[pos].astype(np.int64)
  back = flat[drawn].astype(np.float32) / np.float32(255)
  assert (back.view(np.uint32) == obs.view(np.uint32)).all(), 'an observation that is no row of the table'
  return drawn


def oracle_words(g, orc, before, st, obs):
  """The state word the engine holds where the oracle is after a call: `before` the words before it, st / obs the
  reference's step types and observations of the call.  bandit: the reset flag.  mnist: a stepped lane keeps index and
  label under the reset bit; a reset lane shows the drawn index (read off the observation) with its label."""
  if g['family'] == BD:
    return orc.reset_next.astype(np.int32)
  labels = dataset(g['kwargs']['dataset'])[1]
  words = ((np.asarray(before, np.int64) & 0x0FFFFFFF) | MN_RESET_BIT).astype(np.int32)
  first = np.asarray(st) == 0
  if first.any():
    drawn = drawn_index(g, np.asarray(obs)[first])
    np.testing.assert_array_equal(orc.s['correct_label'][first], labels[drawn])
    words[first] = mnist_words(drawn, labels[drawn], False)
  assert ((words & MN_RESET_BIT != 0) == (orc.reset_next != 0)).all()
  return words


def load(env, g, rows=None, step0=STEP0):
  """Loads the grid into an engine environment (possibly wrapped) through state_dict() / load_state_dict().  step0 = None
  keeps the environment's own call index."""
  import torch          # pylint: disable=import-outside-toplevel
  from tests import engine_util as eu          # pylint: disable=import-outside-toplevel
  r = eu.raw(env)
  rows = np.arange(g['lanes']) if rows is None else np.asarray(rows)
  d = r.state_dict()
  dev = d['state'].device
  for k, v in dict(state=g['state'][rows], __info=g['info'][:, rows]).items():
    t = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    assert tuple(t.shape) == tuple(d[k].shape) and t.dtype == d[k].dtype, (k, t.shape, t.dtype, d[k].shape, d[k].dtype)
    d[k] = t
  if step0 is not None:
    d['__step_index'] = step0
  r.load_state_dict(d)


def draw_rows(g):
  """bool [B]: the rows whose first step consumes a draw that decides the state the lane is left in and what it shows —
  mnist's reset rows (the image index).  Runs on another lane id or another generator agree with the grid's own on the
  other rows only.  bandit draws nothing."""
  return g['reset'].copy() if g['family'] == MN else np.zeros(g['lanes'], bool)


# ------------------------------------------------------------------------------------------------ branch predicates
def predicates(g, want):
  """{name: bool [B]}: which branch each row takes, from the input state and the reference's output."""
  st, reward = want[0], want[1]
  fam, running = g['family'], ~g['reset']
  assert ((st == 0) == g['reset']).all() and ((st == 2) == running).all()
  a = g['action'].astype(np.int64)
  big = running & (g['info'][0] == BIG)
  if fam == BD:
    p = dict(resets=g['reset'].copy(), steps=running.copy(), clamped_low=running & (a < 0), clamped_high=running & (a >= g['na']),
             best_arm=running & (reward == 1.0), worst_arm=running & (reward == 0.0), big_regret=big)
  else:
    hit = running & (a == g['label'])
    p = dict(resets=g['reset'].copy(), hit=hit, miss=running & ~hit, miss_out_of_spec=running & ~hit & ((a < 0) | (a > 9)),
             top_index=running & (g['idx'] == g['num_data'] - 1), big_regret=big, label_over_9=running & (g['label'] > 9))
    assert (hit == (running & (reward == 1.0))).all()
  return {k: p[k] for k in predicate_names(fam, g['kwargs'])}


def expected_info(g, want):
  """float64 [1, B]: the regret column after the step — regret + (1 - reward) on the stepped rows, as one f64 addition, and
  nothing on the reset rows."""
  st, reward = want[0], want[1]
  info = g['info'].copy()
  stepped = st == 2
  info[0, stepped] = info[0, stepped] + (1.0 - reward[stepped])
  return info


def observe_blocks(g):
  """The workgroups of the mnist observation stream over the grid's [B, num_pixels] array: (full blocks, whether there is a
  partial one, how many blocks hold lanes of both phases)."""
  cells, total = g['num_pixels'], g['lanes'] * g['num_pixels']
  full, partial = total // OBS_BLOCK, total % OBS_BLOCK != 0
  mixed = 0
  for b in range(full + int(partial)):
    lo, hi = b * OBS_BLOCK // cells, (min((b + 1) * OBS_BLOCK, total) - 1) // cells
    mixed += len(set(g['reset'][lo:hi + 1].tolist())) == 2
  return full, partial, mixed


# ------------------------------------------------------------------------- C. several episodes inside one call
# (family, arguments, T): every lane in a seeded random phase, so on every step of the call some lanes reset and the others
# end an episode — 20 episodes per lane in 40 calls.
EPISODE_T = 40
EPISODE_CASES = [CASES[1], CASES[3], CASES[4], CASES[6]]
EPISODE_LANES = 8 * BLOCK + 1
_MIXED = {}


def mixed_grid(family, kwargs, lanes=EPISODE_LANES):
  """Every lane in a seeded random phase, a zero info column, seeded in-spec actions."""
  key = _key(family, kwargs) + (lanes,)
  if key in _MIXED:
    return _MIXED[key]
  rng = np.random.default_rng(909)
  reset = rng.integers(0, 2, size=lanes).astype(bool)
  g = dict(family=family, kwargs=dict(kwargs), n_product=lanes, lanes=lanes, reset=reset, info=np.zeros((1, lanes)))
  if family == BD:
    g.update(na=num_actions_of(kwargs), rewards=rewards_of(kwargs), state=reset.astype(np.int32))
  else:
    images, labels = dataset(kwargs['dataset'])
    idx = rng.integers(0, len(labels), size=lanes)
    label = labels[idx].astype(np.int64)
    g.update(num_data=len(labels), num_pixels=int(np.prod(images.shape[1:])), idx=idx, label=label, state=mnist_words(idx, label, reset))
  g['action'] = random_actions(g, lanes, seed=77)
  _MIXED[key] = _frozen(g)
  return _MIXED[key]
