"""The mixed-phase edge grid of the chain families (memory_chain, umbrella_chain, discounting_chain) and its reference side,
for tests/test_chain_edges_host.py (CPU) and tests/test_gpu_chain_edges.py (GPU).

The episodes of the three families have a fixed length, so from a fresh reset every lane of a batch is at the same step on
every call, and a wave of the kernels never diverges between FIRST, MID and LAST.  The grid puts the lanes of one batch at
different points of an episode: a deterministic product of state fields and actions on both sides of every branch of
csrc/memory_chain_env.h, csrc/umbrella_chain_env.h and csrc/discounting_chain_env.h, padded with seeded random rows of the same
product to m * 256 + 1 lanes.  The reference side is oracle/coracle.OracleEnv with its numpy state written in place; the
engine side is loaded through the public state_dict() / load_state_dict().

Only words the kernels themselves write: running rows with memory_chain t <= L, umbrella_chain t <= L - 1, discounting_chain
t <= 99; reset rows shaped as a LAST step leaves them, with the field values kept (memory_chain t = L + 1 | query << 20 |
1 << 28, umbrella_chain t = L | need | has | 1 << 22, discounting_chain t = 100 | context | 1 << 12).

Out-of-spec actions: discounting_chain's (an episode's first action outside -5..4) are in the grid — the engine clamps and
counts them, the oracle gets the clamped action (`oracle_actions`).  Those of memory_chain / umbrella_chain are not: the
reference does not range-check them, and the engine reads any action other than 1 as 0.
"""
import numpy as np

from oracle import coracle
from tests.grid_edge_util import _padded, _product      # (shared with the grid families; their grids are not touched)

BLOCK = 256                      # lanes per workgroup (csrc/bsx_device.h)
STEP0 = 5                        # the call index the grids are loaded at: resets inside a T = 3 run draw at 6 and 7
SEED = 23
LANE_OFFSET = (1 << 32) - 300    # the global lane ids cross 2^32 inside the second workgroup
MIN_LANES = 64                   # every predicate on at least one full wave
MIN_BLOCKS = 8
MT_STRIDE = 17                   # the rows the rng='mt19937' environment is loaded with: every 17th
BIG = 16777217.0                 # 2^24 + 1 in an info column: an f32 (or otherwise inexact) accumulation shows

MC_RESET_BIT, UC_RESET_BIT, DC_RESET_BIT = 1 << 28, 1 << 22, 1 << 12
MAX_CHAIN = 1000000              # the largest memory_length / chain_length csrc/memory_chain.hip, csrc/umbrella_chain.hip accept
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
PAY_STEPS = (1, 3, 10, 30, 100)  # discounting_chain.py:49
DC_T0_REPEATS = 40               # discounting_chain: the t == 0 rows (the action chooses the context), this many times
DC_PAY_REPEATS = 4               # ... and the (t, context) rows whose step pays

MC, UC, DC = 'memory_chain', 'umbrella_chain', 'discounting_chain'


def _mc(L, nb):
  return (MC, dict(memory_length=L, num_bits=nb))


def _uc(L, nd):
  return (UC, dict(chain_length=L, n_distractor=nd))


# (family, constructor arguments) — what each case is there for:
CASES = [
    _mc(100, 1),          # top of memory_len; register-resident rollout, variant 0, TAB; quiet info atomics
    _mc(3, 1),            # L < 8: the plain info add
    _mc(4095, 1),         # the last chain whose time table fits 16 KiB of LDS (table_fits) ...
    _mc(4096, 1),         # ... and the first that does not
    _mc(1, 6),            # 8-float direct rows; context and query in the same observation (L - 1 == 0)
    _mc(5, 3),            # 5-float rows: rows not 16-byte aligned
    _mc(5, 40),           # top of memory_size: two bit words, context high word
    _mc(2, 62),           # query 61, context bit 61
    _mc(1023, 12),        # tf_table_fits of the packed tile ...
    _mc(1024, 12),        # ... both sides
    _mc(MAX_CHAIN, 1),    # the 20-bit time field at the top of its range (t = L + 1)
    _uc(100, 0),          # 3-float rows
    _uc(4, 5),            # 8-float direct rows
    _uc(1, 33),           # t == 1 is both "the action sets has" and LAST; two bit words
    _uc(100, 20),         # umbrella_length-like packed rows
    _uc(20, 100),         # top of umbrella_distract
    _uc(1023, 20),        # tf_table_fits, read at index t + 1 = L ...
    _uc(1024, 20),        # ... both sides
    _uc(MAX_CHAIN, 2),    # the time field at the top of its range
    (DC, dict(mapping_seed=2)),      # bonus on chain 2
    (DC, dict(mapping_seed=4)),      # bonus 1.1 paid on the LAST step
]
# the segments of the grouped test: the sweep ids whose settings are these
GROUPED_IDS = {'memory_len/22': _mc(100, 1), 'memory_size/16': _mc(2, 40), 'umbrella_length/22': _uc(100, 20),
               'umbrella_distract/22': _uc(20, 100), 'discounting_chain/4': (DC, dict(mapping_seed=4))}
GROUPED_CASES = [c for c in GROUPED_IDS.values() if c not in CASES]


def case_id(family, kwargs):
  if family == MC:
    return f'memory_chain_L{kwargs["memory_length"]}_nb{kwargs["num_bits"]}'
  if family == UC:
    return f'umbrella_chain_L{kwargs["chain_length"]}_nd{kwargs["n_distractor"]}'
  return f'discounting_chain_seed{kwargs["mapping_seed"]}'


CASE_IDS = [case_id(*c) for c in CASES]


def numel_of(family, kwargs):
  return kwargs['num_bits'] + 2 if family == MC else 3 + kwargs['n_distractor'] if family == UC else 2


def rollout_class(family, kwargs):
  """Which kernel a lean rollout() of the case is, by the shape rule of launch_small_obs (csrc/small_obs.h): the
  register-resident lean rollout (memory_chain with one context bit, discounting_chain) with or without its LDS time table
  (memory_chain_env::table_fits: (L + 1) * 4 <= 16384), the generic lean rollout for the other rows of at most 8 floats, the
  packed bit-plane tile for wider rows."""
  if family == DC:
    return 'regs_lean'
  if family == MC and kwargs['num_bits'] == 1:
    return 'regs_lean_table' if (kwargs['memory_length'] + 1) * 4 <= 16384 else 'regs_lean'
  return 'generic_lean' if numel_of(family, kwargs) <= 8 else 'packed_tile'


MC_PREDICATES = ('resets', 'first_obs_shows_context', 'shows_query', 'ends_hit', 'ends_miss', 'mid', 'query_in_high_word')
UC_PREDICATES = ('resets', 'action_sets_has', 'ends_match', 'ends_mismatch', 'mid_drawn_reward')
DC_PREDICATES = ('resets', 'chooses_context', 'negative_context') + tuple(f'pays_at_{k}' for k in PAY_STEPS) + (
    'pays_bonus', 'pays_on_last', 'ends', 'invalid_action')


def predicate_names(family, kwargs):
  """The predicates that can occur in the case."""
  if family == MC:
    return MC_PREDICATES if kwargs['num_bits'] > 32 else MC_PREDICATES[:-1]
  if family == UC:
    return UC_PREDICATES if kwargs['chain_length'] > 1 else UC_PREDICATES[:-1]      # L == 1: no MID step
  return DC_PREDICATES


def _edge_t(L, top):
  return np.asarray(sorted({min(max(t, 0), top) for t in (0, 1, L // 2, L - 2, L - 1, L)}))


def memory_words(t, query, reset=0):
  return (np.asarray(t, np.int64) | (np.asarray(query, np.int64) << 20) | (np.asarray(reset, np.int64) * MC_RESET_BIT)).astype(np.int32)


def umbrella_words(t, need, has, reset=0):
  return (np.asarray(t, np.int64) | (np.asarray(need, np.int64) << 20) | (np.asarray(has, np.int64) << 21)
          | (np.asarray(reset, np.int64) * UC_RESET_BIT)).astype(np.int32)


def discounting_words(t, ctx, reset=0):
  return (np.asarray(t, np.int64) | ((np.asarray(ctx, np.int64) + 6) << 8) | (np.asarray(reset, np.int64) * DC_RESET_BIT)).astype(np.int32)


def memory_grid(kwargs):
  L, nb = kwargs['memory_length'], kwargs['num_bits']
  ts = _edge_t(L, L)
  qs = np.asarray(sorted({q for q in (0, 1, 31, 32, nb - 2, nb - 1) if 0 <= q < nb}))
  bit, other, ac, big = np.asarray([0, 1]), np.asarray([0, 1, 2]), np.asarray([0, 1]), np.asarray([0, 1])
  t, q, b, o, a, h = _product(ts, qs, bit, other, ac, big)
  # reset rows: the word a LAST step leaves (t = L + 1, the reset bit), query and context kept
  rq, rb, ro, ra, rh = _product(qs, bit, other, ac, big)
  t, q, b, o, a, h = (np.concatenate(p) for p in ((t, np.full(len(rq), L + 1)), (q, rq), (b, rb), (o, ro), (a, ra), (h, rh)))
  reset = (t == L + 1).astype(np.int64)
  # the context: the other bits all 0, all 1 or seeded random; the bit at `query` as the axis says
  mask = np.uint64((1 << nb) - 1)
  rnd = np.random.default_rng(505).integers(0, 1 << 62, size=len(t), dtype=np.uint64) & mask
  ctx = np.where(o == 0, np.uint64(0), np.where(o == 1, mask, rnd)).astype(np.uint64)
  qbit = np.uint64(1) << q.astype(np.uint64)
  ctx = np.where(b == 1, ctx | qbit, ctx & ~qbit).astype(np.uint64).view(np.int64)
  (t, q, ctx, a, h, reset), n = _padded([t, q, ctx, a, h, reset], 606, 1, False)
  info = np.repeat((h * BIG)[None], 2, axis=0).astype(np.float64)
  return dict(family=MC, kwargs=dict(kwargs), n_product=n, lanes=len(t), L=L, nb=nb, t=t, query=q, ctx=ctx, reset=reset.astype(bool),
              action=a.astype(np.int32), state=memory_words(t, q, reset), info=info)


def umbrella_grid(kwargs):
  L, nd = kwargs['chain_length'], kwargs['n_distractor']
  ts = _edge_t(L, L - 1)
  two = np.asarray([0, 1])
  t, need, has, a, h = _product(ts, two, two, two, two)
  rn, rh_, ra, rb = _product(two, two, two, two)
  t, need, has, a, h = (np.concatenate(p) for p in ((t, np.full(len(rn), L)), (need, rn), (has, rh_), (a, ra), (h, rb)))
  reset = (t == L).astype(np.int64)
  (t, need, has, a, h, reset), n = _padded([t, need, has, a, h, reset], 707, 1, False)
  return dict(family=UC, kwargs=dict(kwargs), n_product=n, lanes=len(t), L=L, nd=nd, t=t, need=need, has=has, reset=reset.astype(bool),
              action=a.astype(np.int32), state=umbrella_words(t, need, has, reset), info=(h * BIG)[None].astype(np.float64))


def _dc_chain(ctx):
  return np.where(ctx < 0, ctx + 5, ctx)


def discounting_grid(kwargs):
  ctxs, acts = np.arange(-5, 5), np.arange(-5, 5)
  # t == 0: the context is -1 (as a reset leaves it) and the action chooses it; out-of-range actions only here
  a0, _ = _product(np.concatenate([acts, [-6, 5, INT_MIN, INT_MAX]]), np.arange(DC_T0_REPEATS))
  t0, c0 = np.zeros(len(a0), np.int64), np.full(len(a0), -1)
  t1, c1, a1 = _product(np.asarray([1, 2, 3, 9, 10, 29, 30, 98, 99]), ctxs, acts)
  # the rows whose step pays (t + 1 is the chain's reward step), some more times
  pays = np.isin(t1 + 1, PAY_STEPS[1:]) & (np.asarray(PAY_STEPS)[_dc_chain(c1)] == t1 + 1)
  pt, pc, pa = (np.tile(v[pays], DC_PAY_REPEATS - 1) for v in (t1, c1, a1))
  rc, ra = _product(ctxs, acts)                 # reset rows: t = 100, the context kept
  t, c, a = (np.concatenate(p) for p in ((t0, t1, pt, np.full(len(rc), 100)), (c0, c1, pc, rc), (a0, a1, pa, ra)))
  reset = (t == 100).astype(np.int64)
  (t, c, a, reset), n = _padded([t, c, a, reset], 808, 1, False)
  return dict(family=DC, kwargs=dict(kwargs), n_product=n, lanes=len(t), t=t, ctx=c, reset=reset.astype(bool), action=a.astype(np.int32),
              state=discounting_words(t, c, reset), info=np.zeros((1, len(t))), bonus=kwargs['mapping_seed'] % 5)


_BUILDERS = {MC: memory_grid, UC: umbrella_grid, DC: discounting_grid}
_GRIDS = {}


def _frozen(g):
  g['numel'] = numel_of(g['family'], g['kwargs'])
  for v in g.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return g


def grid(family, kwargs):
  """The (cached, read-only) grid of a case."""
  key = (family, tuple(sorted(kwargs.items())))
  if key not in _GRIDS:
    _GRIDS[key] = _frozen(_BUILDERS[family](kwargs))
  return _GRIDS[key]


def invalid_rows(g):
  """bool [B]: the running rows whose action the engine clamps and counts (discounting_chain, t == 0, action outside -5..4)."""
  if g['family'] != DC:
    return np.zeros(g['lanes'], bool)
  return ~g['reset'] & (g['t'] == 0) & ((g['action'] < -5) | (g['action'] > 4))


def oracle_actions(family, a):
  """The actions as the oracle gets them: discounting_chain's clamped by the documented rule (below -5: 0, above 4: 4) — the
  reference raises IndexError there and the oracle does not model it; the other families' as they are."""
  a = np.asarray(a, np.int32)
  return np.where(a < -5, 0, np.where(a > 4, 4, a)).astype(np.int32) if family == DC else a


def random_actions(family, shape, seed=31):
  """Seeded in-spec actions: 0 / 1, discounting_chain's -5..4 (the legal indices of the reference's lists)."""
  lo, hi = (-5, 5) if family == DC else (0, 2)
  return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.int32)


def mt_rows(g):
  return np.arange(0, g['lanes'], MT_STRIDE)


def make_oracle(g, rows=None, lane_ids=None):
  """The reference at the grid's states (rows: an index array — those rows of the grid on lanes LANE_OFFSET + rows, or on
  `lane_ids` if given)."""
  rows = np.arange(g['lanes']) if rows is None else np.asarray(rows)
  ids = np.uint64(LANE_OFFSET) + rows.astype(np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
  fam = g['family']
  orc = coracle.OracleEnv(fam, g['kwargs'], ids, seed=SEED)
  orc.s['timestep'][:] = g['t'][rows]
  if fam == MC:
    orc.s['query'][:] = g['query'][rows]
    orc.s['context'][:] = (g['ctx'][rows][:, None] >> np.arange(g['nb'])[None]) & 1
    orc.info['total_perfect'][:] = g['info'][0, rows]
    orc.info['total_regret'][:] = g['info'][1, rows]
  elif fam == UC:
    orc.s['need'][:] = g['need'][rows]
    orc.s['has'][:] = g['has'][rows]
    orc.info['total_regret'][:] = g['info'][0, rows]
  else:
    orc.s['context'][:] = g['ctx'][rows]
  orc.reset_next[:] = g['reset'][rows]
  return orc


def _copies(out):
  return tuple(v.copy() for v in out)


def oracle_step(g, rows=None, lane_ids=None, reset_mask=None):
  """One step of the reference from the grid: (orc, (step_type, reward, discount, obs) copies)."""
  orc = make_oracle(g, rows, lane_ids)
  if reset_mask is not None:
    orc.reset_next[np.asarray(reset_mask)] = 1
  a = g['action'] if rows is None else g['action'][np.asarray(rows)]
  return orc, _copies(orc.call(oracle_actions(g['family'], a), STEP0))


def oracle_run(g, actions, step0=STEP0):
  """The reference from the grid through actions [T, B]: (orc, step_type [T, B], float64 reward [T, B], obs [T, B, ...])."""
  orc = make_oracle(g)
  st, r, obs = [], [], []
  for t, a in enumerate(np.asarray(actions)):
    s, rew, _, o = orc.call(oracle_actions(g['family'], a), step0 + t)
    st.append(s.copy())
    r.append(rew.copy())
    obs.append(o.copy())
  return orc, np.stack(st), np.stack(r), np.stack(obs)


def oracle_words(g, orc):
  """The packed state word (and memory_chain's context column, else None) the engine holds where the oracle is."""
  fam, s = g['family'], orc.s
  if fam == MC:
    ctx = (s['context'].astype(np.uint64) << np.arange(g['nb'], dtype=np.uint64)[None]).sum(axis=1, dtype=np.uint64).view(np.int64)
    return memory_words(s['timestep'], s['query'], orc.reset_next), ctx
  if fam == UC:
    return umbrella_words(s['timestep'], s['need'], s['has'], orc.reset_next), None
  return discounting_words(s['timestep'], s['context'], orc.reset_next), None


def load(env, g, rows=None, step0=STEP0):
  """Loads the grid into an engine environment (possibly wrapped) through state_dict() / load_state_dict().  step0 = None
  keeps the environment's own call index."""
  import torch          # pylint: disable=import-outside-toplevel
  from tests import engine_util as eu          # pylint: disable=import-outside-toplevel
  r = eu.raw(env)
  rows = np.arange(g['lanes']) if rows is None else np.asarray(rows)
  d = r.state_dict()
  dev = d['state'].device
  new = dict(state=g['state'][rows], __info=g['info'][:, rows])
  if g['family'] == MC:
    new['context'] = g['ctx'][rows]
  for k, v in new.items():
    t = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    assert tuple(t.shape) == tuple(d[k].shape) and t.dtype == d[k].dtype, (k, t.shape, t.dtype, d[k].shape, d[k].dtype)
    d[k] = t
  if step0 is not None:
    d['__step_index'] = step0
  r.load_state_dict(d)


def draw_rows(g):
  """bool [B]: the rows whose first step consumes a draw that decides the state the lane is left in — memory_chain's reset
  rows (context and query), umbrella_chain's (need and has).  Runs on another lane id or another generator (tiled batches,
  rng='mt19937') agree with the grid's own on the other rows only.  (umbrella_chain also draws every row's distractor
  elements and a MID row's reward: those show in the TimeStep alone, see the tests that leave them out.)"""
  return np.zeros(g['lanes'], bool) if g['family'] == DC else g['reset'].copy()


# ------------------------------------------------------------------------------------------------ branch predicates
def predicates(g, want):
  """{name: bool [B]}: which branch each row takes, from the input state and the reference's output."""
  st, reward = want[0], want[1]
  fam, running, t = g['family'], ~g['reset'], g['t']
  assert ((st == 0) == g['reset']).all()
  if fam == MC:
    L = g['L']
    assert ((st == 2) == (running & (t == L))).all()
    p = dict(resets=g['reset'].copy(), first_obs_shows_context=running & (t == 0), shows_query=running & (t == L - 1),
             ends_hit=(st == 2) & (reward == 1.0), ends_miss=(st == 2) & (reward == -1.0), mid=st == 1,
             query_in_high_word=running & (g['query'] >= 32))
  elif fam == UC:
    assert ((st == 2) == (running & (t == g['L'] - 1))).all()
    p = dict(resets=g['reset'].copy(), action_sets_has=running & (t == 0), ends_match=(st == 2) & (reward == 1.0),
             ends_mismatch=(st == 2) & (reward == -1.0), mid_drawn_reward=st == 1)
  else:
    assert ((st == 2) == (running & (t == 99))).all()
    ctx = np.where(t == 0, oracle_actions(DC, g['action']), g['ctx'])      # the context the step runs with
    p = dict(resets=g['reset'].copy(), chooses_context=running & (t == 0), negative_context=running & (ctx < 0))
    paid = running & (reward != 0.0)
    for k in PAY_STEPS:
      p[f'pays_at_{k}'] = paid & (t + 1 == k)
    p.update(pays_bonus=paid & (reward == 1.1), pays_on_last=paid & (st == 2), ends=st == 2, invalid_action=invalid_rows(g))
  return {k: p[k] for k in predicate_names(fam, g['kwargs'])}


def expected_info(g, want):
  """float64 [n, B]: the info columns after the step, from the grid and the reference's TimeStep — +1 on total_perfect at a
  hit, +2 on total_regret at a miss / a mismatch, nothing anywhere else."""
  st, reward = want[0], want[1]
  info = g['info'].copy()
  if g['family'] == MC:
    info[0] += (st == 2) & (reward == 1.0)
    info[1] += 2.0 * ((st == 2) & (reward == -1.0))
  elif g['family'] == UC:
    info[0] += 2.0 * ((st == 2) & (reward == -1.0))
  return info


# ------------------------------------------------------------------------- C. several episodes inside one call
# (family, constructor arguments, T, episodes every lane ends at least).  Every lane starts at a seeded random point of an
# episode, reset words included, so on every step of the call some lanes end an episode and others are in the middle of
# one.  umbrella_chain L = 4 is an episode every 5 calls: 50 steps for its 10 episodes.
EPISODE_CASES = [(MC, dict(memory_length=3, num_bits=1), 64, 10), (MC, dict(memory_length=2, num_bits=40), 40, 10),
                 (UC, dict(chain_length=4, n_distractor=20), 50, 10), (DC, dict(mapping_seed=4), 230, 2)]
EPISODE_LANES = 8 * BLOCK + 1
_MIXED = {}


def mixed_grid(family, kwargs, lanes=EPISODE_LANES):
  """Every lane at a seeded random point of an episode (the reset word one of them), fields seeded random."""
  key = (family, tuple(sorted(kwargs.items())), lanes)
  if key in _MIXED:
    return _MIXED[key]
  rng = np.random.default_rng(909)
  z = np.zeros(lanes)
  if family == MC:
    L, nb = kwargs['memory_length'], kwargs['num_bits']
    t, q = rng.integers(0, L + 2, size=lanes), rng.integers(0, nb, size=lanes)
    ctx = (rng.integers(0, 1 << 62, size=lanes, dtype=np.uint64) & np.uint64((1 << nb) - 1)).view(np.int64)
    reset = t == L + 1
    g = dict(family=MC, kwargs=dict(kwargs), L=L, nb=nb, t=t, query=q, ctx=ctx, state=memory_words(t, q, reset), info=np.stack([z, z]))
  elif family == UC:
    L = kwargs['chain_length']
    t, need, has = rng.integers(0, L + 1, size=lanes), rng.integers(0, 2, size=lanes), rng.integers(0, 2, size=lanes)
    reset = t == L
    g = dict(family=UC, kwargs=dict(kwargs), L=L, nd=kwargs['n_distractor'], t=t, need=need, has=has,
             state=umbrella_words(t, need, has, reset), info=z[None].copy())
  else:
    t = rng.integers(0, 101, size=lanes)
    ctx = np.where(t == 0, -1, rng.integers(-5, 5, size=lanes))
    reset = t == 100
    g = dict(family=DC, kwargs=dict(kwargs), t=t, ctx=ctx, state=discounting_words(t, ctx, reset), info=z[None].copy(),
             bonus=kwargs['mapping_seed'] % 5)
  g.update(n_product=lanes, lanes=lanes, reset=reset, action=random_actions(family, lanes, seed=77))
  _MIXED[key] = _frozen(g)
  return _MIXED[key]


def episode_actions(g, T):
  """int32 [T, B]: the grid's action first, seeded random ones after it."""
  return np.concatenate([g['action'][None], random_actions(g['family'], (T - 1, g['lanes']), seed=78)])
