"""GPU: the memory_chain, umbrella_chain and discounting_chain kernels on the mixed-phase edge grid of
tests/chain_edge_util.py, across every launch path.

The episodes of the three families have a fixed length, so from a fresh reset every lane of a batch is at the same step on
every call — which is how nearly every other chain test runs.  A wave then never diverges between FIRST, MID and LAST: either
all 256 lanes of a workgroup OR their context bits into the packed bit-plane tile or none does, the LDS time-fraction tables
are read at one broadcast index, the quiet info atomic (bsx_info_add, L >= 8) is taken by every lane of a wave at once, the
register-resident lean rollout resets all lanes at the same step of its loop, and the late branches of long chains are
reached in lockstep or not at all.  The grid puts the lanes of one batch at different points of an episode
(tests/test_chain_edges_host.py proves each branch on at least a wave of lanes).  Everything is exact: int32 bit patterns of
every TimeStep field, state column (memory_chain's int64 context included), info column, bsuite_info(), episode counter and
the call index.  No tolerances.

  A. the eager lean step() from the loaded grid against oracle/coracle.OracleEnv, three steps with resets inside;
  B. every other path against that eager run from the same loaded state, T = 1 and T = 3;
  C. several episodes inside ONE fused launch from mixed phases, against an eager twin and the oracle.

Out-of-spec actions of memory_chain / umbrella_chain are not asserted: the reference does not range-check them and the engine
reads any action other than 1 as 0.  discounting_chain's are in the grid (the engine clamps and counts them).

Which test drives the grid through which kernel:
  small_obs_kernel, one lean step            the eager step of A: every umbrella_chain case, memory_chain with num_bits > 1
                                             (direct rows up to 8 floats, the packed bit-plane tile above)
  small_obs_eager2_kernel                    test_tiled_large_batch (memory_chain L = 100 at 2^19 + 257 lanes, discounting_chain
                                             at 2^20 + 257); at small shapes, two and four lanes per thread, through
                                             test_gpu_pair_path_small_shapes.test_two_lanes_per_thread_eager_step_at_small_shapes
  small_obs_kernel, wrapped / mt19937 step   test_logging_paths, test_reward_noise_paths, test_logging_and_noise_paths ('step'),
                                             test_mt19937_step
  small_obs_lean_rollout_kernel, TAB         test_rollout and part C: memory_chain num_bits = 1, L <= 4095
  small_obs_lean_rollout_kernel, no TAB      test_rollout: memory_chain L = 4096 and 10^6; discounting_chain (part C as well)
  small_obs_kernel, lean rollout             test_rollout: rows of at most 8 floats without a register form (generic_lean)
  small_obs_kernel, packed-tile rollout      test_rollout and part C: rows over 8 floats, tf_table_fits both ways
  small_obs_kernel, wrapped rollouts         the 'rollout' halves of the Logging / RewardNoise tests, part C under Logging
  the row path (advance + row stream)        test_chain_edges_rows_on_the_row_path; with 1 and 4 chunks per thread through
                                             test_gpu_pair_path_small_shapes.test_wide_row_stream_chunk_counts
  small_obs_group_kernel, the duo group      test_grouped_launches, per_family
  the small_mixed group kernel               test_grouped_launches, small_mixed
  the sweep's phase 0 / split / pipelined    test_grouped_launches, whole_sweep (rows in phase 0 and in the store stream),
                                             whole_sweep_split, whole_sweep_pipelined
  bsx_mark_reset + any of the above          test_reset_mask_and_mark_reset
"""
import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import sweep
from bsuite_amd import sweep_batch as sb
from bsuite_amd.environments import base
from bsuite_amd.utils import wrappers
from oracle import logging_oracle
from tests import chain_edge_util as cu
from tests import edge_snap_util as es
from tests import engine_util as eu

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]      # every test under its own time limit

CASE_PARAMS = [pytest.param(*c, id=i) for c, i in zip(cu.CASES, cu.CASE_IDS)]
WIDE_PARAMS = [p for p, c in zip(CASE_PARAMS, cu.CASES) if cu.numel_of(*c) > 8]
T_MAX = 3
TS_FIELDS = es.TS_FIELDS
NO_REWARD = ('step_type', 'discount', 'observation')
_bits, _snap_ts, _snap_after, _stack, _assert_ts = es.bits, es.snap_ts, es.snap_after, es.stack, es.assert_ts


def _assert_after(got, want, what, **kw):
  es.assert_after(got, want, what, raw_info=True, **kw)      # here always with the info columns themselves


def _make(family, kwargs, batch, **engine_kwargs):
  return eu.make_env(family, dict(kwargs), batch=batch, lane_offset=cu.LANE_OFFSET, seed=cu.SEED, **engine_kwargs)


def _cuda(a):
  return torch.from_numpy(np.array(a)).cuda()          # (a copy: the grids are read-only)


def _run(env, actions, T, path):
  """[T, ...] TimeStep snapshots through step() or rollout()."""
  if path == 'step':
    return _stack([_snap_ts(env.step(actions[t].contiguous())) for t in range(T)], T)
  return _snap_ts(env.rollout(actions[:T].contiguous()))


def _invalid(env):
  return int(eu.raw(env).invalid_action_count().item())


_EAGER = {}


def eager(family, kwargs):
  """The eager lean step() from the loaded grid, T_MAX times (the grid's action, then seeded random ones): per step the
  TimeStep and what the environment holds afterwards, as bit patterns on the device.  Computed once per case and shared,
  never modified."""
  key = (family, tuple(sorted(kwargs.items())))
  if key not in _EAGER:
    g = cu.grid(family, kwargs)
    env = _make(family, kwargs, g['lanes'])
    cu.load(env, g)
    assert env.step_index == cu.STEP0
    acts = _cuda(cu.episode_actions(g, T_MAX))
    ts, after, invalid = [], [], []
    for t in range(T_MAX):
      ts.append(_snap_ts(env.step(acts[t])))
      after.append(_snap_after(env))
      invalid.append(_invalid(env))
    _EAGER[key] = dict(ts=ts, after=after, actions=acts, invalid=invalid)
  return _EAGER[key]


def _f32(ts_snap, f):
  return ts_snap[f].view(torch.float32).cpu().numpy()


def _assert_vs_oracle(ts, want, what):
  """One TimeStep snapshot against the oracle's (step_type, reward, discount, obs): the oracle's float64 reward rounded to
  float32; a FIRST step carries reward 0 and discount 1."""
  st, r, d, obs = want
  live = st != 0
  np.testing.assert_array_equal(ts['step_type'].cpu().numpy(), st, err_msg=f'{what} step_type')
  got_r, got_d = _f32(ts, 'reward'), _f32(ts, 'discount')
  np.testing.assert_array_equal(eu.f32_bits(got_r[live]), eu.f32_bits(r[live].astype(np.float32)), err_msg=f'{what} reward')
  np.testing.assert_array_equal(got_d[live], d[live].astype(np.float32), err_msg=f'{what} discount')
  assert (got_r[~live] == 0).all() and (got_d[~live] == 1).all(), what
  np.testing.assert_array_equal(eu.f32_bits(_f32(ts, 'observation')), eu.f32_bits(obs), err_msg=f'{what} observation')


def _assert_holds_the_oracle(g, after, orc, what, rows=slice(None)):
  """What the environment holds against the oracle: the packed words field by field, the info columns, bsuite_info()."""
  words, ctx = cu.oracle_words(g, orc)
  state = after['state']['state'].cpu().numpy()[rows]
  fields = {cu.MC: dict(timestep=(0, 0xFFFFF), query=(20, 0xFF), reset=(28, 1)), cu.UC: dict(timestep=(0, 0xFFFFF), need=(20, 1),
            has=(21, 1), reset=(22, 1)), cu.DC: dict(timestep=(0, 0xFF), context=(8, 0xF), reset=(12, 1))}[g['family']]
  for name, (shift, mask) in fields.items():
    np.testing.assert_array_equal((state >> shift) & mask, (words >> shift) & mask, err_msg=f'{what} {name}')
  np.testing.assert_array_equal(state, words, err_msg=f'{what} state word')
  if ctx is not None:
    np.testing.assert_array_equal(after['state']['context'].cpu().numpy()[rows], ctx, err_msg=f'{what} context')
  raw_info = after['raw_info'].view(torch.float64).cpu().numpy()[:, rows]
  for j, (k, v) in enumerate(orc.bsuite_info().items()):
    np.testing.assert_array_equal(raw_info[j], v, err_msg=f'{what} info column {k}')
    np.testing.assert_array_equal(after['info'][k].view(torch.float64).cpu().numpy()[rows], v, err_msg=f'{what} bsuite_info {k}')


# ------------------------------------------------------------------------------------- A. the eager step and the reference
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_eager_step_against_the_oracle(family, kwargs):
  g, e = cu.grid(family, kwargs), eager(family, kwargs)
  ts, after = e['ts'][0], e['after'][0]
  orc, want = cu.oracle_step(g)
  _assert_vs_oracle(ts, want, family)
  _assert_holds_the_oracle(g, after, orc, family)
  pred = cu.predicates(g, want)
  for name, rows in pred.items():
    assert rows.sum() >= cu.MIN_LANES, name
  # the episode's one info update: exactly +1 / +2 on the rows that end, from 0 and from 2^24 + 1, and nothing elsewhere
  raw_info = after['raw_info'].view(torch.float64).cpu().numpy()
  np.testing.assert_array_equal(raw_info, cu.expected_info(g, want))
  if family == cu.MC:
    hit, miss = pred['ends_hit'], pred['ends_miss']
    np.testing.assert_array_equal(raw_info[0][hit], g['info'][0][hit] + 1.0)
    np.testing.assert_array_equal(raw_info[1][miss], g['info'][1][miss] + 2.0)
    np.testing.assert_array_equal(raw_info[0][~hit], g['info'][0][~hit])
    np.testing.assert_array_equal(raw_info[1][~miss], g['info'][1][~miss])
    running = ~g['reset']
    np.testing.assert_array_equal(after['state']['context'].cpu().numpy()[running], g['ctx'][running])      # only a reset draws
  elif family == cu.UC:
    miss = pred['ends_mismatch']
    np.testing.assert_array_equal(raw_info[0][miss], g['info'][0][miss] + 2.0)
    np.testing.assert_array_equal(raw_info[0][~miss], g['info'][0][~miss])
  else:
    assert not after['raw_info'].any()
  # discounting_chain clamps and counts an episode's first action outside -5..4; nothing else is counted anywhere
  assert e['invalid'][0] == int(cu.invalid_rows(g).sum()) and (family == cu.DC) == (e['invalid'][0] > 0)
  assert e['invalid'][T_MAX - 1] == e['invalid'][0]
  counters = after['counters'].cpu().numpy()
  assert counters.tolist() == [int((want[0] == 2).sum()), int((want[0] == 0).sum())]
  assert after['step_index'] == cu.STEP0 + 1
  # the two steps that follow (random actions, resets inside) against the oracle as well: B compares with them
  acts = e['actions'].cpu().numpy()
  for t in range(1, T_MAX):
    want = tuple(v.copy() for v in orc.call(cu.oracle_actions(family, acts[t]), cu.STEP0 + t))
    _assert_vs_oracle(e['ts'][t], want, (family, t))
    _assert_holds_the_oracle(g, e['after'][t], orc, (family, t))
  assert bool((e['ts'][1]['step_type'] == 0).any())                            # resets inside the run


# ------------------------------------------------------------------------------------- B. every path equals the eager step
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_rollout_equals_eager_steps(family, kwargs, T):
  g, e = cu.grid(family, kwargs), eager(family, kwargs)
  # which kernel the lean rollout of the case is (the shape rule of launch_small_obs, csrc/small_obs.h)
  kind = cu.rollout_class(family, kwargs)
  numel = cu.numel_of(family, kwargs)
  if family == cu.DC:
    assert kind == 'regs_lean' and numel == 2
  elif family == cu.MC and kwargs['num_bits'] == 1:
    assert kind == ('regs_lean_table' if kwargs['memory_length'] <= 4095 else 'regs_lean') and numel == 3
  else:
    assert kind == ('generic_lean' if numel <= 8 else 'packed_tile')
  env = _make(family, kwargs, g['lanes'])
  cu.load(env, g)
  assert tuple(env.observation_spec().shape) == (1, numel)
  _assert_ts(_run(env, e['actions'], T, 'rollout'), _stack(e['ts'], T), (family, T, 'rollout', kind))
  _assert_after(_snap_after(env), e['after'][T - 1], (family, T, 'rollout', kind))
  assert _invalid(env) == e['invalid'][T - 1]
  if T > 1:
    assert bool((e['ts'][1]['step_type'] == 0).any())                          # a reset inside the fused loop


def _wrapped_paths(family, kwargs, T, wrap, fields, what_wrap):
  g, e = cu.grid(family, kwargs), eager(family, kwargs)
  for path in ('step', 'rollout'):
    what = (family, T, what_wrap, path)
    env = wrap(_make(family, kwargs, g['lanes']))
    cu.load(env, g)
    got = _run(env, e['actions'], T, path)
    _assert_ts(got, _stack(e['ts'], T), what, fields=fields)
    _assert_after(_snap_after(env), e['after'][T - 1], what)
    assert _invalid(env) == e['invalid'][T - 1]
    if 'reward' not in fields:
      live = e['ts'][0]['step_type'] != 0
      noisy = got['reward'].view(torch.float32)[0] != e['ts'][0]['reward'].view(torch.float32)
      assert float(noisy[live].float().mean()) > 0.99                           # the wrapper was in the kernel


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_logging_paths_equal_the_eager_step(family, kwargs, T):
  _wrapped_paths(family, kwargs, T, lambda env: wrappers.Logging(env, None, max_rows=8), TS_FIELDS, 'Logging')


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_reward_noise_paths_equal_the_eager_step(family, kwargs, T):
  """The reward is the base reward plus noise: not compared.  The info columns of the three families are functions of the
  base reward, the state and the action alone, so they are."""
  _wrapped_paths(family, kwargs, T, lambda env: wrappers.RewardNoise(env, noise_scale=0.1, seed=3), NO_REWARD, 'RewardNoise')


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_logging_and_noise_paths_equal_the_eager_step(family, kwargs, T):
  _wrapped_paths(family, kwargs, T, lambda env: wrappers.Logging(wrappers.RewardNoise(env, noise_scale=0.1, seed=3), None, max_rows=8),
                 NO_REWARD, 'Logging(RewardNoise)')


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_mt19937_step_equals_the_eager_step(family, kwargs):
  """T = 1 on every 17th row, the lanes' draws from their own MT19937 generators.  No draw decides a step type, a discount,
  the time field or an info column on this step: compared on every row.  Compared on the rows that consume no visible draw
  only: memory_chain's state, context and observation (a reset row draws context and query); umbrella_chain's need / has
  fields and observation head (a reset row draws them) and its reward (a MID row draws it).  umbrella_chain's distractor
  elements are drawn on every row and are left to tests/test_gpu_wide_rows.py.  (121 rows cannot hold a wave per predicate:
  every predicate is among them, at least half a wave is compared in full; tests/test_chain_edges_host.py holds both.)"""
  g, e = cu.grid(family, kwargs), eager(family, kwargs)
  rows = cu.mt_rows(g)
  env = _make(family, kwargs, len(rows), rng='mt19937')
  cu.load(env, g, rows)
  rows_t = _cuda(rows)
  got = _snap_ts(env.step(e['actions'][0][rows_t].contiguous()))
  want = {f: e['ts'][0][f][rows_t] for f in TS_FIELDS}
  _assert_ts(got, e['ts'][0], (family, 'mt19937'), fields=('step_type', 'discount'), rows=rows_t)
  keep = _cuda(~cu.draw_rows(g)[rows])
  assert int(keep.sum()) >= cu.MIN_LANES // 2                                  # (of the 121 rows the environment holds)
  st = want['step_type']
  for p, r in cu.predicates(g, cu.oracle_step(g)[1]).items():
    assert r[rows].any(), (p, 'not among the rows')
  if family == cu.UC:
    paid = st != 1
    assert int((st == 2).sum()) >= 8
    assert torch.equal(got['reward'][paid], want['reward'][paid]), (family, 'mt19937', 'reward')
    assert torch.equal(got['observation'][keep][..., :3], want['observation'][keep][..., :3]), (family, 'mt19937', 'observation head')
  else:
    assert torch.equal(got['reward'], want['reward']), (family, 'mt19937', 'reward')
    assert torch.equal(got['observation'][keep], want['observation'][keep]), (family, 'mt19937', 'observation')
  after, want_after = _snap_after(env), e['after'][0]
  state, want_state = after['state']['state'], want_after['state']['state'][rows_t]
  drawn_fields = {cu.MC: 0xFF << 20, cu.UC: 3 << 20, cu.DC: 0}[family]          # query | need, has: a reset row draws them
  assert torch.equal(state & ~drawn_fields, want_state & ~drawn_fields), (family, 'mt19937', 'time field and reset bit')
  assert torch.equal(state[keep], want_state[keep]), (family, 'mt19937', 'state')
  if family == cu.MC:
    assert torch.equal(after['state']['context'][keep], want_after['state']['context'][rows_t][keep]), (family, 'mt19937', 'context')
  assert torch.equal(after['raw_info'], want_after['raw_info'][:, rows_t])
  for k, w in want_after['info'].items():
    assert torch.equal(after['info'][k], w[rows_t]), (family, 'mt19937', k)
  assert after['counters'].tolist() == [int((st == 2).sum()), int((st == 0).sum())]
  assert _invalid(env) == int(cu.invalid_rows(g)[rows].sum())


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_reset_mask_and_mark_reset_on_the_grid(family, kwargs):
  """A seeded third of the lanes is marked, lanes about to end and lanes already holding the reset word among them: the
  TimeStep, the words and the info columns equal the oracle's with reset_next set on those lanes."""
  g = cu.grid(family, kwargs)
  B = g['lanes']
  mask = np.random.default_rng(41).random(B) < 1.0 / 3.0
  mask_t, acts = _cuda(mask), _cuda(g['action'])
  orc, want = cu.oracle_step(g, reset_mask=mask)
  assert (want[0][mask] == 0).all() and (mask & ~g['reset']).sum() >= cu.MIN_LANES
  pred = cu.predicates(g, cu.oracle_step(g)[1])
  for name, rows in pred.items():
    assert (rows & ~mask).sum() >= cu.MIN_LANES // 2 and (rows & mask).sum() >= 8, name
  env = _make(family, kwargs, B)
  cu.load(env, g)
  ts = _snap_ts(env.step(acts, reset_mask=mask_t))
  after = _snap_after(env)
  _assert_vs_oracle(ts, want, (family, 'reset_mask'))
  _assert_holds_the_oracle(g, after, orc, (family, 'reset_mask'))
  assert after['counters'].tolist() == [int((want[0] == 2).sum()), int((want[0] == 0).sum())]
  assert _invalid(env) == int((cu.invalid_rows(g) & ~mask).sum())             # a marked lane's action is not looked at
  marked_info = after['raw_info'].view(torch.float64).cpu().numpy()[:, mask]
  np.testing.assert_array_equal(marked_info, g['info'][:, mask])               # an abandoned episode moves no column
  # mark_reset(), then the plain step: the same words, the same TimeStep
  env2 = _make(family, kwargs, B)
  cu.load(env2, g)
  loaded = env2._state['state'].clone()                                         # pylint: disable=protected-access
  env2.mark_reset(mask_t.to(torch.uint8))
  bit = {cu.MC: cu.MC_RESET_BIT, cu.UC: cu.UC_RESET_BIT, cu.DC: cu.DC_RESET_BIT}[family]
  assert torch.equal(env2._state['state'], torch.where(mask_t, loaded | bit, loaded))      # pylint: disable=protected-access
  _assert_ts(_snap_ts(env2.step(acts)), ts, (family, 'mark_reset'))
  _assert_after(_snap_after(env2), after, (family, 'mark_reset'))
  assert _invalid(env2) == _invalid(env)


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_device_step_counter_paths_equal_the_eager_step(family, kwargs):
  g, e = cu.grid(family, kwargs), eager(family, kwargs)
  for path in ('step', 'rollout'):
    what = (family, 'device_step_counter', path)
    env = _make(family, kwargs, g['lanes'], device_step_counter=True)
    cu.load(env, g)
    _assert_ts(_run(env, e['actions'], T_MAX, path), _stack(e['ts'], T_MAX), what)
    assert eu.raw(env).device_step_index() == cu.STEP0 + T_MAX, what
    after = _snap_after(env)
    after['step_index'] = eu.raw(env).device_step_index()                       # (the device counter is the authority here)
    _assert_after(after, e['after'][T_MAX - 1], what)


@pytest.fixture
def row_path(monkeypatch):
  """Every batched chain environment with a wide row brings a row scratch, whatever its size (tests/test_gpu_wide_rows.py)."""
  monkeypatch.setattr(base.Environment, 'row_path_min_bytes', 0)


@pytest.mark.parametrize('family,kwargs', WIDE_PARAMS)
def test_chain_edges_rows_on_the_row_path(row_path, family, kwargs):
  """Rows over 8 floats, a single step, a row scratch: lane advance + the store stream that decodes the packed rows — lean,
  under RewardNoise (the wrapped advance) and under Logging."""
  g, e = cu.grid(family, kwargs), eager(family, kwargs)
  wraps = [(lambda env: env, TS_FIELDS, 'lean'), (lambda env: wrappers.RewardNoise(env, noise_scale=0.1, seed=3), NO_REWARD, 'RewardNoise'),
           (lambda env: wrappers.Logging(env, None, max_rows=8), TS_FIELDS, 'Logging')]
  for wrap, fields, name in wraps:
    env = wrap(_make(family, kwargs, g['lanes']))
    cu.load(env, g)
    _assert_ts(_run(env, e['actions'], T_MAX, 'step'), _stack(e['ts'], T_MAX), (family, 'row path', name), fields=fields)
    assert bool(eu.raw(env)._call_desc.row_scratch), (family, name, 'not on the row path')      # pylint: disable=protected-access
    _assert_after(_snap_after(env), e['after'][T_MAX - 1], (family, 'row path', name))


def test_the_longest_chain_is_the_bound():
  """The state word holds the time in 20 bits; memory_chain reaches t = L + 1.  Both families refuse a chain longer than the
  10^6 steps of the grid's longest cases (BSX_ERANGE from the ABI check, before anything is launched)."""
  assert cu.MAX_CHAIN + 1 < 1 << 20
  for family, kwargs in ((cu.MC, dict(memory_length=cu.MAX_CHAIN + 1, num_bits=1)), (cu.UC, dict(chain_length=cu.MAX_CHAIN + 1, n_distractor=2))):
    env = _make(family, kwargs, 64)
    with pytest.raises(RuntimeError, match=r'\(code -4\)'):
      env.step(torch.zeros(64, dtype=torch.int32, device='cuda'))


# ------------------------------------------------------------------------------------- grouped launches
GROUPED_MODES = ['per_family', 'per_family_streams', 'small_mixed', 'small_mixed_streams', 'whole_sweep', 'whole_sweep_streams',
                 'whole_sweep_rows_in_stream', 'whole_sweep_split', 'whole_sweep_pipelined']


@pytest.mark.parametrize('mode', GROUPED_MODES, ids=['grouped_' + m for m in GROUPED_MODES])
def test_grouped_launches_equal_standalone_envs(mode):
  """A SweepBatch of the chain ids whose settings are grid cases (the longest memory_len, the widest memory_size, an
  umbrella_length, the widest umbrella_distract, a discounting_chain) and catch/0, so that the whole-sweep group has a phase
  1, with grid rows loaded into its segment environments before prepare_groups (each segment's own state_dict(), so its call
  index is kept): three grouped steps against stand-alone environments loaded with the same rows.  per_family:
  small_obs_group_kernel and the duo group kernel; small_mixed: ONE group for all of them; whole_sweep: the sweep's phase 0,
  with the wide rows built there or (rows_in_stream) written by the store stream, cut as two launches the other way (split),
  or pipelined (the lanes run one advance ahead of the TimeSteps)."""
  ids, reps = list(cu.GROUPED_IDS) + ['catch/0'], 3
  grids = [cu.grid(*c) for c in cu.GROUPED_IDS.values()]
  for bid, (family, kwargs) in cu.GROUPED_IDS.items():
    given = {k: v for k, v in kwargs.items() if k in sweep.SETTINGS[bid]}
    assert given == sweep.SETTINGS[bid], bid
  lanes = max(g['lanes'] for g in grids)
  batch = sb.SweepBatch(ids, len(ids) * lanes, seed=cu.SEED)
  acts, refs = [], []
  for (bid, begin, n), env, g in zip(batch.segments, batch.envs, grids + [None]):
    assert n == lanes
    ref = bsuite_amd.load_from_id(bid, batch=n, lane_offset=begin, num_buffers=1, seed=cu.SEED)
    if g is None:                                  # catch/0: from its fresh reset
      acts.append(torch.ones(n, dtype=torch.int32, device='cuda'))
    else:
      assert (eu.raw(env)._abi_name, tuple(env.observation_spec().shape)) == (g['family'], (1, g['numel']))      # pylint: disable=protected-access
      rows = np.arange(n) % g['lanes']
      cu.load(env, g, rows, step0=None)
      cu.load(ref, g, rows, step0=None)
      acts.append(_cuda(g['action'][rows]))
    refs.append(ref)
  base_mode = mode.replace('_streams', '')
  whole = base_mode.startswith('whole_sweep')
  pipelined = base_mode == 'whole_sweep_pipelined'
  extra = dict(rows_in_stream=base_mode == 'whole_sweep_rows_in_stream', split=base_mode == 'whole_sweep_split') if whole else {}
  batch.prepare_groups(acts, mix_all=whole, mix_pairs=False, mix_small=base_mode == 'small_mixed', pipelined=pipelined, **extra)
  if base_mode == 'whole_sweep_rows_in_stream':
    assert sum(v is not None for v in batch._row_scratch.values()) == 3        # pylint: disable=protected-access
  for s in range(reps):
    if mode.endswith('_streams'):
      outs = batch.step_grouped_streams()
      batch.join_streams()
    else:
      outs = batch.step_grouped()
    torch.cuda.synchronize()
    for bid, out, ref, a in zip(ids, outs, refs, acts):
      _assert_ts(_snap_ts(out), _snap_ts(ref.step(a)), (mode, bid, s))
  if base_mode == 'whole_sweep_split':
    assert batch._split, 'the split cut fell back to the ordinary one'          # pylint: disable=protected-access
  batch.sync()
  if pipelined:
    for ref, a in zip(refs, acts):
      ref.step(a)
  batch.release_groups()                         # (the lanes come back in the environments' own state columns)
  for bid, env, ref in zip(ids, batch.envs, refs):
    for k, v in ref.bsuite_info().items():
      assert torch.equal(_bits(env.bsuite_info()[k]), _bits(v)), (mode, bid, k)
    assert torch.equal(eu.raw(env).episode_counters(), eu.raw(ref).episode_counters()), (mode, bid)
    assert torch.equal(eu.raw(env).invalid_action_count(), eu.raw(ref).invalid_action_count()), (mode, bid)
    mine, theirs = eu.raw(env).state_dict(), eu.raw(ref).state_dict()
    for k in eu.raw(ref)._state:                                                # pylint: disable=protected-access
      assert torch.equal(mine[k], theirs[k]), (mode, bid, k)
    assert torch.equal(_bits(eu.raw(env)._info), _bits(eu.raw(ref)._info)), (mode, bid, 'info columns')      # pylint: disable=protected-access
  # the stand-alone discounting_chain counted its clamped first actions on each of the three steps that found the lane there
  assert int(eu.raw(refs[4]).invalid_action_count().item()) >= int(cu.invalid_rows(grids[4]).sum())


# ------------------------------------------------------------------------------------- large batches, one step
LARGE = [pytest.param(cu.CASES[0], (1 << 19) + 257, id='memory_chain_L100_nb1_2p19_257'),
         pytest.param(cu.CASES[-1], (1 << 20) + 257, id='discounting_chain_seed4_2p20_257')]


@pytest.mark.parametrize('case,B', LARGE)
def test_tiled_large_batch_equals_the_small_batch(case, B):
  """The grid tiled to a large batch, ONE step: past EAGER_LPT_MIN_BLOCKS workgroups (2048 for memory_chain, 4096 for
  discounting_chain) the lean eager step is small_obs_eager2_kernel, two lanes per thread, here with a ragged tail.  Every
  tile equals the small-batch result of A — except memory_chain's reset rows, which draw context and query by their global
  lane id: those are held to the oracle on their own lane ids."""
  family, kwargs = case
  assert (family, kwargs) == ((cu.MC, dict(memory_length=100, num_bits=1)) if family == cu.MC else (cu.DC, dict(mapping_seed=4)))
  assert -(-B // cu.BLOCK) > {cu.MC: 2048, cu.DC: 4096}[family] and B % (2 * cu.BLOCK) == 257
  g, e = cu.grid(family, kwargs), eager(family, kwargs)
  rows = np.arange(B) % g['lanes']
  env = _make(family, kwargs, B)
  cu.load(env, g, rows)
  rows_t = _cuda(rows)
  got = _snap_ts(env.step(e['actions'][0][rows_t].contiguous()))
  after = _snap_after(env)
  st = e['ts'][0]['step_type'][rows_t]
  assert after['counters'].tolist() == [int((st == 2).sum()), int((st == 0).sum())]
  assert after['step_index'] == cu.STEP0 + 1
  assert _invalid(env) == int(cu.invalid_rows(g)[rows].sum())
  drawn = cu.draw_rows(g)[rows]
  assert drawn.any() == (family == cu.MC)
  keep = _cuda(~drawn)
  want, want_after = e['ts'][0], e['after'][0]
  for f in TS_FIELDS:
    assert torch.equal(got[f][keep], want[f][rows_t][keep]), (family, B, f)
  for f in ('step_type', 'reward', 'discount'):
    assert torch.equal(got[f], want[f][rows_t]), (family, B, f)
  for k, w in want_after['info'].items():
    assert torch.equal(after['info'][k], w[rows_t]), (family, B, k)
  assert torch.equal(after['raw_info'], want_after['raw_info'][:, rows_t])
  for k, w in want_after['state'].items():
    assert torch.equal(after['state'][k][keep], w[rows_t][keep]), (family, B, k)
  if not drawn.any():
    return
  sel = np.flatnonzero(drawn)
  assert len(sel) >= cu.MIN_LANES
  orc, o_want = cu.oracle_step(g, rows[sel], lane_ids=np.uint64(cu.LANE_OFFSET) + sel.astype(np.uint64))
  sel_t = _cuda(sel)
  _assert_vs_oracle({f: got[f][sel_t] for f in TS_FIELDS}, o_want, (family, B, 'reset rows'))
  words, ctx = cu.oracle_words(g, orc)
  np.testing.assert_array_equal(after['state']['state'][sel_t].cpu().numpy(), words)
  np.testing.assert_array_equal(after['state']['context'][sel_t].cpu().numpy(), ctx)
  assert set(ctx.tolist()) == {0, 1}                                           # both contexts drawn


# ------------------------------------------------------------------------------------- C. several episodes inside one call
_TWINS = {}


def _episode_twin(family, kwargs, T):
  """The eager step() of a twin loaded with the mixed-phase grid, one call at a time, and the oracle through the same actions
  (with the Logging bookkeeping of oracle/logging_oracle.py): computed once per case, never modified."""
  key = (family, tuple(sorted(kwargs.items())), T)
  if key not in _TWINS:
    g = cu.mixed_grid(family, kwargs)
    acts = cu.episode_actions(g, T)
    twin = _make(family, kwargs, g['lanes'])
    cu.load(twin, g)
    acts_t = _cuda(acts)
    snaps = [_snap_ts(twin.step(acts_t[t])) for t in range(T)]
    orc = cu.make_oracle(g)
    trk = logging_oracle.TrackOracle(g['lanes'], list(orc.bsuite_info()))
    st, r, obs = [], [], []
    for t in range(T):
      s, rew, _, o = orc.call(cu.oracle_actions(family, acts[t]), cu.STEP0 + t)
      trk.track(s, rew, orc.bsuite_info())
      st.append(s.copy())
      r.append(rew.copy())
      obs.append(o.copy())
    _TWINS[key] = dict(ts=_stack(snaps, T), after=_snap_after(twin), actions=acts_t, orc=orc, trk=trk, st=np.stack(st), r=np.stack(r),
                       obs=np.stack(obs))
  return _TWINS[key]


EPISODE_PARAMS = [pytest.param(*c, id=cu.case_id(*c[:2])) for c in cu.EPISODE_CASES]


@pytest.mark.parametrize('logged', [False, True], ids=['lean', 'Logging'])
@pytest.mark.parametrize('family,kwargs,T,episodes', EPISODE_PARAMS)
def test_several_episodes_inside_one_call(family, kwargs, T, episodes, logged):
  """ONE fused rollout(T) from mixed phases — on every step of the loop some lanes end an episode, some reset and the others
  are in the middle of one (tests/test_chain_edges_host.py asserts that on the reference): the register-resident lean
  rollout with its time table (memory_chain L = 3) and without (discounting_chain, 230 steps: every reward step and the bonus
  on the LAST step), the packed-tile rollout (memory_chain 40 bits, umbrella_chain 20 distractors), and the same under
  Logging."""
  g, w = cu.mixed_grid(family, kwargs), _episode_twin(family, kwargs, T)
  B = g['lanes']
  assert (w['st'] == 2).sum(axis=0).min() >= episodes and ((w['st'] == 2).sum(axis=1) > 0).all()
  env = _make(family, kwargs, B)
  if logged:
    env = wrappers.Logging(env, None, max_rows=32)
  cu.load(env, g)
  ts = env.rollout(w['actions'])
  got = _snap_ts(ts)
  what = (family, T, 'Logging' if logged else 'lean')
  _assert_ts(got, w['ts'], what)
  after = _snap_after(env)
  _assert_after(after, w['after'], what)
  # ... and the oracle: step types, rewards, observations, the state it ends in, the info columns, the counters
  st = ts.step_type.cpu().numpy()
  np.testing.assert_array_equal(st, w['st'])
  live = w['st'] != 0
  reward = ts.reward.cpu().numpy()
  np.testing.assert_array_equal(eu.f32_bits(reward[live]), eu.f32_bits(w['r'][live].astype(np.float32)))
  assert (reward[~live] == 0).all()
  np.testing.assert_array_equal(eu.f32_bits(ts.observation.cpu().numpy()), eu.f32_bits(w['obs']))
  _assert_holds_the_oracle(g, after, w['orc'], what)
  assert after['counters'].tolist() == [int((w['st'] == 2).sum()), int((w['st'] == 0).sum())]
  assert after['step_index'] == cu.STEP0 + T and _invalid(env) == 0
  if logged:
    trk, c = w['trk'], env.counters(check=True)
    for k in ('steps', 'episode', 'total_return'):
      np.testing.assert_array_equal(c[k].cpu().numpy(), getattr(trk, k), err_msg=f'{what} {k}')
    np.testing.assert_array_equal(env.num_rows().cpu().numpy(), [len(r) for r in trk.rows])
