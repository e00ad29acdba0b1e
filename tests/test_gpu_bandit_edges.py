"""GPU: the bandit and mnist kernels on the mixed-phase edge grid of tests/bandit_edge_util.py, across every launch path.

An episode of both families is two calls (FIRST, LAST), so from a fresh reset every lane of a batch is in the same phase on
every call — which is how nearly every other test of the two families runs.  A wave of bandit_env::core / ::step or of
mnist_advance_body then never diverges between the reset branch and the step branch, bandit's fused rollout adds to the
regret it carries in a register (IREGS) on the same loop iterations for all lanes, every chunk of mnist_observe_chunks sees
all lanes showing or none — a wrong select (row = show ? idx * cells : 0, v = show ? lut : 0, dl = live ? dl : 0) is invisible
when the whole batch agrees — and the pipelined sweep's stream never reads another state column than the one a uniform batch
would have.  The grid puts the lanes of one batch in both phases, with values no natural run produces: an mnist index at the
top of its 24-bit field next to the label, pixel bytes of 128 and above on lanes that must show zeros, image geometries from
4 to 4096 pixels, a regret column above 2^24, bandit tables of 1 and 32 arms, actions at INT_MIN, -1, num_actions, INT_MAX
(tests/test_bandit_edges_host.py proves each branch on at least a wave of lanes).  Everything is exact: int32 bit patterns of
every TimeStep field, the state column, the info column, bsuite_info(), the episode counters, invalid_action_count() and the
call index.  No tolerances.

  A. the eager lean step() from the loaded grid against oracle/coracle.OracleEnv, three steps with resets inside;
  B. every other path against that eager run from the same loaded state, T = 1 and T = 3;
  C. twenty episodes inside ONE call from mixed phases, against an eager twin and the oracle.

Out-of-spec actions: bandit's are clamped and counted by the engine (the oracle gets the clamped action); mnist's are
compared with the label as they are, like the reference does, and nothing is counted.

Which test drives the grid through which kernel (launch_small_obs of csrc/small_obs.h for bandit; csrc/mnist.hip,
csrc/pair_mixed.hip, csrc/sweep_mixed.hip):
  small_obs_kernel, one lean step              bandit: the eager step of A
  small_obs_eager2_kernel                      bandit: test_tiled_large_batch (2^19 + 257 lanes); at small shapes, two and four
                                               lanes per thread, through
                                               test_gpu_pair_path_small_shapes.test_two_lanes_per_thread_eager_step_at_small_shapes
  small_obs_kernel, wrapped / mt19937 step     bandit: test_logging_paths, test_reward_noise_paths, test_logging_and_noise_paths
                                               ('step'), test_mt19937_paths ('step')
  small_obs_lean_rollout_kernel (IREGS)        bandit: test_rollout, test_device_step_counter_paths and part C (no TAB and no
                                               pooled form: bandit has neither)
  small_obs_kernel, wrapped rollouts           bandit: the 'rollout' halves of the Logging / RewardNoise tests, part C under Logging
  small_obs_kernel, mt19937 rollouts           bandit: test_mt19937_paths — plain (the generic loop of a rollout that is not lean),
                                               under Logging, RewardNoise and both (the MT = -1 instantiations)
  mnist_advance_kernel + mnist_observe_kernel  mnist: A, test_rollout (the pair once per step), the wrapped tests, mt19937,
                                               device_step_counter, part C; FULL and guarded blocks in every case but 64x64
                                               (whose blocks are all full), the nt stores in the 2^24-image case
  small_obs_duo_group_kernel                   test_grouped_launches, per_family (bandit beside the chain segment)
  small_obs_mixed_group_kernel                 test_grouped_launches, small_mixed and pair_mixed (bandit)
  mnist_group_kernel, both phases              test_grouped_launches, per_family and small_mixed (mix_pairs off)
  pair_mixed_advance_kernel / _stream_kernel   test_grouped_launches, pair_mixed (mnist beside catch)
  sweep_phase0_kernel + the store stream       test_grouped_launches, whole_sweep (mnist_advance_body<0>)
  the split cut, sweep_pipelined_kernel        test_grouped_launches, whole_sweep_split, whole_sweep_pipelined (the stream reads the
                                               other state column, state_alt)
  bsx_lane_reset_mark + the eager step         test_reset_mask_and_mark_reset
Not reachable from Python, so not here: mnist_observe_chunks with a caller-defined pixel table (ARITH = false; the constructor
always passes numpy's own 256 values, which mnist_make recognises).
"""
import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import sweep
from bsuite_amd import sweep_batch as sb
from bsuite_amd.utils import datasets, wrappers
from oracle import logging_oracle
from tests import bandit_edge_util as bu
from tests import edge_snap_util as es
from tests import engine_util as eu

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]      # every test under its own time limit

CASE_PARAMS = [pytest.param(*c, id=i) for c, i in zip(bu.CASES, bu.CASE_IDS)]
BANDIT_PARAMS = [p for p, c in zip(CASE_PARAMS, bu.CASES) if c[0] == bu.BD]
T_MAX = 3
TS_FIELDS = es.TS_FIELDS
NO_REWARD = ('step_type', 'discount', 'observation')
_bits, _snap_ts, _snap_after, _stack, _assert_ts = es.bits, es.snap_ts, es.snap_after, es.stack, es.assert_ts


def _assert_after(got, want, what, **kw):
  es.assert_after(got, want, what, raw_info=True, **kw)      # here always with the info column itself


def _make(family, kwargs, batch, **engine_kwargs):
  return eu.make_env(family, bu.ctor_kwargs(family, kwargs), batch=batch, lane_offset=bu.LANE_OFFSET, seed=bu.SEED, **engine_kwargs)


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
  key = bu.case_id(family, kwargs)
  if key not in _EAGER:
    g = bu.grid(family, kwargs)
    env = _make(family, kwargs, g['lanes'])
    bu.load(env, g)
    assert env.step_index == bu.STEP0
    assert tuple(env.observation_spec().shape) == ((1, 1) if family == bu.BD else bu.dataset(kwargs['dataset'])[0].shape[1:])
    acts = _cuda(bu.episode_actions(g, T_MAX))
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


def _assert_holds_the_oracle(after, orc, words, what, rows=slice(None)):
  """What the environment holds against the oracle: the state word (`words`: bandit_edge_util.oracle_words), the info
  column, bsuite_info()."""
  state = after['state']['state'].cpu().numpy()[rows]
  np.testing.assert_array_equal(state, words, err_msg=f'{what} state word')
  raw_info = after['raw_info'].view(torch.float64).cpu().numpy()[:, rows]
  assert list(orc.bsuite_info()) == ['total_regret'] and raw_info.shape[0] == 1
  v = orc.bsuite_info()['total_regret']
  np.testing.assert_array_equal(raw_info[0].view(np.int64), v.view(np.int64), err_msg=f'{what} info column')
  np.testing.assert_array_equal(after['info']['total_regret'].cpu().numpy()[rows], v.view(np.int64), err_msg=f'{what} bsuite_info')


# ------------------------------------------------------------------------------------- A. the eager step and the reference
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_eager_step_against_the_oracle(family, kwargs):
  g, e = bu.grid(family, kwargs), eager(family, kwargs)
  ts, after = e['ts'][0], e['after'][0]
  orc, want = bu.oracle_step(g)
  _assert_vs_oracle(ts, want, family)
  words = bu.oracle_words(g, orc, g['state'], want[0], want[3])
  _assert_holds_the_oracle(after, orc, words, family)
  pred = bu.predicates(g, want)
  for name, rows in pred.items():
    assert rows.sum() >= bu.MIN_LANES, name
  # the regret column: regret + (1 - reward) as one f64 addition on the stepped rows — from 0, from a column with low bits
  # set and from 2^24 + 1 — and nothing on the reset rows
  raw_info = after['raw_info'].view(torch.float64).cpu().numpy()
  np.testing.assert_array_equal(raw_info.view(np.int64), bu.expected_info(g, want).view(np.int64))
  np.testing.assert_array_equal(raw_info[0][g['reset']], g['info'][0][g['reset']])
  state = after['state']['state'].cpu().numpy()
  if family == bu.BD:
    if 'best_arm' in pred:
      np.testing.assert_array_equal(raw_info[0][pred['best_arm']], g['info'][0][pred['best_arm']])
    np.testing.assert_array_equal(raw_info[0][pred['worst_arm']], g['info'][0][pred['worst_arm']] + 1.0)
    np.testing.assert_array_equal(state, (~g['reset']).astype(np.int32))
  else:
    np.testing.assert_array_equal(raw_info[0][pred['miss']], g['info'][0][pred['miss']] + 2.0)
    np.testing.assert_array_equal(raw_info[0][pred['hit']], g['info'][0][pred['hit']])
    stepped = ~g['reset']
    np.testing.assert_array_equal(state[stepped], (g['state'][stepped] & 0x0FFFFFFF) | bu.MN_RESET_BIT)      # index and label kept
    assert ((state[g['reset']] >> 28) == 2).all()                                # a reset lane shows, and nothing else is set
    obs = _f32(ts, 'observation').reshape(g['lanes'], -1)
    assert not obs[stepped].any() and obs[g['reset']].any(axis=1).all()         # zeros after the guess, bit for bit +0
    assert not ts['observation'].reshape(g['lanes'], -1)[_cuda(stepped)].any()
    # the stream's workgroups: full ones and a guarded one, and lanes of both phases inside one block (64x64: one lane per block)
    full, partial, mixed = bu.observe_blocks(g)
    one_lane = g['num_pixels'] == bu.OBS_BLOCK
    assert full >= 1 and (partial or one_lane) and (mixed >= 1 or one_lane), (full, partial, mixed)
  # bandit clamps and counts an action outside its arms; mnist counts nothing
  assert e['invalid'][0] == int(bu.invalid_rows(g).sum()) and (family == bu.BD) == (e['invalid'][0] > 0)
  assert e['invalid'][T_MAX - 1] == e['invalid'][0]
  counters = after['counters'].cpu().numpy()
  assert counters.tolist() == [int((want[0] == 2).sum()), int((want[0] == 0).sum())]
  assert after['step_index'] == bu.STEP0 + 1
  # the two steps that follow (random actions, resets inside) against the oracle as well: B compares with them
  acts = e['actions'].cpu().numpy()
  for t in range(1, T_MAX):
    want = tuple(v.copy() for v in orc.call(bu.oracle_actions(g, acts[t]), bu.STEP0 + t))
    _assert_vs_oracle(e['ts'][t], want, (family, t))
    words = bu.oracle_words(g, orc, words, want[0], want[3])
    _assert_holds_the_oracle(e['after'][t], orc, words, (family, t))
  assert bool((e['ts'][1]['step_type'] == 0).any()) and bool((e['ts'][2]['step_type'] == 0).any())      # resets inside the run


# ------------------------------------------------------------------------------------- B. every path equals the eager step
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_rollout_equals_eager_steps(family, kwargs, T):
  """bandit: the register-resident lean rollout, the regret in a register across the loop (IREGS) — lanes add on different
  iterations.  mnist: the kernel pair once per step."""
  g, e = bu.grid(family, kwargs), eager(family, kwargs)
  env = _make(family, kwargs, g['lanes'])
  bu.load(env, g)
  _assert_ts(_run(env, e['actions'], T, 'rollout'), _stack(e['ts'], T), (family, T, 'rollout'))
  _assert_after(_snap_after(env), e['after'][T - 1], (family, T, 'rollout'))
  assert _invalid(env) == e['invalid'][T - 1]
  if T > 1:
    assert bool((e['ts'][1]['step_type'] == 0).any()) and bool((e['ts'][1]['step_type'] == 2).any())      # both branches inside the loop


def _wrapped_paths(family, kwargs, T, wrap, fields, what_wrap):
  g, e = bu.grid(family, kwargs), eager(family, kwargs)
  for path in ('step', 'rollout'):
    what = (family, T, what_wrap, path)
    env = wrap(_make(family, kwargs, g['lanes']))
    bu.load(env, g)
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
  """The reward is the base reward plus noise: not compared.  The regret column is a function of the base reward alone, so
  it is."""
  _wrapped_paths(family, kwargs, T, lambda env: wrappers.RewardNoise(env, noise_scale=0.1, seed=3), NO_REWARD, 'RewardNoise')


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_logging_and_noise_paths_equal_the_eager_step(family, kwargs, T):
  _wrapped_paths(family, kwargs, T, lambda env: wrappers.Logging(wrappers.RewardNoise(env, noise_scale=0.1, seed=3), None, max_rows=8),
                 NO_REWARD, 'Logging(RewardNoise)')


MT_WRAPS = [('plain', lambda env: env, TS_FIELDS), ('Logging', lambda env: wrappers.Logging(env, None, max_rows=8), TS_FIELDS),
            ('RewardNoise', lambda env: wrappers.RewardNoise(env, noise_scale=0.1, seed=3), NO_REWARD),
            ('Logging(RewardNoise)', lambda env: wrappers.Logging(wrappers.RewardNoise(env, noise_scale=0.1, seed=3), None, max_rows=8),
             NO_REWARD)]


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_mt19937_paths_equal_the_eager_step(family, kwargs):
  """Every 17th row, the lanes' draws from their own MT19937 generators.  bandit draws nothing: step() and rollout(3), plain
  and under the wrappers (the MT = -1 instantiations of the generic loop), compared on every row in full.  mnist: one step;
  a reset row draws its image index, so its word and observation are compared on the other rows only, and on the reset rows
  the step type, reward, discount, the flag bits of the word and the info column.  (121 rows cannot hold a wave per
  predicate: every predicate is among them; tests/test_bandit_edges_host.py holds that.)"""
  g, e = bu.grid(family, kwargs), eager(family, kwargs)
  rows = bu.mt_rows(g)
  rows_t = _cuda(rows)
  for p, r in bu.predicates(g, bu.oracle_step(g)[1]).items():
    assert r[rows].any(), (p, 'not among the rows')
  acts = e['actions'][:, rows_t].contiguous()
  if family == bu.BD:
    for name, wrap, fields in MT_WRAPS:
      for path, T in (('step', 1), ('rollout', T_MAX)):
        what = (family, 'mt19937', name, path)
        env = wrap(_make(family, kwargs, len(rows), rng='mt19937'))
        bu.load(env, g, rows)
        got = _run(env, acts, T, path)
        want = {f: torch.stack([e['ts'][t][f][rows_t] for t in range(T)]) for f in TS_FIELDS}
        _assert_ts(got, want, what, fields=fields)
        after = _snap_after(env)
        _assert_after(after, e['after'][T - 1], what, rows=rows_t)
        assert after['counters'].tolist() == [sum(int((e['ts'][t]['step_type'][rows_t] == k).sum()) for t in range(T)) for k in (2, 0)]
        assert _invalid(env) == int(bu.invalid_rows(g)[rows].sum())
    return
  env = _make(family, kwargs, len(rows), rng='mt19937')
  bu.load(env, g, rows)
  got = _snap_ts(env.step(acts[0]))
  _assert_ts(got, e['ts'][0], (family, 'mt19937'), fields=('step_type', 'reward', 'discount'), rows=rows_t)
  keep = _cuda(~bu.draw_rows(g)[rows])
  assert int(keep.sum()) >= bu.MIN_LANES // 2                                    # (of the 121 rows the environment holds)
  want_obs = e['ts'][0]['observation'][rows_t]
  assert torch.equal(got['observation'][keep], want_obs[keep]), (family, 'mt19937', 'observation')
  shown = got['observation'][~keep].reshape(int((~keep).sum()), -1)
  assert bool(shown.any(dim=1).all())                                            # a reset row shows an image
  after, want_after = _snap_after(env), e['after'][0]
  state, want_state = after['state']['state'], want_after['state']['state'][rows_t]
  assert torch.equal(state >> 28, want_state >> 28), (family, 'mt19937', 'flag bits')
  assert torch.equal(state[keep], want_state[keep]), (family, 'mt19937', 'state')
  drawn = (state[~keep] & 0xFFFFFF).cpu().numpy()
  labels = bu.dataset(kwargs['dataset'])[1]
  assert (drawn < g['num_data']).all()
  np.testing.assert_array_equal((state[~keep] >> 24).cpu().numpy() & 0xF, labels[drawn])
  assert torch.equal(after['raw_info'], want_after['raw_info'][:, rows_t])
  st = e['ts'][0]['step_type'][rows_t]
  assert after['counters'].tolist() == [int((st == 2).sum()), int((st == 0).sum())] and _invalid(env) == 0


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_reset_mask_and_mark_reset_on_the_grid(family, kwargs):
  """A seeded third of the lanes is marked, lanes about to step and lanes already holding the reset word among them: the
  TimeStep, the words and the info column equal the oracle's with reset_next set on those lanes.  A marked lane's action —
  out-of-range ones among them — is neither read nor counted, and its info column does not move."""
  g = bu.grid(family, kwargs)
  B = g['lanes']
  mask = bu.reset_mask(g)
  mask_t, acts = _cuda(mask), _cuda(g['action'])
  orc, want = bu.oracle_step(g, reset_mask=mask)
  assert (want[0][mask] == 0).all() and (mask & ~g['reset']).sum() >= bu.MIN_LANES and (mask & g['reset']).sum() >= bu.MIN_LANES
  pred = bu.predicates(g, bu.oracle_step(g)[1])
  for name, rows in pred.items():
    assert (rows & ~mask).sum() >= bu.MIN_LANES // 2 and (rows & mask).sum() >= 8, name
  env = _make(family, kwargs, B)
  bu.load(env, g)
  ts = _snap_ts(env.step(acts, reset_mask=mask_t))
  after = _snap_after(env)
  _assert_vs_oracle(ts, want, (family, 'reset_mask'))
  _assert_holds_the_oracle(after, orc, bu.oracle_words(g, orc, g['state'], want[0], want[3]), (family, 'reset_mask'))
  assert after['counters'].tolist() == [int((want[0] == 2).sum()), int((want[0] == 0).sum())]
  assert _invalid(env) == int((bu.invalid_rows(g) & ~mask).sum())               # a marked lane's action is not looked at
  if family == bu.BD:
    assert (bu.invalid_rows(g) & mask).sum() >= 8
  marked_info = after['raw_info'].view(torch.float64).cpu().numpy()[:, mask]
  np.testing.assert_array_equal(marked_info, g['info'][:, mask])                 # an abandoned episode moves no column
  # mark_reset(), then the plain step: the same words, the same TimeStep
  env2 = _make(family, kwargs, B)
  bu.load(env2, g)
  loaded = env2._state['state'].clone()                                           # pylint: disable=protected-access
  env2.mark_reset(mask_t.to(torch.uint8))
  marked = torch.ones_like(loaded) if family == bu.BD else loaded | bu.MN_RESET_BIT
  assert torch.equal(env2._state['state'], torch.where(mask_t, marked, loaded))  # pylint: disable=protected-access
  _assert_ts(_snap_ts(env2.step(acts)), ts, (family, 'mark_reset'))
  _assert_after(_snap_after(env2), after, (family, 'mark_reset'))
  assert _invalid(env2) == _invalid(env)


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_device_step_counter_paths_equal_the_eager_step(family, kwargs):
  g, e = bu.grid(family, kwargs), eager(family, kwargs)
  for path in ('step', 'rollout'):
    what = (family, 'device_step_counter', path)
    env = _make(family, kwargs, g['lanes'], device_step_counter=True)
    bu.load(env, g)
    _assert_ts(_run(env, e['actions'], T_MAX, path), _stack(e['ts'], T_MAX), what)
    assert eu.raw(env).device_step_index() == bu.STEP0 + T_MAX, what
    after = _snap_after(env)
    after['step_index'] = eu.raw(env).device_step_index()                         # (the device counter is the authority here)
    _assert_after(after, e['after'][T_MAX - 1], what)
    assert _invalid(env) == e['invalid'][T_MAX - 1]


# ------------------------------------------------------------------------------------- grouped launches
GROUPED_MODES = ['per_family', 'per_family_streams', 'small_mixed', 'small_mixed_streams', 'pair_mixed', 'pair_mixed_streams', 'whole_sweep',
                 'whole_sweep_streams', 'whole_sweep_rows_in_stream', 'whole_sweep_split', 'whole_sweep_pipelined']
GROUPED_IDS = ['bandit/3', 'mnist/0', 'catch/0', 'memory_len/22']


@pytest.mark.parametrize('mode', GROUPED_MODES, ids=['grouped_' + m for m in GROUPED_MODES])
def test_grouped_launches_equal_standalone_envs(tmp_path, mode):
  """A SweepBatch of bandit/3 and mnist/0 (on the small synthetic dataset) with grid rows loaded into their segment
  environments before prepare_groups (each segment's own state_dict(), so its call index is kept), catch/0 and a chain id
  from their fresh resets: three grouped steps against stand-alone environments loaded with the same rows.  per_family:
  the duo group kernel (bandit) and mnist_group_kernel; small_mixed: ONE small group, mnist still on its own; pair_mixed:
  the mixed two-kernel group (mnist beside catch); whole_sweep: the sweep's phase 0 and store stream, cut as two launches
  the other way (split), or pipelined — the lanes run one advance ahead and the stream reads the other state column."""
  images, labels = bu.dataset('28x28')
  datasets.write_idx_files(str(tmp_path), images.view(np.uint8), labels)
  mn = dict(data_dir=str(tmp_path))
  ids, reps = GROUPED_IDS, 3
  cases = [bu.GROUPED_BANDIT, bu.GROUPED_MNIST, None, None]
  assert sweep.SETTINGS['bandit/3'] == bu.GROUPED_BANDIT[1] and sweep.SETTINGS['mnist/0'] == dict(seed=None)
  assert bu.GROUPED_MNIST[1] == dict(dataset='28x28')
  grids = [None if c is None else bu.grid(*c) for c in cases]
  lanes = max(g['lanes'] for g in grids if g is not None)
  batch = sb.SweepBatch(ids, len(ids) * lanes, seed=bu.SEED, env_kwargs=dict(mnist=mn))
  acts, refs = [], []
  for (bid, begin, n), env, g in zip(batch.segments, batch.envs, grids):
    assert n == lanes
    ekw = mn if bid == 'mnist/0' else {}
    ref = bsuite_amd.load_from_id(bid, batch=n, lane_offset=begin, num_buffers=1, seed=bu.SEED, **ekw)
    if g is None:                                  # from its fresh reset
      acts.append(torch.ones(n, dtype=torch.int32, device='cuda'))
    else:
      assert (eu.raw(env)._abi_name, int(np.prod(env.observation_spec().shape))) == (g['family'], g['numel'])      # pylint: disable=protected-access
      rows = np.arange(n) % g['lanes']
      bu.load(env, g, rows, step0=None)
      bu.load(ref, g, rows, step0=None)
      acts.append(_cuda(g['action'][rows]))
    refs.append(ref)
  base_mode = mode.replace('_streams', '')
  whole = base_mode.startswith('whole_sweep')
  pipelined = base_mode == 'whole_sweep_pipelined'
  extra = dict(rows_in_stream=base_mode == 'whole_sweep_rows_in_stream', split=base_mode == 'whole_sweep_split') if whole else {}
  batch.prepare_groups(acts, mix_all=whole, mix_pairs=base_mode == 'pair_mixed', mix_small=base_mode in ('small_mixed', 'pair_mixed'),
                       pipelined=pipelined, **extra)
  if whole:                                      # ONE group for the sweep (a pipelined pair: two)
    assert len(batch._groups) == (2 if pipelined else 1)                          # pylint: disable=protected-access
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
    assert batch._split, 'the split cut fell back to the ordinary one'            # pylint: disable=protected-access
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
    for k in eu.raw(ref)._state:                                                  # pylint: disable=protected-access
      assert torch.equal(mine[k], theirs[k]), (mode, bid, k)
    assert torch.equal(_bits(eu.raw(env)._info), _bits(eu.raw(ref)._info)), (mode, bid, 'info columns')      # pylint: disable=protected-access
  # the stand-alone bandit counted its clamped actions on each step that found the lane running; mnist counted nothing
  assert int(eu.raw(refs[0]).invalid_action_count().item()) >= int(bu.invalid_rows(grids[0]).sum())
  assert int(eu.raw(refs[1]).invalid_action_count().item()) == 0


# ------------------------------------------------------------------------------------- large batches, one step
@pytest.mark.parametrize('family,kwargs', BANDIT_PARAMS[1:2] + BANDIT_PARAMS[3:4])
def test_tiled_large_batch_equals_the_small_batch(family, kwargs):
  """The grid tiled to 2^19 + 257 lanes, ONE step: from 2048 workgroups up bandit's lean eager step is
  small_obs_eager2_kernel, two lanes per thread, here with a ragged tail.  bandit draws nothing: every tile equals the
  small-batch result of A.  (mnist needs no large batch: 257 lanes of 784 pixels are 49 full 16 KiB blocks and a guarded
  one, and its grids hold both — asserted in A.)"""
  B = (1 << 19) + 257
  assert -(-B // bu.BLOCK) > 2048 and B % (2 * bu.BLOCK) == 257
  g, e = bu.grid(family, kwargs), eager(family, kwargs)
  rows = np.arange(B) % g['lanes']
  env = _make(family, kwargs, B)
  bu.load(env, g, rows)
  rows_t = _cuda(rows)
  got = _snap_ts(env.step(e['actions'][0][rows_t].contiguous()))
  after = _snap_after(env)
  st = e['ts'][0]['step_type'][rows_t]
  assert after['counters'].tolist() == [int((st == 2).sum()), int((st == 0).sum())]
  assert _invalid(env) == int(bu.invalid_rows(g)[rows].sum())
  assert not bu.draw_rows(g).any()
  _assert_ts(got, e['ts'][0], (family, B), rows=rows_t)
  _assert_after(after, e['after'][0], (family, B), rows=rows_t)


# ------------------------------------------------------------------------------------- C. several episodes inside one call
_TWINS = {}


def _episode_twin(family, kwargs, T):
  """The eager step() of a twin loaded with the mixed-phase grid, one call at a time, and the oracle through the same actions
  (with the Logging bookkeeping of oracle/logging_oracle.py): computed once per case, never modified."""
  key = (bu.case_id(family, kwargs), T)
  if key not in _TWINS:
    g = bu.mixed_grid(family, kwargs)
    acts = bu.episode_actions(g, T)
    twin = _make(family, kwargs, g['lanes'])
    bu.load(twin, g)
    acts_t = _cuda(acts)
    snaps = [_snap_ts(twin.step(acts_t[t])) for t in range(T)]
    orc = bu.make_oracle(g)
    trk = logging_oracle.TrackOracle(g['lanes'], list(orc.bsuite_info()))
    st, r, obs, words = [], [], [], g['state']
    for t in range(T):
      s, rew, _, o = orc.call(bu.oracle_actions(g, acts[t]), bu.STEP0 + t)
      trk.track(s, rew, orc.bsuite_info())
      words = bu.oracle_words(g, orc, words, s, o)
      st.append(s.copy())
      r.append(rew.copy())
      obs.append(o.copy())
    _TWINS[key] = dict(ts=_stack(snaps, T), after=_snap_after(twin), actions=acts_t, orc=orc, trk=trk, st=np.stack(st), r=np.stack(r),
                       obs=np.stack(obs), words=words)
  return _TWINS[key]


@pytest.mark.parametrize('logged', [False, True], ids=['lean', 'Logging'])
@pytest.mark.parametrize('family,kwargs', [pytest.param(*c, id=bu.case_id(*c)) for c in bu.EPISODE_CASES])
def test_several_episodes_inside_one_call(family, kwargs, logged):
  """ONE rollout(40) from mixed phases — on every step of the loop half of the lanes reset and the others end an episode, 20
  episodes per lane (tests/test_bandit_edges_host.py asserts that on the reference): bandit's register-resident rollout
  carries each lane's regret through 20 additions at alternating iterations, mnist's kernel pair sees both phases in every
  block of every step; and the same under Logging."""
  T = bu.EPISODE_T
  g, w = bu.mixed_grid(family, kwargs), _episode_twin(family, kwargs, T)
  B = g['lanes']
  assert ((w['st'] == 2).sum(axis=0) == T // 2).all() and ((w['st'] == 2).sum(axis=1) > 0).all() and ((w['st'] == 0).sum(axis=1) > 0).all()
  env = _make(family, kwargs, B)
  if logged:
    env = wrappers.Logging(env, None, max_rows=32)
  bu.load(env, g)
  ts = env.rollout(w['actions'])
  got = _snap_ts(ts)
  what = (family, T, 'Logging' if logged else 'lean')
  _assert_ts(got, w['ts'], what)
  after = _snap_after(env)
  _assert_after(after, w['after'], what)
  # ... and the oracle: step types, rewards (its returns), observations, the state it ends in, the regret, the counters
  st = ts.step_type.cpu().numpy()
  np.testing.assert_array_equal(st, w['st'])
  live = w['st'] != 0
  reward = ts.reward.cpu().numpy()
  np.testing.assert_array_equal(eu.f32_bits(reward[live]), eu.f32_bits(w['r'][live].astype(np.float32)))
  assert (reward[~live] == 0).all()
  np.testing.assert_array_equal(eu.f32_bits(ts.observation.cpu().numpy()), eu.f32_bits(w['obs']))
  _assert_holds_the_oracle(after, w['orc'], w['words'], what)
  assert after['counters'].tolist() == [int((w['st'] == 2).sum()), int((w['st'] == 0).sum())]
  assert after['step_index'] == bu.STEP0 + T and _invalid(env) == 0
  if logged:
    trk, c = w['trk'], env.counters(check=True)
    for k in ('steps', 'episode', 'total_return'):
      np.testing.assert_array_equal(c[k].cpu().numpy(), getattr(trk, k), err_msg=f'{what} {k}')
    np.testing.assert_array_equal(env.num_rows().cpu().numpy(), [len(r) for r in trk.rows])
