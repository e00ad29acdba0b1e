"""GPU: the physics kernels on the edge-state grid of tests/physics_edge_util.py, across every launch path.

Every closed-loop call (rollout, evaluate_*, rollout_*, sample_*, evaluate_sampled_*) compiles its own copy of
cartpole_env::core / mountain_car_env::core, and the eager step has a lean, a run-time (Logging, RewardNoise, mt19937)
and — mountain_car — a two-lanes-per-thread form.  All are promised to equal the eager step() bit for bit, and the eager
step to stay within 1e-6*max(1,|b|) of the float64 reference.  Natural trajectories never reach the branches the grid is
made of (tests/test_physics_edges_host.py proves the grid reaches each on at least a wave of lanes):

  A. one eager step() from the loaded grid against oracle/coracle.OracleEnv with engine_util.PhysicsChecker as it stands
     (plus the wall rule of physics_edge_util for mountain_car).  The rows with |theta_dot| > 50 — states only
     load_state_dict reaches — are held to max(1e-6, 2 x the error measured on the MI355X) per family and theta_dot band,
     which is 1e-6 everywhere (MEASURED below; profiles/physics_edges/README.md has the measurement per component);
  B. every other path against the eager step from the same loaded state, T = 1 and T = 3 (a lane that ends at step 1
     resets inside the fused loop at step 2): int32 bit patterns, no tolerance, every row.  Among them the per-lane reset
     (step(reset_mask=) / mark_reset(): unmarked lanes against the eager step, marked lanes against the reference's reset),
     the device-resident call counter, and the grouped launches of a SweepBatch (the duo / small_mixed group kernels, the
     sweep's phase 0, its split cut and the pipelined kernel) against stand-alone environments loaded with the same rows.
"""
import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import sweep
from bsuite_amd import sweep_batch as sb
from bsuite_amd.utils import wrappers
from tests import edge_snap_util as es
from tests import engine_util as eu
from tests import physics_edge_util as pu
from tests import policy_eval_util as pe

pytestmark = pytest.mark.gpu

CASES = list(zip(pu.CASES, pu.CASE_IDS))
CASE_PARAMS = [pytest.param(f, kw, id=i) for (f, kw), i in CASES]
T_MAX = 3
_bits, _snap_ts, _snap_after, _stack, _assert_ts, _assert_after = es.bits, es.snap_ts, es.snap_after, es.stack, es.assert_ts, es.assert_after

# Measured on the MI355X by test_eager_step_against_the_oracle itself (it prints the table per component):
# max |a-b| / max(1,|b|) over the continuous observation components of the rows of each theta_dot band (bands 1..3 of
# physics_edge_util.theta_dot_band; band 0 and mountain_car are held to the contract, 1e-6, as it stands).  The bound
# asserted on band b is max(1e-6, 2 x MEASURED[family][b]): the arithmetic is deterministic, the factor 2 leaves room
# for another schedule of the non-contracted operations.  Every one of them comes to 1e-6, so the test holds the whole
# grid to the contract with engine_util.PhysicsChecker; a band that measured above 5e-7 would need a checker of its own.
MEASURED = {
    'cartpole': {1: 2.384e-07, 2: 2.384e-07, 3: 3.427e-07},
    'cartpole_swingup': {1: 2.384e-07, 2: 2.384e-07, 3: 3.427e-07},
}
CONTINUOUS = dict(cartpole=('x', 'x_dot', 'sin', 'cos', 'theta_dot', 'time'),
                  cartpole_swingup=('x', 'x_dot', 'sin', 'cos', 'theta_dot', 'time'),
                  mountain_car=('position', 'velocity', 'time'))


def band_bound(family, band):
  if band == 0 or family == 'mountain_car':
    return eu.PHYS_TOL
  return max(eu.PHYS_TOL, 2.0 * MEASURED[family][band])


def _make(family, kwargs, batch, **engine_kwargs):
  return eu.make_env(family, dict(kwargs), batch=batch, lane_offset=pu.LANE_OFFSET, seed=pu.SEED, **engine_kwargs)


def _actions(g, T):
  """int32 [T, B] on the device: the grid's action first, seeded random ones after it."""
  rng = np.random.default_rng(31)
  a = np.concatenate([g['action'][None], rng.integers(0, 3, size=(T - 1, g['lanes'])).astype(np.int32)])
  return torch.from_numpy(a).cuda()


_EAGER = {}


def eager(family, kwargs):
  """The eager lean step() from the loaded grid, T_MAX times with _actions: per step the TimeStep and what the
  environment holds afterwards, as bit patterns on the device.  Computed once per case and shared, never modified."""
  key = (family, tuple(sorted(kwargs.items())))
  if key not in _EAGER:
    g = pu.grid(family, kwargs)
    env = _make(family, kwargs, g['lanes'])
    pu.load(env, g)
    assert env.step_index == pu.STEP0
    if family != 'mountain_car':
      assert env._last_step == g['last_step']                                    # pylint: disable=protected-access
    acts = _actions(g, T_MAX)
    ts, after = [], []
    for t in range(T_MAX):
      ts.append(_snap_ts(env.step(acts[t])))
      after.append(_snap_after(env))
    _EAGER[key] = dict(ts=ts, after=after, actions=acts)
  return _EAGER[key]


# ------------------------------------------------------------------------------------- A. the eager step and the reference
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_eager_step_against_the_oracle(family, kwargs):
  g = pu.grid(family, kwargs)
  B = g['lanes']
  e = eager(family, kwargs)
  ts, after = e['ts'][0], e['after'][0]
  got = (ts['step_type'].cpu().numpy(), ts['reward'].view(torch.float32).cpu().numpy(), ts['discount'].view(torch.float32).cpu().numpy(),
         ts['observation'].view(torch.float32).cpu().numpy().reshape(B, -1))
  orc, want = pu.oracle_step(g)
  want = want[:3] + (want[3].reshape(B, -1),)
  state = eu.oracle_physics_state(orc, family)
  band = pu.theta_dot_band(g)
  # the measurement: per band and continuous component, printed before anything is asserted
  names = CONTINUOUS[family]
  err = np.abs(got[3].astype(np.float64) - want[3]) / np.maximum(1.0, np.abs(want[3].astype(np.float64)))
  for b in sorted(set(band.tolist())):
    rows = band == b
    cells = ' | '.join(f'{err[rows, j].max():.3e}' for j in range(len(names)))
    print(f'| {family} | {pu.BAND_NAMES[b]} | {int(rows.sum())} | {cells} | {err[rows][:, :len(names)].max():.3e} |')
  want_obs, walled = pu.apply_wall_rule(g, got[3], want[3])
  want = want[:3] + (want_obs,)
  waived = walled.copy()
  # every band's bound is the project's contract (band_bound): PhysicsChecker as it stands, on the whole grid
  assert all(band_bound(family, b) == eu.PHYS_TOL for b in set(band.tolist()))
  chk = eu.PhysicsChecker(family, g['kwargs'], B)
  chk.check(got, want, state, msg=family)
  assert chk.max_err['observation'] <= eu.PHYS_TOL
  waived |= chk.tainted
  print(f'{family} {kwargs}: waived {int(waived.sum())} of {B} lanes ({int(walled.sum())} by the wall rule)')
  assert int(waived.sum()) <= pu.MAX_WAIVED * B
  # bsuite_info exact on the lanes that never tied; the LAST counter is the reference's count
  for k, v in orc.bsuite_info().items():
    np.testing.assert_array_equal(after['info'][k].view(torch.float64).cpu().numpy()[~waived], v[~waived], err_msg=k)
  counters = after['counters'].cpu().numpy()
  assert counters[0] == int((np.where(waived, got[0], want[0]) == 2).sum()) and counters[1] == 0
  assert counters[0] == int((got[0] == 2).sum())


# ------------------------------------------------------------------------------------- B. every path equals the eager step
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_rollout_equals_eager_steps(family, kwargs, T):
  g, e = pu.grid(family, kwargs), eager(family, kwargs)
  env = _make(family, kwargs, g['lanes'])
  pu.load(env, g)
  ro = env.rollout(e['actions'][:T].contiguous())
  _assert_ts(_snap_ts(ro), _stack(e['ts'], T), (family, T, 'rollout'))
  _assert_after(_snap_after(env), e['after'][T - 1], (family, T, 'rollout'))
  if T > 1:
    assert bool((e['ts'][1]['step_type'] == 0).any()) and bool((e['ts'][2]['step_type'] == 0).any())      # resets inside the loop


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_logging_paths_equal_the_eager_step(family, kwargs, T):
  g, e = pu.grid(family, kwargs), eager(family, kwargs)
  for path in ('step', 'rollout'):
    env = wrappers.Logging(_make(family, kwargs, g['lanes']), None, max_rows=8)
    pu.load(env, g)
    if path == 'step':
      got = _stack([_snap_ts(env.step(e['actions'][t])) for t in range(T)], T)
    else:
      got = _snap_ts(env.rollout(e['actions'][:T].contiguous()))
    _assert_ts(got, _stack(e['ts'], T), (family, T, 'Logging', path))
    _assert_after(_snap_after(env), e['after'][T - 1], (family, T, 'Logging', path))


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_reward_noise_paths_equal_the_eager_step(family, kwargs, T):
  """The reward is the base reward plus noise: not compared (and bsuite_info, which sums it, neither)."""
  g, e = pu.grid(family, kwargs), eager(family, kwargs)
  fields = ('step_type', 'discount', 'observation')
  for path in ('step', 'rollout'):
    env = wrappers.RewardNoise(_make(family, kwargs, g['lanes']), noise_scale=0.1, seed=3)
    pu.load(env, g)
    if path == 'step':
      got = _stack([_snap_ts(env.step(e['actions'][t])) for t in range(T)], T)
    else:
      got = _snap_ts(env.rollout(e['actions'][:T].contiguous()))
    _assert_ts(got, _stack(e['ts'], T), (family, T, 'RewardNoise', path), fields=fields)
    _assert_after(_snap_after(env), e['after'][T - 1], (family, T, 'RewardNoise', path), info=False)
    noisy = got['reward'].view(torch.float32)[0] != e['ts'][0]['reward'].view(torch.float32)
    assert float(noisy.float().mean()) > 0.99                                   # the wrapper was in the kernel


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_mt19937_step_equals_the_eager_step(family, kwargs):
  """T = 1 only: resets draw from another stream there, and no row of the grid resets at step 0.  The generators are
  seeded on the host lane by lane, so a large grid is loaded by every MT_STRIDE-th row (physics_edge_util.mt_rows: the
  host test holds every branch predicate to a full wave among them, too)."""
  g, e = pu.grid(family, kwargs), eager(family, kwargs)
  rows = pu.mt_rows(g)
  env = _make(family, kwargs, len(rows), rng='mt19937')
  pu.load(env, g, rows)
  rows_t = torch.from_numpy(rows).cuda()
  got = _snap_ts(env.step(e['actions'][0][rows_t].contiguous()))
  _assert_ts(got, e['ts'][0], (family, 'mt19937'), rows=rows_t)
  after = _snap_after(env)
  _assert_after(after, e['after'][0], (family, 'mt19937'), rows=rows_t)
  assert after['counters'].tolist() == [int((e['ts'][0]['step_type'][rows_t] == 2).sum()), 0]


def _f64_rewards(family, env, st, r32, acts):
  """The exact f64 reward of every step from what the recording call reported (never the engine's f64): cartpole 0 / 1
  and mountain_car -1 are exact when widened; swing-up's are -|a - 1| * move_cost, plus 1.0 where upright."""
  if family != 'cartpole_swingup':
    assert set(np.unique(r32[st != 0]).tolist()) <= ({0.0, 1.0} if family == 'cartpole' else {-1.0})
    return r32.astype(np.float64)
  r = -1.0 * np.abs((acts - 1).astype(np.float64)) * float(env._move_cost)     # pylint: disable=protected-access
  return np.where(r32 > 0.5, r + 1.0, r)


def _policies(family, B):
  """(name, recording call, evaluating call, arguments, keywords) with seeded random weights, and the seeded random
  observation rows the first action is taken from (the contract reads whatever row is passed).  The generator's seed is
  one under which both greedy policies take each action on at least 9 % of such rows, for every family."""
  D = dict(cartpole=6, cartpole_swingup=8, mountain_car=3)[family]
  H = 5
  gen = torch.Generator(device='cpu')
  gen.manual_seed(31)
  w = torch.randn((3, D + 1), generator=gen).cuda().contiguous()
  w1 = torch.randn((H, D + 1), generator=gen).cuda().contiguous()
  w2 = torch.randn((3, H + 1), generator=gen).cuda().contiguous()
  obs = torch.randn((B, 1, D), generator=gen).cuda().contiguous()
  draw = dict(temperature=1.0, sample_seed=(1 << 40) + 77)
  # the two-hidden-layer triple from a generator of its own (the draws above stay what they were).  Under seed 31 it leaves an
  # action out in every family (cartpole 2 %, swing-up 0.1 %, mountain_car 5 %); 884 was chosen on the CPU with the host
  # restatement of tests/test_mlp2_host.py (_restate) over seeds 1..1499: every action on at least 8 % of the rows, every family
  gen2 = torch.Generator(device='cpu')
  gen2.manual_seed(884)
  H1, H2 = 5, 4
  v1 = torch.randn((H1, D + 1), generator=gen2).cuda().contiguous()
  v2 = torch.randn((H2, H1 + 1), generator=gen2).cuda().contiguous()
  v3 = torch.randn((3, H2 + 1), generator=gen2).cuda().contiguous()
  return obs, [('rollout_linear', 'evaluate_linear', (w,), {}), ('rollout_mlp', 'evaluate_mlp', (w1, w2), {}),
               ('rollout_mlp2', 'evaluate_mlp2', (v1, v2, v3), {}),
               ('sample_linear', 'evaluate_sampled_linear', (w,), draw), ('sample_mlp', 'evaluate_sampled_mlp', (w1, w2), draw)]


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_closed_loop_calls_equal_the_eager_step(family, kwargs, T):
  g = pu.grid(family, kwargs)
  B = g['lanes']
  obs, policies = _policies(family, B)
  for record, evaluate, weights, kw in policies:
    what = (family, T, record)
    env = _make(family, kwargs, B)
    pu.load(env, g)
    ts, actions = getattr(env, record)(*weights, obs, T, **kw)
    assert set(actions[0].unique().tolist()) == {0, 1, 2}, what
    # the returned actions replayed through the eager step() of a twin loaded with the same state
    twin = _make(family, kwargs, B)
    pu.load(twin, g)
    want = _stack([_snap_ts(twin.step(actions[t].contiguous())) for t in range(T)], T)
    _assert_ts(_snap_ts(ts), want, what)
    want_after = _snap_after(twin)
    _assert_after(_snap_after(env), want_after, what)
    # the returns-only call with the same arguments: the same final state, the columns of the host loop over `ts`
    what = (family, T, evaluate)
    env2 = _make(family, kwargs, B)
    pu.load(env2, g)
    ev = getattr(env2, evaluate)(*weights, obs, T, **kw)
    _assert_after(_snap_after(env2), want_after, what)
    st = ts.step_type.cpu().numpy()
    r64 = _f64_rewards(family, env, st, ts.reward.cpu().numpy(), actions.cpu().numpy())
    n, total, done = pe.host_loop(st, r64)
    np.testing.assert_array_equal(ev.episodes.cpu().numpy(), n, err_msg=f'{what} episodes')
    np.testing.assert_array_equal(pe.bits(ev.return_sum.cpu().numpy()), pe.bits(total), err_msg=f'{what} return_sum')
    np.testing.assert_array_equal(pe.bits(ev.episode_return_sum.cpu().numpy()), pe.bits(done), err_msg=f'{what} episode_return_sum')
    assert torch.equal(_bits(ev.observation), _bits(ts.observation[-1])), (what, 'observation')


@pytest.mark.parametrize('family,kwargs', [p for p in CASE_PARAMS if p.values[0] == 'mountain_car'])
def test_two_lanes_per_thread_step_equals_the_small_batch(family, kwargs):
  """mountain_car's lean eager step handles two lanes per thread from 2048 workgroups up: the grid tiled to 2^19 + 257
  lanes, one step, every tile bit for bit the small-batch result of A."""
  g, e = pu.grid(family, kwargs), eager(family, kwargs)
  B = (1 << 19) + 257
  assert -(-B // pu.BLOCK) >= 2048
  rows = np.arange(B) % g['lanes']
  env = _make(family, kwargs, B)
  pu.load(env, g, rows)
  rows_t = torch.from_numpy(rows).cuda()
  got = _snap_ts(env.step(e['actions'][0][rows_t].contiguous()))
  _assert_ts(got, e['ts'][0], (family, 'two lanes per thread'), rows=rows_t)
  after = _snap_after(env)
  _assert_after(after, e['after'][0], (family, 'two lanes per thread'), rows=rows_t)
  assert after['counters'].tolist() == [int((e['ts'][0]['step_type'][rows_t] == 2).sum()), 0]


# ------------------------------------------------------------------------------------- per-lane resets, the device counter
@pytest.mark.timeout(300)
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_reset_mask_and_mark_reset_on_the_grid(family, kwargs):
  """A seeded third of the lanes is marked — lanes about to time out, to cross a threshold, at the wall among them.  The
  marked lanes give FIRST with the oracle's reset observation (PhysicsChecker as it stands: a marked lane has no threshold
  to tie on) and the info columns of the reference called with reset(); the unmarked lanes equal the eager run bit for bit,
  every one of them.  mark_reset() followed by the plain step is the same call."""
  g, e = pu.grid(family, kwargs), eager(family, kwargs)
  B = g['lanes']
  mask = np.random.default_rng(41).random(B) < 1.0 / 3.0
  mask_t, acts = torch.from_numpy(mask).cuda(), e['actions'][0]
  orc, want = pu.oracle_step(g, reset_mask=mask)
  assert (want[0][mask] == 0).all() and (want[0][~mask] != 0).all()
  pred = pu.predicates(g, *pu.oracle_step(g))
  for name in pu.PREDICATES[family]:
    assert (pred[name] & ~mask).sum() >= pu.MIN_LANES // 2 and (pred[name] & mask).sum() >= 8, name      # (held on the CPU, too)
  env = _make(family, kwargs, B)
  pu.load(env, g)
  ts = _snap_ts(env.step(acts, reset_mask=mask_t))
  after = _snap_after(env)
  # unmarked lanes: the eager step, bit for bit
  keep = ~mask_t
  want_ts, want_after = e['ts'][0], e['after'][0]
  for f in es.TS_FIELDS:
    assert torch.equal(ts[f][keep], want_ts[f][keep]), (family, 'reset_mask', f, 'unmarked lanes')
  for k, w in want_after['state'].items():
    assert torch.equal(after['state'][k][..., keep], w[..., keep]), (family, 'reset_mask', k, 'unmarked lanes')
  for k, w in want_after['info'].items():
    assert torch.equal(after['info'][k][keep], w[keep]), (family, 'reset_mask', k, 'unmarked lanes')
  # marked lanes: FIRST, reward 0, discount 1, the reference's reset observation within the contract
  got = (ts['step_type'].cpu().numpy(), ts['reward'].view(torch.float32).cpu().numpy(), ts['discount'].view(torch.float32).cpu().numpy(),
         ts['observation'].view(torch.float32).cpu().numpy().reshape(B, -1))
  assert (got[0][mask] == 0).all() and (got[1][mask] == 0).all() and (got[2][mask] == 1).all()
  n = int(mask.sum())
  state = {k: v[mask] for k, v in eu.oracle_physics_state(orc, family).items()}
  chk = eu.PhysicsChecker(family, g['kwargs'], n)
  chk.check(tuple(v[mask] for v in got), (want[0][mask], want[1][mask], want[2][mask], want[3].reshape(B, -1)[mask]), state,
            msg=f'{family} marked lanes')
  assert chk.max_err['observation'] <= eu.PHYS_TOL and not chk.tainted.any()
  for k, v in orc.bsuite_info().items():      # an abandoned episode keeps what it has earned and ends nothing
    np.testing.assert_array_equal(after['info'][k].view(torch.float64).cpu().numpy()[mask], v[mask], err_msg=f'{k} marked lanes')
  last = int((want_ts['step_type'][keep] == 2).sum())
  assert after['counters'].tolist() == [last, n] and after['step_index'] == pu.STEP0 + 1
  # mark_reset(), then the plain step: the same words, the same TimeStep
  env2 = _make(family, kwargs, B)
  pu.load(env2, g)
  loaded = env2._state['steps'].clone()                                         # pylint: disable=protected-access
  env2.mark_reset(mask_t.to(torch.uint8))
  assert torch.equal(env2._state['steps'], torch.where(mask_t, loaded | pu.RESET_BIT, loaded))      # pylint: disable=protected-access
  _assert_ts(_snap_ts(env2.step(acts)), ts, (family, 'mark_reset'))
  _assert_after(_snap_after(env2), after, (family, 'mark_reset'))


@pytest.mark.timeout(300)
@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_device_step_counter_paths_equal_the_eager_step(family, kwargs):
  g, e = pu.grid(family, kwargs), eager(family, kwargs)
  for path in ('step', 'rollout'):
    what = (family, 'device_step_counter', path)
    env = _make(family, kwargs, g['lanes'], device_step_counter=True)
    pu.load(env, g)
    if path == 'step':
      got = _stack([_snap_ts(env.step(e['actions'][t])) for t in range(T_MAX)], T_MAX)
    else:
      got = _snap_ts(env.rollout(e['actions'][:T_MAX].contiguous()))
    _assert_ts(got, _stack(e['ts'], T_MAX), what)
    assert eu.raw(env).device_step_index() == pu.STEP0 + T_MAX, what
    after = _snap_after(env)
    after['step_index'] = eu.raw(env).device_step_index()                       # (the device counter is the authority here)
    _assert_after(after, e['after'][T_MAX - 1], what)


# ------------------------------------------------------------------------------------- grouped launches
GROUPED_MODES = ['per_family', 'per_family_streams', 'small_mixed', 'small_mixed_streams', 'whole_sweep', 'whole_sweep_streams',
                 'whole_sweep_rows_in_stream', 'whole_sweep_split', 'whole_sweep_pipelined']


@pytest.mark.timeout(300)
@pytest.mark.parametrize('mode', GROUPED_MODES, ids=['grouped_' + m for m in GROUPED_MODES])
def test_grouped_launches_equal_standalone_envs(mode):
  """A SweepBatch of cartpole/0, cartpole_swingup/0 and mountain_car/0 with grid rows loaded into their segment environments
  before prepare_groups (each segment's own state_dict(), so its call index is kept), and catch/0 from its fresh reset so that
  the whole-sweep group has a store stream: three grouped steps against stand-alone environments loaded with the same rows,
  bit for bit on every row — the same kernels' cores, the same draws, identical even for f32 physics."""
  ids, reps = list(pu.GROUPED_IDS) + ['catch/0'], 3
  for bid, (family, kwargs) in pu.GROUPED_IDS.items():
    assert {k: v for k, v in sweep.SETTINGS[bid].items() if k != 'seed'} == kwargs, bid
  assert [c for c in pu.GROUPED_IDS.values() if c in pu.CASES] == [pu.CASES[0], pu.CASES[2]]      # the default-argument cases
  grids = [pu.grid(*c) for c in pu.GROUPED_IDS.values()]
  lanes = 16 * pu.BLOCK + 1
  batch = sb.SweepBatch(ids, len(ids) * lanes, seed=pu.SEED)
  acts, refs = [], []
  for k, ((bid, begin, n), env, g) in enumerate(zip(batch.segments, batch.envs, grids + [None])):
    assert n == lanes
    ref = bsuite_amd.load_from_id(bid, batch=n, lane_offset=begin, num_buffers=1, seed=pu.SEED)
    if g is None:                                  # catch/0: from its fresh reset
      acts.append(torch.ones(n, dtype=torch.int32, device='cuda'))
    else:
      # (the cartpole grids are larger than a segment: a wave of every branch predicate, then seeded random rows)
      rows = pu.segment_rows(g, n, 50 + k)
      pred = pu.predicates(g, *pu.oracle_step(g))
      for name in pu.PREDICATES[g['family']]:
        assert pred[name][rows].sum() >= pu.MIN_LANES, (bid, name)
      pu.load(env, g, rows, step0=None)
      pu.load(ref, g, rows, step0=None)
      acts.append(torch.from_numpy(np.array(g['action'][rows])).cuda())
    refs.append(ref)
  base_mode = mode.replace('_streams', '')
  whole = base_mode.startswith('whole_sweep')
  pipelined = base_mode == 'whole_sweep_pipelined'
  extra = dict(rows_in_stream=base_mode == 'whole_sweep_rows_in_stream', split=base_mode == 'whole_sweep_split') if whole else {}
  batch.prepare_groups(acts, mix_all=whole, mix_pairs=False, mix_small=base_mode == 'small_mixed', pipelined=pipelined, **extra)
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
