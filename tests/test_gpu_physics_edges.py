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
     resets inside the fused loop at step 2): int32 bit patterns, no tolerance, every row.
"""
import numpy as np
import pytest
import torch

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
  return obs, [('rollout_linear', 'evaluate_linear', (w,), {}), ('rollout_mlp', 'evaluate_mlp', (w1, w2), {}),
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
