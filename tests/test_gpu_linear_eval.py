"""GPU: evaluate_linear — the closed loop of a linear agent on cartpole, swing-up and mountain_car in one launch, returns
only.  A twin environment of the same seed and lane offset runs the contract's eager loop — `a = 0 where the lane resets,
else utils.observations.linear_select(weights[row], obs)` (ε draws restated from oracle/stream.py), `step(a)` — and
everything is compared bit for bit: `episodes` against the count of LAST in the twin, the two float64 sums against the
contract's loop over f64 rewards that never come from the engine's float32 column (cartpole 0 / 1 and mountain_car -1
are exact when widened; swing-up's are rebuilt as -|a - 1| * move_cost, plus 1.0 where the float32 reward exceeds 0.5),
`ev.observation` against the twin's last observation, state, bsuite_info, counters, the call index, and one further step."""
import numpy as np
import pytest
import torch

from bsuite_amd import _native
from bsuite_amd.utils import observations
from oracle import stream
from tests import engine_util as eu
from tests import policy_eval_util as pe

pytestmark = pytest.mark.gpu

OFFSET = (1 << 32) - 17                       # the global lane ids cross 2^32 inside the first workgroup
SEED = 11
STREAM_POLICY = 2                             # BSX_STREAM_POLICY (include/bsx_stream.h)
RESET_BIT = 1 << 30
# episodes that run past the call (defaults), time out inside it, and time tables too long for any LDS staging (> 4095)
LONG = [('cartpole', {}), ('cartpole_swingup', {}), ('mountain_car', {})]
SHORT = [('cartpole', dict(max_time=0.05)), ('cartpole_swingup', dict(max_time=0.05)), ('mountain_car', dict(max_steps=5))]
HUGE = [('cartpole', dict(max_time=50.)), ('cartpole_swingup', dict(max_time=50.)), ('mountain_car', dict(max_steps=5000))]
ids = lambda cases: [f + ('_' + '_'.join(f'{k}{v}' for k, v in kw.items()) if kw else '') for f, kw in cases]


def _make(fam, kwargs, B):
  return eu.make_env(fam, dict(kwargs), batch=B, lane_offset=OFFSET, seed=SEED)


def _dim(env):
  return int(np.prod(env.observation_spec().shape))


def _bits(t):
  return t.contiguous().view(torch.int64 if t.dtype is torch.float64 else torch.int32) if t.is_floating_point() else t


def _weights(fam, seed, P=None):
  """Weights under which all three actions occur: l_0 = -k s, l_1 = a bias, l_2 = +k s for a signed feature s that differs
  from lane to lane and from step to step (cartpole: sin(theta) + theta_dot; mountain_car: position + 0.5), plus small
  random terms everywhere — and, for a population, a different random part per row."""
  D = dict(cartpole=6, cartpole_swingup=8, mountain_car=3)[fam]
  g = torch.Generator(device='cpu')
  g.manual_seed(seed)
  n = 1 if P is None else P
  w = torch.randn((n, 3, D + 1), generator=g) * 0.05
  k = 20.0 * (1.0 + 0.5 * torch.rand((n,), generator=g))
  if fam == 'mountain_car':
    w[:, 0, 0] -= k; w[:, 2, 0] += k
    w[:, 0, D] -= 0.5 * k; w[:, 2, D] += 0.5 * k
    w[:, 0, 1] -= 200.0; w[:, 2, 1] += 200.0
  else:
    w[:, 0, 2] -= k; w[:, 2, 2] += k
    w[:, 0, 4] -= 0.3 * k; w[:, 2, 4] += 0.3 * k
  w[:, 1, D] += 0.4
  w = w.to(torch.float32).cuda().contiguous()
  return w[0].contiguous() if P is None else w


def _f64_rewards(fam, env, st, r32, acts):
  """The exact f64 reward of every step from what the twin reported (never the engine's f64)."""
  if fam != 'cartpole_swingup':
    assert set(np.unique(r32[st != 0]).tolist()) <= ({0.0, 1.0} if fam == 'cartpole' else {-1.0})
    return r32.astype(np.float64)
  r = -1.0 * np.abs((acts - 1).astype(np.float64)) * float(env._move_cost)     # pylint: disable=protected-access
  return np.where(r32 > 0.5, r + 1.0, r)


class Twin:
  """The eager loop of the contract on an environment of its own."""

  def __init__(self, fam, kwargs, B):
    self.fam, self.env, self.B = fam, _make(fam, kwargs, B), B
    self.lanes = np.uint64(OFFSET) + np.arange(B, dtype=np.uint64)
    self.obs = torch.zeros((B, 1, _dim(self.env)), dtype=torch.float32, device='cuda')
    self.seen = set()

  def run(self, weights, T, policy_index=None, epsilon=0.0, explore_seed=0):
    env = self.env
    if weights.dim() == 3:                                               # (a population of one takes no policy_index)
      rows = torch.zeros(self.B, dtype=torch.int32, device='cuda') if policy_index is None else policy_index
      weights = weights[rows.clamp(0, weights.shape[0] - 1).long()]
    st, r32, acts = [], [], []
    for _ in range(T):
      if not env._allocated:                                             # pylint: disable=protected-access
        resets = torch.ones(self.B, dtype=torch.bool, device='cuda')     # a fresh environment: every lane begins an episode
      else:
        resets = (env._state['steps'] & RESET_BIT) != 0                  # pylint: disable=protected-access
      a = observations.linear_select(weights, self.obs)
      if epsilon > 0.0:
        w = stream.words(int(explore_seed), self.lanes, env.step_index, STREAM_POLICY, 3).astype(np.uint64)
        u = stream.k53(w[:, 0], w[:, 1]).astype(np.float64) * 2.0 ** -53
        rand = ((w[:, 2] * np.uint64(3)) >> np.uint64(32)).astype(np.int32)
        a = torch.where(torch.from_numpy(u < epsilon).cuda(), torch.from_numpy(rand).cuda(), a)
      a = torch.where(resets, torch.zeros_like(a), a).contiguous()
      self.seen |= set(a[~resets].unique().tolist())
      ts = env.step(a)
      st.append(ts.step_type.cpu().numpy()); r32.append(ts.reward.cpu().numpy()); acts.append(a.cpu().numpy())
      assert bool((ts.step_type[resets] == 0).all()) and bool((ts.step_type[~resets] != 0).all())
      self.obs = ts.observation.clone()
    st, r32, acts = np.stack(st), np.stack(r32), np.stack(acts)
    return st, _f64_rewards(self.fam, env, st, r32, acts)


def _same(env, twin, what):
  ref = twin.env
  for k, v in ref._state.items():                                        # pylint: disable=protected-access
    assert torch.equal(_bits(env._state[k]), _bits(v)), (what, k)        # pylint: disable=protected-access
  assert torch.equal(_bits(env._info), _bits(ref._info)), what           # pylint: disable=protected-access
  for k, v in ref.bsuite_info().items():
    assert torch.equal(_bits(env.bsuite_info()[k]), _bits(v)), (what, k)
  assert torch.equal(env.episode_counters(), ref.episode_counters()), what
  assert env.step_index == ref.step_index, what


def _check(env, twin, weights, obs, T, what, **kw):
  """One evaluate_linear call against the twin's eager loop of the same arguments; returns the result."""
  st, r64 = twin.run(weights, T, **kw)
  ev = env.evaluate_linear(weights, obs, T, **kw)
  want = pe.host_loop(st, r64)
  np.testing.assert_array_equal(want[0], (st == 2).sum(axis=0))
  assert ev.episodes.dtype is torch.int32 and ev.return_sum.dtype is torch.float64 and ev.episode_return_sum.dtype is torch.float64
  assert ev.observation.dtype is torch.float32 and tuple(ev.observation.shape) == tuple(twin.obs.shape)
  np.testing.assert_array_equal(ev.episodes.cpu().numpy(), want[0], err_msg=f'{what} episodes')
  np.testing.assert_array_equal(pe.bits(ev.return_sum.cpu().numpy()), pe.bits(want[1]), err_msg=f'{what} return_sum')
  np.testing.assert_array_equal(pe.bits(ev.episode_return_sum.cpu().numpy()), pe.bits(want[2]), err_msg=f'{what} episode_return_sum')
  assert torch.equal(_bits(ev.observation), _bits(twin.obs)), (what, 'observation')
  _same(env, twin, what)
  return ev, st


def _one_more_step(env, twin, what):
  a = torch.arange(twin.B, device='cuda', dtype=torch.int32) % 3
  x, y = env.step(a), twin.env.step(a)
  for f in ('step_type', 'reward', 'discount', 'observation'):
    assert torch.equal(_bits(getattr(x, f)), _bits(getattr(y, f))), (what, f)
  _same(env, twin, what)
  twin.obs = y.observation.clone()
  return x.observation.clone()


def _garbage(env, B):
  return torch.full((B, 1, _dim(env)), float('nan'), dtype=torch.float32, device='cuda')


# ---------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize('B', [1, 64, 257])
@pytest.mark.parametrize('T', [1, 7, 40])
@pytest.mark.parametrize('fam,kwargs', LONG[:1] + SHORT, ids=ids(LONG[:1] + SHORT))
def test_equals_the_eager_loop_of_a_twin(fam, kwargs, T, B):
  env, twin = _make(fam, kwargs, B), Twin(fam, kwargs, B)
  w = _weights(fam, 3)
  # a fresh environment: every lane resets on the first step and its observation row is not read — garbage
  ev, st = _check(env, twin, w, _garbage(env, B), T, (fam, T, B, 'fresh'))
  assert (st[0] == 0).all()
  # ... then in the middle of its episodes, the returned observation passed back in (the same buffer)
  ev, st2 = _check(env, twin, w, ev.observation, T, (fam, T, B, 'running'))
  if B >= 64 and T >= 7:
    assert twin.seen == {0, 1, 2}, twin.seen                            # not a constant policy
  if kwargs and T >= 7:
    assert (np.concatenate([st, st2]) == 2).sum() >= B                   # episodes end inside the calls
  obs = _one_more_step(env, twin, (fam, T, B, 'one more step'))
  ev = _check(env, twin, w, obs.reshape(B, -1), T, (fam, T, B, 'after a step, [B, D] rows'))[0]
  # populations: P = 3 with rows named outside [0, P-1], exploring; P = B
  g = torch.Generator(device='cuda')
  g.manual_seed(B + T)
  pop = _weights(fam, 5, P=3)
  pidx = torch.randint(-1, 8, (B,), generator=g, device='cuda', dtype=torch.int32)
  pidx[0], pidx[-1] = 7, -1
  ev = _check(env, twin, pop, ev.observation, T, (fam, T, B, 'population'), policy_index=pidx)[0]
  ev = _check(env, twin, pop, ev.observation, T, (fam, T, B, 'population exploring'), policy_index=pidx, epsilon=0.3,
              explore_seed=(1 << 45) + 9)[0]
  each = _weights(fam, 6, P=B)
  lanes = torch.arange(B, device='cuda', dtype=torch.int32) if B > 1 else None      # (P == 1: policy_index must be None)
  _check(env, twin, each, ev.observation, T, (fam, T, B, 'one matrix per lane'), policy_index=lanes)
  _one_more_step(env, twin, (fam, T, B, 'last step'))
  assert int(env.episode_counters()[1]) >= B


@pytest.mark.parametrize('fam,kwargs', LONG + SHORT, ids=ids(LONG + SHORT))
def test_split_calls_exploration_and_mark_reset(fam, kwargs):
  B = 257
  env, twin = _make(fam, kwargs, B), Twin(fam, kwargs, B)
  w = _weights(fam, 8)
  # 3 + 4 steps are the 7 steps of one call: the same twin loop, the sums taken per call
  ev = _check(env, twin, w, _garbage(env, B), 3, (fam, 'first 3'))[0]
  ev = _check(env, twin, w, ev.observation, 4, (fam, 'then 4'))[0]
  whole, twin7 = _make(fam, kwargs, B), Twin(fam, kwargs, B)
  _check(whole, twin7, w, _garbage(whole, B), 7, (fam, 'whole 7'))
  _same(env, twin7, (fam, '3 + 4 == 7'))
  assert torch.equal(_bits(ev.observation), _bits(twin7.obs))
  # exploration: two seeds, ε in {0.3, 1.0}; ε = 0 draws nothing, whatever the seed
  for eps in (0.3, 1.0):
    for seed in (77, (1 << 63) + 5):
      ev = _check(env, twin, w, ev.observation, 7, (fam, 'eps', eps, seed), epsilon=eps, explore_seed=seed)[0]
  ev = _check(env, twin, w, ev.observation, 7, (fam, 'eps 0 with a seed'), epsilon=0.0, explore_seed=123)[0]
  assert twin.seen == {0, 1, 2}
  # mark_reset of some lanes between two calls: they begin an episode on the first step and do not read their rows
  g = torch.Generator(device='cuda')
  g.manual_seed(4)
  mask = torch.rand(B, generator=g, device='cuda') < 0.3
  env.mark_reset(mask)
  twin.env.mark_reset(mask)
  obs = ev.observation.clone()
  obs[mask] = float('nan')
  ev, st = _check(env, twin, w, obs, 7, (fam, 'after mark_reset'))
  assert (st[0][mask.cpu().numpy()] == 0).all()
  _one_more_step(env, twin, (fam, 'one more step'))
  # interleaved with rollout(): its last observation is the next call's input
  acts = torch.randint(3, (5, B), generator=g, device='cuda', dtype=torch.int32)
  ro, rt = env.rollout(acts), twin.env.rollout(acts)
  twin.obs = rt.observation[-1].clone()
  ev2 = _check(env, twin, w, ro.observation[-1], 7, (fam, 'after rollout'))[0]
  assert ev2.observation.data_ptr() == ev.observation.data_ptr() and ev2.episodes.data_ptr() == ev.episodes.data_ptr()     # cached buffers


@pytest.mark.parametrize('fam,kwargs', HUGE, ids=ids(HUGE))
def test_time_tables_beyond_4095_steps(fam, kwargs):
  B, T = 257, 3
  env, twin = _make(fam, kwargs, B), Twin(fam, kwargs, B)
  last = env._cfg.max_steps if fam == 'mountain_car' else env._cfg.last_step     # pylint: disable=protected-access
  assert last > 4095
  w = _weights(fam, 9)
  ev = _check(env, twin, w, _garbage(env, B), T, (fam, 'fresh'))[0]
  _check(env, twin, w, ev.observation, T, (fam, 'running'), epsilon=0.3, explore_seed=5)
  _one_more_step(env, twin, (fam, 'one more step'))


# ---------------------------------------------------------------------------------------------- 2. what paid for the kernel
@pytest.mark.parametrize('nontemporal', [0, 1])
def test_the_calibration_fill_writes_the_same_bytes(nontemporal):
  """bsx_calib_fill(nontemporal = 1) is a mode of calib_copy_n_kernel now: zeros over exactly n_bytes, whichever the flag."""
  n16 = 257 * 3 + 1                                                     # a partial last workgroup
  buf = torch.full((n16 * 4 + 8,), 7.0, dtype=torch.float32, device='cuda')
  st = torch.cuda.current_stream().cuda_stream
  assert _native.lib.bsx_calib_fill(buf.data_ptr(), n16 * 16, nontemporal, st) == 0
  torch.cuda.synchronize()
  assert bool((buf[:n16 * 4] == 0).all()) and bool((buf[n16 * 4:] == 7.0).all())
  # ... and bsx_calib_copy's one-store and three-store mixes, which share that kernel, copy as before
  src = torch.arange(n16 * 4, dtype=torch.float32, device='cuda')
  for writes in (1, 3):
    dst = torch.full((writes * n16 * 4 + 8,), -1.0, dtype=torch.float32, device='cuda')
    assert _native.lib.bsx_calib_copy(dst.data_ptr(), src.data_ptr(), n16 * 16, writes, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst[:writes * n16 * 4], src.repeat(writes)) and bool((dst[writes * n16 * 4:] == -1.0).all())
