"""GPU: rollout_linear / rollout_mlp — the closed loop of a linear or hidden-layer agent on cartpole, swing-up and mountain_car
in one launch, writing the trajectory.  The twin method of tests/test_gpu_mlp_eval.py, whose helpers are imported: a second
environment of the same seed and lane offset runs the contract's eager loop and keeps every TimeStep it got; step_type,
reward, discount, observation and the actions are compared bit for bit, and so is everything left behind.  Further twins
replay the returned actions through rollout() and run evaluate_linear / evaluate_mlp with the same arguments.  And the kernel
that paid for the new one: bsx_bsuite_info and bsx_stream_dump are served by one merged kernel."""
import types

import numpy as np
import pytest
import torch

from bsuite_amd import _native
from bsuite_amd.environments import catch
from bsuite_amd.utils import observations
from oracle import stream
from tests.test_gpu_mlp_eval import (HIDDEN, HUGE, LONG, MAIN, OFFSET, SEED, SHORT, Twin, _bits, _garbage, _linear_weights, _make,
                                     _one_more_step, _pair, _rows, _same, case_id)

pytestmark = pytest.mark.gpu

FIELDS = ('step_type', 'reward', 'discount', 'observation')
KINDS = ['linear', 'mlp']
BATCHES, STEPS = [1, 257], [1, 9]
# one hidden width per (family, B, T), rotated; both kinds of policy meet every case
CASES = [pytest.param(kind, f, kw, T, B, HIDDEN[(fi + ti + bi) % 3], id=f'{kind}-{case_id(f, kw)}-T{T}-B{B}-H{HIDDEN[(fi + ti + bi) % 3]}')
         for kind in KINDS for fi, (f, kw) in enumerate(MAIN) for ti, T in enumerate(STEPS) for bi, B in enumerate(BATCHES)]


class Recorder(Twin):
  """The eager twin, keeping every TimeStep its environment returns and the action that led to it."""

  def __init__(self, fam, kwargs, B):
    super().__init__(fam, kwargs, B)
    self.kept = []
    step = self.env.step

    def keep(action, *args, **kw):
      ts = step(action, *args, **kw)
      self.kept.append(tuple(getattr(ts, f).clone() for f in FIELDS) + (action.clone(),))
      return ts
    self.env.step = keep

  def last(self, T):
    """The last T steps, stacked: (step_type, reward, discount, observation, actions), [T,B,...] each."""
    return tuple(torch.stack(col) for col in zip(*self.kept[-T:]))

  def select(self, kind, pol, policy_index):
    if kind == 'mlp':
      return self.select_mlp(pol[0], pol[1], policy_index)
    w = pol[0] if pol[0].dim() == 2 else _rows(pol[0], policy_index, self.B)
    return lambda obs, live: observations.linear_select(w, obs)


def _policy(kind, fam, H, seed, P=None):
  """The policy tensors of one call: (weights,) or (w1, w2); a population of P with a different random part per row."""
  if kind == 'mlp':
    w1, w2 = _pair(fam, H, seed, P=P, nan_unit=P is not None)
    if H == 1:
      # one unit alone sees one sign of the feature s: h = relu(k s) leaves action 0 or the other two.  A bias of 0.6 puts
      # h = relu(k s + 0.6) on both sides of l_1 = h > l_0 = 0.3 and of l_2 = 2 h - 1 > l_1, and s < -0.6 / k switches it off
      w1 = w1.clone()
      w1[..., 0, -1] += 0.6
    return w1, w2
  w = _linear_weights(fam, seed)
  if P is None:
    return (w,)
  g = torch.Generator(device='cpu')
  g.manual_seed(seed + 1)
  return ((w.cpu().unsqueeze(0) + 0.05 * torch.randn((P,) + tuple(w.shape), generator=g)).to(torch.float32).cuda().contiguous(),)


def _rollout(env, kind, pol, obs, T, **kw):
  return (env.rollout_mlp if kind == 'mlp' else env.rollout_linear)(*pol, obs, T, **kw)


def _evaluate(env, kind, pol, obs, T, **kw):
  return (env.evaluate_mlp if kind == 'mlp' else env.evaluate_linear)(*pol, obs, T, **kw)


def _equal_steps(ts, actions, want, what):
  B = want[0].shape[1]
  assert ts.step_type.dtype is torch.int8 and ts.reward.dtype is torch.float32 and ts.discount.dtype is torch.float32
  assert ts.observation.dtype is torch.float32 and actions.dtype is torch.int32
  assert tuple(ts.observation.shape) == tuple(want[3].shape) and tuple(actions.shape) == (want[0].shape[0], B)
  for f, w in zip(FIELDS, want):
    assert torch.equal(_bits(getattr(ts, f)), _bits(w)), (what, f)
  assert torch.equal(actions, want[4]), (what, 'actions')


def _check(env, twin, kind, pol, obs, T, what, policy_index=None, **kw):
  """One rollout_linear / rollout_mlp call against the twin's eager loop of the same arguments; returns (ts, actions)."""
  twin.run(twin.select(kind, pol, policy_index), T, **kw)
  ts, actions = _rollout(env, kind, pol, obs, T, policy_index=policy_index, **kw)
  _equal_steps(ts, actions, twin.last(T), what)
  _same(env, twin, what)
  return ts, actions


def _state_of(env):
  return types.SimpleNamespace(env=env)


# ---------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize('kind,fam,kwargs,T,B,H', CASES)
def test_equals_the_eager_loop_of_a_twin(kind, fam, kwargs, T, B, H):
  env, twin = _make(fam, kwargs, B), Recorder(fam, kwargs, B)
  pol = _policy(kind, fam, H, 3)
  # 1. a fresh environment: every lane resets on the first step and its observation row is not read — garbage
  ts, actions = _check(env, twin, kind, pol, _garbage(fam, B), T, (kind, fam, T, B, H, 'fresh'))
  assert bool((ts.step_type[0] == 0).all()) and bool((actions[0] == 0).all())
  n_last = int((ts.step_type == 2).sum())
  # 2. in the middle of its episodes, the last observation passed back in (a slice of the buffer the call overwrites)
  ts, actions = _check(env, twin, kind, pol, ts.observation[-1], T, (kind, fam, T, B, H, 'running'))
  n_last += int((ts.step_type == 2).sum())
  if B == 257 and T == 9:
    if kind == 'mlp':
      assert twin.positive and twin.negative                             # units switch on and off: not a linear policy
    assert twin.seen == {0, 1, 2}, twin.seen                             # not a constant policy
  if kwargs and T == 9:
    assert n_last >= B                                                   # episodes end inside the calls
  # 3. [B, D] rows after a step()
  obs = _one_more_step(env, twin, (kind, fam, T, B, H, 'one more step'))
  ts, _ = _check(env, twin, kind, pol, obs.reshape(B, -1), T, (kind, fam, T, B, H, 'after a step, [B, D] rows'))
  # 4. a population of three with rows named outside [0, P-1], exploring
  g = torch.Generator(device='cuda')
  g.manual_seed(B + T)
  pop = _policy(kind, fam, H, 5, P=3)
  pidx = torch.randint(-1, 8, (B,), generator=g, device='cuda', dtype=torch.int32)
  pidx[0], pidx[-1] = 7, -1
  ts, _ = _check(env, twin, kind, pop, ts.observation[-1], T, (kind, fam, T, B, H, 'population exploring'), policy_index=pidx,
                 epsilon=0.3, explore_seed=(1 << 45) + 9)
  # 5. one policy per lane
  each = _policy(kind, fam, H, 6, P=B)
  lanes = torch.arange(B, device='cuda', dtype=torch.int32) if B > 1 else None      # (P == 1: policy_index must be None)
  _check(env, twin, kind, each, ts.observation[-1], T, (kind, fam, T, B, H, 'one policy per lane'), policy_index=lanes)
  _one_more_step(env, twin, (kind, fam, T, B, H, 'last step'))
  assert int(env.episode_counters()[1]) >= B


# ---------------------------------------------------------------------------------------------- 2. / 3. replay and evaluate twins
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam,kwargs,H', [(f, kw, HIDDEN[k % 3]) for k, (f, kw) in enumerate(MAIN)], ids=[case_id(f, kw) for f, kw in MAIN])
def test_replayed_actions_and_the_evaluation_agree(kind, fam, kwargs, H):
  B, T = 257, 9
  env, replay, scored = _make(fam, kwargs, B), _make(fam, kwargs, B), _make(fam, kwargs, B)
  pol = _policy(kind, fam, H, 4)
  obs = _garbage(fam, B)
  for n, kw in enumerate((dict(), dict(epsilon=0.3, explore_seed=(1 << 63) + 1), dict())):
    obs_in = obs.clone()
    ts, actions = _rollout(env, kind, pol, obs, T, **kw)
    # a second twin's rollout(actions) reproduces ts, and the state
    again = replay.rollout(actions)
    for f in FIELDS:
      assert torch.equal(_bits(getattr(again, f)), _bits(getattr(ts, f))), (kind, fam, n, f)
    _same(env, _state_of(replay), (kind, fam, n, 'replay'))
    # a third twin's evaluation with the same arguments ends in the same state
    ev = _evaluate(scored, kind, pol, obs_in, T, **kw)
    _same(env, _state_of(scored), (kind, fam, n, 'evaluate'))
    assert torch.equal(_bits(ev.observation), _bits(ts.observation[-1])), (kind, fam, n)
    assert torch.equal(ev.episodes, (ts.step_type == 2).sum(0).to(torch.int32)), (kind, fam, n)
    obs = ts.observation[-1]
  if kwargs:
    assert int(env.episode_counters()[0]) >= B


# ---------------------------------------------------------------------------------------------- 4. - 8.
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam,kwargs,H', [(f, kw, HIDDEN[k % 3]) for k, (f, kw) in enumerate(LONG + SHORT)],
                         ids=[case_id(f, kw) for f, kw in LONG + SHORT])
def test_split_calls_exploration_mark_reset_buffers_and_interleaving(kind, fam, kwargs, H):
  B = 257
  env, twin = _make(fam, kwargs, B), Recorder(fam, kwargs, B)
  pol = _policy(kind, fam, H, 8)
  # 4. 3 + 4 steps leave what 7 leave, and the concatenated trajectories equal the whole
  a3 = _check(env, twin, kind, pol, _garbage(fam, B), 3, (kind, fam, 'first 3'))
  parts = [[t.clone() for t in (*a3[0], a3[1])]]
  a4 = _check(env, twin, kind, pol, a3[0].observation[-1], 4, (kind, fam, 'then 4'))
  parts.append([t.clone() for t in (*a4[0], a4[1])])
  whole, twin7 = _make(fam, kwargs, B), Recorder(fam, kwargs, B)
  w7 = _check(whole, twin7, kind, pol, _garbage(fam, B), 7, (kind, fam, 'whole 7'))
  _same(env, twin7, (kind, fam, '3 + 4 == 7'))
  for k, t in enumerate((*w7[0], w7[1])):
    assert torch.equal(_bits(torch.cat([parts[0][k], parts[1][k]])), _bits(t)), (kind, fam, k)
  # 7. buffers are cached per T: the same on a second call of the same T, others for another T
  ptrs3, ptrs4 = ([t.data_ptr() for t in (*a[0], a[1])] for a in (a3, a4))
  ts, actions = _check(env, twin, kind, pol, a4[0].observation[-1], 7, (kind, fam, 'seven more'))
  first7 = [t.data_ptr() for t in (*ts, actions)]
  assert not set(ptrs3) & set(ptrs4) and not set(first7) & set(ptrs3 + ptrs4)      # (all of the same environment)
  again4 = _check(env, twin, kind, pol, ts.observation[-1], 4, (kind, fam, 'four again'))
  assert [t.data_ptr() for t in (*again4[0], again4[1])] == ptrs4
  ts, actions = _check(env, twin, kind, pol, again4[0].observation[-1], 7, (kind, fam, 'and seven'))
  assert [t.data_ptr() for t in (*ts, actions)] == first7
  # 5. exploration: two seeds, ε in {0.3, 1.0}; ε = 0 draws nothing, whatever the seed
  for eps in (0.3, 1.0):
    for seed in (77, (1 << 63) + 5):
      ts, actions = _check(env, twin, kind, pol, ts.observation[-1], 7, (kind, fam, 'eps', eps, seed), epsilon=eps, explore_seed=seed)
  ts, actions = _check(env, twin, kind, pol, ts.observation[-1], 7, (kind, fam, 'eps 0 with a seed'), epsilon=0.0, explore_seed=(1 << 63) + 5)
  assert [t.data_ptr() for t in (*ts, actions)] == first7
  assert twin.seen == {0, 1, 2}
  # 6. mark_reset of a random third of the lanes between two calls: FIRST on step 0, action 0, their NaN rows never read
  g = torch.Generator(device='cuda')
  g.manual_seed(4)
  mask = torch.rand(B, generator=g, device='cuda') < 1.0 / 3.0
  env.mark_reset(mask)
  twin.env.mark_reset(mask)
  obs = ts.observation[-1].clone()
  obs[mask] = float('nan')
  ts, actions = _check(env, twin, kind, pol, obs, 7, (kind, fam, 'after mark_reset'))
  assert bool((ts.step_type[0][mask] == 0).all()) and bool((actions[0][mask] == 0).all())
  assert not bool(torch.isnan(ts.observation).any())
  _one_more_step(env, twin, (kind, fam, 'one more step'))
  # 8. interleaved with rollout(): its last observation is the next call's input ...
  acts = torch.randint(3, (5, B), generator=g, device='cuda', dtype=torch.int32)
  ro, rt = env.rollout(acts), twin.env.rollout(acts)
  twin.obs = rt.observation[-1].clone()
  ts, _ = _check(env, twin, kind, pol, ro.observation[-1], 7, (kind, fam, 'after rollout'))
  # ... with both evaluations (the twin runs their eager loops), and with the other kind of recording call
  lin, mlp = _policy('linear', fam, H, 9), _policy('mlp', fam, H, 10)
  twin.run(twin.select('linear', lin, None), 5)
  ev = env.evaluate_linear(*lin, ts.observation[-1], 5)
  _same(env, twin, (kind, fam, 'evaluate_linear'))
  twin.run(twin.select('mlp', mlp, None), 4)
  ev = env.evaluate_mlp(*mlp, ev.observation, 4)
  _same(env, twin, (kind, fam, 'evaluate_mlp'))
  other = 'mlp' if kind == 'linear' else 'linear'
  ts, _ = _check(env, twin, other, lin if other == 'linear' else mlp, ev.observation, 7, (kind, fam, 'the other call'))
  assert [t.data_ptr() for t in ts] == first7[:4]                          # (the two calls share their buffers)
  _check(env, twin, kind, pol, ts.observation[-1], 3, (kind, fam, 'and back'))
  _one_more_step(env, twin, (kind, fam, 'last step'))


# ---------------------------------------------------------------------------------------------- 9.
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam,kwargs,H', [(f, kw, HIDDEN[(k + 1) % 3]) for k, (f, kw) in enumerate(HUGE)], ids=[case_id(f, kw) for f, kw in HUGE])
def test_time_tables_beyond_4095_steps(kind, fam, kwargs, H):
  B, T = 257, 3
  env, twin = _make(fam, kwargs, B), Recorder(fam, kwargs, B)
  last = env._cfg.max_steps if fam == 'mountain_car' else env._cfg.last_step     # pylint: disable=protected-access
  assert last > 4095
  pol = _policy(kind, fam, H, 9)
  ts, _ = _check(env, twin, kind, pol, _garbage(fam, B), T, (kind, fam, 'fresh'))
  _check(env, twin, kind, pol, ts.observation[-1], T, (kind, fam, 'running'), epsilon=0.3, explore_seed=5)
  _one_more_step(env, twin, (kind, fam, 'one more step'))


# ---------------------------------------------------------------------------------------------- 10. what paid for the kernel
def test_the_merged_cold_kernel_reports_bsuite_info_as_the_python_side_computes_it():
  """bsuite_info() of cartpole, mountain_car and catch goes through bsx_bsuite_info — now one branch of bsx_lane_tool_kernel:
  it equals the columns plus the part still pending in the lanes' state, computed by torch from `_pending_info()`."""
  B = 300                                                                  # a ragged second workgroup
  g = torch.Generator(device='cuda')
  g.manual_seed(6)
  envs = [_make('cartpole', dict(max_time=0.05), B), _make('mountain_car', dict(max_steps=5), B), catch.Catch(seed=SEED, batch=B)]
  for env in envs:
    seen_pending = False
    for t in range(16):                                                    # episodes end and others are under way
      env.step(torch.randint(3, (B,), generator=g, device='cuda', dtype=torch.int32))
      if t < 12:
        continue
      want = env._info.clone()                                             # pylint: disable=protected-access
      pending = env._pending_info()                                        # pylint: disable=protected-access
      assert pending
      for col, v in pending.items():
        want[col] += v
      got = env._info_columns()                                            # pylint: disable=protected-access
      assert got.data_ptr() != env._info.data_ptr()                        # pylint: disable=protected-access
      assert torch.equal(_bits(got), _bits(want)), (type(env).__name__, t)
      seen_pending |= bool((env._info != want).any())                      # pylint: disable=protected-access
    assert seen_pending, type(env).__name__


def test_the_merged_cold_kernel_dumps_the_draw_stream_of_the_oracle():
  """... and bsx_stream_dump is its other branch: words and normals of a lane range that crosses 2^32, against oracle/stream.py."""
  seed, lane0, step, stream_id, n_lanes, n_words = 0xC0FFEE, OFFSET, (1 << 34) + 3, 2, 300, 6
  words = torch.zeros((n_lanes, n_words), dtype=torch.int32, device='cuda')
  normals = torch.zeros((n_lanes, n_words // 2), dtype=torch.float64, device='cuda')
  rc = _native.lib.bsx_stream_dump(seed, lane0, n_lanes, step, stream_id, n_words, words.data_ptr(), normals.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
  assert rc == 0
  ref = stream.words(seed, np.arange(lane0, lane0 + n_lanes, dtype=np.uint64), step, stream_id, n_words)
  np.testing.assert_array_equal(words.cpu().numpy().view(np.uint32), ref)
  z = stream.normal_from_k53(stream.k53(ref[:, 0::2], ref[:, 1::2]).reshape(-1))
  np.testing.assert_array_equal(normals.cpu().numpy().reshape(-1).view(np.uint64), z.view(np.uint64))
