"""GPU: evaluate_mlp2 / rollout_mlp2 — the closed loop of an agent with two ReLU hidden layers on cartpole, swing-up and
mountain_car in one launch, returns only or recorded.  The twin method of tests/test_gpu_mlp_eval.py and
tests/test_gpu_trajectory.py, whose helpers are imported: a second environment of the same seed and lane offset runs the
contract's eager loop — `a = 0 where the lane resets, else utils.observations.mlp2_select(w1[row], w2[row], w3[row], obs)`,
`step(a)` — through the existing kernels and the torch rule, never the new kernel.  Everything returned and everything left
behind is compared bit for bit."""
import numpy as np
import pytest
import torch

from bsuite_amd.utils import observations
from tests.test_gpu_mlp_eval import DIMS, _bits, _compare, _garbage, _make, _one_more_step, _pair, _rows, _same
from tests.test_gpu_trajectory import Recorder, _equal_steps

pytestmark = pytest.mark.gpu

# episodes of five steps: every lane meets LAST and FIRST inside a window of 40
FAMILIES = [('cartpole', dict(max_time=0.05)), ('cartpole_swingup', dict(max_time=0.05)), ('mountain_car', dict(max_steps=5))]
BATCHES = [1, 63, 64, 65, 257, 300]
WIDTHS = [(1, 1), (64, 1), (1, 64), (33, 7), (64, 64)]
STEPS = [1, 2, 40]
TIME = dict(cartpole=5, cartpole_swingup=5, mountain_car=2)     # the row's time fraction: 0, 0.2, .. 1.0 over an episode


def _triple(fam, H1, H2, seed, P=None, special=False):
  """A triple under which all three actions occur inside every episode and units of both layers switch on and off.  With u
  the row's time fraction: layer-1 unit j sees +g (u - 0.1) (j even) or -g (u - 0.1) (j odd), layer-2 unit k + or - the mean
  of the even layer-1 units, and l_0 = 0.3, l_1 = 1.5 m, l_2 = 3 m - 0.8 with m the mean of the even layer-2 units (about
  g (u - 0.1) from u = 0.2 on, 0 before) — action 0 at the start of an episode, 1 in its middle, 2 at its end.  Small random terms everywhere (every other feature included),
  scaled so that they do not change that order; for a population, another gain g in [1, 1.5] and another random part per
  row.  `special`: rows 1.. carry NaN, +inf, -inf and -0.0 weights in one place each."""
  D = DIMS[fam]
  g = torch.Generator(device='cpu')
  g.manual_seed(seed)
  n = 1 if P is None else P
  w1 = torch.randn((n, H1, D + 1), generator=g) * 0.01
  w2 = torch.randn((n, H2, H1 + 1), generator=g) * 0.01 / max(1, H1 // 8)
  w3 = torch.randn((n, 3, H2 + 1), generator=g) * 0.01 / max(1, H2 // 8)
  gain = 1.0 + 0.5 * torch.rand((n, 1), generator=g)
  s1 = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(H1)]).unsqueeze(0)
  s2 = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(H2)]).unsqueeze(0)
  w1[:, :, TIME[fam]] += gain * s1
  w1[:, :, D] -= 0.1 * gain * s1
  even1 = torch.tensor([1.0 / len(range(0, H1, 2)) if j % 2 == 0 else 0.0 for j in range(H1)])
  w2[:, :, :H1] += s2.unsqueeze(2) * even1.view(1, 1, H1)
  even2 = torch.tensor([1.0 / len(range(0, H2, 2)) if k % 2 == 0 else 0.0 for k in range(H2)])
  w3[:, 0, H2] += 0.3
  w3[:, 1, :H2] += 1.5 * even2
  w3[:, 2, :H2] += 3.0 * even2
  w3[:, 2, H2] -= 0.8
  if special:
    assert n >= 6
    w1[1, -1, D] = float('nan')                   # a NaN pre-activation in layer 1: the unit is off
    w2[2, -1, H1] = float('nan')                  # ... in layer 2
    w2[3, 0, 0] = float('inf')                    # +inf * h: an inf pre-activation, or a NaN where h is 0
    w1[4, 0, D] = float('-inf')                   # -inf in layer 1: off
    w3[5, 1, 0] = float('-inf')                   # a logit of -inf or NaN
    w3[1, 0, H2] = -0.0
    w2[4, 0, H1] = -0.0
  out = tuple(w.to(torch.float32).cuda().contiguous() for w in (w1, w2, w3))
  return tuple(w[0].contiguous() for w in out) if P is None else out


class Twin2(Recorder):
  """The recording eager twin under the torch rule of two hidden layers."""

  def select_mlp2(self, pol, policy_index):
    w1, w2, w3 = pol
    if w1.dim() == 3:
      w1, w2, w3 = (_rows(w, policy_index, self.B) for w in (w1, w2, w3))

    def select(obs, live):
      a, s1, s2 = observations.mlp2_select(w1, w2, w3, obs, return_preactivations=True)
      self.positive |= bool((s1[live] > 0).any()) and bool((s2[live] > 0).any())
      self.negative |= bool((s1[live] < 0).any()) or bool((s2[live] < 0).any())
      return a
    return select


def _record(env, twin, pol, obs, T, what, policy_index=None, **kw):
  """One rollout_mlp2 call against the twin's eager loop of the same arguments; returns (ts, actions)."""
  twin.run(twin.select_mlp2(pol, policy_index), T, **kw)
  ts, actions = env.rollout_mlp2(*pol, obs, T, policy_index=policy_index, **kw)
  _equal_steps(ts, actions, twin.last(T), what)
  _same(env, twin, what)
  return ts, actions


def _evaluate(env, twin, pol, obs, T, what, policy_index=None, **kw):
  """One evaluate_mlp2 call against the twin's eager loop of the same arguments; returns the result."""
  st, r64 = twin.run(twin.select_mlp2(pol, policy_index), T, **kw)
  ev = env.evaluate_mlp2(*pol, obs, T, policy_index=policy_index, **kw)
  _compare(ev, st, r64, env, twin, what)
  return ev


def _shuffled_index(B, P, seed):
  """Rows in a shuffled order, some outside [0, P - 1] (they are clamped)."""
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  pidx = torch.randint(-2, P + 3, (B,), generator=g, device='cuda', dtype=torch.int32)
  pidx[0], pidx[-1] = P + 2, -1
  return pidx


def _mark_third(env, twin, seed):
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  mask = torch.rand(twin.B, generator=g, device='cuda') < (1.0 / 3.0)
  mask[0] = True
  env.mark_reset(mask)
  twin.env.mark_reset(mask)


# ---------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize('T', STEPS)
@pytest.mark.parametrize('H1,H2', WIDTHS)
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=[f for f, _ in FAMILIES])
def test_both_calls_equal_the_eager_loop_of_a_twin(fam, kwargs, B, H1, H2, T):
  """Shared and a population of 5 under a shuffled policy_index with rows out of range, epsilon 0 and 0.3, record and
  evaluate: eight calls on one environment, each against the twin."""
  env, twin = _make(fam, kwargs, B), Twin2(fam, kwargs, B)
  one, pop = _triple(fam, H1, H2, 3), _triple(fam, H1, H2, 5, P=5)
  pidx = _shuffled_index(B, 5, B + T)
  what = (fam, B, H1, H2, T)
  # a fresh environment: every lane arrives with its reset pending and its observation row is not read — garbage
  ts, actions = _record(env, twin, one, _garbage(fam, B), T, what + ('shared', 'fresh'))
  assert bool((ts.step_type[0] == 0).all()) and bool((actions[0] == 0).all())
  obs = ts.observation[-1]
  # what the GREEDY policy shows, from the calls without the coin alone (an epsilon call takes every action whatever the
  # network says): the first call above and the epsilon = 0 calls below
  greedy, seen_last_first = set(twin.seen), False
  for who, pol, index in (('shared', one, None), ('population', pop, pidx)):
    for eps in (0.0, 0.3):
      kw = dict(policy_index=index, epsilon=eps, explore_seed=(1 << 45) + 9)
      if fam == 'mountain_car':
        _mark_third(env, twin, B + H1)                                     # these lanes begin the call with FIRST
      twin.seen = set()
      ts, _ = _record(env, twin, pol, obs, T, what + (who, eps, 'record'), **kw)
      if eps == 0.0:
        st = twin.last(T)[0]
        seen_last_first |= bool(((st[:-1] == 2) & (st[1:] == 0)).any()) if T > 1 else False
        greedy |= twin.seen
      ev = _evaluate(env, twin, pol, ts.observation[-1], T, what + (who, eps, 'evaluate'), **kw)
      if eps == 0.0:
        greedy |= twin.seen
      obs = ev.observation
  if T == 40:
    # not vacuous, by the twin's own output under epsilon = 0: episodes end and begin inside the window, the network itself
    # selects every action, units of both layers switch on and off
    assert seen_last_first
    assert greedy == {0, 1, 2}, greedy
    assert twin.positive and twin.negative
  _one_more_step(env, twin, what + ('one more step',))


# ---------------------------------------------------------------------------------------------- 2. replay
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=[f for f, _ in FAMILIES])
def test_replay_and_the_evaluation_of_the_same_arguments(fam, kwargs):
  B, T = 257, 40
  env, replay, scorer = _make(fam, kwargs, B), _make(fam, kwargs, B), _make(fam, kwargs, B)
  pop = _triple(fam, 33, 7, 8, P=5)
  pidx = _shuffled_index(B, 5, 2)
  for k, obs in enumerate((_garbage(fam, B), None)):
    obs = last if obs is None else obs                                     # noqa: F821  pylint: disable=used-before-assignment
    kw = dict(policy_index=pidx, epsilon=0.3, explore_seed=77 + k)
    ts, actions = env.rollout_mlp2(*pop, obs, T, **kw)
    again = replay.rollout(actions)
    for f in ('step_type', 'reward', 'discount', 'observation'):
      assert torch.equal(_bits(getattr(again, f)), _bits(getattr(ts, f))), (fam, k, f)
    ev = scorer.evaluate_mlp2(*pop, obs, T, **kw)
    assert torch.equal(_bits(ev.observation), _bits(ts.observation[-1]))
    assert torch.equal(ev.episodes, (ts.step_type == 2).sum(0).to(torch.int32))
    for other in (replay, scorer):
      for name, v in env._state.items():                                   # pylint: disable=protected-access
        assert torch.equal(_bits(other._state[name]), _bits(v)), (fam, k, name)   # pylint: disable=protected-access
      assert torch.equal(_bits(other._info), _bits(env._info))             # pylint: disable=protected-access
      assert torch.equal(other.episode_counters(), env.episode_counters()) and other.step_index == env.step_index
    last = ts.observation[-1].clone()


# ---------------------------------------------------------------------------------------------- 3. the old kernel
@pytest.mark.parametrize('H', [16, 64])
@pytest.mark.parametrize('fam,kwargs', [FAMILIES[0], FAMILIES[2]], ids=['cartpole', 'mountain_car'])
def test_an_identity_second_layer_is_evaluate_mlp(fam, kwargs, H):
  """w2 = [I | 0] and finite weights: h2 = relu(0 + 1 * h1 + 0 * ...) = h1 exactly, so the call is evaluate_mlp's, in every
  column and in what it leaves behind."""
  B, T = 130, 40
  env, old = _make(fam, kwargs, B), _make(fam, kwargs, B)
  w1, w3 = _pair(fam, H, 4)
  eye = torch.cat([torch.eye(H), torch.zeros((H, 1))], 1).cuda().contiguous()
  obs_a = obs_b = _garbage(fam, B)
  for k in range(2):
    kw = dict(epsilon=0.2 * k, explore_seed=5)
    a = env.evaluate_mlp2(w1, eye, w3, obs_a, T, **kw)
    b = old.evaluate_mlp(w1, w3, obs_b, T, **kw)
    for f in a._fields:
      assert torch.equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (fam, H, k, f)
    for name, v in old._state.items():                                     # pylint: disable=protected-access
      assert torch.equal(_bits(env._state[name]), _bits(v)), (fam, H, k, name)    # pylint: disable=protected-access
    assert torch.equal(_bits(env._info), _bits(old._info))                 # pylint: disable=protected-access
    assert torch.equal(env.episode_counters(), old.episode_counters()) and env.step_index == old.step_index
    assert int(a.episodes.sum()) >= B
    obs_a, obs_b = a.observation, b.observation


# ---------------------------------------------------------------------------------------------- 4. special values
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=[f for f, _ in FAMILIES])
def test_special_values_in_the_weights(fam, kwargs):
  B, T = 130, 9
  env, twin = _make(fam, kwargs, B), Twin2(fam, kwargs, B)
  pop = _triple(fam, 9, 6, 12, P=7, special=True)
  pidx = (torch.arange(B, device='cuda', dtype=torch.int32) * 3) % 7
  ts, _ = _record(env, twin, pop, _garbage(fam, B), T, (fam, 'special', 'record'), policy_index=pidx)
  own = [_rows(w, pidx, B) for w in pop]
  l = observations.mlp2_logits(*own, ts.observation[-1])
  s2 = observations.mlp2_select(*own, ts.observation[-1], return_preactivations=True)[2]
  assert not bool(torch.isfinite(l).all()) and bool(torch.isnan(s2).any())                          # the values do arrive
  _evaluate(env, twin, pop, ts.observation[-1], T, (fam, 'special', 'evaluate'), policy_index=pidx, epsilon=0.3, explore_seed=3)


# ---------------------------------------------------------------------------------------------- 5. buffers, interleaving
def test_cached_buffers_and_observation_passed_back():
  fam, kwargs = FAMILIES[1]
  B = 65
  env, twin = _make(fam, kwargs, B), Twin2(fam, kwargs, B)
  one = _triple(fam, 33, 7, 3)
  w1, w2 = _pair(fam, 5, 4)
  ev = _evaluate(env, twin, one, _garbage(fam, B), 7, 'first')
  ev2 = _evaluate(env, twin, one, ev.observation, 7, 'its own observation passed back')
  assert ev2.observation.data_ptr() == ev.observation.data_ptr()            # the cached LinearEvaluation buffers
  twin.run(twin.select_mlp(w1, w2, None), 3)
  ev3 = env.evaluate_mlp(w1, w2, ev2.observation, 3)                        # ... shared with evaluate_mlp
  assert ev3.observation.data_ptr() == ev.observation.data_ptr()
  _same(env, twin, 'evaluate_mlp in between')
  ts, actions = _record(env, twin, one, ev3.observation, 4, 'record T=4')
  kept = ts.observation.clone(), actions.clone()
  ts9, _ = _record(env, twin, one, ts.observation[-1], 9, 'record T=9')     # another T: the T=4 buffers are left alone
  assert torch.equal(_bits(ts.observation), _bits(kept[0])) and torch.equal(actions, kept[1])
  twin.run(twin.select_mlp(w1, w2, None), 4)
  ts4, _ = env.rollout_mlp(w1, w2, ts9.observation[-1], 4)                  # the per-T buffers are rollout_mlp's too
  assert ts4.observation.data_ptr() == ts.observation.data_ptr()
  _same(env, twin, 'rollout_mlp on the same T')


def test_interleaving_with_step_rollout_mlp_and_mark_reset():
  fam, kwargs = FAMILIES[0]
  B = 300
  env, twin = _make(fam, kwargs, B), Twin2(fam, kwargs, B)
  one, pop = _triple(fam, 64, 64, 3), _triple(fam, 1, 64, 5, P=5)
  w1, w2 = _pair(fam, 5, 4)
  pidx = _shuffled_index(B, 5, 1)
  ts, _ = _record(env, twin, one, _garbage(fam, B), 3, 'record')
  obs = _one_more_step(env, twin, 'step')
  ev = _evaluate(env, twin, pop, obs, 6, 'evaluate after a step', policy_index=pidx, epsilon=0.3, explore_seed=2)
  twin.run(twin.select_mlp(w1, w2, None), 5)
  ts, _ = env.rollout_mlp(w1, w2, ev.observation, 5)
  _same(env, twin, 'rollout_mlp')
  _mark_third(env, twin, 4)
  obs = ts.observation[-1].clone()
  obs[0] = float('nan')                                                     # a marked lane never reads its row
  ts, actions = _record(env, twin, one, obs, 7, 'after mark_reset')
  assert int(ts.step_type[0, 0]) == 0 and int(actions[0, 0]) == 0
  _one_more_step(env, twin, 'last step')


# ---------------------------------------------------------------------------------------------- 6. large batches
def _large(fam, kwargs, record):
  B, T = (1 << 20) + 257, 2
  env, twin = _make(fam, kwargs, B), Twin2(fam, kwargs, B)
  one = _triple(fam, 64, 64, 3)
  for k, obs in enumerate((_garbage(fam, B), None)):                        # (first never read: every lane resets)
    obs = twin.obs.clone() if obs is None else obs
    if record:
      _record(env, twin, one, obs, T, (fam, 'large', k))
    else:
      _evaluate(env, twin, one, obs, T, (fam, 'large', k))


def test_large_batch_cartpole_evaluate():
  _large(*FAMILIES[0], record=False)


def test_large_batch_mountain_car_record():
  _large(*FAMILIES[2], record=True)
