"""GPU: evaluate_sampled_linear / evaluate_sampled_mlp — the closed loop of a linear or hidden-layer SOFTMAX agent on cartpole,
swing-up and mountain_car in one launch, returns only.  The twin method of tests/test_gpu_sample.py, whose helpers are
imported: a second environment of the same seed and lane offset runs the contract's eager loop — `a = 0 where the lane resets,
else gumbel_select(*_logits(policy[row], obs), words(sample_seed, lane, call index), temperature)` with the words restated by
oracle/stream.py (stream 3), `step(a)` — and everything is compared bit for bit: `episodes` and the two float64 sums against
the contract's loop (tests/policy_eval_util.py) over the twin's step types and f64 rewards rebuilt from what the twin reported
(Twin.run, through _f64_rewards of tests/test_gpu_mlp_eval.py), never the engine's own f64; `.observation` against the twin's
last row; state, `_info`, bsuite_info, counters and the call index.  Then the recording call with the same arguments on a further twin, calls that compose, and the kernel that paid for
the new one: the delta-mode lane advance of deep_sea and catch is one merged kernel, both branches in one process."""
import numpy as np
import pytest
import torch

from bsuite_amd.utils import wrappers
from tests import engine_util as eu
from tests import policy_eval_util as pe
from tests.test_gpu_mlp_eval import HIDDEN, LONG, MAIN, OFFSET, SEED, SHORT, _bits, _garbage, _make, _one_more_step, _same, case_id
from tests.test_gpu_sample import Sampler, _sample
from tests.test_gpu_trajectory import _evaluate, _policy, _rollout, _state_of

pytestmark = pytest.mark.gpu

KINDS = ['linear', 'mlp']
BATCHES, STEPS = [1, 257], [1, 9]
SEEDS = (77, (1 << 63) + 5)
CASES = [pytest.param(kind, f, kw, T, B, HIDDEN[(fi + ti + bi) % 3], id=f'{kind}-{case_id(f, kw)}-T{T}-B{B}-H{HIDDEN[(fi + ti + bi) % 3]}')
         for kind in KINDS for fi, (f, kw) in enumerate(MAIN) for ti, T in enumerate(STEPS) for bi, B in enumerate(BATCHES)]


def _evaluate_sampled(env, kind, pol, obs, T, **kw):
  return (env.evaluate_sampled_mlp if kind == 'mlp' else env.evaluate_sampled_linear)(*pol, obs, T, **kw)


def _compare(ev, st, r64, env, twin, what):
  """The result against the contract's loop over the twin's step types and rebuilt f64 rewards, the twin's last row, and
  everything left behind."""
  want = pe.host_loop(st, r64)
  np.testing.assert_array_equal(want[0], (st == 2).sum(axis=0))
  assert ev.episodes.dtype is torch.int32 and ev.return_sum.dtype is torch.float64 and ev.episode_return_sum.dtype is torch.float64
  assert ev.observation.dtype is torch.float32 and tuple(ev.observation.shape) == tuple(twin.obs.shape)
  np.testing.assert_array_equal(ev.episodes.cpu().numpy(), want[0], err_msg=f'{what} episodes')
  np.testing.assert_array_equal(pe.bits(ev.return_sum.cpu().numpy()), pe.bits(want[1]), err_msg=f'{what} return_sum')
  np.testing.assert_array_equal(pe.bits(ev.episode_return_sum.cpu().numpy()), pe.bits(want[2]), err_msg=f'{what} episode_return_sum')
  assert torch.equal(_bits(ev.observation), _bits(twin.obs)), (what, 'observation')
  _same(env, twin, what)


def _check(env, twin, kind, pol, obs, T, what, policy_index=None, temperature=1.0, sample_seed=0, defaults=False):
  """One evaluate_sampled_* call against the twin's eager loop of the same arguments; returns (result, step types)."""
  st, r64 = twin.run(twin.sample(kind, pol, policy_index, temperature, sample_seed), T)
  kw = dict() if defaults else dict(temperature=temperature, sample_seed=sample_seed)
  ev = _evaluate_sampled(env, kind, pol, obs, T, policy_index=policy_index, **kw)
  _compare(ev, st, r64, env, twin, what)
  return ev, st


# ---------------------------------------------------------------------------------------------- 1. against the eager twin
@pytest.mark.parametrize('kind,fam,kwargs,T,B,H', CASES)
def test_equals_the_eager_loop_of_a_twin(kind, fam, kwargs, T, B, H):
  env, twin = _make(fam, kwargs, B), Sampler(fam, kwargs, B)
  pol = _policy(kind, fam, H, 3)
  # 1. a fresh environment: every lane resets on the first step and its observation row is not read — NaN.  The defaults:
  #    temperature 1, seed 0
  ev, st = _check(env, twin, kind, pol, _garbage(fam, B), T, (kind, fam, T, B, H, 'fresh'), defaults=True)
  assert (st[0] == 0).all() and not bool(torch.isnan(ev.observation).any())
  n_last = int((st == 2).sum())
  # 2. in the middle of its episodes, the returned observation passed back in: the very buffer the call overwrites
  same = ev.observation
  ev, st = _check(env, twin, kind, pol, same, T, (kind, fam, T, B, H, 'running'), temperature=1.0, sample_seed=SEEDS[0])
  assert ev.observation.data_ptr() == same.data_ptr()
  n_last += int((st == 2).sum())
  if B == 257 and T == 9:
    # the case samples — by the restatement alone: all three actions, and not the greedy policy
    assert twin.seen == {0, 1, 2}, twin.seen
    assert twin.off_greedy >= 0.05 * twin.live_steps, (twin.off_greedy, twin.live_steps)
  if kwargs and T == 9:
    assert n_last >= B                                                   # episodes end inside the calls
  # 3. [B, D] rows after a step(); a cold policy, the seed beyond 2^63
  obs = _one_more_step(env, twin, (kind, fam, T, B, H, 'one more step'))
  ev, _ = _check(env, twin, kind, pol, obs.reshape(B, -1), T, (kind, fam, T, B, H, 'after a step, [B, D] rows'), temperature=0.25,
                 sample_seed=SEEDS[1])
  # 4. a population of three with rows named outside [0, P-1], a hot policy
  g = torch.Generator(device='cuda')
  g.manual_seed(B + T)
  pop = _policy(kind, fam, H, 5, P=3)
  pidx = torch.randint(-1, 8, (B,), generator=g, device='cuda', dtype=torch.int32)
  pidx[0], pidx[-1] = 7, -1
  ev, _ = _check(env, twin, kind, pop, ev.observation, T, (kind, fam, T, B, H, 'population'), policy_index=pidx, temperature=4.0,
                 sample_seed=SEEDS[0])
  # 5. one policy per lane
  each = _policy(kind, fam, H, 6, P=B)
  lanes = torch.arange(B, device='cuda', dtype=torch.int32) if B > 1 else None      # (P == 1: policy_index must be None)
  _check(env, twin, kind, each, ev.observation, T, (kind, fam, T, B, H, 'one policy per lane'), policy_index=lanes, temperature=1.0,
         sample_seed=SEEDS[1])
  _one_more_step(env, twin, (kind, fam, T, B, H, 'last step'))
  assert int(env.episode_counters()[1]) >= B


# ---------------------------------------------------------------------------------------------- 2. against the recording call
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam,kwargs,H', [(f, kw, HIDDEN[k % 3]) for k, (f, kw) in enumerate(MAIN)], ids=[case_id(f, kw) for f, kw in MAIN])
def test_the_recording_call_with_the_same_arguments_agrees(kind, fam, kwargs, H):
  B, T = 257, 9
  env, recorded = _make(fam, kwargs, B), _make(fam, kwargs, B)
  pol = _policy(kind, fam, H, 4)
  obs = _garbage(fam, B)
  for n, kw in enumerate((dict(), dict(temperature=0.25, sample_seed=SEEDS[1]), dict(temperature=4.0, sample_seed=SEEDS[0]))):
    ts, _ = _sample(recorded, kind, pol, obs, T, **kw)
    ev = _evaluate_sampled(env, kind, pol, obs.clone(), T, **kw)
    _same(env, _state_of(recorded), (kind, fam, n, 'sample_*'))
    assert torch.equal(_bits(ev.observation), _bits(ts.observation[-1])), (kind, fam, n)
    assert torch.equal(ev.episodes, (ts.step_type == 2).sum(0).to(torch.int32)), (kind, fam, n)
    obs = ts.observation[-1].clone()
  if kwargs:
    assert int(env.episode_counters()[0]) >= B
  # another sample_seed draws other actions (two fresh twins of the recording call), and leaves another state behind here
  a, b = _make(fam, kwargs, B), _make(fam, kwargs, B)
  (_, acts_a), (_, acts_b) = _sample(a, kind, pol, _garbage(fam, B), T, sample_seed=1), _sample(b, kind, pol, _garbage(fam, B), T, sample_seed=2)
  assert not torch.equal(acts_a, acts_b)
  x, y = _make(fam, kwargs, B), _make(fam, kwargs, B)
  ex = _evaluate_sampled(x, kind, pol, _garbage(fam, B), T, sample_seed=1).observation.clone()
  ey = _evaluate_sampled(y, kind, pol, _garbage(fam, B), T, sample_seed=2).observation.clone()
  _same(x, _state_of(a), (kind, fam, 'seed 1'))
  _same(y, _state_of(b), (kind, fam, 'seed 2'))
  assert not torch.equal(_bits(ex), _bits(ey))
  # there is no exploration argument: the softmax explores
  for word in ('epsilon', 'explore_seed'):
    with pytest.raises(TypeError, match=word):
      _evaluate_sampled(x, kind, pol, ex, T, **{word: 0})


# ---------------------------------------------------------------------------------------------- 3. calls compose
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam,kwargs,H', [(f, kw, HIDDEN[k % 3]) for k, (f, kw) in enumerate(LONG + SHORT)],
                         ids=[case_id(f, kw) for f, kw in LONG + SHORT])
def test_split_calls_mark_reset_buffers_interleaving_and_a_device_counter(kind, fam, kwargs, H):
  B = 257
  env, twin = _make(fam, kwargs, B), Sampler(fam, kwargs, B)
  counted = eu.make_env(fam, dict(kwargs), batch=B, lane_offset=OFFSET, seed=SEED, device_step_counter=True)
  pol = _policy(kind, fam, H, 8)
  how = dict(temperature=1.0, sample_seed=SEEDS[1])

  def also_counted(obs, T, what, **kw):
    """The environment whose call index lives in device memory takes the same call: the same result, the same state."""
    ev = env._linear_eval_out                                            # pylint: disable=protected-access
    got = _evaluate_sampled(counted, kind, pol, obs, T, **kw)
    for f in ('episodes', 'return_sum', 'episode_return_sum', 'observation'):
      assert torch.equal(_bits(getattr(got, f)), _bits(getattr(ev, f))), (kind, fam, what, f)
    _same(counted, twin, (kind, fam, what, 'device counter'))
    assert counted.device_step_index() == counted.step_index == env.step_index
    return got

  # 4 + 5 steps leave what 9 leave, and the episode counts add
  e4, _ = _check(env, twin, kind, pol, _garbage(fam, B), 4, (kind, fam, 'first 4'), **how)
  c = also_counted(_garbage(fam, B), 4, 'first 4', **how)
  n4 = e4.episodes.clone()
  e5, _ = _check(env, twin, kind, pol, e4.observation, 5, (kind, fam, 'then 5'), **how)
  c = also_counted(c.observation, 5, 'then 5', **how)
  whole, twin9 = _make(fam, kwargs, B), Sampler(fam, kwargs, B)
  e9, _ = _check(whole, twin9, kind, pol, _garbage(fam, B), 9, (kind, fam, 'whole 9'), **how)
  _same(env, twin9, (kind, fam, '4 + 5 == 9'))
  assert torch.equal(n4 + e5.episodes, e9.episodes) and torch.equal(_bits(e5.observation), _bits(e9.observation))
  if kwargs:
    assert int(e9.episodes.sum()) >= B
  # mark_reset of a random third of the lanes between two calls: their NaN rows are never read
  g = torch.Generator(device='cuda')
  g.manual_seed(4)
  mask = torch.rand(B, generator=g, device='cuda') < 1.0 / 3.0
  for e in (env, twin.env, counted):
    e.mark_reset(mask)
  obs = e5.observation.clone()
  obs[mask] = float('nan')
  ev, st = _check(env, twin, kind, pol, obs, 7, (kind, fam, 'after mark_reset'), **how)
  c = also_counted(obs, 7, 'after mark_reset', **how)
  assert (st[0][mask.cpu().numpy()] == 0).all() and not bool(torch.isnan(ev.observation).any())
  obs = _one_more_step(env, twin, (kind, fam, 'one more step'))
  # interleaved with rollout(): its last observation is the next call's input ...
  acts = torch.randint(3, (5, B), generator=g, device='cuda', dtype=torch.int32)
  ro, rt = env.rollout(acts), twin.env.rollout(acts)
  twin.obs = rt.observation[-1].clone()
  ev, _ = _check(env, twin, kind, pol, ro.observation[-1], 7, (kind, fam, 'after rollout'), temperature=0.25, sample_seed=SEEDS[0])
  # ... with evaluate_linear, whose buffers these are, and which overwrites them
  lin, mlp = _policy('linear', fam, H, 9), _policy('mlp', fam, H, 10)
  ptrs = [getattr(ev, f).data_ptr() for f in ('episodes', 'return_sum', 'episode_return_sum', 'observation')]
  kept = ev.observation.clone()
  twin.run(twin.select('linear', lin, None), 5)
  greedy = _evaluate(env, 'linear', lin, ev.observation, 5)
  _same(env, twin, (kind, fam, 'evaluate_linear'))
  assert [getattr(greedy, f).data_ptr() for f in ('episodes', 'return_sum', 'episode_return_sum', 'observation')] == ptrs
  assert greedy is ev and not torch.equal(_bits(kept), _bits(ev.observation))
  # ... with the recording sampled call of the hidden-layer kind, and with the other kind of this call
  twin.run(twin.sample('mlp', mlp, None, 4.0, SEEDS[0]), 4)
  ts, _ = _sample(env, 'mlp', mlp, greedy.observation, 4, temperature=4.0, sample_seed=SEEDS[0])
  _same(env, twin, (kind, fam, 'sample_mlp'))
  other = 'mlp' if kind == 'linear' else 'linear'
  ev, _ = _check(env, twin, other, lin if other == 'linear' else mlp, ts.observation[-1], 7, (kind, fam, 'the other kind'), **how)
  assert [getattr(ev, f).data_ptr() for f in ('episodes', 'return_sum', 'episode_return_sum', 'observation')] == ptrs
  # ... and with the greedy recording call
  twin.run(twin.select(kind, pol, None), 3)
  ts, _ = _rollout(env, kind, pol, ev.observation, 3)
  _same(env, twin, (kind, fam, 'rollout_*'))
  _check(env, twin, kind, pol, ts.observation[-1], 3, (kind, fam, 'and back'), temperature=4.0, sample_seed=SEEDS[0])
  _one_more_step(env, twin, (kind, fam, 'last step'))


# ---------------------------------------------------------------------------------------------- 4. what paid for the kernel
PAIRS = [('deep_sea', dict(size=3, mapping_seed=3), 2), ('deep_sea', dict(size=10, mapping_seed=42), 2), ('catch', {}, 3)]


def _delta_equals_dense(dense, delta, num_actions, B, what):
  raw_dense, raw_delta = eu.raw(dense), eu.raw(delta)
  g = torch.Generator(device='cuda')
  g.manual_seed(B)
  for t in range(26):
    a = torch.randint(num_actions, (B,), device='cuda', generator=g, dtype=torch.int32)
    x, y = (dense.reset(), delta.reset()) if t == 13 else (dense.step(a), delta.step(a))       # an explicit reset in mid-episode
    assert torch.equal(_bits(x.observation), _bits(y.observation)), (what, t)                   # the persistent board, patched
    for f in ('step_type', 'reward', 'discount'):
      assert torch.equal(_bits(getattr(x, f)), _bits(getattr(y, f))), (what, t, f)
    for k, v in raw_dense._state.items():                                  # pylint: disable=protected-access
      assert torch.equal(raw_delta._state[k], v), (what, t, k)             # pylint: disable=protected-access
    assert torch.equal(raw_dense.episode_counters(), raw_delta.episode_counters()), (what, t)
  assert int(raw_delta.episode_counters()[0]) >= 1
  assert torch.equal(_bits(raw_dense._info), _bits(raw_delta._info)), what                      # pylint: disable=protected-access
  for k, v in dense.bsuite_info().items():
    assert torch.equal(_bits(v), _bits(delta.bsuite_info()[k])), (what, k)


def test_the_merged_cold_kernel_patches_the_boards_of_both_families():
  """The lane advance of observation_mode='delta' is one kernel for deep_sea and catch now, the family a uniform switch: both
  branches in one process, at a lone lane and with a ragged second workgroup — 25 steps of random actions and a reset(), the
  persistent board against a dense twin's observation on every step, and the scalar columns, the state and the counters.  Then
  once under RewardNoise + Logging: the call that is not lean, which the delta kernel serves too."""
  for fam, kwargs, num_actions in PAIRS:
    for B in (1, 257):
      mk = lambda **k: eu.make_env(fam, kwargs, batch=B, lane_offset=OFFSET, seed=9, **k)      # pylint: disable=cell-var-from-loop
      _delta_equals_dense(mk(), mk(observation_mode='delta'), num_actions, B, (fam, kwargs, B))
  for fam, kwargs, num_actions in PAIRS[1:]:
    mk = lambda **k: wrappers.Logging(eu.make_env(fam, kwargs, batch=257, lane_offset=OFFSET, seed=9, wrap=('noise', 0.5), **k), None)   # pylint: disable=cell-var-from-loop
    _delta_equals_dense(mk(), mk(observation_mode='delta'), num_actions, 257, (fam, kwargs, 'RewardNoise + Logging'))
