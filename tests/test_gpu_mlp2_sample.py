"""GPU: sample_mlp2 / evaluate_sampled_mlp2 — the closed loop of a SOFTMAX agent with two ReLU hidden layers on cartpole,
swing-up and mountain_car in one launch, recorded or returns only (the drawn mode of bsx_torso_kernel).  The twin method of
tests/test_gpu_mlp2.py, tests/test_gpu_sample.py and tests/test_gpu_sampled_eval.py, whose helpers are imported: a second
environment of the same seed and lane offset runs the contract's eager loop — `a = 0 where the lane resets, else
gumbel_select(mlp2_logits(w1[row], w2[row], w3[row], obs), words(sample_seed, lane, call index), temperature)` with the
words restated by oracle/stream.py (stream 3), `step(a)` — through the existing kernels and the torch rule, never the new
mode.  Everything returned and everything left behind is compared bit for bit.  Last, both calls over the edge-state grid of
tests/physics_edge_util.py, driven the way tests/test_gpu_physics_edges.py drives rollout_mlp2 / evaluate_mlp2."""
import numpy as np
import pytest
import torch

from bsuite_amd.utils import observations
from oracle import stream
from tests import physics_edge_util as pu
from tests import policy_eval_util as pe
from tests import test_gpu_physics_edges as edges
from tests.test_gpu_mlp2 import FAMILIES, Twin2, _mark_third, _shuffled_index, _triple
from tests.test_gpu_mlp_eval import OFFSET, _bits, _compare, _garbage, _make, _one_more_step, _pair, _rows, _same
from tests.test_gpu_sample import STREAM_SAMPLE, Sampler, _greedy
from tests.test_gpu_trajectory import FIELDS, _equal_steps, _state_of

pytestmark = pytest.mark.gpu

BATCHES = [1, 64, 65, 257]                    # a single lane, a full wave, a wave plus one, a workgroup plus one
WIDTHS = [(1, 1), (33, 7), (7, 17), (64, 64)]  # the minimum, and each register tier of layer 2: 16, 32 (17), 64
STEPS = [1, 9]
BIG_SEED = (1 << 63) + 5
EVAL_FIELDS = ('episodes', 'return_sum', 'episode_return_sum', 'observation')


class Sampler2(Sampler, Twin2):
  """The sampling twin with an `mlp2` kind: utils.observations.mlp2_logits + gumbel_select on the oracle's words."""

  def __init__(self, fam, kwargs, B):
    super().__init__(fam, kwargs, B)
    self.nonfinite = False

  def sample_mlp2(self, pol, policy_index, temperature, sample_seed):
    own = tuple(w if w.dim() == 2 else _rows(w, policy_index, self.B) for w in pol)

    def select(obs, live):
      logits = observations.mlp2_logits(*own, obs)
      words = stream.words(int(sample_seed), self.lanes, self.env.step_index, STREAM_SAMPLE, 3)
      a = observations.gumbel_select(logits.cpu(), words, temperature).cuda()
      self.live_steps += int(live.sum())
      self.off_greedy += int((a != _greedy(logits))[live].sum())
      self.nonfinite |= not bool(torch.isfinite(logits[live]).all())
      return a
    return select


def _record(env, twin, pol, obs, T, what, policy_index=None, temperature=1.0, sample_seed=0, defaults=False):
  """One sample_mlp2 call against the twin's eager loop of the same arguments; returns (ts, actions)."""
  twin.run(twin.sample_mlp2(pol, policy_index, temperature, sample_seed), T)
  kw = dict() if defaults else dict(temperature=temperature, sample_seed=sample_seed)
  ts, actions = env.sample_mlp2(*pol, obs, T, policy_index=policy_index, **kw)
  _equal_steps(ts, actions, twin.last(T), what)
  _same(env, twin, what)
  return ts, actions


def _evaluate(env, twin, pol, obs, T, what, policy_index=None, temperature=1.0, sample_seed=0, defaults=False):
  """One evaluate_sampled_mlp2 call against the twin's eager loop of the same arguments; returns the result."""
  st, r64 = twin.run(twin.sample_mlp2(pol, policy_index, temperature, sample_seed), T)
  kw = dict() if defaults else dict(temperature=temperature, sample_seed=sample_seed)
  ev = env.evaluate_sampled_mlp2(*pol, obs, T, policy_index=policy_index, **kw)
  _compare(ev, st, r64, env, twin, what)
  return ev


def _left_behind_equal(a, b, what):
  _same(a, _state_of(b), what)
  assert int(a.invalid_action_count()) == int(b.invalid_action_count()) == 0, what


def _third(B, seed):
  """The mask _mark_third(.., seed) marks."""
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  mask = torch.rand(B, generator=g, device='cuda') < (1.0 / 3.0)
  mask[0] = True
  return mask


# ---------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize('T', STEPS)
@pytest.mark.parametrize('H1,H2', WIDTHS)
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=[f for f, _ in FAMILIES])
def test_both_calls_equal_the_eager_loop_of_a_twin(fam, kwargs, B, H1, H2, T):
  """Fresh with garbage rows and the defaults; running with the buffer's own last row passed back, temperature 1; shared at
  temperature 0.25 with the seed 2^63 + 5; a population of 5 under a shuffled policy_index with rows out of range at
  temperature 4 — each as sample_mlp2, then as evaluate_sampled_mlp2: eight calls on one environment, each against the twin."""
  env, twin = _make(fam, kwargs, B), Sampler2(fam, kwargs, B)
  one, pop = _triple(fam, H1, H2, 3), _triple(fam, H1, H2, 5, P=5)
  pidx = _shuffled_index(B, 5, B + T)
  what = (fam, B, H1, H2, T)
  seen_last_first = False

  def both(pol, obs, tag, **kw):
    nonlocal seen_last_first
    ts, _ = _record(env, twin, pol, obs, T, what + (tag, 'record'), **kw)
    st = twin.last(T)[0]
    seen_last_first |= bool(((st[:-1] == 2) & (st[1:] == 0)).any()) if T > 1 else False
    return ts, _evaluate(env, twin, pol, ts.observation[-1], T, what + (tag, 'evaluate'), **kw)

  # a fresh environment: every lane arrives with its reset pending and its observation row is not read — garbage
  ts, actions = _record(env, twin, one, _garbage(fam, B), T, what + ('fresh', 'record'), defaults=True)
  assert bool((ts.step_type[0] == 0).all()) and bool((actions[0] == 0).all())
  ev = _evaluate(env, twin, one, ts.observation[-1], T, what + ('fresh', 'evaluate'), defaults=True)
  # in the middle of its episodes, each call with its own buffer's last row passed back in: a slice of the [T,B,D] buffer the
  # recording call overwrites, the very buffer the evaluation overwrites
  ts, _ = _record(env, twin, one, ev.observation, T, what + ('running', 'record'), temperature=1.0, sample_seed=77)
  same = ts.observation[-1]
  ts, _ = _record(env, twin, one, same, T, what + ('running', 'record, own row'), temperature=1.0, sample_seed=77)
  assert ts.observation[-1].data_ptr() == same.data_ptr()
  ev = _evaluate(env, twin, one, ts.observation[-1], T, what + ('running', 'evaluate'), temperature=1.0, sample_seed=77)
  same = ev.observation
  ev = _evaluate(env, twin, one, same, T, what + ('running', 'evaluate, own row'), temperature=1.0, sample_seed=77)
  assert ev.observation.data_ptr() == same.data_ptr()
  ts, ev = both(one, ev.observation, 'cold', temperature=0.25, sample_seed=BIG_SEED)
  if fam == 'mountain_car':
    _mark_third(env, twin, B + H1)                                         # these lanes begin the call with FIRST
  both(pop, ev.observation, 'population', policy_index=pidx, temperature=4.0, sample_seed=77)
  if B == 257 and T == 9:
    # not vacuous, by the twin's restatement alone (at temperature 1, 0.25 and 4 together: _triple's logits lie within about
    # 3 of each other, so the softmax at temperature 1 already leaves the greedy action often): episodes end and begin inside
    # the window, all three actions are drawn, and not the greedy policy
    assert seen_last_first
    assert twin.seen == {0, 1, 2}, twin.seen
    assert twin.off_greedy >= 0.05 * twin.live_steps, (twin.off_greedy, twin.live_steps)
  _one_more_step(env, twin, what + ('one more step',))


# ---------------------------------------------------------------------------------------------- 2. two calls, one walk
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=[f for f, _ in FAMILIES])
def test_two_calls_one_walk_and_replay(fam, kwargs):
  B, T = 257, 9
  env, scorer, replay = _make(fam, kwargs, B), _make(fam, kwargs, B), _make(fam, kwargs, B)
  pop = _triple(fam, 33, 7, 8, P=5)
  pidx = _shuffled_index(B, 5, 2)
  obs = _garbage(fam, B)
  for k, kw in enumerate((dict(), dict(temperature=0.25, sample_seed=BIG_SEED), dict(temperature=4.0, sample_seed=77))):
    ts, actions = env.sample_mlp2(*pop, obs, T, policy_index=pidx, **kw)
    ev = scorer.evaluate_sampled_mlp2(*pop, obs.clone(), T, policy_index=pidx, **kw)
    again = replay.rollout(actions)
    for f in FIELDS:
      assert torch.equal(_bits(getattr(again, f)), _bits(getattr(ts, f))), (fam, k, f)
    assert torch.equal(_bits(ev.observation), _bits(ts.observation[-1])), (fam, k)
    assert torch.equal(ev.episodes, (ts.step_type == 2).sum(0).to(torch.int32)), (fam, k)
    for other in (scorer, replay):
      _left_behind_equal(other, env, (fam, k))
    obs = ts.observation[-1].clone()
  assert int(env.episode_counters()[0]) >= B
  # another sample_seed draws other actions
  a, b = _make(fam, kwargs, B), _make(fam, kwargs, B)
  acts_a = a.sample_mlp2(*pop, _garbage(fam, B), T, policy_index=pidx, sample_seed=1)[1]
  acts_b = b.sample_mlp2(*pop, _garbage(fam, B), T, policy_index=pidx, sample_seed=2)[1]
  assert not torch.equal(acts_a, acts_b)
  # there is no exploration argument: the softmax explores
  for call in (a.sample_mlp2, a.evaluate_sampled_mlp2):
    for word in ('epsilon', 'explore_seed'):
      with pytest.raises(TypeError, match=word):
        call(*pop, obs, T, policy_index=pidx, **{word: 0})


# ---------------------------------------------------------------------------------------------- 3. the one-layer kernels
@pytest.mark.parametrize('H', [16, 64])
@pytest.mark.parametrize('fam,kwargs', [FAMILIES[0], FAMILIES[2]], ids=['cartpole', 'mountain_car'])
def test_an_identity_second_layer_is_sample_mlp(fam, kwargs, H):
  """w2 = [I | 0] and finite weights: h2 = relu(0 + 1 * h1 + 0 * ...) = h1 exactly, so the logits are mlp_logits' and both
  calls are bit for bit the one-hidden-layer sampled calls of the same temperature and seed."""
  B, T = 130, 9
  w1, w3 = _pair(fam, H, 4)
  eye = torch.cat([torch.eye(H), torch.zeros((H, 1))], 1).cuda().contiguous()
  env, old = _make(fam, kwargs, B), _make(fam, kwargs, B)
  obs_a = obs_b = _garbage(fam, B)
  for k, kw in enumerate((dict(temperature=1.0, sample_seed=5), dict(temperature=0.25, sample_seed=BIG_SEED), dict(temperature=4.0, sample_seed=5))):
    (ts_a, act_a), (ts_b, act_b) = env.sample_mlp2(w1, eye, w3, obs_a, T, **kw), old.sample_mlp(w1, w3, obs_b, T, **kw)
    for f in FIELDS:
      assert torch.equal(_bits(getattr(ts_a, f)), _bits(getattr(ts_b, f))), (fam, H, k, f)
    assert torch.equal(act_a, act_b), (fam, H, k)
    _left_behind_equal(env, old, (fam, H, k, 'sample'))
    a = env.evaluate_sampled_mlp2(w1, eye, w3, ts_a.observation[-1], T, **kw)
    b = old.evaluate_sampled_mlp(w1, w3, ts_b.observation[-1], T, **kw)
    for f in EVAL_FIELDS:
      assert torch.equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (fam, H, k, f)
    _left_behind_equal(env, old, (fam, H, k, 'evaluate'))
    obs_a, obs_b = a.observation, b.observation
  assert int(env.episode_counters()[0]) >= B
  assert set(act_a.unique().tolist()) == {0, 1, 2}


# ---------------------------------------------------------------------------------------------- 4. frequencies on the device
def test_action_frequencies_of_a_known_softmax():
  """MountainCar under a shared triple with all weights zero and head biases (0, ln 2, ln 4): every live lane-step draws from
  (1/7, 2/7, 4/7).  B = 4096, T = 17: step 0 resets (action 0, nothing drawn), the 16 others are live.  The words depend only
  on seed, lane and step, so the restatement is the one tests/test_gpu_sample.py holds within the same bound."""
  B, T, seed = 4096, 17, 2
  H1, H2 = 5, 4
  w1, w2, w3 = torch.zeros((H1, 4)), torch.zeros((H2, H1 + 1)), torch.zeros((3, H2 + 1))
  w3[1, H2], w3[2, H2] = float(np.float32(np.log(2.0))), float(np.float32(np.log(4.0)))
  lanes = np.uint64(OFFSET) + np.arange(B, dtype=np.uint64)
  logits = observations.mlp2_logits(w1, w2, w3, torch.randn((B, 3)))
  assert torch.equal(_bits(logits), _bits(w3[:, H2].unsqueeze(0).expand(B, 3).contiguous()))
  want = torch.stack([torch.zeros(B, dtype=torch.int32)] +
                     [observations.gumbel_select(logits, stream.words(seed, lanes, t, STREAM_SAMPLE, 3)) for t in range(1, T)])
  l64 = w3[:, H2].to(torch.float64).numpy()
  p = np.exp(l64) / np.exp(l64).sum()
  np.testing.assert_allclose(p, [1 / 7, 2 / 7, 4 / 7], rtol=1e-7)
  n = B * (T - 1)
  sigma = np.sqrt(p * (1 - p) / n)

  def within(actions, what):
    freq = np.bincount(actions[1:].reshape(-1).numpy(), minlength=3) / n
    print(what, 'frequencies', freq, 'in sigma', (freq - p) / sigma)
    assert (np.abs(freq - p) <= 4 * sigma).all(), (what, freq, (freq - p) / sigma)

  within(want, 'restatement')
  env = _make('mountain_car', {}, B)
  ts, actions = env.sample_mlp2(w1.cuda(), w2.cuda(), w3.cuda(), _garbage('mountain_car', B), T, sample_seed=seed)
  assert bool((ts.step_type[0] == 0).all()) and bool((ts.step_type[1:] == 1).all())
  assert torch.equal(actions.cpu(), want)
  within(actions.cpu(), 'device')


# ---------------------------------------------------------------------------------------------- 5. special values
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=[f for f, _ in FAMILIES])
def test_special_values_in_the_weights(fam, kwargs):
  B, T = 130, 9
  env, twin = _make(fam, kwargs, B), Sampler2(fam, kwargs, B)
  pop = _triple(fam, 9, 6, 12, P=7, special=True)
  pidx = (torch.arange(B, device='cuda', dtype=torch.int32) * 3) % 7
  ts, _ = _record(env, twin, pop, _garbage(fam, B), T, (fam, 'special', 'record'), policy_index=pidx, temperature=1.0, sample_seed=3)
  own = [_rows(w, pidx, B) for w in pop]
  l = observations.mlp2_logits(*own, ts.observation[-1])
  s2 = observations.mlp2_select(*own, ts.observation[-1], return_preactivations=True)[2]
  assert not bool(torch.isfinite(l).all()) and bool(torch.isnan(s2).any())                          # the values do arrive
  _evaluate(env, twin, pop, ts.observation[-1], T, (fam, 'special', 'evaluate'), policy_index=pidx, temperature=0.25, sample_seed=BIG_SEED)
  assert twin.nonfinite                                                    # ... on live steps of the twin's own loop too


# ---------------------------------------------------------------------------------------------- 6. composition
def test_split_calls_mark_reset_buffers_and_interleaving():
  fam, kwargs = FAMILIES[1]
  B = 257
  env, twin = _make(fam, kwargs, B), Sampler2(fam, kwargs, B)
  one, pop = _triple(fam, 33, 7, 3), _triple(fam, 7, 17, 5, P=5)
  w1, w2 = _pair(fam, 5, 4)
  pidx = _shuffled_index(B, 5, 1)
  how = dict(temperature=1.0, sample_seed=BIG_SEED)
  # 3 + 4 steps leave what 7 leave, and the concatenated trajectories equal the whole
  a3 = _record(env, twin, one, _garbage(fam, B), 3, 'first 3', **how)
  parts = [[t.clone() for t in (*a3[0], a3[1])]]
  a4 = _record(env, twin, one, a3[0].observation[-1], 4, 'then 4', **how)
  parts.append([t.clone() for t in (*a4[0], a4[1])])
  whole, twin7 = _make(fam, kwargs, B), Sampler2(fam, kwargs, B)
  w7 = _record(whole, twin7, one, _garbage(fam, B), 7, 'whole 7', **how)
  _same(env, twin7, '3 + 4 == 7')
  for k, t in enumerate((*w7[0], w7[1])):
    assert torch.equal(_bits(torch.cat([parts[0][k], parts[1][k]])), _bits(t)), k
  # ... and for the evaluation: the episode counts add, the last rows agree
  e3 = _evaluate(env, twin, one, a4[0].observation[-1], 3, 'evaluate 3', **how)
  n3 = e3.episodes.clone()
  e4 = _evaluate(env, twin, one, e3.observation, 4, 'evaluate 4', **how)
  e7 = _evaluate(whole, twin7, one, w7[0].observation[-1], 7, 'evaluate 7', **how)
  _same(env, twin7, 'evaluate 3 + 4 == 7')
  assert torch.equal(n3 + e4.episodes, e7.episodes) and torch.equal(_bits(e4.observation), _bits(e7.observation))
  # the per-T buffers are rollout_mlp2's, the evaluation buffers evaluate_mlp2's
  ptrs4 = [t.data_ptr() for t in (*a4[0], a4[1])]
  twin.run(twin.select_mlp2(one, None), 4)
  ts, actions = env.rollout_mlp2(*one, e4.observation, 4)
  _equal_steps(ts, actions, twin.last(4), 'rollout_mlp2 of the same T')
  assert [t.data_ptr() for t in (*ts, actions)] == ptrs4
  eval_ptrs = [getattr(e4, f).data_ptr() for f in EVAL_FIELDS]
  st, r64 = twin.run(twin.select_mlp2(pop, pidx), 5, epsilon=0.3, explore_seed=2)
  ev = env.evaluate_mlp2(*pop, ts.observation[-1], 5, policy_index=pidx, epsilon=0.3, explore_seed=2)
  _compare(ev, st, r64, env, twin, 'evaluate_mlp2 in between')
  assert ev is e4 and [getattr(ev, f).data_ptr() for f in EVAL_FIELDS] == eval_ptrs
  # mark_reset of a third of the lanes between two calls: FIRST on step 0, action 0, their NaN rows never read
  _mark_third(env, twin, 4)
  marked = _third(B, 4)
  assert bool(marked[0]) and 0 < int(marked.sum()) < B
  obs = ev.observation.clone()
  obs[marked] = float('nan')
  ts, actions = _record(env, twin, pop, obs, 7, 'after mark_reset', policy_index=pidx, temperature=4.0, sample_seed=77)
  assert bool((ts.step_type[0][marked] == 0).all()) and bool((actions[0][marked] == 0).all())
  assert not bool(torch.isnan(ts.observation).any())
  _mark_third(env, twin, 5)
  marked = _third(B, 5)
  obs = ts.observation[-1].clone()
  obs[marked] = float('nan')
  ev = _evaluate(env, twin, pop, obs, 7, 'evaluate after mark_reset', policy_index=pidx, temperature=4.0, sample_seed=77)
  assert not bool(torch.isnan(ev.observation).any())
  # interleaved with step, rollout, and sample_mlp
  obs = _one_more_step(env, twin, 'step')
  g = torch.Generator(device='cuda')
  g.manual_seed(4)
  acts = torch.randint(3, (5, B), generator=g, device='cuda', dtype=torch.int32)
  ro, rt = env.rollout(acts), twin.env.rollout(acts)
  twin.obs = rt.observation[-1].clone()
  ts, _ = _record(env, twin, one, ro.observation[-1], 7, 'after rollout', **how)
  twin.run(twin.sample('mlp', (w1, w2), None, 4.0, 77), 4)
  ts, _ = env.sample_mlp(w1, w2, ts.observation[-1], 4, temperature=4.0, sample_seed=77)
  _same(env, twin, 'sample_mlp')
  assert [t.data_ptr() for t in ts] == ptrs4[:4]
  _evaluate(env, twin, one, ts.observation[-1], 3, 'and back', temperature=0.25, sample_seed=77)
  _one_more_step(env, twin, 'last step')


# ---------------------------------------------------------------------------------------------- 7. large batches
def _large(fam, kwargs, record):
  B, T = (1 << 20) + 257, 2
  env, twin = _make(fam, kwargs, B), Sampler2(fam, kwargs, B)
  one = _triple(fam, 64, 64, 3)
  for k, obs in enumerate((_garbage(fam, B), None)):                        # (first never read: every lane resets)
    obs = twin.obs.clone() if obs is None else obs
    (_record if record else _evaluate)(env, twin, one, obs, T, (fam, 'large', k), temperature=1.0, sample_seed=BIG_SEED)


def test_large_batch_cartpole_evaluate_sampled():
  _large(*FAMILIES[0], record=False)


def test_large_batch_mountain_car_sample():
  _large(*FAMILIES[2], record=True)


# ---------------------------------------------------------------------------------------------- 8. the edge-state grid
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs', edges.CASE_PARAMS)
def test_both_calls_on_the_edge_state_grid(family, kwargs, T):
  """tests/test_gpu_physics_edges.py's test_closed_loop_calls_equal_the_eager_step for the two new calls, with its triple and
  its temperature and seed: the actions sample_mlp2 returns, replayed through the eager step() of a twin loaded with the same
  edge states, give its TimeSteps and its final state; evaluate_sampled_mlp2 ends in that state with the host loop's columns."""
  g = pu.grid(family, kwargs)
  B = g['lanes']
  D = dict(cartpole=6, cartpole_swingup=8, mountain_car=3)[family]
  gen = torch.Generator(device='cpu')
  gen.manual_seed(884)
  H1, H2 = 5, 4
  weights = tuple(torch.randn(shape, generator=gen).cuda().contiguous() for shape in ((H1, D + 1), (H2, H1 + 1), (3, H2 + 1)))
  obs = torch.randn((B, 1, D), generator=gen).cuda().contiguous()
  kw = dict(temperature=1.0, sample_seed=(1 << 40) + 77)
  what = (family, T, 'sample_mlp2')
  env = edges._make(family, kwargs, B)                                     # pylint: disable=protected-access
  pu.load(env, g)
  ts, actions = env.sample_mlp2(*weights, obs, T, **kw)
  assert set(actions[0].unique().tolist()) == {0, 1, 2}, what
  twin = edges._make(family, kwargs, B)                                    # pylint: disable=protected-access
  pu.load(twin, g)
  want = edges._stack([edges._snap_ts(twin.step(actions[t].contiguous())) for t in range(T)], T)   # pylint: disable=protected-access
  edges._assert_ts(edges._snap_ts(ts), want, what)                         # pylint: disable=protected-access
  want_after = edges._snap_after(twin)                                     # pylint: disable=protected-access
  edges._assert_after(edges._snap_after(env), want_after, what)            # pylint: disable=protected-access
  what = (family, T, 'evaluate_sampled_mlp2')
  env2 = edges._make(family, kwargs, B)                                    # pylint: disable=protected-access
  pu.load(env2, g)
  ev = env2.evaluate_sampled_mlp2(*weights, obs, T, **kw)
  edges._assert_after(edges._snap_after(env2), want_after, what)           # pylint: disable=protected-access
  st = ts.step_type.cpu().numpy()
  r64 = edges._f64_rewards(family, env, st, ts.reward.cpu().numpy(), actions.cpu().numpy())   # pylint: disable=protected-access
  n, total, done = pe.host_loop(st, r64)
  np.testing.assert_array_equal(ev.episodes.cpu().numpy(), n, err_msg=f'{what} episodes')
  np.testing.assert_array_equal(pe.bits(ev.return_sum.cpu().numpy()), pe.bits(total), err_msg=f'{what} return_sum')
  np.testing.assert_array_equal(pe.bits(ev.episode_return_sum.cpu().numpy()), pe.bits(done), err_msg=f'{what} episode_return_sum')
  assert torch.equal(_bits(ev.observation), _bits(ts.observation[-1])), (what, 'observation')
