"""GPU: sample_linear / sample_mlp — the closed loop of a linear or hidden-layer SOFTMAX agent on cartpole, swing-up and
mountain_car in one launch, writing the trajectory.  The twin method of tests/test_gpu_trajectory.py, whose helpers are
imported: a second environment of the same seed and lane offset runs the contract's eager loop — `a = 0 where the lane
resets, else gumbel_select(*_logits(policy[row], obs), words(sample_seed, lane, call index), temperature)` with the words
restated by oracle/stream.py (stream 3), `step(a)` — and keeps every TimeStep it got; step_type, reward, discount, observation
and the actions are compared bit for bit, and so is everything left behind.  Then the frequencies of the actions the device
draws under a known softmax, and the kernel that paid for the new one: the two launches of a group of mnist segments are one
merged kernel, exercised through bsx_group_step and through bsx_group_step_phase."""
import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import sweep
from bsuite_amd import sweep_batch as sb
from bsuite_amd.utils import datasets, observations
from oracle import stream
from tests import engine_util as eu
from tests import golden_util as gu
from tests.test_gpu_mlp_eval import HIDDEN, LONG, MAIN, OFFSET, SHORT, _bits, _garbage, _make, _one_more_step, _rows, _same, case_id
from tests.test_gpu_trajectory import FIELDS, Recorder, _equal_steps, _evaluate, _policy, _rollout, _state_of

pytestmark = pytest.mark.gpu

STREAM_SAMPLE = 3                             # BSX_STREAM_SAMPLE (include/bsx_stream.h)
KINDS = ['linear', 'mlp']
BATCHES, STEPS = [1, 257], [1, 9]
SEEDS = (77, (1 << 63) + 5)
TEMPERATURES = (0.25, 1.0, 4.0)
CASES = [pytest.param(kind, f, kw, T, B, HIDDEN[(fi + ti + bi) % 3], id=f'{kind}-{case_id(f, kw)}-T{T}-B{B}-H{HIDDEN[(fi + ti + bi) % 3]}')
         for kind in KINDS for fi, (f, kw) in enumerate(MAIN) for ti, T in enumerate(STEPS) for bi, B in enumerate(BATCHES)]


def _logits(kind, pol, obs):
  return observations.mlp_logits(pol[0], pol[1], obs) if kind == 'mlp' else observations.linear_logits(pol[0], obs)


def _greedy(logits):
  """The greedy rule of linear_select / mlp_select on logits [B, 3]."""
  best = torch.zeros(logits.shape[0], dtype=torch.int32, device=logits.device)
  l_best = logits[:, 0]
  for a in (1, 2):
    better = logits[:, a] > l_best
    best = torch.where(better, torch.full_like(best, a), best)
    l_best = torch.where(better, logits[:, a], l_best)
  return best


class Sampler(Recorder):
  """The eager twin of a sampled call: the recorder, selecting with *_logits + gumbel_select on the oracle's words.  The
  float64 part of the rule runs on the host (IEEE division), the float32 logits where the observation is."""

  def __init__(self, fam, kwargs, B):
    super().__init__(fam, kwargs, B)
    self.live_steps, self.off_greedy = 0, 0

  def sample(self, kind, pol, policy_index, temperature, sample_seed):
    own = tuple(w if w.dim() == 2 else _rows(w, policy_index, self.B) for w in pol)

    def select(obs, live):
      logits = _logits(kind, own, obs)
      words = stream.words(int(sample_seed), self.lanes, self.env.step_index, STREAM_SAMPLE, 3)
      a = observations.gumbel_select(logits.cpu(), words, temperature).cuda()
      self.live_steps += int(live.sum())
      self.off_greedy += int((a != _greedy(logits))[live].sum())
      return a
    return select


def _sample(env, kind, pol, obs, T, **kw):
  return (env.sample_mlp if kind == 'mlp' else env.sample_linear)(*pol, obs, T, **kw)


def _check(env, twin, kind, pol, obs, T, what, policy_index=None, temperature=1.0, sample_seed=0, defaults=False):
  """One sample_linear / sample_mlp call against the twin's eager loop of the same arguments; returns (ts, actions)."""
  twin.run(twin.sample(kind, pol, policy_index, temperature, sample_seed), T)
  kw = dict() if defaults else dict(temperature=temperature, sample_seed=sample_seed)
  ts, actions = _sample(env, kind, pol, obs, T, policy_index=policy_index, **kw)
  _equal_steps(ts, actions, twin.last(T), what)
  _same(env, twin, what)
  return ts, actions


# ---------------------------------------------------------------------------------------------- 1. against the eager twin
@pytest.mark.parametrize('kind,fam,kwargs,T,B,H', CASES)
def test_equals_the_eager_loop_of_a_twin(kind, fam, kwargs, T, B, H):
  env, twin = _make(fam, kwargs, B), Sampler(fam, kwargs, B)
  pol = _policy(kind, fam, H, 3)
  # 1. a fresh environment: every lane resets on the first step and its observation row is not read — garbage.  The defaults:
  #    temperature 1, seed 0
  ts, actions = _check(env, twin, kind, pol, _garbage(fam, B), T, (kind, fam, T, B, H, 'fresh'), defaults=True)
  assert bool((ts.step_type[0] == 0).all()) and bool((actions[0] == 0).all())
  n_last = int((ts.step_type == 2).sum())
  # 2. in the middle of its episodes, the last observation passed back in (a slice of the buffer the call overwrites)
  ts, actions = _check(env, twin, kind, pol, ts.observation[-1], T, (kind, fam, T, B, H, 'running'), temperature=1.0, sample_seed=SEEDS[0])
  n_last += int((ts.step_type == 2).sum())
  if B == 257 and T == 9:
    # the case samples — by the restatement alone: all three actions, and not the greedy policy
    assert twin.seen == {0, 1, 2}, twin.seen
    assert twin.off_greedy >= 0.05 * twin.live_steps, (twin.off_greedy, twin.live_steps)
  if kwargs and T == 9:
    assert n_last >= B                                                   # episodes end inside the calls
  # 3. [B, D] rows after a step(); a cold policy, the seed beyond 2^63
  obs = _one_more_step(env, twin, (kind, fam, T, B, H, 'one more step'))
  ts, _ = _check(env, twin, kind, pol, obs.reshape(B, -1), T, (kind, fam, T, B, H, 'after a step, [B, D] rows'), temperature=0.25,
                 sample_seed=SEEDS[1])
  # 4. a population of three with rows named outside [0, P-1], a hot policy
  g = torch.Generator(device='cuda')
  g.manual_seed(B + T)
  pop = _policy(kind, fam, H, 5, P=3)
  pidx = torch.randint(-1, 8, (B,), generator=g, device='cuda', dtype=torch.int32)
  pidx[0], pidx[-1] = 7, -1
  ts, _ = _check(env, twin, kind, pop, ts.observation[-1], T, (kind, fam, T, B, H, 'population'), policy_index=pidx, temperature=4.0,
                 sample_seed=SEEDS[0])
  # 5. one policy per lane
  each = _policy(kind, fam, H, 6, P=B)
  lanes = torch.arange(B, device='cuda', dtype=torch.int32) if B > 1 else None      # (P == 1: policy_index must be None)
  _check(env, twin, kind, each, ts.observation[-1], T, (kind, fam, T, B, H, 'one policy per lane'), policy_index=lanes, temperature=1.0,
         sample_seed=SEEDS[1])
  _one_more_step(env, twin, (kind, fam, T, B, H, 'last step'))
  assert int(env.episode_counters()[1]) >= B


# ---------------------------------------------------------------------------------------------- 2. calls compose
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam,kwargs,H', [(f, kw, HIDDEN[k % 3]) for k, (f, kw) in enumerate(LONG + SHORT)],
                         ids=[case_id(f, kw) for f, kw in LONG + SHORT])
def test_split_calls_replay_mark_reset_buffers_and_interleaving(kind, fam, kwargs, H):
  B = 257
  env, twin, replay = _make(fam, kwargs, B), Sampler(fam, kwargs, B), _make(fam, kwargs, B)
  pol = _policy(kind, fam, H, 8)
  how = dict(temperature=1.0, sample_seed=SEEDS[1])

  def replayed(ts, actions, what):
    """A third environment's rollout(actions) reproduces ts, and the state."""
    again = replay.rollout(actions)
    for f in FIELDS:
      assert torch.equal(_bits(getattr(again, f)), _bits(getattr(ts, f))), (kind, fam, what, f)
    _same(env, _state_of(replay), (kind, fam, what, 'replay'))

  # 3 + 4 steps leave what 7 leave, and the concatenated trajectories equal the whole
  a3 = _check(env, twin, kind, pol, _garbage(fam, B), 3, (kind, fam, 'first 3'), **how)
  replayed(*a3, 'first 3')
  parts = [[t.clone() for t in (*a3[0], a3[1])]]
  a4 = _check(env, twin, kind, pol, a3[0].observation[-1], 4, (kind, fam, 'then 4'), **how)
  replayed(*a4, 'then 4')
  parts.append([t.clone() for t in (*a4[0], a4[1])])
  whole, twin7 = _make(fam, kwargs, B), Sampler(fam, kwargs, B)
  w7 = _check(whole, twin7, kind, pol, _garbage(fam, B), 7, (kind, fam, 'whole 7'), **how)
  _same(env, twin7, (kind, fam, '3 + 4 == 7'))
  for k, t in enumerate((*w7[0], w7[1])):
    assert torch.equal(_bits(torch.cat([parts[0][k], parts[1][k]])), _bits(t)), (kind, fam, k)
  # the buffers are cached per T, and they are rollout_*'s
  ptrs3, ptrs4 = ([t.data_ptr() for t in (*a[0], a[1])] for a in (a3, a4))
  ts, actions = _check(env, twin, kind, pol, a4[0].observation[-1], 7, (kind, fam, 'seven more'), temperature=0.25, sample_seed=SEEDS[0])
  replayed(ts, actions, 'seven more')
  first7 = [t.data_ptr() for t in (*ts, actions)]
  assert not set(ptrs3) & set(ptrs4) and not set(first7) & set(ptrs3 + ptrs4)
  again4 = _check(env, twin, kind, pol, ts.observation[-1], 4, (kind, fam, 'four again'), temperature=4.0, sample_seed=SEEDS[0])
  replayed(*again4, 'four again')
  assert [t.data_ptr() for t in (*again4[0], again4[1])] == ptrs4
  twin.run(twin.select(kind, pol, None), 4)
  ts, actions = _rollout(env, kind, pol, again4[0].observation[-1], 4)
  _equal_steps(ts, actions, twin.last(4), (kind, fam, 'rollout_* of the same T'))
  replayed(ts, actions, 'greedy four')
  assert [t.data_ptr() for t in (*ts, actions)] == ptrs4                  # (shared with rollout_linear / rollout_mlp)
  assert twin.seen == {0, 1, 2}
  # mark_reset of a random third of the lanes between two calls: FIRST on step 0, action 0, their NaN rows never read
  g = torch.Generator(device='cuda')
  g.manual_seed(4)
  mask = torch.rand(B, generator=g, device='cuda') < 1.0 / 3.0
  for e in (env, twin.env, replay):
    e.mark_reset(mask)
  obs = ts.observation[-1].clone()
  obs[mask] = float('nan')
  ts, actions = _check(env, twin, kind, pol, obs, 7, (kind, fam, 'after mark_reset'), **how)
  replayed(ts, actions, 'after mark_reset')
  assert bool((ts.step_type[0][mask] == 0).all()) and bool((actions[0][mask] == 0).all())
  assert not bool(torch.isnan(ts.observation).any())
  _one_more_step(env, twin, (kind, fam, 'one more step'))
  # interleaved with rollout(): its last observation is the next call's input ...
  acts = torch.randint(3, (5, B), generator=g, device='cuda', dtype=torch.int32)
  ro, rt = env.rollout(acts), twin.env.rollout(acts)
  twin.obs = rt.observation[-1].clone()
  ts, _ = _check(env, twin, kind, pol, ro.observation[-1], 7, (kind, fam, 'after rollout'), **how)
  # ... with the greedy recording call of the other kind, with evaluate_mlp, and with the other kind of sampled call
  lin, mlp = _policy('linear', fam, H, 9), _policy('mlp', fam, H, 10)
  other = 'mlp' if kind == 'linear' else 'linear'
  twin.run(twin.select(other, lin if other == 'linear' else mlp, None), 5)
  ts, actions = _rollout(env, other, lin if other == 'linear' else mlp, ts.observation[-1], 5)
  _equal_steps(ts, actions, twin.last(5), (kind, fam, 'rollout of the other kind'))
  twin.run(twin.select('mlp', mlp, None), 4)
  ev = _evaluate(env, 'mlp', mlp, ts.observation[-1], 4)
  _same(env, twin, (kind, fam, 'evaluate_mlp'))
  ts, _ = _check(env, twin, other, lin if other == 'linear' else mlp, ev.observation, 7, (kind, fam, 'the other sampled call'), **how)
  assert [t.data_ptr() for t in ts] == first7[:4]                          # (the two sampled calls share their buffers)
  _check(env, twin, kind, pol, ts.observation[-1], 3, (kind, fam, 'and back'), temperature=4.0, sample_seed=SEEDS[0])
  _one_more_step(env, twin, (kind, fam, 'last step'))


# ---------------------------------------------------------------------------------------------- 3. frequencies on the device
def test_action_frequencies_of_a_known_softmax():
  """MountainCar under a shared linear policy with zero weights and the biases (0, ln 2, ln 4): every live lane-step draws from
  (1/7, 2/7, 4/7).  B = 4096, T = 17: step 0 resets (action 0, nothing drawn), the 16 others are live — episodes of 1000 steps
  do not end.  The layout is verified with the restatement first, on the host; the device then has to reproduce it exactly."""
  B, T, seed = 4096, 17, 2
  w = torch.zeros((3, 4), dtype=torch.float32)
  w[1, 3], w[2, 3] = float(np.float32(np.log(2.0))), float(np.float32(np.log(4.0)))
  lanes = np.uint64(OFFSET) + np.arange(B, dtype=np.uint64)
  logits = w[:, 3].unsqueeze(0).expand(B, 3).contiguous()
  want = torch.stack([torch.zeros(B, dtype=torch.int32)] +
                     [observations.gumbel_select(logits, stream.words(seed, lanes, t, STREAM_SAMPLE, 3)) for t in range(1, T)])
  l64 = w[:, 3].to(torch.float64).numpy()
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
  ts, actions = env.sample_linear(w.cuda(), _garbage('mountain_car', B), T, sample_seed=seed)
  assert bool((ts.step_type[0] == 0).all()) and bool((ts.step_type[1:] == 1).all())
  assert torch.equal(actions.cpu(), want)
  within(actions.cpu(), 'device')


# ---------------------------------------------------------------------------------------------- 4. what paid for the kernel
@pytest.mark.parametrize('through', ['bsx_group_step', 'bsx_group_step_phase'])
def test_the_merged_cold_kernel_steps_a_group_of_mnist_segments(tmp_path, through):
  """A launch group of mnist segments alone (the sweep without its mixed groups) advances its lanes and writes its observations
  with ONE kernel now, its phase a uniform switch: through bsx_group_step (both launches) and through bsx_group_step_phase
  (phase 0, then phase 1, as the two-stream schedule issues them) the segments equal stand-alone environments.  B = 300 per
  segment: a ragged second workgroup."""
  imgs, labels = gu.mnist_dataset()
  datasets.write_idx_files(str(tmp_path), imgs.view(np.uint8), labels)
  mn = dict(data_dir=str(tmp_path))
  kw = dict(mnist=mn, mnist_scale=mn)
  ids, seed, reps = ['mnist/0', 'mnist_scale/3'], 31, 5
  batch = sb.SweepBatch(ids, 600, seed=seed, env_kwargs=kw)
  assert [s[2] for s in batch.segments] == [300, 300]
  acts = batch.random_actions(seed=3)
  outs = batch.prepare_groups(acts, mix_small=False, mix_pairs=False, mix_all=False)
  assert len(batch._groups) == 1                                          # pylint: disable=protected-access
  for _ in range(reps):
    if through == 'bsx_group_step':
      batch.step_grouped()
    else:
      batch.step_grouped_streams()
  if through != 'bsx_group_step':
    batch.join_streams()
  batch.sync()
  for (bid, begin, lanes), a, out, env in zip(batch.segments, acts, outs, batch.envs):
    name = bid.split('/')[0]
    ekw = dict(kw[name])
    if sweep.SETTINGS[bid].get('seed', 0) is None or 'seed' not in sweep.SETTINGS[bid]:
      ekw['seed'] = seed
    ref = bsuite_amd.load_from_id(bid, batch=lanes, lane_offset=begin, num_buffers=1, **ekw)
    for _ in range(reps):
      ts = ref.step(a)
    for x, y in zip(eu.to_np(out), eu.to_np(ts)):
      np.testing.assert_array_equal(x, y, err_msg=bid)
    for k, v in ref.bsuite_info().items():
      torch.testing.assert_close(env.bsuite_info()[k], v, rtol=0, atol=0)
    torch.testing.assert_close(eu.raw(env).episode_counters(), eu.raw(ref).episode_counters(), rtol=0, atol=0)
  batch.release_groups()
