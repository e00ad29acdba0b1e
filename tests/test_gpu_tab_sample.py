"""GPU: sample_policy / evaluate_sampled_policy — T closed-loop steps of deep_sea / catch in ONE launch, the actions drawn
inside the kernel from softmax(logits[row, key] / temperature) by Gumbel-max on stream 3.  Against the loop the contract
restates — a = 0 where the lane resets, else gumbel_select(logits[row, key(observation before the call)], words, temperature),
then step(a) — run on a twin environment of the same seed through the eager step(), the words from oracle/stream.py: everything
returned and everything left behind bit for bit, at one lane and at a ragged second workgroup, lane ids crossing 2^32, a table
in LDS and one read from global memory, populations with wild indices and one table per lane; a replay of the actions through
rollout(); the returns-only call against the contract's loop over float64 rewards that never come from the engine (the C
oracle's for deep_sea); logits at a 4-byte offset; a masked action; chained calls; the device's action frequencies against the
restatement's, exactly; and the folded cold kernel that paid for the new one, through its unchanged entry points."""
import types

import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import sweep
from bsuite_amd import sweep_batch as sb
from bsuite_amd.utils import observations
from oracle import stream as S
from tests import engine_util as eu
from tests import policy_eval_util as pe
from tests import tab_sample_util as tu
from tests.test_gpu_policy_eval import OFFSET, Ref, _make, _same_columns, _same_envs
from tests.test_gpu_policy_rollout import RESET_BIT

pytestmark = pytest.mark.gpu

FAMILIES = [('deep_sea', dict(size=4, mapping_seed=42)),                       # episodes end inside a call
            ('deep_sea', dict(size=6, deterministic=False, mapping_seed=1)),
            ('deep_sea', dict(size=40, mapping_seed=3)),                       # 12800 bytes: the smallest table read from global memory
            ('catch', dict())]
IDS = ['deep_sea_4', 'deep_sea_stochastic', 'deep_sea_40_global_table', 'catch']
LDS_BYTES = 12288


def _logits(env, seed, P=None, scale=2.0):
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  shape = (env.policy_num_states, env.action_spec().num_values)
  return torch.randn(shape if P is None else (P,) + shape, generator=g, device='cuda', dtype=torch.float32) * scale


class Twin:
  """The loop of the contract on an environment of the same seed, through the eager step()."""

  def __init__(self, fam, env):
    self.fam, self.env, self.obs = fam, env, None
    self.lanes = np.uint64(env.lane_offset) + np.arange(env.batch_size, dtype=np.uint64)

  def note(self, ts, rollout=False):
    self.obs = (ts.observation[-1] if rollout else ts.observation).clone()

  def sample_policy(self, logits, T, policy_index=None, temperature=1.0, sample_seed=0):
    env, B = self.env, self.env.batch_size
    Sn, A = logits.shape[-2:]
    logits = logits.reshape(-1, Sn, A)
    P = logits.shape[0]
    row = policy_index.clamp(0, P - 1).to(torch.int64) if policy_index is not None else torch.zeros(B, dtype=torch.int64, device='cuda')
    out = dict(step_type=[], reward=[], discount=[], observation=[], actions=[])
    for _ in range(T):
      if not env._allocated:                   # pylint: disable=protected-access
        resets = torch.ones(B, dtype=torch.bool, device='cuda')
        key = torch.zeros(B, dtype=torch.int64, device='cuda')
        step = env.step_index
      else:
        resets = (env._state['state'] & RESET_BIT[self.fam]) != 0      # pylint: disable=protected-access
        key = (observations.policy_key(self.obs, env.board_shape).clamp(0, Sn - 1) if self.obs is not None
               else torch.zeros(B, dtype=torch.int64, device='cuda'))
        step = env.device_step_index()
      words = S.words(sample_seed, self.lanes, step, tu.STREAM_SAMPLE, A)
      a = observations.gumbel_select(logits[row, key], words, temperature)
      a = torch.where(resets, torch.zeros_like(a), a)
      ts = env.step(a)
      self.note(ts)
      for k in ('step_type', 'reward', 'discount', 'observation'):
        out[k].append(getattr(ts, k).clone())
      out['actions'].append(a)
    return {k: torch.stack(v) for k, v in out.items()}


def _same_outputs(got, want, what):
  ts, actions = got
  assert actions.dtype is torch.int32 and ts.step_type.dtype is torch.int8 and ts.observation.dtype is torch.int32, what
  assert ts.reward.dtype is torch.float32 and ts.discount.dtype is torch.float32, what
  assert torch.equal(actions, want['actions']), what
  assert torch.equal(ts.step_type, want['step_type']), what
  assert torch.equal(ts.reward.view(torch.int32), want['reward'].view(torch.int32)), what
  assert torch.equal(ts.discount, want['discount']), what
  assert torch.equal(ts.observation, want['observation']), what


class Quad:
  """The environment under test, the eager twin, an environment that replays the actions through rollout(), one that takes
  the same steps through evaluate_sampled_policy, and the float64 rewards of those steps."""

  def __init__(self, fam, kwargs, B):
    self.fam = fam
    self.env, self.replay, self.ev = (_make(fam, kwargs, B, lane_offset=OFFSET) for _ in range(3))
    self.twin = Twin(fam, _make(fam, kwargs, B, lane_offset=OFFSET))
    self.ref = Ref(fam, kwargs, B)

  def check(self, logits, T, what, **kw):
    got = self.env.sample_policy(logits, T, **kw)
    _same_outputs(got, self.twin.sample_policy(logits, T, **kw), what)
    peer = types.SimpleNamespace(env=self.twin.env)
    _same_envs(self.env, peer, what)
    ts, actions = got
    # stream 0 is untouched: the actions replayed through rollout() give the same TimeSteps
    again = self.replay.rollout(actions) if T > 1 else self.replay.step(actions[0])
    for k in ('step_type', 'discount', 'observation'):
      assert torch.equal(getattr(again, k).reshape(getattr(ts, k).shape), getattr(ts, k)), (what, k)
    assert torch.equal(again.reward.reshape(ts.reward.shape).view(torch.int32), ts.reward.view(torch.int32)), what
    # the returns-only call: the contract's loop over f64 rewards, and the same state afterwards
    ev = self.ev.evaluate_sampled_policy(logits, T, **kw)
    st, r64 = self.ref.rewards(ts, actions)
    want = pe.host_loop(st, r64)
    np.testing.assert_array_equal(want[0], (st == 2).sum(axis=0))
    _same_columns(ev, want, what)
    _same_envs(self.ev, peer, what)
    return ts, actions, ev


@pytest.mark.parametrize('B', [1, 257])
@pytest.mark.parametrize('T', [1, 11])
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=IDS)
def test_equals_the_eager_loop_of_the_contract_on_a_twin(fam, kwargs, T, B):
  q = Quad(fam, kwargs, B)
  env = q.env
  Sn, A = env.policy_num_states, env.action_spec().num_values
  assert A == (3 if fam == 'catch' else 2)
  assert (Sn * A * 4 > LDS_BYTES) == (kwargs.get('size') == 40)                  # which look-up the shared table takes
  g = torch.Generator(device='cuda')
  g.manual_seed(B + T)
  table = _logits(env, 5)
  ts, _, _ = q.check(table, T, (fam, T, B, 'fresh, defaults'))                    # 1. a fresh batch with the defaults
  assert bool((ts.step_type[0] == 0).all())
  q.check(table, T, (fam, T, B, 'running'))                                       # 2. a running batch
  q.check(table, T, (fam, T, B, 'cold, large seed'), temperature=0.25, sample_seed=(1 << 63) + 12345)                   # 3.
  pop = _logits(env, 6, P=3)                                                      # 4. a population, wild indices, hot
  pidx = torch.randint(-3, 7, (B,), generator=g, device='cuda', dtype=torch.int32)
  if B > 4:
    pidx[0], pidx[1], pidx[2], pidx[3] = -(1 << 31), (1 << 31) - 1, 3, -1
  q.check(pop, T, (fam, T, B, 'population'), policy_index=pidx, temperature=4.0, sample_seed=77)
  each = _logits(env, 7, P=max(B, 2))                                             # 5. one table per lane
  own = torch.arange(B, device='cuda', dtype=torch.int32)
  q.check(each, T, (fam, T, B, 'one table per lane'), policy_index=own, sample_seed=3)
  assert env.step_index == 5 * T and int(env.episode_counters()[1]) >= B


@pytest.mark.parametrize('fam,kwargs', [FAMILIES[1], FAMILIES[2], FAMILIES[3]], ids=[IDS[1], IDS[2], IDS[3]])
def test_logits_at_a_four_byte_offset(fam, kwargs):
  """A view that starts one float into a buffer (4-byte, not 8-byte aligned) gives what an aligned copy gives: a shared table
  (staged in LDS, or read from global memory at size 40) and a population, for both values of A."""
  B, T = 257, 11
  envs = [_make(fam, kwargs, B, lane_offset=OFFSET) for _ in range(4)]
  Sn, A = envs[0].policy_num_states, envs[0].action_spec().num_values
  for P, (a, b) in ((None, envs[:2]), (2, envs[2:])):
    n = Sn * A * (P or 1)
    buf = _logits(a, 21, P=P).reshape(-1)
    shifted = torch.empty(n + 1, device='cuda', dtype=torch.float32)
    view = shifted[1:]
    view.copy_(buf)
    view = view.reshape((Sn, A) if P is None else (P, Sn, A))
    assert view.is_contiguous() and view.data_ptr() % 8 == 4 and buf.data_ptr() % 16 == 0
    kw = dict(temperature=0.5, sample_seed=9)
    if P is not None:
      kw['policy_index'] = (torch.arange(B, device='cuda', dtype=torch.int32) % P)
    ts, actions = a.sample_policy(view, T, **kw)
    want_ts, want_actions = b.sample_policy(buf.reshape(view.shape), T, **kw)
    assert torch.equal(actions, want_actions) and torch.equal(ts.observation, want_ts.observation)
    assert torch.equal(ts.reward.view(torch.int32), want_ts.reward.view(torch.int32))
    assert sorted(set(actions[ts.step_type != 0].tolist())) == list(range(A))
    ev_a, ev_b = a.evaluate_sampled_policy(view, T, **kw), None
    kept = [x.clone() for x in ev_a]
    ev_b = b.evaluate_sampled_policy(buf.reshape(view.shape), T, **kw)
    for x, y in zip(kept, ev_b):
      assert torch.equal(x, y)
    assert torch.equal(a._state['state'], b._state['state'])                       # pylint: disable=protected-access


@pytest.mark.parametrize('fam,kwargs', [FAMILIES[0], FAMILIES[2], FAMILIES[3]], ids=[IDS[0], IDS[2], IDS[3]])
def test_a_minus_infinity_column_masks_its_action(fam, kwargs):
  B, T = 257, 11
  env = _make(fam, kwargs, B, lane_offset=OFFSET)
  table = _logits(env, 8)
  table[:, 0] = float('-inf')
  ts, actions = env.sample_policy(table, T, temperature=4.0, sample_seed=5)
  live = ts.step_type != 0
  assert int(live.sum()) > 0 and bool((actions[live] != 0).all()) and bool((actions[~live] == 0).all())
  # ... and with every column masked nothing beats action 0
  table[:] = float('-inf')
  _, actions = env.sample_policy(table, T)
  assert bool((actions == 0).all())


@pytest.mark.parametrize('fam,kwargs', [FAMILIES[1], FAMILIES[3]], ids=[IDS[1], IDS[3]])
def test_calls_chain_with_step_mark_reset_rollout_policy_and_evaluate_policy(fam, kwargs):
  B = 257
  q = Quad(fam, kwargs, B)
  env, twin, peers = q.env, q.twin, (q.replay, q.ev)
  na = env.action_spec().num_values
  table = _logits(env, 9)
  greedy = torch.argmax(table, dim=1).to(torch.uint8)
  g = torch.Generator(device='cuda')
  g.manual_seed(3)
  q.check(table, 5, (fam, 'first'))
  # step
  a = torch.randint(na, (B,), generator=g, device='cuda', dtype=torch.int32)
  twin.note(twin.env.step(a))
  for e in (env,) + peers:
    e.step(a)
  q.ref.step(a)
  q.check(table, 4, (fam, 'after step'), sample_seed=1)
  # mark_reset
  mask = torch.rand(B, generator=g, device='cuda') < 0.3
  for e in (env, twin.env, q.ref) + peers:
    e.mark_reset(mask)
  ts, actions, _ = q.check(table, 6, (fam, 'after mark_reset'), temperature=2.0)
  assert bool((ts.step_type[0][mask] == 0).all()) and bool((actions[0][mask] == 0).all())
  # rollout_policy: the greedy call, on every environment
  got = env.rollout_policy(greedy, 3)
  twin.note(twin.env.rollout_policy(greedy, 3)[0], rollout=True)
  for e in peers:
    e.rollout_policy(greedy, 3)
  q.ref.rewards(*got)
  q.check(table, 4, (fam, 'after rollout_policy'), sample_seed=2)
  # evaluate_policy: its cached columns are the ones evaluate_sampled_policy returns
  ev = env.evaluate_policy(greedy, 3)
  ts_g, acts_g = twin.env.rollout_policy(greedy, 3)
  twin.note(ts_g, rollout=True)
  for e in peers:
    e.evaluate_policy(greedy, 3)
  q.ref.rewards(ts_g, acts_g)
  _, _, ev2 = q.check(table, 7, (fam, 'after evaluate_policy'), sample_seed=4)
  assert ev2.episodes.data_ptr() == q.ev.evaluate_policy(greedy, 1).episodes.data_ptr() and ev.episodes.shape == (B,)
  # the per-T buffers are rollout_policy's
  e2 = _make(fam, kwargs, B)
  assert e2.sample_policy(table, 3)[1].data_ptr() == e2.rollout_policy(greedy, 3)[1].data_ptr()


@pytest.mark.parametrize('A', [2, 3])
def test_the_devices_action_frequencies_are_the_restatements(A):
  """The frequency case (tests/tab_sample_util.py; the CPU test holds the restatement's counts within 4 sigma of the softmax):
  constant rows, 4096 lanes from lane 2^32 - 17 on, one fresh call of 11 steps — the device's actions on the live steps are the
  restatement's, lane by lane, so the counts are equal exactly."""
  fam, kwargs = tu.FREQ_FAMILY[A]
  env = _make(fam, kwargs, tu.FREQ_B, lane_offset=tu.FREQ_LANE0)
  assert env.action_spec().num_values == A
  table = torch.from_numpy(tu.freq_row(A)).cuda().repeat(env.policy_num_states, 1).contiguous()
  ts, actions = env.sample_policy(table, tu.FREQ_T, temperature=1.0, sample_seed=tu.FREQ_SEED[A])
  live = (ts.step_type != 0).cpu().numpy()
  want_live = np.zeros(tu.FREQ_T, bool)
  want_live[list(tu.FREQ_LIVE[A])] = True
  np.testing.assert_array_equal(live, np.broadcast_to(want_live[:, None], live.shape))          # no lane resets on a live call index
  got = actions.cpu().numpy()
  want = tu.restated_actions(A)
  np.testing.assert_array_equal(got[list(tu.FREQ_LIVE[A])], want)
  assert (got[~want_live] == 0).all()
  counts = np.bincount(got[live], minlength=A)
  np.testing.assert_array_equal(counts, tu.restated_counts(A))
  print('A', A, 'device counts', counts)


# ---------------------------------------------------------------------------------------------- what paid for the kernel
@pytest.mark.parametrize('through', ['bsx_group_step', 'bsx_group_step_phase'])
def test_the_folded_cold_kernel_advances_single_family_groups(through):
  """Launch groups of deep_sea segments alone and of catch segments alone (the sweep without its mixed groups) advance their
  lanes with ONE kernel now, the family a uniform switch: through bsx_group_step and through bsx_group_step_phase the segments
  equal stand-alone environments.  B = 300 per segment: a ragged second workgroup."""
  ids, seed, reps = ['deep_sea/0', 'deep_sea/3', 'catch/0', 'catch/1'], 31, 13
  batch = sb.SweepBatch(ids, 1200, seed=seed)
  assert [s[2] for s in batch.segments] == [300] * 4
  acts = batch.random_actions(seed=3)
  outs = batch.prepare_groups(acts, mix_small=False, mix_pairs=False, mix_all=False)
  assert len(batch._groups) == 2                                          # pylint: disable=protected-access
  for _ in range(reps):
    if through == 'bsx_group_step':
      batch.step_grouped()
    else:
      batch.step_grouped_streams()
  if through != 'bsx_group_step':
    batch.join_streams()
  batch.sync()
  for (bid, begin, lanes), a, out, env in zip(batch.segments, acts, outs, batch.envs):
    ekw = {}
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
  assert int(eu.raw(batch.envs[0]).episode_counters()[0]) > 0               # episodes ended inside the run
  batch.release_groups()
