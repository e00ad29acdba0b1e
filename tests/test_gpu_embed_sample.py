"""GPU: sample_embedding / evaluate_sampled_embedding — T closed-loop steps of deep_sea / catch in ONE launch, the actions drawn
inside the kernel from softmax(logits / temperature) of a one-hidden-layer network on the lane's index row, by Gumbel-max on
stream 3.  Against the loop the contract restates — a = 0 where the lane resets, else gumbel_select(embedding_logits(w1, w2,
observation before the call), words, temperature), then step(a) — run on a twin environment of the same seed through the eager
step(), the words from oracle/stream.py: everything returned and everything left behind bit for bit, at one lane and at a ragged
second workgroup, lane ids crossing 2^32, H in {1, 5, 64}, a pair staged in LDS and the smallest one that is read from global
memory, populations with wild indices and one pair per lane; a replay of the actions through rollout(); the returns-only call
against the contract's loop over float64 rewards that never come from the engine; matrices at a 4-byte offset; masked actions;
chained calls; and the greedy calls of the same kernel after a drawn one."""
import types

import numpy as np
import pytest
import torch

from bsuite_amd.utils import observations
from oracle import stream as S
from tests import embed_sample_util as su
from tests import embed_util as mu
from tests import policy_eval_util as pe
from tests import tab_sample_util as tu
from tests.test_gpu_policy_eval import OFFSET, SEED, Ref, _make, _same_columns, _same_envs
from tests.test_gpu_policy_rollout import RESET_BIT, _table

pytestmark = pytest.mark.gpu

assert (OFFSET, SEED) == (mu.LANE0, mu.ENV_SEED)
IDS = [c[0] for c in su.CASES]
BY_NAME = {c[0]: c for c in su.CASES}


def _pair(name, seed=None, P=None):
  _, fam, kwargs, H = BY_NAME[name]
  C, _, A = mu.geometry(fam, kwargs)
  w1, w2 = mu.pair(C, A, H, su.PAIR_SEED[name] if seed is None else seed, P)
  return torch.from_numpy(w1).cuda(), torch.from_numpy(w2).cuda()


class Twin:
  """The loop of the contract on an environment of the same seed, through the eager step().  It keeps what the drawn calls saw
  on live steps: the actions and the signs of the pre-activations."""

  def __init__(self, fam, env):
    self.fam, self.env, self.obs = fam, env, None
    self.lanes = np.uint64(env.lane_offset) + np.arange(env.batch_size, dtype=np.uint64)
    self.seen, self.positive, self.negative = set(), False, False

  def note(self, ts, rollout=False):
    self.obs = (ts.observation[-1] if rollout else ts.observation).clone()

  def sample_embedding(self, w1, w2, T, policy_index=None, temperature=1.0, sample_seed=0):
    env, B = self.env, self.env.batch_size
    A = env.action_spec().num_values
    K = 1 if self.fam == 'deep_sea' else 2
    if w1.dim() == 3:
      row = policy_index.clamp(0, w1.shape[0] - 1).to(torch.int64)
      w1, w2 = w1[row], w2[row]                                           # lane b's own pair
    out = dict(step_type=[], reward=[], discount=[], observation=[], actions=[])
    for _ in range(T):
      if not env._allocated:                   # pylint: disable=protected-access
        resets = torch.ones(B, dtype=torch.bool, device='cuda')
        step = env.step_index
      else:
        resets = (env._state['state'] & RESET_BIT[self.fam]) != 0      # pylint: disable=protected-access
        step = env.device_step_index()
      obs = self.obs if self.obs is not None else torch.zeros((B, K), dtype=torch.int32, device='cuda')
      logits, s = observations.embedding_logits(w1, w2, obs, return_preactivations=True)
      words = S.words(sample_seed, self.lanes, step, tu.STREAM_SAMPLE, A)
      a = observations.gumbel_select(logits, words, temperature)
      live = ~resets
      if bool(live.any()):
        self.seen |= set(a[live].tolist())
        self.positive |= bool((s[live] > 0).any())
        self.negative |= bool((s[live] < 0).any())
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
  the same steps through evaluate_sampled_embedding, and the float64 rewards of those steps."""

  def __init__(self, fam, kwargs, B):
    self.fam = fam
    self.env, self.replay, self.ev = (_make(fam, kwargs, B, lane_offset=OFFSET) for _ in range(3))
    self.twin = Twin(fam, _make(fam, kwargs, B, lane_offset=OFFSET))
    self.ref = Ref(fam, kwargs, B)

  def check(self, w1, w2, T, what, **kw):
    got = self.env.sample_embedding(w1, w2, T, **kw)
    _same_outputs(got, self.twin.sample_embedding(w1, w2, T, **kw), what)
    peer = types.SimpleNamespace(env=self.twin.env)
    _same_envs(self.env, peer, what)
    ts, actions = got
    # stream 0 is untouched: the actions replayed through rollout() give the same TimeSteps
    again = self.replay.rollout(actions) if T > 1 else self.replay.step(actions[0])
    for k in ('step_type', 'discount', 'observation'):
      assert torch.equal(getattr(again, k).reshape(getattr(ts, k).shape), getattr(ts, k)), (what, k)
    assert torch.equal(again.reward.reshape(ts.reward.shape).view(torch.int32), ts.reward.view(torch.int32)), what
    # the returns-only call: the contract's loop over f64 rewards, and the same state afterwards
    ev = self.ev.evaluate_sampled_embedding(w1, w2, T, **kw)
    st, r64 = self.ref.rewards(ts, actions)
    want = pe.host_loop(st, r64)
    np.testing.assert_array_equal(want[0], (st == 2).sum(axis=0))
    _same_columns(ev, want, what)
    _same_envs(self.ev, peer, what)
    return ts, actions, ev


@pytest.mark.parametrize('B', [1, 257])
@pytest.mark.parametrize('T', [1, 11])
@pytest.mark.parametrize('name', IDS)
def test_equals_the_eager_loop_of_the_contract_on_a_twin(name, T, B):
  _, fam, kwargs, H = BY_NAME[name]
  q = Quad(fam, kwargs, B)
  env = q.env
  C, _, A = mu.geometry(fam, kwargs)
  assert (C, A) == (int(np.prod(env.board_shape)), env.action_spec().num_values) and A == (3 if fam == 'catch' else 2)
  assert (mu.staged_bytes(C, H) > mu.LDS_BYTES) == name.endswith('_global')       # which look-up the shared pair takes
  g = torch.Generator(device='cuda')
  g.manual_seed(B + T)
  w1, w2 = _pair(name)
  assert tuple(w1.shape) == (C + 2, H) and tuple(w2.shape) == (A, H + 1)
  ts, _, _ = q.check(w1, w2, T, (name, T, B, 'fresh, defaults'))                  # 1. a fresh batch with the defaults
  assert bool((ts.step_type[0] == 0).all())
  q.check(w1, w2, T, (name, T, B, 'running'))                                     # 2. a running batch
  if (T, B) == (11, 257):
    # every action on live steps and both signs of pre-activation, on the twin's side: the weight seed was chosen so that these
    # two calls alone show them (tests/embed_sample_util.py; test_embed_sample_host.py repeats that on the C oracle)
    assert sorted(q.twin.seen) == list(range(A)) and q.twin.positive and q.twin.negative, (q.twin.seen, q.twin.positive, q.twin.negative)
  q.check(w1, w2, T, (name, T, B, 'cold, large seed'), temperature=0.25, sample_seed=(1 << 63) + 12345)                # 3.
  p1, p2 = _pair(name, seed=6, P=3)                                               # 4. a population, wild indices, hot
  pidx = torch.randint(-3, 7, (B,), generator=g, device='cuda', dtype=torch.int32)
  if B > 4:
    pidx[0], pidx[1], pidx[2], pidx[3] = -(1 << 31), (1 << 31) - 1, 3, -1
  q.check(p1, p2, T, (name, T, B, 'population'), policy_index=pidx, temperature=4.0, sample_seed=77)
  e1, e2 = _pair(name, seed=7, P=max(B, 2))                                       # 5. one pair per lane
  own = torch.arange(B, device='cuda', dtype=torch.int32)
  q.check(e1, e2, T, (name, T, B, 'one pair per lane'), policy_index=own, sample_seed=3)
  assert env.step_index == 5 * T and int(env.episode_counters()[1]) >= B


@pytest.mark.parametrize('name', ['deep_sea_stochastic_h5', 'deep_sea_8_h64_global', 'catch_h64', 'catch_h1'])
def test_matrices_at_a_four_byte_offset(name):
  """Views that start one float into a buffer (4-byte, not 8-byte aligned) give what aligned copies give: a shared pair (staged
  in LDS, or read from global memory) and a population, for both families; every action is seen on live steps."""
  _, fam, kwargs, _ = BY_NAME[name]
  B, T = 257, 11
  envs = [_make(fam, kwargs, B, lane_offset=OFFSET) for _ in range(4)]
  A = envs[0].action_spec().num_values

  def shifted(x):
    buf = torch.empty(x.numel() + 1, device='cuda', dtype=torch.float32)
    view = buf[1:]
    view.copy_(x.reshape(-1))
    view = view.reshape(x.shape)
    assert view.is_contiguous() and view.data_ptr() % 8 == 4 and x.data_ptr() % 16 == 0
    return view

  for P, (a, b) in ((None, envs[:2]), (2, envs[2:])):
    w1, w2 = _pair(name, P=P)
    v1, v2 = shifted(w1), shifted(w2)
    kw = dict(temperature=0.5, sample_seed=9)
    if P is not None:
      kw['policy_index'] = (torch.arange(B, device='cuda', dtype=torch.int32) % P)
    ts, actions = a.sample_embedding(v1, v2, T, **kw)
    want_ts, want_actions = b.sample_embedding(w1, w2, T, **kw)
    assert torch.equal(actions, want_actions) and torch.equal(ts.observation, want_ts.observation)
    assert torch.equal(ts.reward.view(torch.int32), want_ts.reward.view(torch.int32))
    assert sorted(set(actions[ts.step_type != 0].tolist())) == list(range(A))
    kept = [x.clone() for x in a.evaluate_sampled_embedding(v1, v2, T, **kw)]
    for x, y in zip(kept, b.evaluate_sampled_embedding(w1, w2, T, **kw)):
      assert torch.equal(x, y)
    assert torch.equal(a._state['state'], b._state['state'])                       # pylint: disable=protected-access


@pytest.mark.parametrize('name', ['deep_sea_4_h5', 'deep_sea_8_h64_global', 'catch_h64'])
def test_a_minus_infinity_bias_masks_its_action(name):
  _, fam, kwargs, H = BY_NAME[name]
  B, T = 257, 11
  env = _make(fam, kwargs, B, lane_offset=OFFSET)
  w1, w2 = _pair(name)
  w2[0, H] = float('-inf')
  ts, actions = env.sample_embedding(w1, w2, T, temperature=4.0, sample_seed=5)
  live = ts.step_type != 0
  assert int(live.sum()) > 0 and bool((actions[live] != 0).all()) and bool((actions[~live] == 0).all())
  # ... and with every bias masked nothing beats action 0
  w2[:, H] = float('-inf')
  _, actions = env.sample_embedding(w1, w2, T)
  assert bool((actions == 0).all())


@pytest.mark.parametrize('name', ['deep_sea_stochastic_h5', 'catch_h5'])
def test_calls_chain_with_step_mark_reset_the_greedy_and_the_tabular_calls(name):
  _, fam, kwargs, _ = BY_NAME[name]
  B = 257
  q = Quad(fam, kwargs, B)
  env, twin, peers = q.env, q.twin, (q.replay, q.ev)
  na = env.action_spec().num_values
  w1, w2 = _pair(name)
  table = _table(env, 9)
  logits = torch.randn((env.policy_num_states, na), device='cuda', dtype=torch.float32)
  g = torch.Generator(device='cuda')
  g.manual_seed(3)
  q.check(w1, w2, 5, (name, 'first'))
  # step
  a = torch.randint(na, (B,), generator=g, device='cuda', dtype=torch.int32)
  twin.note(twin.env.step(a))
  for e in (env,) + peers:
    e.step(a)
  q.ref.step(a)
  q.check(w1, w2, 4, (name, 'after step'), sample_seed=1)
  # mark_reset
  mask = torch.rand(B, generator=g, device='cuda') < 0.3
  for e in (env, twin.env, q.ref) + peers:
    e.mark_reset(mask)
  ts, actions, _ = q.check(w1, w2, 6, (name, 'after mark_reset'), temperature=2.0)
  assert bool((ts.step_type[0][mask] == 0).all()) and bool((actions[0][mask] == 0).all())
  # rollout_embedding: the greedy call of the same kernel, on every environment
  got = env.rollout_embedding(w1, w2, 3, epsilon=0.2, explore_seed=5)
  twin.note(twin.env.rollout_embedding(w1, w2, 3, epsilon=0.2, explore_seed=5)[0], rollout=True)
  for e in peers:
    e.rollout_embedding(w1, w2, 3, epsilon=0.2, explore_seed=5)
  q.ref.rewards(*got)
  q.check(w1, w2, 4, (name, 'after rollout_embedding'), sample_seed=2)
  # evaluate_embedding: its cached columns are evaluate_policy's, the ones evaluate_sampled_embedding returns
  ev = env.evaluate_embedding(w1, w2, 3)
  ts_g, acts_g = twin.env.rollout_embedding(w1, w2, 3)
  twin.note(ts_g, rollout=True)
  for e in peers:
    e.evaluate_embedding(w1, w2, 3)
  q.ref.rewards(ts_g, acts_g)
  _, _, ev2 = q.check(w1, w2, 7, (name, 'after evaluate_embedding'), sample_seed=4)
  assert ev2.episodes.data_ptr() == q.ev.evaluate_policy(table, 1).episodes.data_ptr() and ev.episodes.shape == (B,)
  # sample_policy: the tabular drawn call, on every environment
  e2, t2 = _make(fam, kwargs, B, lane_offset=OFFSET), Twin(fam, _make(fam, kwargs, B, lane_offset=OFFSET))
  e2.sample_embedding(w1, w2, 5)
  t2.sample_embedding(w1, w2, 5)
  drawn = e2.sample_policy(logits, 4, sample_seed=3)
  t2.note(t2.env.sample_policy(logits, 4, sample_seed=3)[0], rollout=True)
  assert torch.equal(drawn[1], t2.env._policy_rollout_out[4][3])                  # pylint: disable=protected-access
  _same_outputs(e2.sample_embedding(w1, w2, 6, sample_seed=8), t2.sample_embedding(w1, w2, 6, sample_seed=8), (name, 'after sample_policy'))
  _same_envs(e2, types.SimpleNamespace(env=t2.env), (name, 'after sample_policy'))
  # the per-T buffers are rollout_policy's
  e3 = _make(fam, kwargs, B)
  assert e3.sample_embedding(w1, w2, 3)[1].data_ptr() == e3.rollout_policy(table, 3)[1].data_ptr()


@pytest.mark.parametrize('name', ['deep_sea_4_h64', 'deep_sea_8_h64_global', 'catch_h5'])
def test_the_greedy_calls_after_a_sampled_call_are_unchanged(name):
  """rollout_embedding / evaluate_embedding after sampled calls give what they give on a twin that never made one: the twin is
  brought to the same state by replaying the drawn actions through rollout()."""
  _, fam, kwargs, _ = BY_NAME[name]
  B, T = 257, 11
  a, b, c, d = (_make(fam, kwargs, B, lane_offset=OFFSET) for _ in range(4))
  w1, w2 = _pair(name)
  actions = a.sample_embedding(w1, w2, T, temperature=2.0, sample_seed=6)[1].clone()
  last = a.sample_embedding(w1, w2, 1)[1].clone()                                 # (a second drawn call, of another T)
  c.evaluate_sampled_embedding(w1, w2, T, temperature=2.0, sample_seed=6)
  c.evaluate_sampled_embedding(w1, w2, 1)
  for e in (b, d):
    e.rollout(actions)
    e.step(last[0])
  kw = dict(epsilon=0.25, explore_seed=4)
  ts, acts = a.rollout_embedding(w1, w2, T, **kw)
  want_ts, want_acts = b.rollout_embedding(w1, w2, T, **kw)
  assert torch.equal(acts, want_acts) and torch.equal(ts.observation, want_ts.observation) and torch.equal(ts.step_type, want_ts.step_type)
  assert torch.equal(ts.reward.view(torch.int32), want_ts.reward.view(torch.int32))
  _same_envs(a, types.SimpleNamespace(env=b), (name, 'rollout_embedding'))
  kept = [x.clone() for x in c.evaluate_embedding(w1, w2, T, **kw)]
  for x, y in zip(kept, d.evaluate_embedding(w1, w2, T, **kw)):
    assert torch.equal(x, y)
  _same_envs(c, types.SimpleNamespace(env=d), (name, 'evaluate_embedding'))
  _same_envs(c, types.SimpleNamespace(env=a), (name, 'both'))
