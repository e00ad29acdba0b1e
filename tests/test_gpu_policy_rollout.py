"""GPU: rollout_policy — T closed-loop steps of deep_sea / catch in ONE launch, the actions looked up inside the kernel in a
uint8 table at the key of the lane's own index observation.  Against (a) trajectories of the unmodified reference driven
by a tabular agent (tests/golden/.tools/policy_rollout, lane by lane, bit for bit) and (b) the loop the contract restates
— a = 0 where the lane resets, else table[row, key(observation before the call)], then step(a) — run on a twin
environment of the same seed through the eager step(), at one lane, thousands, 2^20 and ragged sizes; with exploration
draws replayed on the host from oracle/stream.py, populations of tables, out-of-range entries, chained and interleaved
calls, 64-bit lane offsets and a HIP-graph replay."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from bsuite_amd.utils import observations
from oracle import stream as S
from tests import engine_util as eu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, 'tests', 'golden', '.tools', 'policy_rollout', '*.npz')))
RESET_BIT = dict(deep_sea=1 << 17, catch=1 << 24)
FAMILIES = [('deep_sea', dict(size=10, mapping_seed=42)), ('deep_sea', dict(size=6, deterministic=False, mapping_seed=1)),
            ('catch', dict())]
IDS = ['deep_sea', 'deep_sea_stochastic', 'catch']


def _load(name):
  with np.load(os.path.join(ROOT, 'tests', 'golden', '.tools', 'policy_rollout', name + '.npz')) as z:
    g = {k: z[k] for k in z.files}
  return json.loads(str(g['meta'])), g


def test_all_seven_fixtures_are_covered():
  assert len(FIXTURES) == 7, FIXTURES


def _make(fam, kwargs, B, seed=11, lane_offset=0, **kw):
  return eu.make_env(fam, dict(kwargs), batch=B, lane_offset=lane_offset, seed=seed, observation_mode='index', **kw)


def _table(env, seed, P=None, high=None):
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  n = env.action_spec().num_values if high is None else high
  shape = (env.policy_num_states,) if P is None else (P, env.policy_num_states)
  return torch.randint(n, shape, generator=g, device='cuda', dtype=torch.int32).to(torch.uint8)


# ---------------------------------------------------------------------------------------------- the reference's trajectories
@pytest.mark.parametrize('name', FIXTURES)
def test_reference_fixtures(name):
  """B reference instances in the closed loop of a tabular agent: every array of the fixture, lane by lane, bit for bit —
  in one call of T steps, and again as two calls of T1 + T2 with bsuite_info compared at the cut."""
  meta, g = _load(name)
  fam, shape = meta['family'], tuple(meta['board_shape'])
  T, B = g['actions'].shape
  lanes = g['lanes']
  assert (np.diff(lanes.astype(np.int64)) == 1).all()
  P = meta['n_policies']
  table = torch.from_numpy(g['table']).cuda()
  pidx = torch.from_numpy(g['policy_index']).cuda() if P > 1 else None
  want_reward = np.where(g['step_type'] == 0, 0.0, np.nan_to_num(g['reward'])).astype(np.float32)
  want_discount = np.where(g['step_type'] == 0, 1.0, np.nan_to_num(g['discount'])).astype(np.float32)
  for cuts in ((T,), (T // 3, T - T // 3)):
    env = _make(fam, meta['kwargs'], B, seed=meta['seed'], lane_offset=int(lanes[0]))
    env._step_index = meta['step0']      # pylint: disable=protected-access
    t0 = 0
    for n in cuts:
      ts, actions = env.rollout_policy(table if P > 1 else table[0], n, policy_index=pidx, epsilon=meta['epsilon'],
                                       explore_seed=meta['explore_seed'])
      sl = slice(t0, t0 + n)
      what = f'{name} calls {cuts} steps {t0}..{t0 + n}'
      assert actions.dtype is torch.int32 and tuple(actions.shape) == (n, B)
      np.testing.assert_array_equal(actions.cpu().numpy(), g['actions'][sl], err_msg=what)
      np.testing.assert_array_equal(ts.step_type.cpu().numpy(), g['step_type'][sl], err_msg=what)
      np.testing.assert_array_equal(eu.f32_bits(ts.reward.cpu().numpy()), eu.f32_bits(want_reward[sl]), err_msg=what)
      np.testing.assert_array_equal(eu.f32_bits(ts.discount.cpu().numpy()), eu.f32_bits(want_discount[sl]), err_msg=what)
      assert ts.observation.dtype is torch.int32
      np.testing.assert_array_equal(ts.observation.cpu().numpy(), g['index'][sl], err_msg=what)
      boards = observations.index_to_dense(ts.observation, shape).cpu().numpy()
      np.testing.assert_array_equal(eu.f32_bits(boards), eu.f32_bits(g['obs'][sl]), err_msg=what)
      # the keys the kernel looked up are the keys of the reference's agent: the observation before each call
      keys = observations.policy_key(ts.observation, shape).cpu().numpy()
      live = g['resets'][sl][1:] == 0
      np.testing.assert_array_equal(keys[:-1][live], g['keys'][sl][1:][live], err_msg=what)
      info = env.bsuite_info()
      for j, k in enumerate(meta['info_keys']):
        np.testing.assert_array_equal(info[k].cpu().numpy(), g['info'][t0 + n - 1, :, j], err_msg=f'{what} {k}')
      t0 += n
    assert env.step_index == meta['step0'] + T
    assert int(env.episode_counters()[0]) == int((g['step_type'] == 2).sum())
    assert int(env.episode_counters()[1]) == int((g['step_type'] == 0).sum())
    assert int(env.invalid_action_count()) == 0


# ---------------------------------------------------------------------------------------------- the restated loop on a twin
class Twin:
  """The loop of the contract on an environment of the same seed, through the eager step()."""

  def __init__(self, fam, env):
    self.fam, self.env, self.obs = fam, env, None
    B = env.batch_size
    self.lanes = (np.uint64(env.lane_offset) + np.arange(B, dtype=np.uint64))

  def note(self, ts, rollout=False):
    self.obs = (ts.observation[-1] if rollout else ts.observation).clone()

  def rollout_policy(self, table, T, policy_index=None, epsilon=0.0, explore_seed=0):
    env, B = self.env, self.env.batch_size
    table = table.reshape(-1, table.shape[-1])
    P = table.shape[0]
    na = env.action_spec().num_values
    row = policy_index.clamp(0, P - 1).to(torch.int64) if policy_index is not None else torch.zeros(B, dtype=torch.int64, device='cuda')
    out = dict(step_type=[], reward=[], discount=[], observation=[], actions=[])
    for _ in range(T):
      if not env._allocated:                   # pylint: disable=protected-access
        resets = torch.ones(B, dtype=torch.bool, device='cuda')
        key = torch.zeros(B, dtype=torch.int64, device='cuda')
      else:
        resets = (env._state['state'] & RESET_BIT[self.fam]) != 0      # pylint: disable=protected-access
        key = (observations.policy_key(self.obs, env.board_shape).clamp(min=0) if self.obs is not None
               else torch.zeros(B, dtype=torch.int64, device='cuda'))
      a = table[row, key].to(torch.int32)
      if epsilon > 0:
        step = env.device_step_index() if env._allocated else env.step_index      # pylint: disable=protected-access
        w = S.words(explore_seed, self.lanes, step, 2, 4).astype(np.uint64)
        u = (((w[:, 0] >> np.uint64(5)) << np.uint64(26)) | (w[:, 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
        r = ((w[:, 2] * np.uint64(na)) >> np.uint64(32)).astype(np.int32)
        a = torch.where(torch.from_numpy(u < epsilon).cuda(), torch.from_numpy(r).cuda(), a)
      a = torch.where(resets, torch.zeros_like(a), a)
      ts = env.step(a)
      self.note(ts)
      for k in ('step_type', 'reward', 'discount', 'observation'):
        out[k].append(getattr(ts, k).clone())
      out['actions'].append(a)
    return {k: torch.stack(v) for k, v in out.items()}


def _same_outputs(got, want, what):
  ts, actions = got
  assert torch.equal(actions, want['actions']), what
  assert torch.equal(ts.step_type, want['step_type']), what
  assert torch.equal(ts.reward.view(torch.int32), want['reward'].view(torch.int32)), what
  assert torch.equal(ts.discount, want['discount']), what
  assert torch.equal(ts.observation, want['observation']), what


def _same_envs(env, twin, what):
  ref = twin.env
  for k, v in ref._state.items():                  # pylint: disable=protected-access
    assert torch.equal(env._state[k], v), (what, k)  # pylint: disable=protected-access
  assert torch.equal(env._info, ref._info), what    # pylint: disable=protected-access
  for k, v in ref.bsuite_info().items():
    assert torch.equal(env.bsuite_info()[k], v), (what, k)
  assert torch.equal(env.episode_counters(), ref.episode_counters()), what
  assert torch.equal(env.invalid_action_count(), ref.invalid_action_count()), what
  assert env.step_index == ref.step_index and env.device_step_index() == ref.device_step_index(), what
  a, b = env.state_dict(), ref.state_dict()
  assert sorted(a) == sorted(b)
  for k in a:
    if k == '__counters':
      assert torch.equal(a[k].sum(dim=0), b[k].sum(dim=0)), what
    elif torch.is_tensor(a[k]):
      assert torch.equal(a[k], b[k]), (what, k)
    else:
      assert a[k] == b[k], (what, k)


@pytest.mark.parametrize('B', [1, 1000, 4099, 1 << 20, (1 << 20) + 257])
@pytest.mark.parametrize('T', [1, 7, 32])
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=IDS)
def test_equals_the_restated_loop_on_a_twin(fam, kwargs, T, B):
  env, twin = _make(fam, kwargs, B), Twin(fam, _make(fam, kwargs, B))
  table = _table(env, 5)
  for call in range(2):                              # a fresh batch, then a batch in the middle of its episodes
    got = env.rollout_policy(table, T)
    want = twin.rollout_policy(table, T)
    _same_outputs(got, want, (fam, T, B, call))
    _same_envs(env, twin, (fam, T, B, call))
  assert int(env.episode_counters()[1]) >= B


@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=IDS)
def test_calls_chain_and_interleave_with_step_rollout_mark_reset_and_reset(fam, kwargs):
  B = 4099
  env, twin = _make(fam, kwargs, B), Twin(fam, _make(fam, kwargs, B))
  one = _make(fam, kwargs, B)
  table = _table(env, 6)
  na = env.action_spec().num_values
  g = torch.Generator(device='cuda')
  g.manual_seed(3)
  # T1 + T2 == one call of T1 + T2
  fields = lambda r: (r[0].step_type, r[0].reward, r[0].discount, r[0].observation, r[1])
  whole = fields(one.rollout_policy(table, 19))
  parts = [[x.clone() for x in fields(env.rollout_policy(table, n))] for n in (8, 11)]
  for a, b, w in zip(parts[0], parts[1], whole):
    assert torch.equal(torch.cat([a, b]), w)
  assert torch.equal(env._state['state'], one._state['state']) and torch.equal(env._info, one._info)   # pylint: disable=protected-access
  assert env.step_index == one.step_index == 19
  tw = [twin.rollout_policy(table, n) for n in (8, 11)]
  for k, w in zip(('step_type', 'reward', 'discount', 'observation', 'actions'), whole):
    assert torch.equal(torch.cat([tw[0][k], tw[1][k]]), w), k
  _same_envs(env, twin, 'chain')
  # ... and freely interleaved with the other entry points
  for round_ in range(3):
    a = torch.randint(na, (B,), generator=g, device='cuda', dtype=torch.int32)
    twin.note(twin.env.step(a))
    env.step(a)
    _same_outputs(env.rollout_policy(table, 5), twin.rollout_policy(table, 5), ('after step', round_))
    acts = torch.randint(na, (3, B), generator=g, device='cuda', dtype=torch.int32)
    twin.note(twin.env.rollout(acts), rollout=True)
    env.rollout(acts)
    _same_outputs(env.rollout_policy(table, 4), twin.rollout_policy(table, 4), ('after rollout', round_))
    mask = torch.rand(B, generator=g, device='cuda') < 0.3
    env.mark_reset(mask)
    twin.env.mark_reset(mask)
    got = env.rollout_policy(table, 6)
    _same_outputs(got, twin.rollout_policy(table, 6), ('after mark_reset', round_))
    assert bool((got[0].step_type[0][mask] == 0).all()) and bool((got[1][0][mask] == 0).all())
    twin.note(twin.env.reset())
    env.reset()
    got = env.rollout_policy(table, 7)
    _same_outputs(got, twin.rollout_policy(table, 7), ('after reset', round_))
    assert bool((got[0].step_type[0] != 0).all())            # reset() left no lane waiting for a reset
    _same_envs(env, twin, ('interleaved', round_))
  # the step after a policy rollout sees what the rollout left
  a = torch.randint(na, (B,), generator=g, device='cuda', dtype=torch.int32)
  ts, tw = env.step(a), twin.env.step(a)
  assert torch.equal(ts.observation, tw.observation) and torch.equal(ts.step_type, tw.step_type)


# ---------------------------------------------------------------------------------------------- exploration
@pytest.mark.parametrize('epsilon', [1.0, 0.3])
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=IDS)
def test_epsilon_greedy_against_a_host_replay_of_the_draws(fam, kwargs, epsilon):
  B, T, seed = 4099, 24, (1 << 45) + 9
  env, twin = _make(fam, kwargs, B), Twin(fam, _make(fam, kwargs, B))
  greedy = _make(fam, kwargs, B)
  table = _table(env, 7)
  got = env.rollout_policy(table, T, epsilon=epsilon, explore_seed=seed)
  want = twin.rollout_policy(table, T, epsilon=epsilon, explore_seed=seed)
  _same_outputs(got, want, (fam, epsilon))
  _same_envs(env, twin, (fam, epsilon))
  na = env.action_spec().num_values
  live = got[0].step_type != 0
  acts = got[1][live]
  assert all(int((acts == a).sum()) > 0 for a in range(na))
  assert not torch.equal(got[1], greedy.rollout_policy(table, T)[1])
  if epsilon == 1.0:        # every non-reset action is RandInt: uniform over the actions, whatever the table says
    frac = torch.bincount(acts.to(torch.int64), minlength=na).to(torch.float64) / acts.numel()
    assert bool(((frac - 1.0 / na).abs() < 0.02).all()), frac
  # another explore_seed: other actions; the same seed again on a fresh batch: the same
  other = _make(fam, kwargs, B).rollout_policy(table, T, epsilon=epsilon, explore_seed=seed + 1)
  assert not torch.equal(other[1], got[1])
  again = _make(fam, kwargs, B).rollout_policy(table, T, epsilon=epsilon, explore_seed=seed)
  assert torch.equal(again[1], got[1]) and torch.equal(again[0].observation, got[0].observation)


def test_the_environments_own_stream_is_untouched():
  """A stochastic deep_sea trajectory under an exploring policy is the one step() gives for the same actions."""
  fam, kwargs = FAMILIES[1]
  B, T = 4099, 40
  env, ref = _make(fam, kwargs, B), _make(fam, kwargs, B)
  ts, actions = env.rollout_policy(_table(env, 8), T, epsilon=0.5, explore_seed=123)
  want = ref.rollout(actions)
  assert torch.equal(ts.step_type, want.step_type) and torch.equal(ts.observation, want.observation)
  assert torch.equal(ts.reward.view(torch.int32), want.reward.view(torch.int32))
  assert torch.equal(env._state['state'], ref._state['state'])          # pylint: disable=protected-access


# ---------------------------------------------------------------------------------------------- populations, bad entries, offsets
@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=IDS)
def test_population_of_tables_with_clamped_policy_index(fam, kwargs):
  B, T, P = 4099, 20, 4
  env, twin = _make(fam, kwargs, B), Twin(fam, _make(fam, kwargs, B))
  table = _table(env, 9, P=P)
  g = torch.Generator(device='cuda')
  g.manual_seed(4)
  pidx = torch.randint(P, (B,), generator=g, device='cuda', dtype=torch.int32)
  got = env.rollout_policy(table, T, policy_index=pidx)
  _same_outputs(got, twin.rollout_policy(table, T, policy_index=pidx), 'population')
  first = got[1].clone()
  # every lane follows ITS table: the same lanes under table p alone
  for p in range(P):
    alone = _make(fam, kwargs, B).rollout_policy(table[p], T)
    sel = pidx == p
    assert int(sel.sum()) > 0
    assert torch.equal(alone[1][:, sel], first[:, sel])
  # indices outside [0, P-1] are clamped, never followed
  wild = pidx.clone()
  wild[::7] = -5
  wild[3::7] = P + 100
  wild[5::7] = -(1 << 31)
  wild[6::7] = (1 << 31) - 1
  got = env.rollout_policy(table, T, policy_index=wild, epsilon=0.2, explore_seed=5)
  _same_outputs(got, twin.rollout_policy(table, T, policy_index=wild, epsilon=0.2, explore_seed=5), 'clamped')
  _same_envs(env, twin, 'clamped')
  # [1, S] is one shared table
  a, b = _make(fam, kwargs, B), _make(fam, kwargs, B)
  assert torch.equal(a.rollout_policy(table[:1], T)[1], b.rollout_policy(table[0], T)[1])


def test_an_out_of_range_table_byte_is_the_same_value_passed_to_step():
  fam, kwargs = FAMILIES[2]
  B, T = 4099, 30
  env, twin = _make(fam, kwargs, B), Twin(fam, _make(fam, kwargs, B))
  table = _table(env, 10, high=256)                          # mostly outside catch's 0..2
  got = env.rollout_policy(table, T)
  _same_outputs(got, twin.rollout_policy(table, T), 'invalid')
  _same_envs(env, twin, 'invalid')
  live = got[0].step_type != 0
  assert int(env.invalid_action_count()) == int(((got[1] > 2) & live).sum()) > 0
  assert int(got[1].max()) > 2                               # the action column reports the entry as it is
  # deep_sea has no invalid actions: any byte other than the cell's mapping is 'left'
  fam, kwargs = FAMILIES[0]
  env, twin = _make(fam, kwargs, B), Twin(fam, _make(fam, kwargs, B))
  table = _table(env, 10, high=256)
  _same_outputs(env.rollout_policy(table, T), twin.rollout_policy(table, T), 'deep_sea bytes')
  assert int(env.invalid_action_count()) == 0


@pytest.mark.parametrize('fam,kwargs', FAMILIES, ids=IDS)
def test_large_lane_offset(fam, kwargs):
  B, T, off = 1000, 20, (1 << 40) + 3
  env, twin = _make(fam, kwargs, B, lane_offset=off), Twin(fam, _make(fam, kwargs, B, lane_offset=off))
  near = _make(fam, kwargs, B, lane_offset=3)
  table = _table(env, 12)
  got = env.rollout_policy(table, T, epsilon=0.4, explore_seed=99)
  _same_outputs(got, twin.rollout_policy(table, T, epsilon=0.4, explore_seed=99), 'lane offset')
  _same_envs(env, twin, 'lane offset')
  assert not torch.equal(got[1], near.rollout_policy(table, T, epsilon=0.4, explore_seed=99)[1])
  # a shard sees the lanes of the whole: lanes 100.. of the batch == a batch that starts there
  shard = _make(fam, kwargs, 200, lane_offset=off + 100)
  part = shard.rollout_policy(table, T, epsilon=0.4, explore_seed=99)
  assert torch.equal(part[1], got[1][:, 100:300]) and torch.equal(part[0].observation, got[0].observation[:, 100:300])


def test_a_table_too_large_for_lds_is_read_from_global_memory():
  """catch 20 x 16: 5120 states, beyond the 4096 bytes a workgroup stages."""
  fam, kwargs = 'catch', dict(rows=20, columns=16)
  B, T = 4099, 45
  env, twin = _make(fam, kwargs, B), Twin(fam, _make(fam, kwargs, B))
  assert env.policy_num_states == 5120
  table = _table(env, 13)
  _same_outputs(env.rollout_policy(table, T), twin.rollout_policy(table, T), 'global table')
  _same_envs(env, twin, 'global table')


# ---------------------------------------------------------------------------------------------- HIP graph
@pytest.mark.parametrize('fam,kwargs', [FAMILIES[1], FAMILIES[2]], ids=[IDS[1], IDS[2]])
def test_hip_graph_replay_with_a_device_step_counter(fam, kwargs):
  B, T = 4099, 6
  env = _make(fam, kwargs, B, device_step_counter=True)
  ref = _make(fam, kwargs, B, device_step_counter=True)
  table = _table(env, 14)
  env.rollout_policy(table, T, epsilon=0.25, explore_seed=8)          # eager: allocates the output buffers
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    ts, actions = env.rollout_policy(table, T, epsilon=0.25, explore_seed=8)
  for replay in range(3):
    graph.replay()
  torch.cuda.synchronize()
  for call in range(4):
    want = ref.rollout_policy(table, T, epsilon=0.25, explore_seed=8)
  assert env.device_step_index() == ref.device_step_index() == 4 * T
  assert torch.equal(actions, want[1]) and torch.equal(ts.observation, want[0].observation)
  assert torch.equal(ts.step_type, want[0].step_type) and torch.equal(ts.reward.view(torch.int32), want[0].reward.view(torch.int32))
  assert torch.equal(env._state['state'], ref._state['state']) and torch.equal(env._info, ref._info)     # pylint: disable=protected-access
  assert torch.equal(env.episode_counters(), ref.episode_counters())


# ---------------------------------------------------------------------------------------------- the optimal table
def test_the_optimal_deep_sea_table_at_2p20_lanes_never_has_a_bad_episode():
  N, B = 10, 1 << 20
  env = _make('deep_sea', dict(size=N, mapping_seed=42), B)
  table = torch.from_numpy(np.asarray(env._action_mapping).reshape(-1).astype(np.uint8)).cuda()     # pylint: disable=protected-access
  ts, actions = env.rollout_policy(table, 5 * (N + 1))
  info = env.bsuite_info()
  assert int(env.episode_counters()[0]) == 5 * B
  assert float(info['total_bad_episodes'].max()) == 0.0
  last = ts.step_type == 2
  assert bool((ts.reward[last] > 0.9).all())
  assert float(info['denoised_return'].min()) == float(info['denoised_return'].max()) == 5.0
  # ... and its complement never reaches the treasure
  worst = _make('deep_sea', dict(size=N, mapping_seed=42), B)
  worst.rollout_policy(1 - table, 5 * (N + 1))
  assert float(worst.bsuite_info()['total_bad_episodes'].min()) == 5.0
