"""GPU: evaluate_policy — rollout_policy's closed loop with every TimeStep store removed: three numbers per lane (episodes
ended, sum of rewards, sum of the returns of the episodes that ended; float64, from the f64 reward of the lane advance).
Against (a) the trajectories of the unmodified reference (tests/golden/.tools/policy_rollout): the columns are, bit for
bit, the contract's loop over the fixture's float64 rewards; (b) a twin environment of the same seed that runs
rollout_policy: equal state, info and counters afterwards, `episodes` the count of LAST in the twin's step types, and the
two sums the contract's loop over f64 rewards that never come from the engine — catch pays -1 / 0 / +1, so the twin's
float32 rewards widened are exact; deep_sea's come from the C oracle driven with the actions the twin reported."""
import types

import numpy as np
import pytest
import torch

from oracle import coracle
from tests import policy_eval_util as pe
from tests.test_gpu_policy_rollout import _make, _same_envs, _table

pytestmark = pytest.mark.gpu

OFFSET = (1 << 32) - 17                       # the global lane ids cross 2^32 inside the first workgroup
CASES = [('deep_sea', dict(size=10, mapping_seed=42)), ('deep_sea', dict(size=6, deterministic=False, mapping_seed=1)),
         ('catch', dict()), ('catch', dict(rows=10, columns=21))]
IDS = ['deep_sea', 'deep_sea_stochastic', 'catch', 'catch_global_table']
SEED = 11


def _same_columns(ev, want, what):
  assert ev.episodes.dtype is torch.int32 and ev.return_sum.dtype is torch.float64 and ev.episode_return_sum.dtype is torch.float64
  np.testing.assert_array_equal(ev.episodes.cpu().numpy(), want[0], err_msg=f'{what} episodes')
  np.testing.assert_array_equal(pe.bits(ev.return_sum.cpu().numpy()), pe.bits(want[1]), err_msg=f'{what} return_sum')
  np.testing.assert_array_equal(pe.bits(ev.episode_return_sum.cpu().numpy()), pe.bits(want[2]), err_msg=f'{what} episode_return_sum')


# ---------------------------------------------------------------------------------------------- 1. the reference's trajectories
@pytest.mark.parametrize('name', pe.FIXTURES)
def test_reference_fixtures(name):
  meta, g = pe.load(name)
  fam = meta['family']
  T, B = g['actions'].shape
  lanes = g['lanes']
  P = meta['n_policies']
  table = torch.from_numpy(g['table']).cuda()
  pidx = torch.from_numpy(g['policy_index']).cuda() if P > 1 else None
  for cuts in ((T,), (T // 3, T - T // 3)):
    env = _make(fam, meta['kwargs'], B, seed=meta['seed'], lane_offset=int(lanes[0]))
    env._step_index = meta['step0']      # pylint: disable=protected-access
    t0 = 0
    for n in cuts:
      ev = env.evaluate_policy(table if P > 1 else table[0], n, policy_index=pidx, epsilon=meta['epsilon'],
                               explore_seed=meta['explore_seed'])
      sl = slice(t0, t0 + n)
      what = f'{name} calls {cuts} steps {t0}..{t0 + n}'
      assert tuple(ev.episodes.shape) == tuple(ev.return_sum.shape) == tuple(ev.episode_return_sum.shape) == (B,)
      _same_columns(ev, pe.host_loop(g['step_type'][sl], g['reward'][sl]), what)     # (accumulators start at zero at each cut)
      info = env.bsuite_info()
      for j, k in enumerate(meta['info_keys']):
        np.testing.assert_array_equal(info[k].cpu().numpy(), g['info'][t0 + n - 1, :, j], err_msg=f'{what} {k}')
      t0 += n
    assert env.step_index == meta['step0'] + T
    assert int(env.episode_counters()[0]) == int((g['step_type'] == 2).sum())
    assert int(env.episode_counters()[1]) == int((g['step_type'] == 0).sum())
    assert int(env.invalid_action_count()) == 0


# ---------------------------------------------------------------------------------------------- 2. twin and oracle
class Ref:
  """The f64 rewards of the steps a twin has taken: catch's float32 rewards widened (exact), deep_sea's from the C oracle
  driven with the twin's actions, call by call."""

  def __init__(self, fam, kwargs, B, lane_offset=OFFSET):
    self.t = 0
    lanes = np.uint64(lane_offset) + np.arange(B, dtype=np.uint64)
    self.orc = coracle.OracleEnv(fam, dict(kwargs), lanes, seed=SEED) if fam == 'deep_sea' else None

  def step(self, actions):
    if self.orc is not None:
      self.orc.call(actions.cpu().numpy(), self.t)
    self.t += 1

  def mark_reset(self, mask):
    if self.orc is not None:
      self.orc.reset_next[mask.cpu().numpy().astype(bool)] = 1        # base.py:59-62

  def rewards(self, ts, actions):
    st, r32, acts = ts.step_type.cpu().numpy(), ts.reward.cpu().numpy(), actions.cpu().numpy()
    T = st.shape[0]
    if self.orc is None:
      self.t += T
      return st, r32.astype(np.float64)
    out = np.zeros(st.shape, np.float64)
    for t in range(T):
      ost, r, _, _ = self.orc.call(acts[t], self.t)
      np.testing.assert_array_equal(ost, st[t])
      out[t] = r
      self.t += 1
    live = st != 0
    np.testing.assert_array_equal(out[live].astype(np.float32), r32[live])      # the twin's rewards are these, rounded
    return st, out


def _check(env, twin, ref, table, T, what, **kw):
  """One evaluate_policy call against the twin's rollout_policy of the same arguments."""
  ts, actions = twin.rollout_policy(table, T, **kw)
  ev = env.evaluate_policy(table, T, **kw)
  st, r64 = ref.rewards(ts, actions)
  want = pe.host_loop(st, r64)
  np.testing.assert_array_equal(want[0], (st == 2).sum(axis=0))
  _same_columns(ev, want, what)
  _same_envs(env, types.SimpleNamespace(env=twin), what)
  return ev, ts


@pytest.mark.parametrize('B', [1, 257, 4099])
@pytest.mark.parametrize('T', [1, 7, 45])
@pytest.mark.parametrize('fam,kwargs', CASES, ids=IDS)
def test_equals_the_twins_rollout_policy_and_the_host_loop(fam, kwargs, T, B):
  env, twin, ref = _make(fam, kwargs, B, lane_offset=OFFSET), _make(fam, kwargs, B, lane_offset=OFFSET), Ref(fam, kwargs, B)
  assert (env.policy_num_states > 4096) == (kwargs.get('columns') == 21)          # the table read from global memory
  g = torch.Generator(device='cuda')
  g.manual_seed(B + T)
  # one shared table, greedy: a fresh batch, then a batch in the middle of its episodes
  table = _table(env, 5)
  for call in range(2):
    _check(env, twin, ref, table, T, (fam, T, B, 'shared', call))
  # a population with policy_index values outside [0, P-1], exploring
  pop = _table(env, 6, P=5)
  pidx = torch.randint(-3, 9, (B,), generator=g, device='cuda', dtype=torch.int32)
  _check(env, twin, ref, pop, T, (fam, T, B, 'population'), policy_index=pidx, epsilon=0.3, explore_seed=(1 << 45) + 9)
  _check(env, twin, ref, pop, T, (fam, T, B, 'population greedy'), policy_index=pidx)
  _check(env, twin, ref, table, T, (fam, T, B, 'shared exploring'), epsilon=0.3, explore_seed=77)
  assert int(env.episode_counters()[1]) >= B


def test_catch_table_entries_outside_the_action_spec():
  fam, kwargs = CASES[2]
  B, T = 4099, 45
  env, twin, ref = _make(fam, kwargs, B, lane_offset=OFFSET), _make(fam, kwargs, B, lane_offset=OFFSET), Ref(fam, kwargs, B)
  table = _table(env, 10, high=256)                          # mostly outside catch's 0..2
  _check(env, twin, ref, table, T, 'invalid entries')
  assert int(env.invalid_action_count()) == int(twin.invalid_action_count()) > 0


@pytest.mark.parametrize('fam,kwargs', CASES[:3], ids=IDS[:3])
def test_calls_chain_with_step_and_mark_reset(fam, kwargs):
  B = 4099
  env, twin, ref = _make(fam, kwargs, B, lane_offset=OFFSET), _make(fam, kwargs, B, lane_offset=OFFSET), Ref(fam, kwargs, B)
  table = _table(env, 7)
  g = torch.Generator(device='cuda')
  g.manual_seed(3)
  _check(env, twin, ref, table, 13, (fam, 'first'))
  a = torch.randint(env.action_spec().num_values, (B,), generator=g, device='cuda', dtype=torch.int32)
  ts, tw = env.step(a), twin.step(a)
  assert torch.equal(ts.observation, tw.observation) and torch.equal(ts.step_type, tw.step_type)
  ref.step(a)
  mask = torch.rand(B, generator=g, device='cuda') < 0.3
  for e in (env, twin, ref):
    e.mark_reset(mask)
  ev, ts = _check(env, twin, ref, table, 9, (fam, 'after step and mark_reset'))
  assert bool((ts.step_type[0][mask] == 0).all())
  # after mark_reset of ALL lanes no episode runs when the call starts: every ended episode is whole
  every = torch.ones(B, dtype=torch.bool, device='cuda')
  for e in (env, twin, ref):
    e.mark_reset(every)
  ev, ts = _check(env, twin, ref, table, 30, (fam, 'after mark_reset of all lanes'))
  assert bool((ts.step_type[0] == 0).all()) and int(ev.episodes.min()) >= 1
  # the buffers are cached per environment: the next call overwrites them
  again = env.evaluate_policy(table, 2)
  assert again.episodes.data_ptr() == ev.episodes.data_ptr() and again.return_sum.data_ptr() == ev.return_sum.data_ptr()


# ---------------------------------------------------------------------------------------------- 3. full size
@pytest.mark.parametrize('fam,kwargs', [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_full_size(fam, kwargs):
  B, T = (1 << 20) + 257, 16
  env, twin, ref = _make(fam, kwargs, B, lane_offset=OFFSET), _make(fam, kwargs, B, lane_offset=OFFSET), Ref(fam, kwargs, B)
  ev, _ = _check(env, twin, ref, _table(env, 5), T, (fam, 'full size'), epsilon=0.1, explore_seed=3)
  assert int(ev.episodes.sum()) == int(env.episode_counters()[0]) > 0


# ---------------------------------------------------------------------------------------------- 4. HIP graph
@pytest.mark.parametrize('fam,kwargs', [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_hip_graph_replay_with_a_device_step_counter(fam, kwargs):
  B, T = 4099, 6
  env = _make(fam, kwargs, B, device_step_counter=True)
  ref = _make(fam, kwargs, B, device_step_counter=True)
  table = _table(env, 14)
  env.evaluate_policy(table, T, epsilon=0.25, explore_seed=8)          # eager: allocates the output buffers
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    ev = env.evaluate_policy(table, T, epsilon=0.25, explore_seed=8)
  for _ in range(2):
    graph.replay()
  torch.cuda.synchronize()
  for _ in range(3):                                                   # the eager call and two replays == three eager calls
    want = ref.evaluate_policy(table, T, epsilon=0.25, explore_seed=8)
  assert env.device_step_index() == ref.device_step_index() == 3 * T
  for a, b in zip(ev, want):
    assert torch.equal(a, b)
  assert torch.equal(env._state['state'], ref._state['state']) and torch.equal(env._info, ref._info)     # pylint: disable=protected-access
  assert torch.equal(env.episode_counters(), ref.episode_counters())
