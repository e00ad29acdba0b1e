"""GPU: the catch and deep_sea kernels on the edge-state grid of tests/grid_edge_util.py, across every launch path.

catch_fam::advance and deep_sea_fam::advance are compiled into some twenty kernels, four of them in the deferred form
(advance_deferred + commit_deferred).  All are promised to equal the eager step() bit for bit, and the eager step to equal
the C oracle.  Trajectories from a fresh reset never reach the branches the grid is made of (tests/test_grid_edges_host.py
proves the grid reaches each on at least a wave of lanes): catch's fold of 127 pending misses into the total_regret column,
with bit 31 of the state word as data; deep_sea's paying corner and its bad-episode bit.  Everything is exact: int32 bit
patterns of every TimeStep field, state column, info column and episode counter.

  A. the eager lean step() from the loaded grid against oracle/coracle.OracleEnv;
  B. every other path against that eager run from the same loaded state, T = 1 and T = 3 (a lane that ends at step 1 resets
     inside the fused loop at step 2);
  C. several folds inside ONE call of 600 steps, the setting the host test verified on the reference.

Which path a dense call takes depends on lanes * cells (csrc/bsx_pair_host.h): the fused tile step, the fused rollout and the
pipelined rollout need a multiple of 4.  The cases with m * 256 + 1 lanes and 50, 130, 10 or 49 cells are not, so each has an
`aligned` twin (grid_edge_util.CASES), and part C runs at 513 and at 514 lanes.

Which test drives the grid through which kernel:
  bsx_advance_kernel, lean                   the eager step of A: catch 13x10 and 64x64, deep_sea 12, every unaligned case
  bsx_advance_kernel, wrapped / mt19937      test_logging_paths, test_reward_noise_paths / test_mt19937_step (boards over 128
                                             cells and unaligned cases; the aligned small boards take the wrapped fused tile)
  bsx_advance2_kernel                        test_large_batch_tiles (catch, 2^20 + 257 lanes); at small shapes through
                                             test_gpu_pair_path_small_shapes.test_two_lanes_per_thread_advance_at_small_shapes
  the fused tile kernels                     the eager step of A on the aligned catch 10x5 / 2x5, deep_sea 4 / 6 / 7 (64-lane
                                             tiles); the 256-lane tiles, lean and wrapped, through
                                             test_gpu_pair_path_small_shapes.test_256_lane_fused_tiles_at_small_shapes
  bsx_fused_rollout_kernel                   test_rollout, T = 3, on the same cases; part C 'rollout' at 514 lanes
  bsx_pipelined_kernel                       test_rollout, T = 3: catch 13x10 aligned and 64x64, deep_sea 12 and 30
  bsx_hot_cells_kernel (4-byte stores)       test_rollout, T = 3, slice 1 of every unaligned case
  bsx_index_step_kernel / _rollout_kernel    test_index_paths, part C 'index_rollout'
  bsx_pair_advance_delta_kernel              test_delta_step
  deep_sea_step1_kernel                      deep_sea 30: A, test_reset_mask_and_mark_reset, test_large_batch_tiles at 2^18 and
                                             2^18 + 257 lanes (2^18 + 2^16 + 1 is past its limit: advance + stream)
  bsx_pair_advance_group_kernel              test_grouped_launches, per_family
  pair_mixed_advance_kernel                  test_grouped_launches, pair_mixed
  the sweep's phase 0 / pipelined kernel     test_grouped_launches, whole_sweep / whole_sweep_pipelined
  bsx_policy_rollout_kernel                  test_closed_loop_calls and part C, rollout_policy
  bsx_tab_eval_kernel (deferred)             the same, evaluate_policy
  the tabular sampling kernel                the same, sample_policy / evaluate_sampled_policy (deferred)
  bsx_embed_kernel, all eight branches       the same, rollout_ / evaluate_ / sample_ / evaluate_sampled_embedding, both families
"""
import functools

import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import sweep
from bsuite_amd import sweep_batch as sb
from bsuite_amd.utils import observations
from bsuite_amd.utils import wrappers
from tests import edge_snap_util as es
from tests import embed_util as emb
from tests import engine_util as eu
from tests import grid_edge_util as gu
from tests import policy_eval_util as pe
from tests import tab_sample_util as tsu

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(*c, id=i) for c, i in zip(gu.CASES, gu.CASE_IDS)]
T_MAX = 3
NO_OBS = ('step_type', 'reward', 'discount')
PENDING_MASK = 0x01FFFFFF          # a catch state word without its pending-miss field

TS_FIELDS = es.TS_FIELDS
_bits, _snap_ts, _snap_after, _stack, _assert_ts = es.bits, es.snap_ts, es.snap_after, es.stack, es.assert_ts
_assert_after = functools.partial(es.assert_after, raw_info=True)      # here always with the info columns themselves


def _make(family, kwargs, batch, **engine_kwargs):
  return eu.make_env(family, dict(kwargs), batch=batch, lane_offset=gu.LANE_OFFSET, seed=gu.SEED, **engine_kwargs)


def _num_actions(family):
  return 3 if family == 'catch' else 2


def _actions(g, T):
  """int32 [T, B] on the device: the grid's action first, seeded random ones after it."""
  rng = np.random.default_rng(31)
  a = np.concatenate([g['action'][None], rng.integers(0, _num_actions(g['family']), size=(T - 1, g['lanes'])).astype(np.int32)])
  return torch.from_numpy(a).cuda()


def _run(env, actions, T, path):
  """[T, ...] TimeStep snapshots through step() or rollout()."""
  if path == 'step':
    return _stack([_snap_ts(env.step(actions[t].contiguous())) for t in range(T)], T)
  return _snap_ts(env.rollout(actions[:T].contiguous()))


_EAGER = {}


def eager(family, kwargs, aligned=False):
  """The eager lean step() from the loaded grid, T_MAX times with _actions: per step the TimeStep and what the environment
  holds afterwards, as bit patterns on the device.  Computed once per case and shared, never modified."""
  key = (family, tuple(sorted(kwargs.items())), aligned)
  if key not in _EAGER:
    g = gu.grid(family, kwargs, aligned)
    env = _make(family, kwargs, g['lanes'])
    gu.load(env, g)
    assert env.step_index == gu.STEP0
    acts = _actions(g, T_MAX)
    ts, after = [], []
    for t in range(T_MAX):
      ts.append(_snap_ts(env.step(acts[t])))
      after.append(_snap_after(env))
    _EAGER[key] = dict(ts=ts, after=after, actions=acts)
  return _EAGER[key]


def _f32(ts_snap, f):
  return ts_snap[f].view(torch.float32).cpu().numpy()


def _assert_vs_oracle(ts, want, what):
  """One TimeStep snapshot against the oracle's (step_type, reward, discount, obs): the oracle's reward rounded to float32;
  a FIRST step carries reward 0 and discount 1."""
  st, r, d, obs = want
  live = st != 0
  np.testing.assert_array_equal(ts['step_type'].cpu().numpy(), st, err_msg=f'{what} step_type')
  got_r, got_d = _f32(ts, 'reward'), _f32(ts, 'discount')
  np.testing.assert_array_equal(eu.f32_bits(got_r[live]), eu.f32_bits(r[live].astype(np.float32)), err_msg=f'{what} reward')
  np.testing.assert_array_equal(got_d[live], d[live].astype(np.float32), err_msg=f'{what} discount')
  assert (got_r[~live] == 0).all() and (got_d[~live] == 1).all(), what
  np.testing.assert_array_equal(eu.f32_bits(_f32(ts, 'observation')), eu.f32_bits(obs), err_msg=f'{what} observation')


def _index_rows(g, state):
  """int32 [..., K]: the index observation of packed state words (catch_hot / deep_sea_hot)."""
  st = state.to(torch.int64)
  if g['family'] == 'catch':
    ball = ((st >> 8) & 0xFF) * g['columns'] + (st & 0xFF)
    paddle = (g['rows'] - 1) * g['columns'] + ((st >> 16) & 0xFF)
    return torch.stack([ball, paddle], dim=-1).to(torch.int32)
  row, col = st & 0xFF, (st >> 8) & 0xFF
  return torch.where(row < g['size'], row * g['size'] + col, torch.full_like(row, -1)).to(torch.int32)[..., None]


# ------------------------------------------------------------------------------------- A. the eager step and the reference
@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_eager_step_against_the_oracle(family, kwargs, aligned):
  g = gu.grid(family, kwargs, aligned)
  e = eager(family, kwargs, aligned)
  ts, after = e['ts'][0], e['after'][0]
  orc, want = gu.oracle_step(g)
  _assert_vs_oracle(ts, want, family)
  for k, v in orc.bsuite_info().items():
    np.testing.assert_array_equal(after['info'][k].view(torch.float64).cpu().numpy(), v, err_msg=k)
  raw_info = after['raw_info'].view(torch.float64).cpu().numpy()
  state = after['state']['state'].cpu().numpy()
  pred = gu.predicates(g, orc, want)
  if family == 'catch':
    # the split of total_regret into the column and the pending field, not only their sum
    column, pending = gu.catch_expected(g, want)
    fold = pred['fold']
    assert fold.sum() >= gu.MIN_LANES
    np.testing.assert_array_equal(raw_info[0][fold], g['column'][fold] + 254.0, err_msg='the column after a fold')
    np.testing.assert_array_equal(raw_info[0][~fold], g['column'][~fold], err_msg='the column without a fold')
    got_pending = gu.pending_of(state)
    assert (got_pending[fold] == 0).all()
    other_miss = pred['lands_miss'] & ~fold
    np.testing.assert_array_equal(got_pending[other_miss], g['pending'][other_miss] + 1, err_msg='pending after any other miss')
    np.testing.assert_array_equal(got_pending, pending)
    np.testing.assert_array_equal(raw_info[0], column)
    np.testing.assert_array_equal(state < 0, pred['sign_bit_out'])
    # the position fields: the oracle's
    np.testing.assert_array_equal(state & 0xFF, orc.s['ball_x'])
    np.testing.assert_array_equal((state >> 8) & 0xFF, orc.s['ball_y'])
    np.testing.assert_array_equal((state >> 16) & 0xFF, orc.s['paddle_x'])
    np.testing.assert_array_equal((state >> 24) & 1, orc.reset_next)
  else:
    np.testing.assert_array_equal(raw_info[0], orc.info['total_bad_episodes'])
    np.testing.assert_array_equal(raw_info[1], orc.info['denoised_return'])
    np.testing.assert_array_equal(raw_info[1], gu.DS_HISTORY[1] + pred['corner_right_pays'])
    np.testing.assert_array_equal(raw_info[0], gu.DS_HISTORY[0] + pred['ends_bad'])
    np.testing.assert_array_equal(state & 0xFF, orc.s['row'])
    np.testing.assert_array_equal((state >> 8) & 0xFF, orc.s['col'])
    np.testing.assert_array_equal((state >> 16) & 1, orc.s['bad'])
    np.testing.assert_array_equal((state >> 17) & 1, orc.reset_next)
    np.testing.assert_array_equal((state >> 18) & 1, np.full(g['lanes'], (gu.STEP0 + 1) & 1))
  counters = after['counters'].cpu().numpy()
  assert counters.tolist() == [int((want[0] == 2).sum()), int((want[0] == 0).sum())]
  # the two steps that follow (random actions, resets inside) against the oracle as well: B compares with them
  acts = e['actions'].cpu().numpy()
  for t in range(1, T_MAX):
    want = tuple(v.copy() for v in orc.call(acts[t], gu.STEP0 + t))
    _assert_vs_oracle(e['ts'][t], want, (family, t))
    for k, v in orc.bsuite_info().items():
      np.testing.assert_array_equal(e['after'][t]['info'][k].view(torch.float64).cpu().numpy(), v, err_msg=f'{k} t={t}')


# ------------------------------------------------------------------------------------- B. every path equals the eager step
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_rollout_equals_eager_steps(family, kwargs, aligned, T):
  g, e = gu.grid(family, kwargs, aligned), eager(family, kwargs, aligned)
  # which side of csrc/bsx_pair_host.h the case is on: lanes * cells a multiple of 4 — ONE fused launch (boards of at most 128
  # cells) or the pipelined rollout; or not — lane advance + store stream per step, slice 1 through the 4-byte store path
  assert ((g['lanes'] * g['cells']) % 4 == 0) == (aligned or g['cells'] % 4 == 0)
  env = _make(family, kwargs, g['lanes'])
  gu.load(env, g)
  _assert_ts(_run(env, e['actions'], T, 'rollout'), _stack(e['ts'], T), (family, T, 'rollout'))
  _assert_after(_snap_after(env), e['after'][T - 1], (family, T, 'rollout'))
  if T > 1:
    assert bool((e['ts'][1]['step_type'] == 0).any()) and bool((e['ts'][2]['step_type'] == 0).any())      # resets inside the loop


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_index_paths_equal_the_eager_step(family, kwargs, aligned, T):
  g, e = gu.grid(family, kwargs, aligned), eager(family, kwargs, aligned)
  want = _stack(e['ts'], T)
  want_index = torch.stack([_index_rows(g, e['after'][t]['state']['state']) for t in range(T)])
  for path in ('step', 'rollout'):
    what = (family, T, 'index', path)
    env = _make(family, kwargs, g['lanes'], observation_mode='index')
    gu.load(env, g)
    got = _run(env, e['actions'], T, path)
    _assert_ts(got, want, what, fields=NO_OBS)
    assert torch.equal(got['observation'], want_index), (what, 'observation against the eager state decoded')
    dense = observations.index_to_dense(got['observation'], env.board_shape)
    assert torch.equal(_bits(dense), want['observation']), (what, 'observation against the eager board')
    _assert_after(_snap_after(env), e['after'][T - 1], what)


@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_delta_step_equals_the_eager_step(family, kwargs, aligned):
  g, e = gu.grid(family, kwargs, aligned), eager(family, kwargs, aligned)
  env = _make(family, kwargs, g['lanes'], observation_mode='delta')
  gu.load(env, g)
  _assert_ts(_run(env, e['actions'], T_MAX, 'step'), _stack(e['ts'], T_MAX), (family, 'delta'))
  _assert_after(_snap_after(env), e['after'][T_MAX - 1], (family, 'delta'))


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_narrow_dtype_paths_equal_the_eager_step(family, kwargs, aligned, T):
  g, e = gu.grid(family, kwargs, aligned), eager(family, kwargs, aligned)
  want = _stack(e['ts'], T)
  boards = want['observation'].view(torch.float32)
  for dtype in (torch.uint8, torch.bfloat16, torch.float16):
    for path in ('step', 'rollout'):
      what = (family, T, str(dtype), path)
      env = _make(family, kwargs, g['lanes'], observation_dtype=dtype)
      gu.load(env, g)
      assert env.observation_dtype == dtype
      got = _run(env, e['actions'], T, path)
      _assert_ts(got, want, what, fields=NO_OBS)
      assert torch.equal(got['observation'], _bits(boards.to(dtype))), (what, 'observation against the eager board re-encoded')
      _assert_after(_snap_after(env), e['after'][T - 1], what)


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_logging_paths_equal_the_eager_step(family, kwargs, aligned, T):
  """Under Logging catch counts nothing in the state word: pending is loaded as 0, its misses moved into the column."""
  g, e = gu.grid(family, kwargs, aligned), eager(family, kwargs, aligned)
  catch = family == 'catch'
  for path in ('step', 'rollout'):
    what = (family, T, 'Logging', path)
    env = wrappers.Logging(_make(family, kwargs, g['lanes']), None, max_rows=8)
    gu.load(env, g, fold_pending=catch)
    _assert_ts(_run(env, e['actions'], T, path), _stack(e['ts'], T), what)
    after = _snap_after(env)
    _assert_after(after, e['after'][T - 1], what, state_mask=PENDING_MASK if catch else None, raw_info=not catch)
    if catch:
      assert bool((after['state']['state'] >> 25 == 0).all()), (what, 'pending under Logging')
      assert torch.equal(after['raw_info'][0], e['after'][T - 1]['info']['total_regret']), (what, 'the column is the total')


def test_logging_takes_over_catch_pending_misses():
  """The hand-over: wrappers.Logging around an environment that holds pending misses (126, bit 31 set, among them) leaves
  pending 0 and the column equal to the oracle's sum."""
  family, kwargs, aligned = gu.CASES[0]
  g = gu.grid(family, kwargs, aligned)
  env = _make(family, kwargs, g['lanes'])
  gu.load(env, g)
  assert int((gu.pending_of(env._state['state'].cpu().numpy()) == 126).sum()) >= gu.MIN_LANES      # pylint: disable=protected-access
  before = env._state['state'].clone()                                                              # pylint: disable=protected-access
  logged = wrappers.Logging(env, None, max_rows=8)
  r = eu.raw(logged)
  assert torch.equal(r._state['state'], before & PENDING_MASK)                                      # pylint: disable=protected-access
  want = gu.make_oracle(g).info['total_regret']
  np.testing.assert_array_equal(r._info[0].cpu().numpy(), want)                                     # pylint: disable=protected-access
  np.testing.assert_array_equal(r.bsuite_info()['total_regret'].cpu().numpy(), want)
  assert want.max() == 254.0 * 3 + 2 * 126


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_reward_noise_paths_equal_the_eager_step(family, kwargs, aligned, T):
  """The reward is the base reward plus noise: not compared.  The info columns of the two families are functions of the
  base reward, the state and the action alone, so they are."""
  g, e = gu.grid(family, kwargs, aligned), eager(family, kwargs, aligned)
  fields = ('step_type', 'discount', 'observation')
  for path in ('step', 'rollout'):
    what = (family, T, 'RewardNoise', path)
    env = wrappers.RewardNoise(_make(family, kwargs, g['lanes']), noise_scale=0.1, seed=3)
    gu.load(env, g)
    got = _run(env, e['actions'], T, path)
    _assert_ts(got, _stack(e['ts'], T), what, fields=fields)
    _assert_after(_snap_after(env), e['after'][T - 1], what)
    live = e['ts'][0]['step_type'] != 0
    noisy = got['reward'].view(torch.float32)[0] != e['ts'][0]['reward'].view(torch.float32)
    assert float(noisy[live].float().mean()) > 0.99                             # the wrapper was in the kernel


@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_mt19937_step_equals_the_eager_step(family, kwargs, aligned):
  """T = 1 on every 17th row.  The rows whose step consumes a draw that shows (grid_edge_util.draw_rows: catch's reset rows,
  the moves right and the corners of the stochastic deep_sea) draw from another generator here: they must agree with the
  eager step in step type and discount, the others in everything."""
  g, e = gu.grid(family, kwargs, aligned), eager(family, kwargs, aligned)
  rows = gu.mt_rows(g)
  env = _make(family, kwargs, len(rows), rng='mt19937')
  gu.load(env, g, rows)
  rows_t = torch.from_numpy(rows).cuda()
  got = _snap_ts(env.step(e['actions'][0][rows_t].contiguous()))
  _assert_ts(got, e['ts'][0], (family, 'mt19937'), fields=('step_type', 'discount'), rows=rows_t)
  keep = torch.from_numpy(~gu.draw_rows(g)[rows]).cuda()
  assert int(keep.sum()) >= gu.MIN_LANES // 2                                   # (of the 121 rows of the smallest grids)
  for f in TS_FIELDS:
    assert torch.equal(got[f][keep], e['ts'][0][f][rows_t][keep]), (family, 'mt19937', f)
  after, want = _snap_after(env), e['after'][0]
  assert torch.equal(after['state']['state'][keep], want['state']['state'][rows_t][keep])
  assert torch.equal(after['raw_info'][:, keep], want['raw_info'][:, rows_t][:, keep])
  for k, w in want['info'].items():
    assert torch.equal(after['info'][k], w[rows_t]), (family, 'mt19937', k)      # no draw decides a column on the first step
  st = e['ts'][0]['step_type'][rows_t]
  assert after['counters'].tolist() == [int((st == 2).sum()), int((st == 0).sum())]


@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_reset_mask_and_mark_reset_on_the_grid(family, kwargs, aligned):
  """A seeded third of the lanes is marked: a marked catch lane keeps its pending count — 126 with the sign bit set
  included — and bsuite_info() equals the oracle's after the step."""
  g = gu.grid(family, kwargs, aligned)
  B = g['lanes']
  mask = np.random.default_rng(41).random(B) < 1.0 / 3.0
  mask_t = torch.from_numpy(mask).cuda()
  acts = torch.from_numpy(g['action']).cuda()
  orc = gu.make_oracle(g)
  orc.reset_next[mask] = 1
  want = tuple(v.copy() for v in orc.call(g['action'], gu.STEP0))
  assert (want[0][mask] == 0).all()
  env = _make(family, kwargs, B)
  gu.load(env, g)
  ts = _snap_ts(env.step(acts, reset_mask=mask_t))
  after = _snap_after(env)
  _assert_vs_oracle(ts, want, (family, 'reset_mask'))
  for k, v in orc.bsuite_info().items():
    np.testing.assert_array_equal(after['info'][k].view(torch.float64).cpu().numpy(), v, err_msg=k)
  assert after['counters'].tolist() == [int((want[0] == 2).sum()), int((want[0] == 0).sum())]
  if family == 'catch':
    state = after['state']['state'].cpu().numpy()
    np.testing.assert_array_equal(gu.pending_of(state)[mask], g['pending'][mask])
    held = mask & ~g['reset'] & (g['pending'] == 126)
    assert held.sum() >= 16 and (state[held] < 0).all()
    np.testing.assert_array_equal(after['raw_info'].view(torch.float64).cpu().numpy()[0][mask], g['column'][mask])
  # mark_reset(), then the plain step: the same words, the same TimeStep
  env2 = _make(family, kwargs, B)
  gu.load(env2, g)
  loaded = env2._state['state'].clone()                                           # pylint: disable=protected-access
  env2.mark_reset(mask_t.to(torch.uint8))
  bit = gu.CATCH_RESET_BIT if family == 'catch' else gu.DS_RESET_BIT
  assert torch.equal(env2._state['state'], torch.where(mask_t, loaded | bit, loaded))      # pylint: disable=protected-access
  np.testing.assert_array_equal(env2.bsuite_info()[list(orc.info)[0]].cpu().numpy(), gu.make_oracle(g).info[list(orc.info)[0]])
  _assert_ts(_snap_ts(env2.step(acts)), ts, (family, 'mark_reset'))
  _assert_after(_snap_after(env2), after, (family, 'mark_reset'))


# ------------------------------------------------------------------------------------- the eight closed-loop calls
def _closed_loop_calls(g, B, population, always_left=False):
  """(recording call, evaluating call, positional arguments, keywords): a seeded shared table / pair, or a population of 3
  with policy_index.  always_left: action 0 on every cell — a zero table, logits and a w2 bias that decide for action 0."""
  fam, kwargs = g['family'], g['kwargs']
  C, _, A = emb.geometry(fam, kwargs)
  S = C * g['columns'] if fam == 'catch' else C
  P = 3 if population else None
  lead = () if P is None else (P,)
  rng = np.random.RandomState(7)
  table = np.zeros(lead + (S,), np.uint8) if always_left else rng.randint(0, A, size=lead + (S,)).astype(np.uint8)
  logits = rng.standard_normal(lead + (S, A)).astype(np.float32)
  w1, w2 = emb.pair(C, A, 5, seed=0, P=P)
  if always_left:
    logits[..., 0] += np.float32(50.0)
    w2[..., 0, -1] += np.float32(1000.0)
    # action 0 is the argmax of every row of the logits and of the network on every pair of cells (the restatements of
    # tab_sample_util / embed_util); at temperature 0.01 the Gumbel noise cannot overturn a margin of 40 / 0.01
    assert not tsu.np_argmax(logits.reshape(-1, A).astype(np.float64)).any()
    assert float((logits[..., 0:1] - logits[..., 1:]).min()) > 40.0
    every = np.stack([m.reshape(-1) for m in np.meshgrid(np.arange(-1, C), np.arange(-1, C), indexing='ij')], axis=1)[:, :2 if fam == 'catch' else 1]
    assert not emb.np_select(w1, w2, every.astype(np.int32)).any()
  cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()             # noqa: E731
  table, logits, w1, w2 = cuda(table), cuda(logits), cuda(w1), cuda(w2)
  kw = dict(policy_index=(torch.arange(B, dtype=torch.int32, device='cuda') % 3).contiguous()) if population else {}
  draw = dict(kw, temperature=0.01 if always_left else 1.0, sample_seed=(1 << 40) + 77)
  return [('rollout_policy', 'evaluate_policy', (table,), kw), ('sample_policy', 'evaluate_sampled_policy', (logits,), draw),
          ('rollout_embedding', 'evaluate_embedding', (w1, w2), kw), ('sample_embedding', 'evaluate_sampled_embedding', (w1, w2), draw)]


def _check_evaluation(ev, orc_st, orc_r, what):
  n, total, done = pe.host_loop(orc_st, np.where(orc_st != 0, orc_r, 0.0))
  np.testing.assert_array_equal(ev.episodes.cpu().numpy(), n, err_msg=f'{what} episodes')
  np.testing.assert_array_equal(pe.bits(ev.return_sum.cpu().numpy()), pe.bits(total), err_msg=f'{what} return_sum')
  np.testing.assert_array_equal(pe.bits(ev.episode_return_sum.cpu().numpy()), pe.bits(done), err_msg=f'{what} episode_return_sum')


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_closed_loop_calls_equal_the_eager_step(family, kwargs, aligned, T):
  g = gu.grid(family, kwargs, aligned)
  B, A = g['lanes'], _num_actions(family)
  running = torch.from_numpy(~g['reset']).cuda()
  index = dict(observation_mode='index')
  for population in (False, True):
    for record, evaluate, args, kw in _closed_loop_calls(g, B, population):
      what = (family, T, record, 'population' if population else 'shared')
      env = _make(family, kwargs, B, **index)
      gu.load(env, g)
      ts, actions = getattr(env, record)(*args, T, **kw)
      assert set(actions[0][running].unique().tolist()) == set(range(A)), what
      assert bool((actions[0][~running] == 0).all()), what
      # the returned actions replayed through the eager step() of a twin loaded with the same grid
      twin = _make(family, kwargs, B, **index)
      gu.load(twin, g)
      want = _run(twin, actions, T, 'step')
      _assert_ts(_snap_ts(ts), want, what)
      want_after = _snap_after(twin)
      _assert_after(_snap_after(env), want_after, what)
      # ... and through the oracle: the float64 rewards of the steps, bsuite_info
      orc, orc_st, orc_r = gu.oracle_run(g, actions.cpu().numpy())
      np.testing.assert_array_equal(ts.step_type.cpu().numpy(), orc_st, err_msg=f'{what} step_type')
      live = orc_st != 0
      np.testing.assert_array_equal(eu.f32_bits(ts.reward.cpu().numpy()[live]), eu.f32_bits(orc_r[live].astype(np.float32)))
      for k, v in orc.bsuite_info().items():
        np.testing.assert_array_equal(env.bsuite_info()[k].cpu().numpy(), v, err_msg=f'{what} {k}')
      # the returns-only call with the same arguments: the same final state, the columns of the host loop over the steps
      what = (family, T, evaluate, 'population' if population else 'shared')
      env2 = _make(family, kwargs, B, **index)
      gu.load(env2, g)
      ev = getattr(env2, evaluate)(*args, T, **kw)
      _assert_after(_snap_after(env2), want_after, what)
      _check_evaluation(ev, orc_st, orc_r, what)


# ------------------------------------------------------------------------------------- grouped launches
GROUPED_MODES = ['whole_sweep', 'whole_sweep_streams', 'whole_sweep_pipelined', 'pair_mixed', 'pair_mixed_streams', 'per_family',
                 'per_family_streams']


@pytest.mark.parametrize('mode', GROUPED_MODES, ids=['catch_deep_sea_' + m for m in GROUPED_MODES])
def test_grouped_launches_equal_standalone_envs(mode):
  """A SweepBatch of catch/0 and deep_sea/0 with grid rows loaded into its segment environments before prepare_groups (each
  segment's own state_dict(), so its call index is kept): three grouped steps against stand-alone environments loaded with
  the same rows.  per_family: bsx_pair_advance_group_kernel; pair_mixed: pair_mixed_advance_kernel; whole_sweep: the sweep's
  phase 0; whole_sweep_pipelined: its pipelined kernel (the lanes run one advance ahead of the TimeSteps)."""
  ids, reps = ['catch/0', 'deep_sea/0'], 3
  grids = [gu.grid(*c) for c in gu.GROUPED_CASES]
  assert sweep.SETTINGS['deep_sea/0'] == gu.GROUPED_CASES[1][1] and (grids[0]['rows'], grids[0]['columns']) == (10, 5)
  lanes = max(g['lanes'] for g in grids)
  batch = sb.SweepBatch(ids, 2 * lanes, seed=gu.SEED)
  acts, refs = [], []
  for (bid, begin, n), env, g in zip(batch.segments, batch.envs, grids):
    assert n == lanes
    rows = np.arange(n) % g['lanes']
    gu.load(env, g, rows, step0=None)
    acts.append(torch.from_numpy(g['action'][rows]).cuda().contiguous())
    ref = bsuite_amd.load_from_id(bid, batch=n, lane_offset=begin, num_buffers=1, seed=gu.SEED)
    gu.load(ref, g, rows, step0=None)
    refs.append(ref)
  base = mode.replace('_streams', '')
  pipelined = base == 'whole_sweep_pipelined'
  batch.prepare_groups(acts, mix_all=base.startswith('whole_sweep'), mix_pairs=(base != 'per_family'),
                       mix_small=(base != 'per_family'), pipelined=pipelined)
  for s in range(reps):
    if mode.endswith('_streams'):
      outs = batch.step_grouped_streams()
      batch.join_streams()
    else:
      outs = batch.step_grouped()
    torch.cuda.synchronize()
    for bid, out, ref, a in zip(ids, outs, refs, acts):
      _assert_ts(_snap_ts(out), _snap_ts(ref.step(a)), (mode, bid, s))
  batch.sync()
  if pipelined:
    for ref, a in zip(refs, acts):
      ref.step(a)
  batch.release_groups()                         # (the lanes come back in the environments' own state columns)
  for bid, env, ref in zip(ids, batch.envs, refs):
    for k, v in ref.bsuite_info().items():
      assert torch.equal(_bits(env.bsuite_info()[k]), _bits(v)), (mode, bid, k)
    assert torch.equal(eu.raw(env).episode_counters(), eu.raw(ref).episode_counters()), (mode, bid)
    assert torch.equal(eu.raw(env).state_dict()['state'], eu.raw(ref).state_dict()['state']), (mode, bid, 'state')
    assert torch.equal(_bits(eu.raw(env)._info), _bits(eu.raw(ref)._info)), (mode, bid, 'info columns')      # pylint: disable=protected-access


# ------------------------------------------------------------------------------------- large batches, one step
CATCH_10X5, DEEP_SEA_30 = ('catch', dict(rows=10, columns=5)), ('deep_sea', dict(size=30, mapping_seed=42))
STEP1_MAX_LANES_30 = (1 << 30) // (900 * 4)       # the single-launch step takes at most 1 GiB of observations (csrc/deep_sea.hip)
LARGE = [pytest.param(CATCH_10X5, (1 << 20) + 257, id='catch_10x5_2p20_257'), pytest.param(DEEP_SEA_30, 1 << 18, id='deep_sea_30_2p18'),
         pytest.param(DEEP_SEA_30, (1 << 18) + 257, id='deep_sea_30_2p18_257'),
         pytest.param(DEEP_SEA_30, (1 << 18) + (1 << 16) + 1, id='deep_sea_30_2p18_2p16_1')]


@pytest.mark.parametrize('case,B', LARGE)
def test_large_batch_tiles_equal_the_small_batch(case, B):
  """The grid tiled to a large batch, ONE step, every tile the small-batch result of A.  catch at 2^20 + 257 lanes: 4097
  workgroups, the two-lanes-per-thread advance.  deep_sea N = 30: 2^18 and 2^18 + 257 lanes are the single-launch step, whose
  limit is 1 GiB of observations, 298261 lanes; 2^18 + 2^16 + 1 lanes are beyond it, lane advance + store stream.
  A catch reset row draws its ball's column by its global lane id, which differs from tile to tile: those rows are held to the
  oracle on their own lane ids instead."""
  family, kwargs = case
  assert (family, kwargs, False) in gu.CASES
  g, e = gu.grid(family, kwargs), eager(family, kwargs)
  if family == 'deep_sea':
    assert 1 << 18 < STEP1_MAX_LANES_30 == 298261 < (1 << 18) + (1 << 16) + 1
  rows = np.arange(B) % g['lanes']
  env = _make(family, kwargs, B)
  gu.load(env, g, rows)
  rows_t = torch.from_numpy(rows).cuda()
  got = _snap_ts(env.step(e['actions'][0][rows_t].contiguous()))
  after = _snap_after(env)
  st = e['ts'][0]['step_type'][rows_t]
  assert after['counters'].tolist() == [int((st == 2).sum()), int((st == 0).sum())]
  assert after['step_index'] == gu.STEP0 + 1
  drawn = gu.draw_rows(g)[rows]
  keep = torch.from_numpy(~drawn).cuda()
  want, want_after = e['ts'][0], e['after'][0]
  for f in TS_FIELDS:
    if drawn.any():
      assert torch.equal(got[f][keep], want[f][rows_t][keep]), (family, B, f)
    else:
      assert torch.equal(got[f], want[f][rows_t]), (family, B, f)
  for k, w in want_after['info'].items():
    assert torch.equal(after['info'][k], w[rows_t]), (family, B, k)
  assert torch.equal(after['raw_info'], want_after['raw_info'][:, rows_t])
  state = after['state']['state']
  if not drawn.any():
    assert torch.equal(state, want_after['state']['state'][rows_t])
    return
  assert torch.equal(state[keep], want_after['state']['state'][rows_t][keep])
  sel = np.flatnonzero(drawn)
  orc, (o_st, _, _, o_obs) = gu.oracle_step(g, rows[sel], lane_ids=np.uint64(gu.LANE_OFFSET) + sel.astype(np.uint64))
  sel_t = torch.from_numpy(sel).cuda()
  assert (o_st == 0).all() and bool((got['step_type'][sel_t] == 0).all())
  assert bool((got['reward'][sel_t] == 0).all()) and bool((got['discount'].view(torch.float32)[sel_t] == 1).all())
  np.testing.assert_array_equal(got['observation'][sel_t].view(torch.float32).cpu().numpy(), o_obs)
  words = gu.catch_words(orc.s['ball_x'], orc.s['ball_y'], orc.s['paddle_x'], g['pending'][rows[sel]])
  np.testing.assert_array_equal(state[sel_t].cpu().numpy(), words)
  assert len(set(orc.s['ball_x'].tolist())) == g['columns']


# ------------------------------------------------------------------------------------- C. several folds inside one call
_FOLD_TWINS = {}


def _fold_twin(mode, actions, B):
  """The eager step() of a twin loaded with the long-run grid, through `actions` [T, B]: cached for the always-left actions
  every path is expected to return (a path that returns others gets a replay of its own)."""
  key = (mode, B) if not bool(actions.any()) else None
  if key is None or key not in _FOLD_TWINS:
    g = gu.folds_grid(B)
    twin = _make('catch', g['kwargs'], g['lanes'], **(dict(observation_mode='index') if mode == 'index' else {}))
    gu.load(twin, g)
    snaps = [_snap_ts(twin.step(actions[t].contiguous())) for t in range(actions.shape[0])]
    out = dict(ts=_stack(snaps, len(snaps)), after=_snap_after(twin))
    if key is None:
      return out
    _FOLD_TWINS[key] = out
  return _FOLD_TWINS[key]


FOLD_PATHS = ['rollout', 'index_rollout', 'rollout_policy', 'sample_policy', 'rollout_embedding', 'sample_embedding',
              'evaluate_policy', 'evaluate_sampled_policy', 'evaluate_embedding', 'evaluate_sampled_embedding']


@pytest.mark.parametrize('lanes', gu.FOLD_LANES)
@pytest.mark.parametrize('path', FOLD_PATHS, ids=['catch_2x5_' + p for p in FOLD_PATHS])
def test_several_folds_inside_one_call(path, lanes):
  """ONE call of 600 always-left steps on the 2-row board from 120 pending misses: two folds on every lane, three on some
  (tests/test_grid_edges_host.py asserts that on the reference).  The four evaluate_* calls count their folds in a register
  and add 254 * folds once after the loop.  At 513 lanes lanes * cells is not a multiple of 4 and `rollout` is lane advance +
  store stream per step; at 514 it is ONE launch of bsx_fused_rollout_kernel with the folds inside its loop."""
  g = gu.folds_grid(lanes)
  B, T = g['lanes'], gu.FOLDS['calls']
  assert ((B * g['cells']) % 4 == 0) == (lanes == 514) == g['aligned']
  zeros = torch.zeros((T, B), dtype=torch.int32, device='cuda')
  calls = {c[0]: c for c in _closed_loop_calls(g, B, population=False, always_left=True)}
  calls.update({c[1]: c for c in calls.values()})
  mode = 'dense' if path == 'rollout' else 'index'
  env = _make('catch', g['kwargs'], B, **(dict(observation_mode='index') if mode == 'index' else {}))
  gu.load(env, g)
  ts = ev = None
  if path in ('rollout', 'index_rollout'):
    ts, actions = env.rollout(zeros), zeros
  elif path.startswith('evaluate'):
    record, _, args, kw = calls[path]
    ev = getattr(env, path)(*args, T, **kw)
    rec = _make('catch', g['kwargs'], B, observation_mode='index')            # its recording twin names the actions taken
    gu.load(rec, g)
    _, actions = getattr(rec, record)(*args, T, **kw)
  else:
    _, _, args, kw = calls[path]
    ts, actions = getattr(env, path)(*args, T, **kw)
  assert not bool(actions.any()), (path, 'an action other than left')
  twin = _fold_twin(mode, actions, B)
  if ts is not None:
    _assert_ts(_snap_ts(ts), twin['ts'], path)
  after = _snap_after(env)
  _assert_after(after, twin['after'], path)
  orc, orc_st, orc_r = gu.oracle_run(g, actions.cpu().numpy())
  if ev is not None:
    _check_evaluation(ev, orc_st, orc_r, path)
  column = after['raw_info'].view(torch.float64).cpu().numpy()[0]
  pending = gu.pending_of(after['state']['state'].cpu().numpy())
  assert (column % 254.0 == 0).all() and column.min() >= 508.0 and column.max() >= 762.0, (path, column.min(), column.max())
  assert pending.max() < gu.CATCH_PENDING_MAX
  np.testing.assert_array_equal(column + 2.0 * pending, orc.info['total_regret'])
  np.testing.assert_array_equal(env.bsuite_info()['total_regret'].cpu().numpy(), orc.info['total_regret'])
