"""CPU: the edge-state grid of tests/grid_edge_util.py, run through the C oracle alone.  The GPU test
(tests/test_gpu_grid_edges.py) is only worth what the grid reaches: every named branch predicate must hold on at least one
full wave of lanes, no row may be a word whose fields the lane advance cannot write, and the long run that the GPU test takes
for 'several folds inside one call' must really fold twice on every lane and three times on some — asserted here on the
reference, so that the GPU test cannot pass vacuously."""
import numpy as np
import pytest

from tests import grid_edge_util as gu

# (the deep_sea segment of the GPU test's grouped launches is a grid of its own: held to the same conditions)
ALL_CASES = gu.CASES + gu.GROUPED_CASES[1:]
CASE_PARAMS = [pytest.param(*c, id=gu.case_id(*c)) for c in ALL_CASES]


@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_grid_rows_are_words_the_library_writes(family, kwargs, aligned):
  g = gu.grid(family, kwargs, aligned)
  assert g['lanes'] > g['n_product'] and g['lanes'] >= gu.MIN_BLOCKS * gu.BLOCK + 1 and g['cells'] == gu.cells_of(family, kwargs)
  if aligned:         # the 16-byte side of csrc/bsx_pair_host.h, and still a ragged last wave; its twin is on the 4-byte side
    assert (g['lanes'] * g['cells']) % 4 == 0 and 2 <= g['lanes'] % gu.BLOCK <= 4
    assert (gu.grid(family, kwargs)['lanes'] * g['cells']) % 4 != 0 and (family, kwargs, False) in gu.CASES
  else:
    assert g['lanes'] % gu.BLOCK == 1
    assert (g['lanes'] * g['cells']) % 4 == 0 or (family, kwargs, True) in gu.CASES
  assert g['state'].dtype == np.int32 and g['info'].dtype == np.float64
  run, rst = ~g['reset'], g['reset']
  assert run.sum() >= gu.MIN_LANES and rst.sum() >= gu.MIN_LANES
  if family == 'catch':
    rows, cols = g['rows'], g['columns']
    assert set(np.unique(g['action']).tolist()) == {0, 1, 2}
    assert sorted(set(g['pending'].tolist())) == list(gu.PENDING) and g['pending'].max() <= gu.CATCH_PENDING_MAX - 1
    assert sorted(set(g['column'].tolist())) == list(gu.COLUMN)
    for k in ('ball_x', 'paddle_x'):
      assert g[k].min() == 0 and g[k].max() == cols - 1
    assert (g['ball_y'][run] <= rows - 2).all() and g['ball_y'][run].max() == rows - 2 and g['ball_y'].min() == 0
    # reset rows as a LAST step leaves them: the ball in the paddle's row, the reset bit, the pending field kept
    assert (g['ball_y'][rst] == rows - 1).all() and sorted(set(g['pending'][rst].tolist())) == list(gu.PENDING)
    w = g['state'].view(np.uint32).astype(np.int64)
    np.testing.assert_array_equal(w & 0xFF, g['ball_x'])
    np.testing.assert_array_equal((w >> 8) & 0xFF, g['ball_y'])
    np.testing.assert_array_equal((w >> 16) & 0xFF, g['paddle_x'])
    np.testing.assert_array_equal((w >> 24) & 1, g['reset'])
    np.testing.assert_array_equal(w >> 25, g['pending'])
    np.testing.assert_array_equal(gu.pending_of(g['state']), g['pending'])
    assert ((g['state'] < 0) == (g['pending'] >= 64)).all() and (g['state'] < 0).sum() >= gu.MIN_LANES      # bit 31 is data
    if rows == 64:
      assert g['ball_x'].max() == g['paddle_x'].max() == 63 and g['ball_y'].max() == 63
  else:
    N = g['size']
    assert set(np.unique(g['action']).tolist()) == {0, 1}
    assert (g['col'] <= g['row']).all() and (g['col'] <= N - 1).all() and (g['row'][run] <= N - 1).all()
    assert (g['row'][rst] == N).all() and set(g['bad'][rst].tolist()) == {0, 1} and set(g['bad'][run].tolist()) == {0, 1}
    cells = set(zip(g['row'][run].tolist(), g['col'][run].tolist()))
    assert cells == {(r, c) for r in range(N) for c in range(r + 1)}              # every cell of the triangle
    w = g['state'].astype(np.int64)
    np.testing.assert_array_equal(w & 0xFF, g['row'])
    np.testing.assert_array_equal((w >> 8) & 0xFF, g['col'])
    np.testing.assert_array_equal((w >> 16) & 1, g['bad'])
    np.testing.assert_array_equal((w >> 17) & 1, g['reset'])
    assert (w >> 18 == 0).all()                                                   # bit 18 belongs to load_state_dict
    assert (g['info'][0] == gu.DS_HISTORY[0]).all() and (g['info'][1] == gu.DS_HISTORY[1]).all()


@pytest.mark.parametrize('family,kwargs,aligned', CASE_PARAMS)
def test_every_branch_is_reached(family, kwargs, aligned):
  g = gu.grid(family, kwargs, aligned)
  orc, want = gu.oracle_step(g)
  st, reward = want[0], want[1]
  pred = gu.predicates(g, orc, want)
  assert tuple(pred) == gu.predicate_names(family, kwargs)
  for name, rows in pred.items():
    print(f'{gu.case_id(family, kwargs, aligned)} {name}: {int(rows.sum())} lanes')
    assert int(rows.sum()) >= gu.MIN_LANES, (name, int(rows.sum()))
  assert all((st == k).sum() >= gu.MIN_LANES for k in (0, 1, 2)) or (family == 'catch' and g['rows'] == 2)
  if family == 'catch':
    # the oracle's own accounting against the expected split of column and pending
    column, pending = gu.catch_expected(g, want)
    np.testing.assert_array_equal(orc.info['total_regret'], column + 2.0 * pending)
    assert pending.max() <= gu.CATCH_PENDING_MAX - 1 and (pending[pred['fold']] == 0).all()
    assert (column[pred['fold']] == g['column'][pred['fold']] + 254.0).all() and (column[~pred['fold']] == g['column'][~pred['fold']]).all()
    assert (pred['sign_bit_in'] & ~pred['sign_bit_out']).sum() >= gu.MIN_LANES      # a fold clears bit 31
    assert (~pred['sign_bit_in'] & pred['sign_bit_out']).sum() >= gu.MIN_LANES      # the miss at 63 sets it
  else:
    live = st != 0
    pays = pred['corner_right_pays']
    np.testing.assert_array_equal(orc.info['denoised_return'], gu.DS_HISTORY[1] + pays)
    np.testing.assert_array_equal(orc.info['total_bad_episodes'], gu.DS_HISTORY[0] + pred['ends_bad'])
    if g['deterministic']:
      mc = g['move_cost']
      assert (reward[pays] == 1.0 - mc).all() and set(np.unique(reward[live & ~pays]).tolist()) == {0.0, 0.0 - mc}
    else:
      noisy = pred['noise_drawn']
      assert len(np.unique(reward[noisy])) > noisy.sum() // 2                     # a normal draw per lane
    assert (orc.s['bad'][pred['sets_bad']] == 1).all()


@pytest.mark.parametrize('lanes', gu.FOLD_LANES)
def test_one_call_of_600_steps_folds_at_least_twice_on_every_lane(lanes):
  """The condition of the GPU test's part C: from 120 pending misses, always-left for 600 calls on the 2-row board, every
  lane misses at least 134 more times (120 + misses >= 254: two folds), and at least one lane reaches three.  At 513 lanes,
  and at the 514 at which a rollout of this board is one fused launch."""
  g = gu.folds_grid(lanes)
  assert g['aligned'] == (lanes == 514) and lanes % 64 in (1, 2)
  T = gu.FOLDS['calls']
  orc, st, r = gu.oracle_run(g, np.zeros((T, g['lanes']), np.int32))
  misses = ((st == 2) & (r == -1.0)).sum(axis=0)
  folds = (gu.FOLDS['pending'] + misses) // gu.CATCH_PENDING_MAX
  print(f'misses per lane {misses.min()} .. {misses.max()}, folds {np.bincount(folds).tolist()}')
  np.testing.assert_array_equal(orc.info['total_regret'], 2.0 * (gu.FOLDS['pending'] + misses))
  assert misses.min() >= 134 and folds.min() >= 2
  assert folds.max() >= 3
