"""CPU: the edge-state grid of tests/physics_edge_util.py, run one step through the float64 reference alone.  The GPU
test (tests/test_gpu_physics_edges.py) is only worth what the grid reaches: every named branch predicate must hold on at
least one full wave of lanes, and the lanes that the tie rules (engine_util.physics_ties plus the mountain_car wall rule)
would waive must be at most 1 % of the grid — a condition that keeps the GPU test from hiding a failure, not a tolerance:
the reference alone has to satisfy it here."""
import numpy as np
import pytest

from tests import physics_edge_util as pu


@pytest.mark.parametrize('family,kwargs', pu.CASES, ids=pu.CASE_IDS)
def test_grid_values_are_float32_and_the_lane_count_is_ragged(family, kwargs):
  g = pu.grid(family, kwargs)
  np.testing.assert_array_equal(g['state'], g['state'].astype(np.float32).astype(np.float64))
  assert g['lanes'] % pu.BLOCK == 1 and g['lanes'] > g['n_product'] and g['lanes'] - g['n_product'] <= pu.BLOCK
  assert (g['k'] >= 0).all() and (g['k'] & pu.RESET_BIT == 0).all()
  assert set(np.unique(g['action']).tolist()) == {0, 1, 2}
  if family != 'mountain_car':
    assert np.abs(g['state'][:, 3]).max() == 700.0
    # the reference's own replay: the step after last_step - 1 is the first whose time exceeds max_time
    assert g['sums'][g['last_step']] > kwargs.get('max_time', 10.) >= g['sums'][g['last_step'] - 1]
    assert (g['last_step'] + 1) * 4 > 16384 if kwargs else (g['last_step'] + 1) * 4 <= 16384      # device memory / LDS table
  else:
    assert (g['max_steps'] + 1) * 4 > 16384 if kwargs else (g['max_steps'] + 1) * 4 <= 16384


# (a grouped segment that is no case of its own is held to the same conditions)
@pytest.mark.parametrize('family,kwargs', pu.CASES + pu.GROUPED_CASES, ids=pu.CASE_IDS + ['grouped_' + c[0] for c in pu.GROUPED_CASES])
def test_every_branch_is_reached_and_few_lanes_tie(family, kwargs):
  g = pu.grid(family, kwargs)
  orc, want = pu.oracle_step(g)
  st, reward, _, obs = want
  assert np.isfinite(obs).all() and np.abs(obs).max() < 1000.0
  assert (st != 0).all()                                            # no row resets at step 0: every lane was running
  pred = pu.predicates(g, orc, want)
  mt_rows = pu.mt_rows(g)
  for name in pu.PREDICATES[family]:
    n = int(pred[name].sum())
    print(f'{family} {kwargs} {name}: {n} lanes, {int(pred[name][mt_rows].sum())} among the mt19937 rows')
    assert n >= pu.MIN_LANES, (name, n)
    assert int(pred[name][mt_rows].sum()) >= pu.MIN_LANES, (name, 'rows of the mt19937 environment')
  # both sides of the seeded reset mask of the GPU file's test_reset_mask_and_mark_reset_on_the_grid
  mask = np.random.default_rng(41).random(g['lanes']) < 1.0 / 3.0
  for name in pu.PREDICATES[family]:
    assert (pred[name] & ~mask).sum() >= pu.MIN_LANES // 2 and (pred[name] & mask).sum() >= 8, name
  first = pu.oracle_step(g, reset_mask=mask)[1][0] == 0
  np.testing.assert_array_equal(first, mask)                        # the reference called with reset() on exactly those lanes
  # both outcomes of LAST, and the time-out lanes end
  assert (st[pred['mc_timeout' if family == 'mountain_car' else 'timeout']] == 2).all()
  assert (st == 1).sum() >= pu.MIN_LANES and (st == 2).sum() >= pu.MIN_LANES
  ties = pu.threshold_ties(g, orc)
  walls = pu.wall_ties(g)
  print(f'{family} {kwargs}: {int(ties.sum())} threshold ties, {int(walls.sum())} wall ties in {g["lanes"]} lanes')
  assert int((ties | walls).sum()) <= pu.MAX_WAIVED * g['lanes']
  # the info accounting of a running episode of k steps: the reference's columns after the step
  k = g['k'].astype(np.float64)
  if family == 'mountain_car':
    np.testing.assert_array_equal(orc.info['raw_return'], -(k + 1.0))
  elif family == 'cartpole':
    np.testing.assert_array_equal(orc.info['raw_return'], k + reward)
    last = st == 2
    np.testing.assert_array_equal(orc.info['best_episode'][last], (k + reward)[last])
    assert (orc.info['best_episode'][~last] == 0.0).all()
  else:
    np.testing.assert_array_equal(orc.info['raw_return'], 0.25 * k + reward)
    np.testing.assert_array_equal(orc.info['total_upright'], pred['up_true'].astype(np.float64))


def test_the_wall_rule_accepts_only_the_two_velocities():
  g = pu.grid('mountain_car', {})
  _, want = pu.oracle_step(g)
  obs = want[3]
  same, used = pu.apply_wall_rule(g, obs, obs)
  np.testing.assert_array_equal(same, obs)
  assert not used.any()
  # a lane in the window whose device velocity is max(v, 0): accepted, counted; any other lane or velocity: unchanged
  fake = dict(g)
  state = g['state'].copy()
  pos = -1.15
  for _ in range(50):                                               # pos + (-0.05 + cos(3 pos) * -0.0025) == -1.2, action 1
    pos = -1.2 + 0.05 + np.cos(3.0 * pos) * 0.0025
  state[0] = (np.float32(pos), np.float32(-0.05))
  fake['state'] = state
  action = g['action'].copy(); action[0] = 1
  fake['action'] = action
  assert pu.wall_ties(fake)[0]
  got = obs.copy().reshape(g['lanes'], -1)
  ref = got.copy()
  ref[0, 1] = -0.05
  got[0, 1] = 0.0
  got[1, 1] = 0.5
  alt, used = pu.apply_wall_rule(fake, got, ref)
  assert used[0] and alt[0, 1] == 0.0 and used.sum() == 1
  np.testing.assert_array_equal(alt[1:], ref[1:])
  got[0, 1] = -0.01                                                 # neither the reference's nor its clamp
  alt, used = pu.apply_wall_rule(fake, got, ref)
  assert used[0] and alt[0, 1] == 0.0 and abs(got[0, 1] - alt[0, 1]) > 1e-6      # the bound then fails on it
