"""CPU: the mixed-phase edge grid of tests/chain_edge_util.py, run through the C oracle alone.  The GPU test
(tests/test_gpu_chain_edges.py) is only worth what the grid reaches: every named branch predicate must hold on at least one
full wave of lanes in every case where it can occur, running and reset rows must each fill a wave, no row may be a word the
kernels cannot write (checked by decoding the packed word back into its fields), and the long calls the GPU test takes for
'several episodes inside one call' must really end episodes on every step — asserted here on the reference, so that the GPU
test cannot pass vacuously."""
import numpy as np
import pytest

from tests import chain_edge_util as cu

ALL_CASES = cu.CASES + cu.GROUPED_CASES      # (a grouped segment that is no case of its own is held to the same conditions)
CASE_PARAMS = [pytest.param(*c, id=cu.case_id(*c)) for c in ALL_CASES]


def test_the_cases_are_the_ones_the_kernels_branch_on():
  assert len(set(cu.CASE_IDS)) == len(cu.CASES) == 21
  kinds = {cu.case_id(*c): cu.rollout_class(*c) for c in cu.CASES}
  assert kinds['memory_chain_L4095_nb1'] == 'regs_lean_table' and kinds['memory_chain_L4096_nb1'] == 'regs_lean'
  assert kinds['memory_chain_L1_nb6'] == 'generic_lean' and kinds['memory_chain_L5_nb3'] == 'generic_lean'
  assert kinds['memory_chain_L5_nb40'] == 'packed_tile' and kinds['umbrella_chain_L4_nd5'] == 'generic_lean'
  assert kinds['umbrella_chain_L100_nd0'] == 'generic_lean' and kinds['umbrella_chain_L20_nd100'] == 'packed_tile'
  assert set(kinds.values()) == {'regs_lean_table', 'regs_lean', 'generic_lean', 'packed_tile'}
  assert max(cu.numel_of(*c) for c in ALL_CASES) == 103
  # the time field is 20 bits wide: the longest chain the library accepts leaves room for t = L + 1
  assert cu.MAX_CHAIN + 1 < 1 << 20


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_grid_rows_are_words_the_library_writes(family, kwargs):
  g = cu.grid(family, kwargs)
  assert g['lanes'] > g['n_product'] and g['lanes'] >= cu.MIN_BLOCKS * cu.BLOCK + 1 and g['lanes'] % cu.BLOCK == 1
  assert g['state'].dtype == np.int32 and g['info'].dtype == np.float64 and g['action'].dtype == np.int32
  run, rst = ~g['reset'], g['reset']
  assert run.sum() >= cu.MIN_LANES and rst.sum() >= cu.MIN_LANES
  w = g['state'].astype(np.int64)
  assert (w >= 0).all()
  if family == cu.MC:
    L, nb = g['L'], g['nb']
    np.testing.assert_array_equal(w & 0xFFFFF, g['t'])
    np.testing.assert_array_equal((w >> 20) & 0xFF, g['query'])
    np.testing.assert_array_equal((w >> 28) & 1, g['reset'])
    assert (w >> 29 == 0).all()
    assert (g['t'][run] <= L).all() and (g['t'][rst] == L + 1).all() and g['t'].min() == 0
    assert set(g['t'][run].tolist()) == {min(max(t, 0), L) for t in (0, 1, L // 2, L - 2, L - 1, L)}
    assert set(g['query'].tolist()) == {q for q in (0, 1, 31, 32, nb - 2, nb - 1) if 0 <= q < nb}
    assert g['ctx'].dtype == np.int64 and (g['ctx'] >= 0).all() and (g['ctx'] >> nb == 0).all()
    qbit = (g['ctx'] >> g['query']) & 1
    full = (1 << nb) - 1
    for rows in (run, rst):                                    # the bit at `query` both ways; the others all 0, all 1, neither
      assert set(qbit[rows].tolist()) == {0, 1}
      others = g['ctx'][rows] | (1 << g['query'][rows])
      assert (others == full).any() and ((g['ctx'][rows] & ~(1 << g['query'][rows])) == 0).any()
      assert nb < 8 or ((others != full) & ((g['ctx'][rows] & ~(1 << g['query'][rows])) != 0)).sum() >= cu.MIN_LANES
    if nb > 32:
      assert ((g['ctx'] >> 32) != 0).sum() >= cu.MIN_LANES and (g['query'] >= 32).sum() >= cu.MIN_LANES
    assert set(g['action'].tolist()) == {0, 1}
    assert g['info'].shape == (2, g['lanes']) and (g['info'][0] == g['info'][1]).all() and set(g['info'][0].tolist()) == {0.0, cu.BIG}
  elif family == cu.UC:
    L = g['L']
    np.testing.assert_array_equal(w & 0xFFFFF, g['t'])
    np.testing.assert_array_equal((w >> 20) & 1, g['need'])
    np.testing.assert_array_equal((w >> 21) & 1, g['has'])
    np.testing.assert_array_equal((w >> 22) & 1, g['reset'])
    assert (w >> 23 == 0).all()
    assert (g['t'][run] <= L - 1).all() and (g['t'][rst] == L).all()
    assert set(g['t'][run].tolist()) == {min(max(t, 0), L - 1) for t in (0, 1, L // 2, L - 2, L - 1)}
    for rows in (run, rst):
      assert set(zip(g['need'][rows].tolist(), g['has'][rows].tolist(), g['action'][rows].tolist())) == {
          (n, h, a) for n in (0, 1) for h in (0, 1) for a in (0, 1)}
    assert g['info'].shape == (1, g['lanes']) and set(g['info'][0].tolist()) == {0.0, cu.BIG}
  else:
    np.testing.assert_array_equal(w & 0xFF, g['t'])
    np.testing.assert_array_equal(((w >> 8) & 0xF) - 6, g['ctx'])
    np.testing.assert_array_equal((w >> 12) & 1, g['reset'])
    assert (w >> 13 == 0).all()
    assert set(g['t'][run].tolist()) == {0, 1, 2, 3, 9, 10, 29, 30, 98, 99} and (g['t'][rst] == 100).all()
    assert (g['ctx'][run & (g['t'] == 0)] == -1).all()
    for rows in (run & (g['t'] > 0), rst):
      assert set(g['ctx'][rows].tolist()) == set(range(-5, 5)) and set(g['action'][rows].tolist()) == set(range(-5, 5))
    assert set(g['action'][run & (g['t'] == 0)].tolist()) == set(range(-5, 5)) | {-6, 5, cu.INT_MIN, cu.INT_MAX}
    assert (np.abs(g['action'][g['t'] > 0].astype(np.int64)) <= 5).all()        # out-of-range actions on t == 0 rows only
    assert (g['info'] == 0).all()


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_every_branch_is_reached(family, kwargs):
  g = cu.grid(family, kwargs)
  orc, want = cu.oracle_step(g)
  st, reward, discount, obs = want
  pred = cu.predicates(g, want)
  assert tuple(pred) == cu.predicate_names(family, kwargs)
  for name, rows in pred.items():
    print(f'{cu.case_id(family, kwargs)} {name}: {int(rows.sum())} lanes')
    assert int(rows.sum()) >= cu.MIN_LANES, (name, int(rows.sum()))
  all_names = {cu.MC: cu.MC_PREDICATES, cu.UC: cu.UC_PREDICATES, cu.DC: cu.DC_PREDICATES}[family]
  for name in set(all_names) - set(pred):                     # left out only where it cannot occur
    assert (name == 'query_in_high_word' and g['nb'] <= 32) or (name == 'mid_drawn_reward' and g['L'] == 1), name
  # the oracle's own accounting against the expected movement of the info columns
  info = cu.expected_info(g, want)
  for j, v in enumerate(orc.bsuite_info().values()):
    np.testing.assert_array_equal(v, info[j])
  if family != cu.DC:
    moved = (info != g['info']).any(axis=0)
    np.testing.assert_array_equal(moved, (st == 2) if family == cu.MC else pred['ends_mismatch'])      # a match moves nothing
    assert (moved & (g['info'][-1] == cu.BIG)).sum() >= cu.MIN_LANES            # ... and from 2^24 + 1 on a wave of lanes
    assert float(np.float32(cu.BIG)) != cu.BIG and float(np.float32(cu.BIG + 2.0)) != cu.BIG + 2.0      # no f32 holds them
  # the state the oracle is left in is again a word of the family
  words, ctx = cu.oracle_words(g, orc)
  assert (words >= 0).all()
  if family == cu.MC:
    L = g['L']
    np.testing.assert_array_equal((words & 0xFFFFF) == L + 1, st == 2)
    first = st == 0
    assert (obs[first, 0, 0] == 1.0).all() and (np.abs(obs[first, 0, 2:]) == 1.0).all()
    shown = pred['first_obs_shows_context']
    bits = (g['ctx'][:, None] >> np.arange(g['nb'])[None]) & 1
    np.testing.assert_array_equal(obs[shown, 0, 2:], (2 * bits[shown] - 1).astype(np.float32))
    q = pred['shows_query']
    np.testing.assert_array_equal(obs[q, 0, 1], g['query'][q].astype(np.float32))
    assert (ctx[~first] == g['ctx'][~first]).all()
    hit = g['action'] == ((g['ctx'] >> g['query']) & 1)
    np.testing.assert_array_equal(pred['ends_hit'], (st == 2) & hit)
    if g['nb'] > 32:
      assert (pred['query_in_high_word'] & pred['ends_hit']).sum() >= 16 and (pred['query_in_high_word'] & pred['ends_miss']).sum() >= 16
  elif family == cu.UC:
    sets = pred['action_sets_has']
    np.testing.assert_array_equal(orc.s['has'][sets], g['action'][sets])
    assert (sets & (g['action'] != g['has'])).sum() >= cu.MIN_LANES              # ... and changes it
    keep = ~g['reset'] & ~sets
    np.testing.assert_array_equal(orc.s['has'][keep], g['has'][keep])
    if g['L'] == 1:
      assert (sets == (st == 2)).all()                                          # t == 1 is both
    else:
      mid = pred['mid_drawn_reward']
      assert set(reward[mid].tolist()) == {-1.0, 1.0}
  else:
    bonus = kwargs['mapping_seed'] % 5
    for k, chain in zip(cu.PAY_STEPS, range(5)):
      rows = pred[f'pays_at_{k}']
      assert set(np.unique(reward[rows]).tolist()) == {1.1 if chain == bonus else 1.0}
    ctx_after = orc.s['context']
    assert set(ctx_after[pred['chooses_context']].tolist()) == set(range(-5, 5))
    assert set(ctx_after[pred['pays_bonus']].tolist()) == {bonus, bonus - 5}
    assert (pred['pays_on_last'] == pred['pays_at_100']).all() and (pred['pays_bonus'] & pred['pays_on_last']).any() == (bonus == 4)
    assert set(g['action'][pred['invalid_action']].tolist()) == {-6, 5, cu.INT_MIN, cu.INT_MAX}
    np.testing.assert_array_equal(ctx_after[pred['invalid_action']], np.where(g['action'][pred['invalid_action']] < 0, 0, 4))
  assert all((st == k).sum() >= cu.MIN_LANES for k in (0, 2)) and ((st == 1).sum() >= cu.MIN_LANES or 'mid_drawn_reward' not in pred)
  # the two steps the GPU test takes after it reset lanes inside the run: FIRST at calls 6 and 7
  _, sts, _, _ = cu.oracle_run(g, cu.episode_actions(g, 3))
  assert (sts[1] == 0).sum() >= cu.MIN_LANES and ((sts[2] == 0).sum() >= cu.MIN_LANES or (family == cu.UC and g['L'] > 1))


def test_the_rows_left_to_other_generators_leave_every_branch_covered():
  """What the tiled and the mt19937 tests of the GPU file leave out (draw_rows) are reset rows alone: every other predicate
  keeps all its rows."""
  for family, kwargs in ALL_CASES:
    g = cu.grid(family, kwargs)
    drawn = cu.draw_rows(g)
    _, want = cu.oracle_step(g)
    for name, rows in cu.predicates(g, want).items():
      if name != 'resets':
        assert not (rows & drawn).any() and rows.sum() >= cu.MIN_LANES, (family, kwargs, name)
    assert (drawn == g['reset']).all() or family == cu.DC
    # what the GPU test asserts about its own subsets: every predicate among the mt19937 rows, and on both sides of the
    # seeded reset mask of test_reset_mask_and_mark_reset_on_the_grid
    mask = np.random.default_rng(41).random(g['lanes']) < 1.0 / 3.0
    for name, rows in cu.predicates(g, want).items():
      assert rows[cu.mt_rows(g)].any(), (family, kwargs, name)
      assert (rows & ~mask).sum() >= cu.MIN_LANES // 2 and (rows & mask).sum() >= 8, (family, kwargs, name)
    assert (mask & ~g['reset']).sum() >= cu.MIN_LANES and (family != cu.UC or (want[0][cu.mt_rows(g)] == 2).sum() >= 8)
    # (the mt19937 environment holds every 17th row, 121 of them: half a wave of those is compared in full)
    assert len(cu.mt_rows(g)) >= cu.MIN_LANES and (~drawn[cu.mt_rows(g)]).sum() >= cu.MIN_LANES // 2


@pytest.mark.parametrize('family,kwargs,T,episodes', cu.EPISODE_CASES, ids=[cu.case_id(*c[:2]) for c in cu.EPISODE_CASES])
def test_one_call_ends_several_episodes_on_every_lane_from_mixed_phases(family, kwargs, T, episodes):
  """The conditions of the GPU test's part C, on the reference."""
  g = cu.mixed_grid(family, kwargs)
  # (a discounting_chain lane holds the reset word on 1 call in 101)
  assert g['lanes'] % cu.BLOCK == 1 and g['reset'].sum() >= (16 if family == cu.DC else cu.MIN_LANES)
  acts = cu.episode_actions(g, T)
  orc, st, r, _ = cu.oracle_run(g, acts)
  ends = (st == 2).sum(axis=0)
  print(f'{cu.case_id(family, kwargs)}: episodes per lane {ends.min()} .. {ends.max()}, ending lanes per step '
        f'{(st == 2).sum(axis=1).min()} .. {(st == 2).sum(axis=1).max()}')
  assert ends.min() >= episodes
  assert ((st == 2).sum(axis=1) > 0).all() and ((st == 0).sum(axis=1)[1:] > 0).all()      # mixed phases: ends on every step
  assert ((st == 1).sum(axis=1) > 0).all()
  if family == cu.DC:
    for k in cu.PAY_STEPS:
      t_in_episode = np.zeros_like(st, dtype=np.int64)                          # the step of the episode each call is
      t = g['t'].copy()
      for s in range(T):
        t = np.where(st[s] == 0, 0, t + 1)
        t_in_episode[s] = t
      lanes = ((r != 0.0) & (t_in_episode == k)).any(axis=0)
      assert lanes.sum() >= cu.MIN_LANES, (k, int(lanes.sum()))
    assert ((r == 1.1) & (st == 2)).any(axis=0).sum() >= cu.MIN_LANES           # the bonus on the LAST step
  else:
    hit, miss = ((st == 2) & (r == 1.0)).any(axis=0), ((st == 2) & (r == -1.0)).any(axis=0)
    assert hit.sum() >= cu.MIN_LANES and miss.sum() >= cu.MIN_LANES
    want = {cu.MC: lambda: [((st == 2) & (r == 1.0)).sum(axis=0), 2.0 * ((st == 2) & (r == -1.0)).sum(axis=0)],
            cu.UC: lambda: [2.0 * ((st == 2) & (r == -1.0)).sum(axis=0)]}[family]()
    for v, w in zip(orc.bsuite_info().values(), want):
      np.testing.assert_array_equal(v, w)
