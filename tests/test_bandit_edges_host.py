"""CPU: the mixed-phase edge grid of tests/bandit_edge_util.py, run through the C oracle alone.  The GPU test
(tests/test_gpu_bandit_edges.py) is only worth what the grid reaches: every named branch predicate must hold on at least one
full wave of lanes in every case where it can occur, on both sides of the seeded reset mask the GPU test marks; no row may be
a word the kernels cannot write; the reference must say FIRST exactly on the reset rows and LAST on the others; and the
expected movement of the regret column must be the reference's own, bit for bit.  Also here: the one host-side check of
environments/mnist.py (a label that does not fit the four bits of the state word is refused)."""
import numpy as np
import pytest

from bsuite_amd.environments import mnist
from tests import bandit_edge_util as bu

CASE_PARAMS = [pytest.param(*c, id=i) for c, i in zip(bu.CASES, bu.CASE_IDS)]
MNIST_PARAMS = [p for p, c in zip(CASE_PARAMS, bu.CASES) if c[0] == bu.MN]


def test_the_cases_are_the_ones_the_kernels_branch_on():
  assert len(set(bu.CASE_IDS)) == len(bu.CASES) == 9
  arms = [bu.num_actions_of(kw) for f, kw in bu.CASES if f == bu.BD]
  assert sorted(arms) == [1, 11, 11, bu.MAX_ARMS]
  # linspace(0, 1, 32) is inexact in binary, and so is 1 - reward: the f64 addition to the regret column rounds
  r = bu.rewards_of(dict(mapping_seed=0, num_actions=bu.MAX_ARMS))
  assert sorted(r.tolist()) == np.linspace(0, 1, bu.MAX_ARMS).tolist() and (r * 31 != np.rint(r * 31)).any()
  assert bu.rewards_of(dict(mapping_seed=0, num_actions=1)).tolist() == [0.0]
  shapes = {kw['dataset']: bu.dataset(kw['dataset'])[0].shape for f, kw in bu.CASES if f == bu.MN}
  assert shapes == {'28x28': (96, 28, 28), '2x2_one': (1, 2, 2), '10x10': (300, 10, 10), '64x64': (64, 64, 64),
                    '2x2_2p24': (bu.MN_MAX_DATA, 2, 2)}
  assert 64 * 64 == 4096 and (10 * 10 * 1) % 16 != 0                           # the widest row; rows that are no multiple of 16 bytes
  # the largest table is beyond the 32 MiB of L2 (csrc/mnist.hip: non-temporal stores), and is the only one
  big = {name: int(np.prod(s)) > (32 << 20) for name, s in shapes.items()}
  assert big == {'28x28': False, '2x2_one': False, '10x10': False, '64x64': False, '2x2_2p24': True}
  assert float(np.float32(bu.BIG)) != bu.BIG and bu.BIG + 2.0 != float(np.float32(bu.BIG + 2.0))      # no f32 holds them


@pytest.mark.parametrize('family,kwargs', MNIST_PARAMS)
def test_the_tables_cover_every_byte_and_have_distinct_rows(family, kwargs):
  images, labels = bu.dataset(kwargs['dataset'])
  assert images.dtype == np.int8 and labels.dtype == np.uint8 and len(images) == len(labels)
  assert bu.rows_are_distinct(kwargs['dataset'])                                # so the index a reset drew is read off its image
  if images.size >= 4096:
    assert set(np.unique(images).tolist()) == set(range(-128, 128))
  assert (images < 0).any() or images.size < 64                                 # bytes of 128 and above
  assert labels.max() <= 15 and ((labels > 9).any() == (kwargs['dataset'] == '10x10'))
  # the image of every index comes back from its observation
  g = bu.grid(family, kwargs)
  idx = np.unique(g['idx'])
  obs = images.reshape(len(images), -1)[idx].astype(np.float32) / np.float32(255)
  np.testing.assert_array_equal(bu.drawn_index(g, obs), idx)


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_grid_rows_are_words_the_library_writes(family, kwargs):
  g = bu.grid(family, kwargs)
  assert g['lanes'] > g['n_product'] and g['lanes'] >= 8 * bu.BLOCK + 1 and g['lanes'] % bu.BLOCK == 1
  assert g['state'].dtype == np.int32 and g['info'].dtype == np.float64 and g['action'].dtype == np.int32
  assert g['info'].shape == (1, g['lanes'])
  run, rst = ~g['reset'], g['reset']
  assert run.sum() >= bu.MIN_LANES and rst.sum() >= bu.MIN_LANES
  w = g['state'].astype(np.int64)
  if family == bu.BD:
    na = g['na']
    np.testing.assert_array_equal(w, g['reset'])
    want = {bu.INT_MIN, -1, 0, 1, na // 2, na - 2, na - 1, na, na + 1, bu.INT_MAX}
    if na == 1:
      want = {bu.INT_MIN, -1, 0, 1, 2, bu.INT_MAX}                              # (1 = na and 2 = na + 1: no such arms)
    for rows in (run, rst):
      assert want <= set(g['action'][rows].tolist()) <= want | {int(np.argmax(g['rewards'])), int(np.argmin(g['rewards']))}
      assert set(g['info'][0][rows].tolist()) == {0.0, bu.SMALL_REGRET, bu.BIG}
  else:
    nd = g['num_data']
    labels = bu.dataset(kwargs['dataset'])[1]
    np.testing.assert_array_equal(w & 0xFFFFFF, g['idx'])
    np.testing.assert_array_equal((w >> 24) & 0xF, labels[g['idx']])
    np.testing.assert_array_equal((w >> 28) & 1, g['reset'])
    np.testing.assert_array_equal((w >> 29) & 1, ~g['reset'])
    assert (w >= 0).all() and (w >> 30 == 0).all()
    assert set(g['idx'].tolist()) == {i for i in (0, 1, nd // 2, nd - 2, nd - 1) if 0 <= i < nd}
    if nd == bu.MN_MAX_DATA:
      assert (w & 0xFFFFFF == 0xFFFFFF).sum() >= bu.MIN_LANES                   # the index field full, next to the label
    for rows in (run, rst):
      a, lab = g['action'][rows].astype(np.int64), g['label'][rows]
      assert {bu.INT_MIN, -1, 0, 9, 10, 15, bu.INT_MAX} <= set(a.tolist())
      assert {-1, 0, 1} <= set((a - lab).tolist())
      assert set(g['info'][0][rows].tolist()) == {0.0, bu.BIG}


@pytest.mark.parametrize('family,kwargs', CASE_PARAMS)
def test_every_branch_is_reached(family, kwargs):
  g = bu.grid(family, kwargs)
  orc, want = bu.oracle_step(g)
  st, reward, discount, obs = want
  # FIRST exactly on the reset rows, LAST on the others
  np.testing.assert_array_equal(st == 0, g['reset'])
  np.testing.assert_array_equal(st == 2, ~g['reset'])
  assert (discount[st == 2] == 0.0).all()
  pred = bu.predicates(g, want)
  assert tuple(pred) == bu.predicate_names(family, kwargs)
  mask = bu.reset_mask(g)
  for name, rows in pred.items():
    print(f'{bu.case_id(family, kwargs)} {name}: {int(rows.sum())} lanes, {int((rows & mask).sum())} of them masked, '
          f'{int(rows[bu.mt_rows(g)].sum())} among the mt19937 rows')
    assert int(rows.sum()) >= bu.MIN_LANES, (name, int(rows.sum()))
    # what the GPU test asserts about its own subsets: the masked third and the mt19937 rows
    assert (rows & ~mask).sum() >= bu.MIN_LANES // 2 and (rows & mask).sum() >= 8, name
    assert rows[bu.mt_rows(g)].any(), name
  assert (mask & ~g['reset']).sum() >= bu.MIN_LANES and (mask & g['reset']).sum() >= bu.MIN_LANES
  all_names = bu.BD_PREDICATES if family == bu.BD else bu.MN_PREDICATES
  for name in set(all_names) - set(pred):                     # left out only where it cannot occur
    assert (name == 'best_arm' and g['na'] == 1) or (name == 'label_over_9' and kwargs['dataset'] != '10x10'), name
  # the oracle's own accounting against the expected movement of the regret column
  info = bu.expected_info(g, want)
  np.testing.assert_array_equal(orc.bsuite_info()['total_regret'].view(np.int64), info[0].view(np.int64))
  moved = info[0] != g['info'][0]
  stepped = st == 2
  if family == bu.BD:
    a = bu.oracle_actions(g, g['action'])
    np.testing.assert_array_equal(reward[stepped], g['rewards'][a[stepped]])
    np.testing.assert_array_equal(a[pred['clamped_low']], 0)
    np.testing.assert_array_equal(a[pred['clamped_high']], g['na'] - 1)
    assert set(g['action'][pred['clamped_low']].tolist()) == {bu.INT_MIN, -1}
    assert {g['na'], g['na'] + 1, bu.INT_MAX} == set(g['action'][pred['clamped_high']].tolist())
    np.testing.assert_array_equal(bu.invalid_rows(g), pred['clamped_low'] | pred['clamped_high'])
    if 'best_arm' in pred:
      assert not moved[pred['best_arm']].any() and (g['info'][0][pred['best_arm']] == bu.BIG).sum() >= 16
    assert (reward[pred['worst_arm']] == 0.0).all()
    np.testing.assert_array_equal(info[0][pred['worst_arm']], g['info'][0][pred['worst_arm']] + 1.0)
    if g['na'] == bu.MAX_ARMS:                                 # 1 - reward inexact: the sum from 0.7... rounds
      wide = g['info'][0].astype(np.longdouble) + (np.longdouble(1.0) - reward.astype(np.longdouble))
      inexact = stepped & (g['info'][0] == bu.SMALL_REGRET) & (wide != info[0].astype(np.longdouble))
      print(f'the f64 addition rounds on {int(inexact.sum())} stepped rows')
      assert np.finfo(np.longdouble).nmant > 52 and inexact.sum() >= bu.MIN_LANES
    assert (obs == 1.0).all()
  else:
    assert not bu.invalid_rows(g).any()
    np.testing.assert_array_equal(moved, pred['miss'])         # a hit moves nothing
    np.testing.assert_array_equal(info[0][pred['miss']], g['info'][0][pred['miss']] + 2.0)
    assert (reward[pred['hit']] == 1.0).all() and (reward[pred['miss']] == -1.0).all()
    assert (pred['miss'] & pred['big_regret']).sum() >= bu.MIN_LANES
    flat = obs.reshape(len(st), -1)
    assert (flat[stepped] == 0.0).all() and (flat[~stepped] != 0.0).any(axis=1).all()
    # lanes that must write zeros while their word points at a row with bytes of 128 and above
    images = bu.dataset(kwargs['dataset'])[0].reshape(g['num_data'], -1)
    assert (stepped & (images[g['idx']] < 0).any(axis=1)).sum() >= bu.MIN_LANES
    if 'label_over_9' in pred:
      over = pred['label_over_9']
      assert (over & pred['hit']).sum() >= 16 and (over & pred['miss']).sum() >= 16      # action 10 / 15 equal to the label
      assert {10, 12, 15} <= set(g['label'][over].tolist())
    words = bu.oracle_words(g, orc, g['state'], st, obs)
    assert ((words[stepped] & 0x0FFFFFFF) == (g['state'][stepped] & 0x0FFFFFFF)).all()
    assert (words[~stepped] & bu.MN_SHOW_BIT != 0).all() and ((words[~stepped] & 0xFFFFFF) < g['num_data']).all()
    # the observation stream's workgroups over the grid: full ones, a guarded one, lanes of both phases in one block
    full, partial, mixed = bu.observe_blocks(g)
    assert full >= 1 and (partial or g['num_pixels'] == bu.OBS_BLOCK) and (mixed >= 1 or g['num_pixels'] == bu.OBS_BLOCK)
  # the two steps the GPU test takes after it: resets inside the run
  _, sts, _, _ = bu.oracle_run(g, bu.episode_actions(g, 3))
  np.testing.assert_array_equal(sts[1] == 0, ~g['reset'])
  np.testing.assert_array_equal(sts[2] == 0, g['reset'])


@pytest.mark.parametrize('family,kwargs', bu.EPISODE_CASES, ids=[bu.case_id(*c) for c in bu.EPISODE_CASES])
def test_one_call_ends_twenty_episodes_on_every_lane_from_mixed_phases(family, kwargs):
  """The conditions of the GPU test's part C, on the reference."""
  g = bu.mixed_grid(family, kwargs)
  T = bu.EPISODE_T
  assert g['lanes'] == 8 * bu.BLOCK + 1 and not g['info'].any()
  assert min(g['reset'].sum(), (~g['reset']).sum()) >= 8 * bu.MIN_LANES
  # neighbouring lanes differ in phase in every wave
  waves = [g['reset'][i:i + 64] for i in range(0, g['lanes'] - 1, 64)]
  assert all(0 < w.sum() < len(w) for w in waves)
  orc, st, r, _ = bu.oracle_run(g, bu.episode_actions(g, T))
  assert ((st == 2).sum(axis=0) == T // 2).all() and ((st == 0).sum(axis=0) == T // 2).all()
  assert ((st == 2).sum(axis=1) > 8 * bu.MIN_LANES).all() and ((st == 0).sum(axis=1) > 8 * bu.MIN_LANES).all()
  regret = np.zeros(g['lanes'])
  for t in range(T):                                           # the column as T f64 additions in call order
    regret = np.where(st[t] == 2, regret + (1.0 - r[t]), regret)
  np.testing.assert_array_equal(orc.bsuite_info()['total_regret'], regret)
  assert (regret > 0).sum() >= g['lanes'] // 2


# ------------------------------------------------------------------------------------- the host-side check of the labels
def _tiny(labels, n=None):
  n = len(labels) if n is None else n
  images = np.arange(n * 4, dtype=np.uint8).view(np.int8).reshape(n, 2, 2)
  return dict(images=images, labels=labels)


@pytest.mark.parametrize('bad', [16, 32, 17, 255])
def test_a_label_that_does_not_fit_the_state_word_is_refused(bad):
  """The word is idx | label << 24 | flags with the reset bit at 28 and the show bit at 29 (csrc/mnist_fam.h): a label of 16
  is the reset bit — the lane would reset again instead of stepping — and one of 32 the show bit."""
  assert 16 << 24 == bu.MN_RESET_BIT and 32 << 24 == bu.MN_SHOW_BIT
  with pytest.raises(ValueError, match='labels'):
    mnist.MNISTBandit(**_tiny(np.asarray([0, 3, bad, 9], np.uint8)))
  with pytest.raises(ValueError, match='labels'):
    mnist.MNISTBandit(**_tiny([0, 3, bad, 9]))
  with pytest.raises(ValueError, match='labels'):                               # wherever it stands, beyond `fraction` too
    mnist.MNISTBandit(fraction=0.5, **_tiny(np.asarray([0, 3, 9, bad], np.uint8)))


def test_labels_ten_to_fifteen_are_accepted():
  """No action of the spec equals them; the reference compares action == label without a range check, and so do the kernels."""
  labels = np.arange(16, dtype=np.uint8)
  env = mnist.MNISTBandit(**_tiny(labels))
  assert env._num_data == 16 and env._labels.tolist() == list(range(16))        # pylint: disable=protected-access
  assert env._labels.__array_interface__['data'][0] == labels.__array_interface__['data'][0]      # pylint: disable=protected-access
  mnist.MNISTBandit(**_tiny(list(range(16))))
  with pytest.raises(ValueError, match='labels'):
    mnist.MNISTBandit(**_tiny([0, -1, 2, 3]))


@pytest.mark.parametrize('n,fraction', [(10, 0.29), (10, 0.3), (96, 0.999), (7, 1 / 7), (100, 0.57), (3, 1.0)])
def test_fraction_keeps_the_reference_truncation(n, fraction):
  """num_data = int(fraction * len(labels)) (mnist.py:47), never rounded: 0.29 * 10 = 2.9 -> 2, 0.57 * 100 = 56.99... -> 56."""
  labels = (np.arange(n) % 10).astype(np.uint8)
  env = mnist.MNISTBandit(fraction=fraction, **_tiny(labels))
  assert env._num_data == int(fraction * n) == len(env._labels)                 # pylint: disable=protected-access
  assert {(10, 0.29): 2, (10, 0.3): 3, (96, 0.999): 95, (7, 1 / 7): 1, (100, 0.57): 56, (3, 1.0): 3}[(n, fraction)] == env._num_data      # pylint: disable=protected-access
