"""CPU: tests/golden/.tools/lane_reset/*.npz are what the unmodified reference returns today when every instance is called
with reset() or step(a) as its mask element says (tools/make_lane_reset_golden.py); skips where the reference is absent.
Where it is absent the committed fixtures are still checked against the generator's own anti-vacuity conditions."""
import glob
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _committed():
  import make_lane_reset_golden as mk  # pylint: disable=import-outside-toplevel
  return mk, sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(mk.OUT_DIR, '*.npz')))


def test_committed_fixtures_cover_every_case_and_meet_the_generators_conditions():
  mk, names = _committed()
  assert names == sorted(c['name'] for c in mk.cases())
  families = set()
  for name in names:
    path = os.path.join(mk.OUT_DIR, name + '.npz')
    assert os.path.getsize(path) < (1 << 20), name
    with np.load(path) as z:
      g = {k: z[k] for k in z.files}
    meta = json.loads(str(g['meta']))
    T, B = g['mask'].shape
    assert B <= 64 and T <= 300 and meta['name'] == name
    s = mk.check(meta, g)
    assert 4 * s['running'] >= s['masked'] and s['after_last'] >= 1
    families.add(meta['family'] if meta['family'] != 'deep_sea' or meta['kwargs'].get('deterministic', True) else 'deep_sea_stochastic')
  assert families == {'deep_sea', 'deep_sea_stochastic', 'catch', 'bandit', 'memory_chain', 'umbrella_chain', 'discounting_chain',
                      'cartpole', 'cartpole_swingup', 'mountain_car', 'mnist'}


@pytest.mark.timeout(600)
def test_lane_reset_fixtures_regenerate_array_for_array():
  from oracle import replay
  if replay.reference_origin() is None:
    pytest.skip('the reference is not on this machine')
  mk, names = _committed()
  fresh = mk.make()
  assert sorted(fresh) == names
  for name in names:
    with np.load(os.path.join(mk.OUT_DIR, name + '.npz')) as z:
      assert sorted(z.files) == sorted(fresh[name]), name
      for k in z.files:
        a, b = z[k], fresh[name][k]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, k)
        if k == 'meta':
          assert str(a) == str(b), name
        else:
          np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f'{name}:{k}')
