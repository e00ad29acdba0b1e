"""CPU: tests/golden/.tools/policy_rollout/*.npz are what the unmodified reference does today in the closed loop of a
tabular agent (tools/make_policy_rollout_golden.py); skips where the reference is absent.  Where it is absent the committed
fixtures are still checked against the generator's own anti-vacuity conditions."""
import glob
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _committed():
  import make_policy_rollout_golden as mk  # pylint: disable=import-outside-toplevel
  return mk, sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(mk.OUT_DIR, '*.npz')))


def test_committed_fixtures_cover_every_case_and_meet_the_generators_conditions():
  mk, names = _committed()
  assert names == sorted(c['name'] for c in mk.cases())
  seen = set()
  for name in names:
    path = os.path.join(mk.OUT_DIR, name + '.npz')
    assert os.path.getsize(path) < (1 << 20), name
    with np.load(path) as z:
      g = {k: z[k] for k in z.files}
    meta = json.loads(str(g['meta']))
    T, B = g['actions'].shape
    assert B <= 64 and T <= 300 and meta['name'] == name
    s = mk.check(meta, g)
    assert s['last'] >= 4
    for k in ('keys', 'resets', 'explored', 'step_type', 'reward', 'discount'):
      assert g[k].shape == (T, B), (name, k)
    assert g['obs'].shape == (T, B) + tuple(meta['board_shape']) and g['index'].shape[:2] == (T, B)
    assert g['info'].shape == (T, B, len(meta['info_keys']))
    assert g['table'].dtype == np.uint8 and g['table'].shape == (meta['n_policies'], meta['n_states'])
    assert g['policy_index'].dtype == np.int32 and g['policy_index'].shape == (B,)
    stochastic = meta['family'] == 'deep_sea' and not meta['kwargs'].get('deterministic', True)
    seen.add((meta['family'] + ('_stochastic' if stochastic else ''), meta['epsilon'] > 0, meta['n_policies'] > 1, meta['table']))
    if meta['epsilon'] > 0:
      assert 10 * s['explored'] >= s['live'] and 10 * (s['live'] - s['explored']) >= s['live']
  assert seen == {('deep_sea', False, False, 'random'), ('deep_sea_stochastic', True, False, 'random'),
                  ('catch', False, False, 'random'), ('catch', True, False, 'random'), ('deep_sea', False, True, 'random'),
                  ('catch', False, True, 'random'), ('deep_sea', False, False, 'optimal')}
  # the 64-bit coordinates of the draw stream are exercised
  by_name = {n: np.load(os.path.join(mk.OUT_DIR, n + '.npz')) for n in names}
  assert int(by_name['catch_greedy']['lanes'][0]) >> 32 and json.loads(str(by_name['deep_sea_stochastic_eps']['meta']))['step0'] >> 32


@pytest.mark.timeout(600)
def test_policy_rollout_fixtures_regenerate_array_for_array():
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
