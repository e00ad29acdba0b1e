"""CPU: the C oracle (oracle/oracle.c), driven lane by lane — `reset_next[i] = 1` before the call for every masked lane,
which is what base.py:59-62 makes of a reset() — reproduces the per-lane reset fixtures the unmodified reference wrote
(tests/golden/.tools/lane_reset).  That is what lets tests/test_gpu_lane_reset.py use the oracle for expected values at
batch sizes no fixture can hold."""
import glob
import json
import os

import numpy as np
import pytest

from oracle import coracle
from tests import golden_util as gu

FIXTURES = os.path.join(gu.GOLDEN_DIR, '.tools', 'lane_reset')
REPLAY = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FIXTURES, '*.npz'))
                if not os.path.basename(p).startswith('mt_') and 'logging' not in os.path.basename(p))


def masked_call(orc, actions, step, mask):
  """One call of the oracle with the masked lanes reset: the reference's step() of an instance whose
  `_reset_next_step` is set IS its reset() (base.py:59-62)."""
  orc.reset_next[np.asarray(mask) != 0] = 1
  return orc.call(actions, step)


@pytest.mark.parametrize('name', REPLAY)
def test_oracle_with_per_lane_reset_flags_reproduces_the_fixture(name):
  with np.load(os.path.join(FIXTURES, name + '.npz')) as z:
    g = {k: z[k] for k in z.files if k != 'meta'}
    meta = json.loads(str(z['meta']))
  fam, kwargs = meta['family'], dict(meta['kwargs'])
  if fam == 'mnist':
    kwargs['images'], kwargs['labels'] = gu.mnist_dataset()
  orc = coracle.OracleEnv(fam, kwargs, g['lanes'], seed=meta['seed'])
  phys = fam in gu.PHYSICS
  T = g['mask'].shape[0]
  for t in range(T):
    st, r, d, o = masked_call(orc, g['actions'][t], meta['step0'] + t, g['mask'][t])
    np.testing.assert_array_equal(st, g['step_type'][t], err_msg=f'{name} t={t}')
    live = st != 0
    if phys:
      np.testing.assert_allclose(o, g['obs'][t], rtol=1e-6, atol=1e-6, err_msg=f'{name} obs t={t}')
      np.testing.assert_allclose(r[live], g['reward'][t][live], rtol=1e-12, atol=1e-12)
    else:
      np.testing.assert_array_equal(o, g['obs'][t], err_msg=f'{name} obs t={t}')
      np.testing.assert_array_equal(r[live], g['reward'][t][live], err_msg=f'{name} reward t={t}')
    np.testing.assert_array_equal(d[live], g['discount'][t][live])
    for j, k in enumerate(meta['info_keys']):
      if k in orc.bsuite_info():
        np.testing.assert_allclose(orc.bsuite_info()[k], g['info'][t, :, j], rtol=0, atol=1e-9 if phys else 0, err_msg=f'{name} {k} t={t}')
