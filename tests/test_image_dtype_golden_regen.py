"""CPU: tests/golden/.tools/image_dtype.npz is what the reference's own `to_image` returns today (tools/make_image_dtype_golden.py,
over the repository's skimage stand-in); skips where the reference is absent."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_image_dtype_fixture_regenerates_array_for_array():
  from oracle import replay
  if replay.reference_origin() is None:
    pytest.skip('the reference is not on this machine')
  import make_image_dtype_golden as mk  # pylint: disable=import-outside-toplevel
  fresh = mk.make()
  with np.load(mk.OUT) as z:
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
      assert z[k].dtype == fresh[k].dtype and z[k].shape == fresh[k].shape, k
      np.testing.assert_array_equal(z[k].view(np.uint8), fresh[k].view(np.uint8), err_msg=k)
