"""CPU: tests/golden/.tools/image_edges.npz is what the reference's own `to_image` returns today on the small cases of the image
edge grid (tools/make_image_edge_golden.py, over the repository's skimage stand-in); skips where the reference is absent."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_image_edge_fixture_regenerates_array_for_array():
  from oracle import replay
  if replay.reference_origin() is None:
    pytest.skip('the reference is not on this machine')
  import make_image_edge_golden as mk  # pylint: disable=import-outside-toplevel
  fresh = mk.make()
  assert os.path.getsize(mk.OUT) < 1 << 20
  with np.load(mk.OUT) as z:
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
      assert z[k].dtype == fresh[k].dtype and z[k].shape == fresh[k].shape, k
      np.testing.assert_array_equal(z[k].view(np.uint8), fresh[k].view(np.uint8), err_msg=k)
