"""Writes tests/golden/.tools/image_edges.npz: the reference's own `to_image` (bsuite/utils/wrappers.py:222-247) on the small
uint8 and float16 cases of the image edge grid (tests/image_edge_util.py), run on the CPU over the repository's
scipy-based skimage stand-in (oracle/ref_shims/skimage).

The grid holds what tools/make_image_dtype_golden.py's list does not: anti-aliasing filters wider than the axis they
filter (up to the radius limit of 64), observations of 4092 and 4096 cells, tails that do not divide a 16-byte chunk or
are longer than one, constant uint8 lanes (clip bounds lo == hi), 0/255 checkerboards.  Images of more than 4096 elements
are not stored: oracle/image_oracle.py, pinned to these arrays and to scipy by tests/test_image_edges_host.py, covers
them.  tests/test_image_edges_golden_regen.py regenerates the file and compares array for array.  Needs the reference
(found the way oracle/make_golden.py finds it).

  python tools/make_image_edge_golden.py            # rewrites the fixture
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import image_edge_util as iu  # noqa: E402  pylint: disable=wrong-import-position

# beside image_dtype.npz, for the same reasons (tools/make_image_dtype_golden.py)
OUT = os.path.join(ROOT, 'tests', 'golden', '.tools', 'image_edges.npz')
MAX_NUMEL = 4096                 # images stored; larger ones are the oracle's
U8_LANES, F16_LANES = 6, 3       # uint8: bytes, checkerboard, board and the three constant lanes


def cases():
  """name -> (image shape, observations [n, *obs_shape]); the names carry the element type of the observations."""
  out = {}
  for i, (obs_shape, shape, _) in enumerate(iu.GRID):
    if int(np.prod(shape)) > MAX_NUMEL:
      continue
    cid = iu.case_id(obs_shape, shape)
    out['u8_' + cid] = (shape, iu.uint8_lanes(obs_shape, U8_LANES, seed=i))
    with np.errstate(over='ignore'):
      out['f16_' + cid] = (shape, iu.float_lanes(obs_shape, F16_LANES, seed=i, finite=True).astype(np.float16))
  # small mode keeps its values verbatim: the float16 subnormals, four per lane
  bits = iu.f16_subnormal_bits()
  sub = iu.padded(bits, 4, fill=bits[0]).view(np.float16)
  out['f16_small_subnormals'] = (iu.VALUE_SMALL_SHAPE, sub)
  return out


def make():
  """{name__obs, name__image, name__shape}: the reference's images of every case."""
  from oracle import replay  # pylint: disable=import-outside-toplevel
  replay.import_reference()
  from bsuite.utils import wrappers as rw  # pylint: disable=import-outside-toplevel
  out = {}
  for name, (shape, obs) in cases().items():
    image = np.stack([rw.to_image(shape, o) for o in obs])
    assert image.dtype == obs.dtype and image.shape == (len(obs),) + tuple(shape), (name, image.dtype, image.shape)
    out[name + '__obs'] = obs
    out[name + '__image'] = image
    out[name + '__shape'] = np.array(shape, np.int32)
  return out


if __name__ == '__main__':
  np.savez_compressed(OUT, **make())
  print(OUT, os.path.getsize(OUT), 'bytes')
