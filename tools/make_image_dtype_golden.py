"""Writes tests/golden/.tools/image_dtype.npz: the reference's own `to_image` (bsuite/utils/wrappers.py:222-247) on uint8 and
float16 observations, run on the CPU over the repository's scipy-based skimage stand-in (oracle/ref_shims/skimage).

The reference keeps the observation's dtype: a uint8 board is resized in float64, clipped to its [min, max] and
truncated by numpy's assignment into the uint8 result; a float16 one is resized in float32 and rounded to float16.
The GPU tests compare the typed image kernel with these arrays; tests/test_image_dtype_golden_regen.py regenerates
them and compares array for array.  Needs the reference (found the way oracle/make_golden.py finds it).

  python tools/make_image_dtype_golden.py            # rewrites the fixture
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

# A dot-directory: tests/test_golden_regen.py requires every other file under tests/golden to be written by
# oracle/make_golden.py, and tests/golden_util.py reads every top-level *.npz as an environment fixture.
OUT = os.path.join(ROOT, 'tests', 'golden', '.tools', 'image_dtype.npz')


def cases():
  """name -> (image shape, observations [n, *obs_shape]); the names carry the element type of the observations."""
  rng = np.random.RandomState(2026)
  boards = lambda n, shape: (rng.rand(n, *shape) < 0.3).astype(np.uint8)       # 0/1 boards, as deep_sea / catch
  bytes_ = lambda n, shape: rng.randint(0, 256, size=(n,) + shape).astype(np.uint8)
  halfs = lambda n, shape: (rng.standard_normal((n,) + shape) * 3).astype(np.float16)
  return {
      # uint8 -> uint8: float64 path, clip, truncation
      'u8_board_10x5__84x84': ((84, 84), boards(20, (10, 5))),           # catch's board: pixels where f32 rounds to 1
      'u8_board_10x10__84x84x4': ((84, 84, 4), boards(4, (10, 10))),     # deep_sea/0
      'u8_board_12x12__21x21x3': ((21, 21, 3), boards(4, (12, 12))),     # tail 3
      'u8_board_30x30__12x12x4': ((12, 12, 4), boards(4, (30, 30))),     # anti-aliased down-scaling, radius 3
      'u8_bytes_7x9__84x84': ((84, 84), bytes_(6, (7, 9))),
      'u8_bytes_28x28__84x84x3': ((84, 84, 3), bytes_(3, (28, 28))),
      'u8_bytes_40x40__5x84': ((5, 84), bytes_(3, (40, 40))),            # rows filtered (radius 14), columns not
      'u8_bytes_vec200__9x20x2': ((9, 20, 2), bytes_(3, (200,))),        # 1-D, radius 18
      'u8_bytes_5x7__11x13': ((11, 13), bytes_(4, (5, 7))),              # 143 B per image: element stores
      'u8_small_1__6x6x2': ((6, 6, 2), bytes_(3, (1,))),
      'u8_small_2__7x5': ((7, 5), bytes_(3, (2,))),
      'u8_small_3__8x8x4': ((8, 8, 4), bytes_(3, (3,))),
      'u8_small_4__9x9': ((9, 9), bytes_(3, (2, 2))),
      # float16 -> float16: float32 path, rounded to float16
      'f16_10x5__84x84x4': ((84, 84, 4), halfs(4, (10, 5))),
      'f16_30x30__12x12x4': ((12, 12, 4), halfs(3, (30, 30))),
      'f16_vec7__14x21': ((14, 21), halfs(3, (7,))),
      'f16_5x7__11x13x3': ((11, 13, 3), halfs(3, (5, 7))),               # 858 B per image: element stores
      'f16_small_3__8x8x3': ((8, 8, 3), halfs(3, (3,))),
  }


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
