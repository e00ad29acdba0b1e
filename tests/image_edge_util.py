"""The edge grid of the image adapter (csrc/image.hip through wrappers.to_image): shapes, values and element types that
natural runs and the shape lists of the older image tests never reach.  Shared by tests/test_image_edges_host.py (CPU: the
oracle against scipy and the reference's fixtures, and the proof that the grid reaches every branch),
tests/test_gpu_image_edges.py (GPU: bit-exact comparison) and tools/make_image_edge_golden.py (the reference's own images
of the small cases).

`path_of` restates what bsx_image_observation_typed selects from a shape and a pair of element types: the run length K,
the elements per 16-byte chunk, the store branch, the workgroups per lane, the two filter radii, whether a filter index
folds more than once, and the dynamic LDS request.  In the regular build K follows from the shape alone; K = 8 for
float16 / bfloat16 and K = 16 for uint8 exist only in the tuning build (BSX_IMAGE_K) and are out of scope here.
"""
import numpy as np

from oracle import image_oracle as io

BLOCK = 256
MAX_RADIUS = 64
MAX_IN, MAX_SIDE, MAX_TAIL, MAX_NUMEL = 4096, 1024, 4096, 1 << 20     # the entry point's limits (numel < MAX_NUMEL)
ELEM_SIZE = {'float32': 4, 'uint8': 1, 'float16': 2, 'bfloat16': 2}
FLOAT_OUT = ('float32', 'float16', 'bfloat16')
IN_DTYPES = ('float32', 'uint8', 'float16', 'bfloat16')

# (observation shape, image shape, why).  Every case is small enough for three lanes everywhere and 257 lanes where the
# image has at most MANY_LANES_NUMEL elements.
GRID = [
    # anti-aliasing filters wider than the axis they filter: img_mirror_index's general fold
    ((3, 3), (1, 1), 'radius 4 on length 3, both axes'),
    ((5, 7), (1, 2), 'radius 8 on 5 and 5 on 7'),
    ((5, 7), (1, 1), 'radius 8 on 5 and 12 on 7'),
    ((33, 5), (1, 9), 'radius 64 (the limit) on y; x grows'),
    ((2, 66), (1, 2), 'radius 2 on 2 and 64 on 66'),
    ((1, 33), (5, 1), 'radius 64 on length 33 beside an axis of length 1; out_cols == 1 divides without a magic'),
    ((1, 132), (3, 4), 'the longest axis radius 64 accepts at this ratio'),
    # more than 64 KiB of dynamic LDS with float64 planes (uint8), just under with float32 ones
    ((64, 64), (2, 2), '65,616 B of LDS in uint8; radius 62 on 64'),
    ((4092,), (3, 124), '68,012 B of LDS in uint8; radius 64'),
    # store branches: tails that do not divide a chunk, tails longer than a chunk, the longest tail
    ((7, 9), (4, 4, 5), 'tail 5: differing pixels in every chunk, K = 4 everywhere'),
    ((9, 9), (4, 4, 5), 'the same from 81 cells: K = 8 in float32 and uint8'),
    ((5, 7), (4, 4, 9), 'tail 9: longer than a float16 chunk'),
    ((5, 7), (4, 4, 17), 'tail 17: longer than a uint8 chunk'),
    ((33, 5), (1, 9, 17), 'tail 17 behind the widest filter'),
    ((62, 66), (2, 2, 16), 'tail 16 behind radius 60 and 64: one uint8 chunk per pixel'),
    ((5, 7), (1, 1, 4096), 'the longest tail, both axes filtered'),
    ((5, 7), (1, 1, 4095), 'tail 4095: element stores'),
    ((5, 7), (4, 4, 8), 'tail 8: one float16 chunk per pixel'),
    ((5, 7), (4, 4, 16), 'tail 16: one uint8 chunk per pixel'),
    ((5, 7), (3, 3, 4), 'four channels in element stores for the narrow types (36 elements)'),
    ((9, 9), (4, 4, 4), 'K = 8 in float32, one pixel per chunk'),
    ((9, 9), (5, 5, 3), 'element stores from 81 cells'),
    ((17, 17), (8, 8, 4), 'K = 16 in float32 (289 cells, four channels), radius 2'),
    # the same branches over several workgroups per lane
    ((7, 9), (84, 84, 3), 'uint8 K = 4: the run of 16,384 elements cuts a pixel\'s tail'),
    ((28, 28), (128, 128, 3), 'uint8 K = 8: the run of 32,768 elements cuts a pixel\'s tail'),
    ((7, 9), (85, 85, 3), 'element stores over several workgroups, K = 4'),
    ((9, 9), (53, 53, 3), 'element stores over several workgroups, K = 8 in float32'),
    ((9, 9), (48, 48, 4), 'float32 K = 8, one pixel per chunk, two workgroups'),
    ((17, 17), (68, 68, 4), 'float32 K = 16 over two workgroups'),
    ((5, 7), (96, 96, 4), 'four channels over two workgroups in the narrow types'),
    ((5, 7), (48, 48, 16), 'one pixel per chunk over two workgroups in the narrow types'),
    ((5, 7), (91, 91, 4), 'narrow element stores with four channels over two workgroups'),
]
# one lane each, float32 and uint8 only: the largest LDS requests and images the entry point accepts (numel just under 2^20)
BIG = [((4096,), (1024, 1023)), ((4096,), (1023, 1024))]
MANY_LANES_NUMEL = 8160                                   # 257 lanes * numel <= 2^21 elements
# the value list goes through small mode (four values per lane) and through this 2x up-scaling (eight per lane), whose
# 1/4 and 3/4 weights make ties and inf * 0 of their own
VALUE_SMALL_SHAPE = (4, 6, 4)
VALUE_ZOOM = ((2, 4), (4, 8, 4))


def lanes_of(shape):
  return (1, 3, 257) if int(np.prod(shape)) <= MANY_LANES_NUMEL else (1, 3)


def case_id(obs_shape, shape):
  return 'x'.join(map(str, obs_shape)) + '-' + 'x'.join(map(str, shape))


# ------------------------------------------------------------------------------------------------------------------
# path selection
def _radius(n_in, n_out):
  half = io.gaussian_half_kernel(n_in, n_out)
  return 0 if half is None else len(half) - 1


def path_of(obs_shape, shape, in_dtype, out_dtype):
  """What bsx_image_observation_typed does with this call, restated from its host code (csrc/image.hip)."""
  obs_shape, shape = tuple(obs_shape), tuple(shape)
  size = int(np.prod(obs_shape))
  tail = int(np.prod(shape[2:])) if len(shape) > 2 else 1
  H, W = shape[:2]
  small = size <= 4
  rows, cols = (1, size) if small else ((1, obs_shape[0]) if len(obs_shape) == 1 else obs_shape)
  in_numel, numel = rows * cols, H * W * tail
  ry = rx = 0
  if not small and (H < rows or W < cols):
    ry, rx = _radius(rows, H), _radius(cols, W)
  filtered = ry > 0 or rx > 0
  out_size = ELEM_SIZE[out_dtype]
  chunk = 16 // out_size
  tail4 = tail % 4 == 0
  if out_dtype == 'float32':
    k = 16 if (in_numel > 256 and tail4) else (8 if in_numel > 64 else 4)
  elif out_dtype == 'uint8':
    k = 8 if (tail4 or in_numel > 64) else 4
  else:
    k = 16 if tail4 else 4
  run = k * BLOCK * chunk
  branch = 'element' if numel % chunk else ('same' if tail % chunk == 0 else 'differ')
  plane = in_numel * (8 if out_dtype == 'uint8' else 4)
  return dict(mode='small' if small else 'bilinear', in_rows=rows, in_cols=cols, in_numel=in_numel, numel=numel, tail=tail,
              k=k, chunk=chunk, run=run, branch=branch, blocks_per_lane=-(-numel // run), radius_y=ry, radius_x=rx,
              filtered=('both' if ry and rx else 'y' if ry else 'x' if rx else 'none'),
              # pos - j reaches below -(len - 1), pos + j beyond 2 * (len - 1): one reflection does not bring it back
              fold_y=rows > 1 and ry > rows - 1, fold_x=cols > 1 and rx > cols - 1,
              len1_beside_filter=(rows == 1 and rx > 0) or (cols == 1 and ry > 0),
              lds=(H + W) * 20 + plane * (2 if filtered else 1), in_dtype=in_dtype, out_dtype=out_dtype)


def combo(p):
  """The store-side instantiation and branch of a path: (output type, K, store branch, several workgroups per lane)."""
  return (p['out_dtype'], p['k'], p['branch'], p['blocks_per_lane'] > 1)


def reachable_combos():
  """Every combo() the regular build can take, found by walking a shape space that holds every threshold of the rule:
  64 / 65 and 256 / 257 cells, tails on both sides of every chunk size, images below and above every run length."""
  out = set()
  sides = [(1, 1), (3, 3), (4, 4), (5, 5), (48, 48), (53, 53), (68, 68), (91, 91), (96, 96), (128, 128)]
  for cells in ((1,), (4,), (5,), (8, 8), (5, 13), (16, 16), (257,), (64, 64)):
    for side in sides:
      for tail in list(range(1, 34)) + [4095, 4096]:
        if side[0] * side[1] * tail >= MAX_NUMEL:
          continue
        for dt in IN_DTYPES:
          out.add(combo(path_of(cells, side + (tail,), dt, dt)))
  return out


# ------------------------------------------------------------------------------------------------------------------
# values
def _f32(bits):
  return np.array(bits, np.uint32).view(np.float32)


def _bits(x):
  return int(np.array(x, np.float32).view(np.uint32))


def _with_neighbours(x):
  """A positive finite float32 between its two float32 neighbours, as bit patterns."""
  b = _bits(x)
  assert 0 < b < 0x7F800000
  return [b - 1, b, b + 1]


F16_TIES = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65520.0, 2.0 ** -25]     # 65520 ties to inf, 2^-25 to zero
BF16_TIES = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, float(_f32(0x7F7F8000))]    # the last ties to inf
BF16_MAX_BITS, FLT_MAX_BITS = 0x7F7F0000, 0x7F7FFFFF
SUBNORMAL_MIN_BITS, SUBNORMAL_MAX_BITS = 0x00000001, 0x007FFFFF
SPECIAL_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000]      # +0 -0 +inf -inf NaN


def value_bits():
  """The float32 value list as uint32 bit patterns: every named value between its two float32 neighbours, the specials in
  the middle, then the negatives.  +0.0, -0.0 and +inf stand side by side on purpose: an up-scaled lane then never has
  -0.0 as its maximum, the one case where the sign of a clipped zero depends on numpy's comparison order."""
  pos = []
  for x in (F16_TIES[0], F16_TIES[1], 65504.0, float(_f32(_bits(65520.0) - 1)), 65520.0,
            2.0 ** -24, 2.0 ** -25, float(_f32(_bits(2.0 ** -25) + 1)), BF16_TIES[0], BF16_TIES[1]):
    pos += _with_neighbours(x)
  pos += _with_neighbours(_f32(BF16_MAX_BITS)) + _with_neighbours(_f32(0x7F7F8000))
  pos += [FLT_MAX_BITS - 1, FLT_MAX_BITS, 0x7F800000]
  pos += [0x00000000, SUBNORMAL_MIN_BITS, SUBNORMAL_MIN_BITS + 1, SUBNORMAL_MAX_BITS - 1, SUBNORMAL_MAX_BITS, 0x00800000]
  neg = [b | 0x80000000 for b in pos]
  return np.array(pos + SPECIAL_BITS + neg, np.uint32)


def bf16_subnormal_bits():
  """Every bfloat16 subnormal, as uint16 bit patterns 0x0001 .. 0x007F."""
  return np.arange(0x0001, 0x0080, dtype=np.uint16)


def f16_subnormal_bits():
  """Every eighth float16 subnormal and the largest, as uint16 bit patterns."""
  return np.array(sorted(set(range(0x0001, 0x0400, 8)) | {0x03FF}), np.uint16)


def value_list():
  """Everything the float paths are fed, as float32 (each value is exact in float32): value_bits(), every bfloat16
  subnormal and every eighth float16 subnormal.  Cast to a narrower input type it keeps that type's own subnormals."""
  return np.concatenate([value_bits().view(np.float32), widen_bf16_bits(bf16_subnormal_bits()),
                         f16_subnormal_bits().view(np.float16).astype(np.float32)])


def uint8_value_list():
  """Every byte, and four more to fill the 65th lane of four."""
  return np.concatenate([np.arange(256), [0, 255, 7, 1]]).astype(np.uint8)


def rne_bf16_bits(bits32):
  """float32 bit patterns -> bfloat16 bit patterns, round to nearest even in integer arithmetic; a NaN stays a NaN
  (quiet bit set, which is all the tests compare)."""
  u = np.asarray(bits32, np.uint32).astype(np.uint64)
  nan = (u & 0x7FFFFFFF) > 0x7F800000
  r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
  return np.where(nan, (u >> 16) | 0x0040, r).astype(np.uint16)


def widen_bf16_bits(bits16):
  return (np.asarray(bits16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def padded(v, per_lane, fill=0):
  """[n] -> [lanes, per_lane], the last lane filled up."""
  v = np.asarray(v)
  lanes = -(-len(v) // per_lane)
  out = np.full(lanes * per_lane, fill, v.dtype)
  out[:len(v)] = v
  return out.reshape(lanes, per_lane)


# ------------------------------------------------------------------------------------------------------------------
# observations
def uint8_lanes(obs_shape, lanes, seed=0):
  """[lanes, *obs_shape] uint8.  By lane: random bytes, a 0/255 checkerboard, a 0/1 board, the constants 0, 7 and 255
  (the clip then has lo == hi), then bytes, checkerboards of the other parity and boards in turn — no two lanes alike
  except the constants' repeats."""
  rng = np.random.RandomState(1000 + seed)
  n = int(np.prod(obs_shape))
  cell = np.arange(n).reshape(obs_shape)
  parity = (np.add.outer(np.arange(obs_shape[0]), np.arange(obs_shape[1])) if len(obs_shape) == 2 else cell) & 1
  out = np.empty((lanes,) + tuple(obs_shape), np.uint8)
  for i in range(lanes):
    kind = i if i < 6 else 6 + i % 3
    if kind in (0, 6):
      out[i] = rng.randint(0, 256, size=obs_shape)
    elif kind in (1, 7):
      out[i] = 255 * (parity ^ (kind == 7))
    elif kind in (2, 8):
      out[i] = rng.rand(*obs_shape) < 0.3
    else:
      out[i] = (0, 7, 255)[kind - 3]
  return out


def float_lanes(obs_shape, lanes, seed=0, finite=False):
  """[lanes, *obs_shape] float32.  By lane: randn * 3, a 0/1 board, draws from the value list (only those below the
  float16 overflow tie when `finite`), then randn * 3 with one cell in sixteen replaced by such a draw."""
  rng = np.random.RandomState(2000 + seed)
  vals = value_bits().view(np.float32)
  if finite:
    vals = vals[np.abs(vals) < 65520]               # finite in every element type: float16 rounds these to 65504 at most
  out = np.empty((lanes,) + tuple(obs_shape), np.float32)
  for i in range(lanes):
    if i == 0:
      out[i] = rng.standard_normal(obs_shape) * 3
    elif i == 1:
      out[i] = rng.rand(*obs_shape) < 0.3
    elif i == 2:
      out[i] = vals[rng.randint(0, len(vals), size=obs_shape)]
    else:
      a = (rng.standard_normal(obs_shape) * 3).astype(np.float32)
      draw = vals[rng.randint(0, len(vals), size=obs_shape)]
      out[i] = np.where(rng.rand(*obs_shape) < 1 / 16, draw, a)
  return out
