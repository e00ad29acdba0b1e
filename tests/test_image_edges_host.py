"""CPU: the image edge grid of tests/image_edge_util.py before any GPU sees it.  The GPU test
(tests/test_gpu_image_edges.py) compares the kernel with oracle/image_oracle.py and is only worth what the oracle and the
grid are worth, so here

  * the float32 oracle equals scipy.ndimage (gaussian_filter, then zoom) bit for bit at every grid shape, the two
    megabyte-sized ones included;
  * the float64 / uint8 path of the oracle equals every uint8 array the reference wrote (image_dtype.npz, image_edges.npz)
    and scipy.ndimage run in float64 at every grid shape;
  * an observation with a NaN keeps scipy's localised NaNs under skimage's clip rule, in the oracle and in the stand-in;
  * the bfloat16 rounding the GPU test's expectations rest on is restated in integers and pinned to torch's CPU cast, and
    every tie of the value list is a tie, and its neighbours round apart, in exact rational arithmetic;
  * the grid reaches every store-side instantiation and branch the regular build can take, every filter combination, the
    general index fold on each axis, the radius limit on each axis, and more than 64 KiB of LDS in float32 and in uint8;
  * the entry point refuses the first shape past each of its limits without a launch.
"""
import ctypes
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from bsuite_amd import _native
from bsuite_amd.utils import wrappers as w
from oracle import image_oracle as io
from tests import image_edge_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS_GOLDEN = os.path.join(ROOT, 'tests', 'golden', '.tools')
ALL_SHAPES = [(o, s) for o, s, _ in iu.GRID] + iu.BIG
SHAPE_PARAMS = [pytest.param(o, s, id=iu.case_id(o, s)) for o, s in ALL_SHAPES]


def _plane_shapes(obs_shape, shape):
  rows, cols = (1, obs_shape[0]) if len(obs_shape) == 1 else obs_shape
  return (rows, cols), tuple(shape[:2])


def _scipy_resize(ndi, a, out_hw):
  """skimage >= 0.19 `resize(a, out_hw, preserve_range=True)` without its clip, in a's own float type."""
  factors = np.divide(a.shape, out_hw)
  if any(o < i for o, i in zip(out_hw, a.shape)):
    a = ndi.gaussian_filter(a, np.maximum(0, (factors - 1) / 2), cval=0, mode='mirror')
  return ndi.zoom(a, [1 / f for f in factors], order=1, mode='mirror', cval=0, grid_mode=True)


@pytest.mark.parametrize('obs_shape,shape', SHAPE_PARAMS)
def test_float32_oracle_equals_scipy_on_the_grid(obs_shape, shape):
  ndi = pytest.importorskip('scipy.ndimage')
  in_hw, out_hw = _plane_shapes(obs_shape, shape)
  lanes = iu.float_lanes(in_hw, 4, seed=7, finite=True)
  got = io.resize_bilinear(lanes, out_hw)
  assert got.dtype == np.float32 and got.shape == (4,) + out_hw
  for a, g in zip(lanes, got):
    ref = _scipy_resize(ndi, a, out_hw)
    assert ref.dtype == np.float32
    np.testing.assert_array_equal(ref.view(np.uint32), g.view(np.uint32))
    assert g.min() >= a.min() and g.max() <= a.max()                 # skimage's clip=True never bites a finite image


@pytest.mark.parametrize('obs_shape,shape', SHAPE_PARAMS)
def test_uint8_oracle_equals_scipy_in_float64_on_the_grid(obs_shape, shape):
  ndi = pytest.importorskip('scipy.ndimage')
  in_hw, out_hw = _plane_shapes(obs_shape, shape)
  n = 7 if np.prod(shape) <= 1 << 16 else 3                        # the megabyte cases: bytes, checkerboard, board
  lanes = iu.uint8_lanes(in_hw, n, seed=7)
  got = io.resize_bilinear_uint8(lanes, out_hw)
  assert got.dtype == np.uint8 and got.shape == (n,) + out_hw
  for a, g in zip(lanes, got):
    ref = np.clip(_scipy_resize(ndi, a.astype(np.float64), out_hw), a.min(), a.max()).astype(np.uint8)
    np.testing.assert_array_equal(ref, g)
  for a, g in zip(lanes[3:6], got[3:6]):                             # constant lanes: lo == hi
    assert (g == a.flat[0]).all()
  full = io.to_image(shape, lanes.reshape((n,) + tuple(obs_shape)), batched=True)
  assert full.dtype == np.uint8 and full.shape == (n,) + tuple(shape)
  np.testing.assert_array_equal(full.reshape((n,) + out_hw + (-1,)), np.broadcast_to(got[..., None], full.shape[:3] + (full[0, 0, 0].size,)))


def _fixture(name):
  with np.load(os.path.join(TOOLS_GOLDEN, name)) as z:
    names = sorted({k.rsplit('__', 1)[0] for k in z.files})
    return [(n, tuple(int(s) for s in z[n + '__shape']), z[n + '__obs'], z[n + '__image']) for n in names]


@pytest.mark.parametrize('name', ['image_dtype.npz', 'image_edges.npz'])
def test_oracle_reproduces_the_reference_fixtures(name):
  n_u8 = n_f16 = 0
  for case, shape, obs, image in _fixture(name):
    if obs.dtype == np.uint8:
      got = io.to_image(shape, obs, batched=True)
      assert got.dtype == np.uint8
      np.testing.assert_array_equal(got, image, err_msg=case)
      np.testing.assert_array_equal(io.to_image(shape, obs[0]), image[0], err_msg=case)
      n_u8 += 1
    else:
      assert obs.dtype == np.float16                               # resized in float32, rounded to float16 by the assignment
      got = io.to_image(shape, obs.astype(np.float32), batched=True).astype(np.float16)
      np.testing.assert_array_equal(got.view(np.uint16), image.view(np.uint16), err_msg=case)
      n_f16 += 1
  assert n_u8 >= 13 and n_f16 >= 5


def test_edge_fixture_holds_the_small_grid_cases():
  small = [(o, s) for o, s, _ in iu.GRID if np.prod(s) <= 4096]
  names = {c[0] for c in _fixture('image_edges.npz')}
  assert names == {p + iu.case_id(o, s) for o, s in small for p in ('u8_', 'f16_')} | {'f16_small_subnormals'}
  for o, s in [((64, 64), (2, 2)), ((4092,), (3, 124)), ((3, 3), (1, 1)), ((5, 7), (1, 2)), ((33, 5), (1, 9, 17)), ((62, 66), (2, 2, 16))]:
    assert 'u8_' + iu.case_id(o, s) in names
  assert os.path.getsize(os.path.join(TOOLS_GOLDEN, 'image_edges.npz')) < 1 << 20


def _stand_in():
  pytest.importorskip('scipy.ndimage')
  path = os.path.join(ROOT, 'oracle', 'ref_shims', 'skimage', 'transform.py')
  spec = importlib.util.spec_from_file_location('_skimage_stand_in_transform', path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_one_nan_keeps_scipys_localised_nans():
  """skimage clips to [nanmin, nanmax] when the plain range is NaN (_clip_warp_output); np.clip to [NaN, NaN] would
  return an image of nothing but NaN.  3x9 -> 2x27 with one NaN column: scipy leaves 12 NaN of 54."""
  ndi = pytest.importorskip('scipy.ndimage')
  a = (np.arange(27, dtype=np.float32).reshape(3, 9) - 13) / 4
  a[:, 4] = np.nan
  ref = _scipy_resize(ndi, a, (2, 27))
  assert np.isnan(ref).sum() == 12
  got = io.resize_bilinear(a, (2, 27))
  shim = _stand_in().resize(a, (2, 27), preserve_range=True)
  for out in (got, shim):
    assert out.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(out), np.isnan(ref))
    keep = ~np.isnan(ref)
    np.testing.assert_array_equal(out[keep].view(np.uint32), ref[keep].view(np.uint32))
  batch = np.stack([a, np.nan_to_num(a), np.full_like(a, np.nan)])          # per lane: one NaN lane does not touch the next
  got = io.resize_bilinear(batch, (2, 27))
  np.testing.assert_array_equal(np.isnan(got[0]), np.isnan(ref))
  assert not np.isnan(got[1]).any() and np.isnan(got[2]).all()
  lo, hi = io.clip_bounds(batch)
  assert lo[0, 0, 0] == a[~np.isnan(a)].min() and hi[0, 0, 0] == a[~np.isnan(a)].max() and np.isnan(lo[2, 0, 0])


def test_batched_oracle_equals_the_stand_in_image_by_image_on_the_value_list():
  """The oracle clips a whole batch with per-lane bounds, the reference one image with scalar bounds.  numpy's clip
  returns the bound where it compares equal when the bounds are broadcast arrays (+0.0 in [-0.0, inf] became -0.0), so
  the oracle writes its clip out (image_oracle.clip); here every up-scaled lane of the value list, as each input type
  widens it, equals the stand-in's image of that lane alone — signed zeros included, NaNs by position."""
  resize = _stand_in().resize
  (obs_shape, shape), n = iu.VALUE_ZOOM, 0
  for dt in (torch.float32, torch.float16, torch.bfloat16):
    lanes = torch.from_numpy(iu.padded(iu.value_list(), 8)).to(dt).float().numpy().reshape((-1,) + obs_shape)
    got = io.resize_bilinear(lanes, shape[:2])
    for a, g in zip(lanes, got):
      with np.errstate(invalid='ignore'):
        ref = resize(a, shape[:2], preserve_range=True)
      np.testing.assert_array_equal(np.isnan(g), np.isnan(ref))
      keep = ~np.isnan(ref)
      np.testing.assert_array_equal(g[keep].view(np.uint32), ref[keep].view(np.uint32))
      n += int(a.min() == 0 and np.signbit(a[a == 0]).any() and not np.signbit(g[g == 0]).any())
  assert n >= 1                                     # a lane whose minimum is -0.0 and whose image holds only +0.0


# ------------------------------------------------------------------------------------------------------------------
# values
def _exact(bits):
  return Fraction(float(np.array(bits, np.uint32).view(np.float32)))


def _ulp(x, precision, e_min):
  """Spacing of a format with `precision` significand bits and smallest normal exponent e_min around |x| > 0."""
  x, e = abs(x), 0
  while x >= 2:
    x, e = x / 2, e + 1
  while x < 1:
    x, e = x * 2, e - 1
  return Fraction(2) ** (max(e, e_min) - (precision - 1))


def _cast_f16(bits):
  with np.errstate(over='ignore'):
    return np.array(bits, np.uint32).view(np.float32).astype(np.float16)


def _cast_bf16(bits):
  return torch.from_numpy(np.array(bits, np.uint32).view(np.float32)).to(torch.bfloat16).float().numpy()


@pytest.mark.parametrize('ties,precision,e_min,f_max,cast', [
    (iu.F16_TIES, 11, -14, Fraction(65504), _cast_f16),
    (iu.BF16_TIES, 8, -126, _exact(iu.BF16_MAX_BITS), _cast_bf16)], ids=['float16', 'bfloat16'])
def test_every_tie_is_a_tie_and_its_neighbours_round_apart(ties, precision, e_min, f_max, cast):
  listed = set(iu.value_bits().tolist())
  for x in ties:
    b = int(np.array(x, np.float32).view(np.uint32))
    assert float(np.array(x, np.float32)) == x and {b - 1, b, b + 1} <= listed and {(b - 1) | 1 << 31, b | 1 << 31} <= listed
    v, ulp = _exact(b), _ulp(_exact(b), precision, e_min)
    q = v / ulp
    assert q.denominator == 2, (x, q)                                        # exactly half way between two neighbours
    down, up = (q - Fraction(1, 2)) * ulp, (q + Fraction(1, 2)) * ulp
    even = down if (q - Fraction(1, 2)) % 2 == 0 else up
    want = lambda r: np.inf if r > f_max else float(r)
    assert _exact(b - 1) < v < _exact(b + 1)
    got = cast([b - 1, b, b + 1])
    assert [float(g) for g in got] == [want(down), want(even), want(up)], (x, got)
    neg = cast([(b - 1) | 1 << 31, b | 1 << 31, (b + 1) | 1 << 31])
    assert [float(g) for g in neg] == [-want(down), -want(even), -want(up)]


def test_bfloat16_rounding_restated_in_integers_equals_torch():
  rng = np.random.RandomState(5)
  bits = np.concatenate([iu.value_bits(), rng.randint(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32),
                         np.arange(0x7F7F7F00, 0x7F800100, dtype=np.uint32), np.arange(0x00007F00, 0x00018100, dtype=np.uint32)])
  want = torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
  got = iu.rne_bf16_bits(bits)
  nan = np.isnan(bits.view(np.float32))
  np.testing.assert_array_equal(got[~nan], want[~nan])
  assert ((got[nan] & 0x7FFF) > 0x7F80).all() and ((want[nan] & 0x7FFF) > 0x7F80).all()
  # widening is exact and inverts the rounding: every bfloat16 subnormal survives the round trip
  sub = iu.bf16_subnormal_bits()
  wide = iu.widen_bf16_bits(sub)
  assert (wide > 0).all() and (wide < np.float32(2.0 ** -126)).all() and len(sub) == 127
  np.testing.assert_array_equal(iu.rne_bf16_bits(wide.view(np.uint32)), sub)
  np.testing.assert_array_equal(torch.from_numpy(sub.view(np.int16)).view(torch.bfloat16).float().numpy().view(np.uint32), wide.view(np.uint32))


def test_value_list_holds_what_it_names():
  bits = iu.value_bits()
  v = bits.view(np.float32)
  every = iu.value_list()
  assert every.dtype == np.float32 and len(iu.padded(every, 4)) >= 65        # small mode: four values per lane
  np.testing.assert_array_equal(every[:len(bits)].view(np.uint32), bits)
  for sub in (iu.widen_bf16_bits(iu.bf16_subnormal_bits()), iu.f16_subnormal_bits().view(np.float16).astype(np.float32)):
    assert set(sub.view(np.uint32).tolist()) <= set(every.view(np.uint32).tolist()) and (sub > 0).all()
  assert len(iu.uint8_value_list()) == 260 and set(iu.uint8_value_list().tolist()) == set(range(256))
  for b in iu.SPECIAL_BITS + [iu.FLT_MAX_BITS, iu.BF16_MAX_BITS, 0x7F7F8000, iu.SUBNORMAL_MIN_BITS, iu.SUBNORMAL_MAX_BITS]:
    assert b in bits
  assert np.isnan(v).sum() == 1 and np.isposinf(v).sum() >= 1 and np.isneginf(v).sum() >= 1
  for x in (65504.0, 65520.0, 2.0 ** -24, 2.0 ** -25):
    assert x in v and -x in v
  # zeros of both signs, given and made: -2^-25 rounds to -0.0 in float16, the float32 subnormals to +-0.0
  h = _cast_f16(bits).view(np.uint16)
  assert (h == 0x0000).sum() >= 3 and (h == 0x8000).sum() >= 3
  assert (bits == 0).sum() >= 1 and (bits == 0x80000000).sum() >= 1
  bf = iu.rne_bf16_bits(bits)
  assert (bf == 0x0000).sum() >= 2 and (bf == 0x8000).sum() >= 2 and (bf == 0x7F80).sum() >= 3 and (bf == 0xFF80).sum() >= 3
  assert (h == 0x7C00).sum() >= 3 and (h == 0x0001).sum() >= 2                # overflow to inf; the smallest subnormal
  f16_sub = iu.f16_subnormal_bits()
  assert f16_sub[0] == 1 and f16_sub[-1] == 0x3FF and len(f16_sub) == 129 and (np.diff(f16_sub[:-1]) == 8).all()
  # an up-scaled lane of eight never has -0.0 as its maximum (image_edge_util.value_bits)
  for lane in iu.padded(bits, 8).view(np.float32):
    m = np.nanmax(lane)
    assert not (m == 0 and np.signbit(m) and (lane[~np.isnan(lane)] <= 0).all() and np.signbit(lane[lane == 0]).all())


# ------------------------------------------------------------------------------------------------------------------
# the grid reaches every branch
def _paths(shapes, pairs):
  return [iu.path_of(o, s, i, d) for o, s in shapes for i, d in pairs]


ALL_PAIRS = [(i, o) for i in iu.IN_DTYPES for o in iu.FLOAT_OUT] + [('uint8', 'uint8')]


def test_path_of_agrees_with_the_host_rule():
  for o, s in ALL_SHAPES + [((2, 2), iu.VALUE_SMALL_SHAPE), iu.VALUE_ZOOM]:
    p, c = iu.path_of(o, s, 'float32', 'float32'), w._image_cfg(s, o)
    assert (c.mode == _native.IMAGE_SMALL) == (p['mode'] == 'small')
    assert (c.in_rows, c.in_cols, c.out_rows, c.out_cols, c.tail) == (p['in_rows'], p['in_cols'], s[0], s[1], p['tail'])
    assert (c.radius_y, c.radius_x) == (p['radius_y'], p['radius_x'])
    assert p['in_numel'] <= iu.MAX_IN and max(s[:2]) <= iu.MAX_SIDE and p['tail'] <= iu.MAX_TAIL and p['numel'] < iu.MAX_NUMEL
    assert max(p['radius_y'], p['radius_x']) <= iu.MAX_RADIUS
  assert iu.path_of((64, 64), (2, 2), 'uint8', 'uint8')['lds'] == 65616
  assert iu.path_of((4092,), (3, 124), 'uint8', 'uint8')['lds'] == 68012
  assert iu.path_of((4096,), (1024, 1023), 'uint8', 'uint8')['lds'] == 106476       # the most the entry point can ask
  assert iu.path_of((64, 64), (1024, 1000), 'float32', 'float32')['lds'] == 56864   # test_gpu_adapters.py's largest


def test_grid_reaches_every_store_branch_of_every_instantiation():
  reachable = iu.reachable_combos()
  # by the rule: float32 K 4 / 8 x three branches and K 16 (four channels: one pixel per chunk) x one, float16 and
  # bfloat16 K 16 x three and K 4 x two (no tail of 8 without four channels), uint8 K 8 x three and K 4 x two — each at
  # one workgroup per lane and at several
  assert len(reachable) == 2 * (7 + 5 + 5 + 5)
  for pairs in ([(i, o)] for i, o in ALL_PAIRS):
    out = pairs[0][1]
    have = {iu.combo(p) for p in _paths([(o, s) for o, s, _ in iu.GRID], pairs)}
    assert have == {c for c in reachable if c[0] == out}, (pairs, sorted({c for c in reachable if c[0] == out} - have))
  for o, s, _ in iu.GRID:
    assert iu.lanes_of(s)[-1] == (257 if np.prod(s) <= iu.MANY_LANES_NUMEL else 3)
  # multi-workgroup runs that cut a pixel's tail, at K = 4 and K = 8 in uint8
  for o, s, k in (((7, 9), (84, 84, 3), 4), ((28, 28), (128, 128, 3), 8)):
    p = iu.path_of(o, s, 'uint8', 'uint8')
    assert iu.combo(p) == ('uint8', k, 'differ', True) and p['run'] % p['tail'] != 0
  tails = {iu.path_of(o, s, 'uint8', 'uint8')['tail'] for o, s, _ in iu.GRID}
  assert {1, 3, 4, 5, 8, 9, 16, 17, 4095, 4096} <= tails


def test_grid_reaches_every_filter_path():
  small = _paths([(o, s) for o, s, _ in iu.GRID], [('float32', 'float32'), ('uint8', 'uint8')])
  for out in ('float32', 'uint8'):
    ps = [p for p in small if p['out_dtype'] == out]
    assert {p['filtered'] for p in ps} == {'y', 'x', 'both', 'none'}
    assert any(p['fold_y'] for p in ps) and any(p['fold_x'] for p in ps)
    assert any(p['radius_y'] == iu.MAX_RADIUS for p in ps) and any(p['radius_x'] == iu.MAX_RADIUS for p in ps)
    assert any(p['len1_beside_filter'] for p in ps)
    assert any(p['filtered'] != 'none' and not p['fold_y'] and not p['fold_x'] for p in ps)
  p = iu.path_of((1, 33), (5, 1), 'float32', 'float32')
  assert p['radius_x'] == 64 and p['fold_x'] and p['len1_beside_filter'] and p['in_rows'] == 1
  every = small + _paths(iu.BIG, [('float32', 'float32'), ('uint8', 'uint8')])
  for out in ('float32', 'uint8'):
    assert max(p['lds'] for p in every if p['out_dtype'] == out) > 65536
  assert sum(p['lds'] > 65536 for p in small if p['out_dtype'] == 'uint8') >= 2      # without the megabyte cases too
  assert max(p['lds'] for p in every) == 106476
  for o, s in iu.BIG:
    assert (1 << 20) - 1024 <= np.prod(s) < 1 << 20


# ------------------------------------------------------------------------------------------------------------------
# refusals without a launch
def _rc(cfg, code=0):
  return _native.lib.bsx_image_observation_typed(ctypes.byref(cfg), 1, None, code, None, code, None)


def test_the_first_shape_past_each_limit_is_refused():
  B, S = _native.IMAGE_BILINEAR, _native.IMAGE_SMALL
  for code in (0, 1, 2, 3):
    assert _rc(_native.ImageCfg(B, 1, 4096, 1024, 1023, 1), code) == _native.BSX_ENULL    # accepted up to the pointers
    assert _rc(_native.ImageCfg(B, 64, 64, 1024, 1, 1023), code) == _native.BSX_ENULL
    assert _rc(_native.ImageCfg(B, 1, 5, 1, 1, 4096), code) == _native.BSX_ENULL
    assert _rc(_native.ImageCfg(B, 1, 4097, 8, 8, 1), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 4097, 1, 8, 8, 1), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 17, 241, 8, 8, 1), code) == _native.BSX_ERANGE           # 4097 cells in two dimensions
    assert _rc(_native.ImageCfg(B, 2, 4, 1025, 8, 1), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 2, 4, 8, 1025, 1), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 2, 4, 8, 8, 4097), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 2, 4, 1024, 1024, 1), code) == _native.BSX_ERANGE        # numel == 2^20
    assert _rc(_native.ImageCfg(B, 2, 4, 1024, 256, 4), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 2, 4, 16, 16, 4096), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 2, 4, 1023, 1025, 1), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 1, 133, 3, 4, 1, 0, 65), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 133, 1, 4, 3, 1, 65, 0), code) == _native.BSX_ERANGE
    assert _rc(_native.ImageCfg(B, 1, 132, 3, 4, 1, 0, 64), code) == _native.BSX_ENULL
    assert _rc(_native.ImageCfg(S, 1, 5, 8, 8, 1), code) == _native.BSX_ERANGE


def test_radius_65_is_a_value_error_before_any_launch():
  c = w._image_cfg((3, 4), (1, 132))
  assert (c.radius_y, c.radius_x) == (0, 64)
  for obs_shape, shape in (((1, 133), (3, 4)), ((133,), (3, 4)), ((133, 2), (4, 3))):
    with pytest.raises(ValueError, match='radius 65'):
      w._image_cfg(shape, obs_shape)
    with pytest.raises(ValueError, match='radius 65'):                       # a host tensor: refused before the device is asked for
      w.to_image(shape, torch.zeros((2,) + obs_shape))
