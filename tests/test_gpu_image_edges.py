"""GPU: the image adapter (csrc/image.hip through wrappers.to_image) on the edge grid of tests/image_edge_util.py, bit for bit
against oracle/image_oracle.py and the reference's own images (tests/golden/.tools/image_edges.npz).  The only difference
allowed anywhere is the sign and payload of a NaN: there NaN-ness is compared, position by position.
tests/test_image_edges_host.py pins the oracle to scipy and to the reference on the CPU and proves that the grid reaches
every branch named below, so that nothing here can pass vacuously.

Which test drives which instantiation and branch (bsx_image_kernel<OUT, K>; K follows from the shape in the regular build):

  test_float_images                  <f32, 4 / 8 / 16>, <f16, 4 / 16>, <bf16, 4 / 16>, each from all four input types: the
                                     same-pixel, differing-pixels and element store branches at one workgroup per lane and
                                     at several; img_gauss_pass with radius > axis length on y, on x and on both
                                     (img_mirror_index's general fold), radius 64 on each axis, an axis of length 1 beside
                                     a filtered one, out_cols == 1; tails 5, 9 and 17 in the narrow types; 1, 3 and 257 lanes
  test_uint8_images                  <u8, 4 / 8>: float64 planes, scipy's second weight, clip (lo == hi on constant lanes)
                                     and truncation on the same shapes; 65,616 B and 68,012 B of dynamic LDS; runs of
                                     16,384 (K = 4) and 32,768 (K = 8) elements that cut a pixel's tail between two
                                     workgroups; tails 4095 (element stores) and 4096; every lane of 257 compared
  test_reference_fixture             the stored uint8 and float16 cases: the reference's own bits, not the oracle's
  test_value_list_in_small_mode      img_load_f32 (all four codes) and img_bits' casts on ties, overflow, subnormals, signed
                                     zeros, inf and NaN copied verbatim (BSX_IMAGE_SMALL, sizes 1 to 4), twelve type pairs
  test_value_list_up_scaled          the same values through the four-term sum with weights 1/4 and 3/4: ties of its own,
                                     inf * 0, float64 -> float32 rounding into the subnormal range
  test_subnormal_inputs_come_back    bfloat16 and float16 subnormal observations in a float32 image: no flushed widening
  test_one_nan_stays_local           a NaN pixel in one lane: scipy's localised NaNs, f32 / f16 / bf16, other lanes untouched
  test_megabyte_images               <f32, 8> and <u8, 8> at 73,708 B / 106,476 B of LDS (the most the entry point asks) and
                                     numel = 2^20 - 1024, one lane each
  test_refusals                      radius 65 (ValueError) and the first shape past each limit of the entry point
"""
import functools
import os

import numpy as np
import pytest
import torch

from bsuite_amd.utils import wrappers
from oracle import image_oracle as io
from tests import image_edge_util as iu

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', '.tools', 'image_edges.npz')
TORCH = {'float32': torch.float32, 'uint8': torch.uint8, 'float16': torch.float16, 'bfloat16': torch.bfloat16}
INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
GRID_PARAMS = [pytest.param(i, id=iu.case_id(o, s)) for i, (o, s, _) in enumerate(iu.GRID)]


def _assert_same(got, want, msg):
  """Device tensor == host tensor, bit for bit; where `want` is NaN, `got` must be some NaN."""
  got = got.cpu()
  assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, got.shape)
  g, w = got.view(INT_VIEW[got.dtype]).numpy(), want.view(INT_VIEW[want.dtype]).numpy()
  if want.dtype != torch.uint8:
    gn, wn = torch.isnan(got).numpy(), torch.isnan(want).numpy()
    np.testing.assert_array_equal(gn, wn, err_msg=msg + ': NaN positions')
    g, w = np.where(wn, 0, g), np.where(wn, 0, w)
  np.testing.assert_array_equal(g, w, err_msg=msg)


def _input(values32, in_dtype):
  """float32 values as a host tensor of the input type (round to nearest even; float16 overflows to inf)."""
  return torch.from_numpy(np.ascontiguousarray(values32)).to(TORCH[in_dtype])


@functools.lru_cache(maxsize=None)
def _fixture():
  with np.load(FIXTURE) as z:
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('case', GRID_PARAMS)
def test_float_images(case):
  obs_shape, shape, _ = iu.GRID[case]
  lanes = iu.lanes_of(shape)
  base = iu.float_lanes(obs_shape, lanes[-1], seed=case)
  for in_dtype in iu.IN_DTYPES:
    # the input type only changes how a cell is loaded: beyond 1024 cells, where the oracle's wide filters take seconds
    # for 257 lanes, the narrow inputs stop at three lanes
    many = lanes if in_dtype == 'float32' or np.prod(obs_shape) <= 1024 else lanes[:2]
    obs = torch.from_numpy(iu.uint8_lanes(obs_shape, many[-1], seed=case)) if in_dtype == 'uint8' else _input(base[:many[-1]], in_dtype)
    want32 = torch.from_numpy(io.to_image(shape, obs.float().numpy(), batched=True))     # of the WIDENED observation
    dev = obs.cuda()
    for out_dtype in iu.FLOAT_OUT:
      want = want32.to(TORCH[out_dtype])                      # the CPU-pinned rounding (tests/test_image_edges_host.py)
      for n in many:
        got = wrappers.to_image(shape, dev[:n], dtype=TORCH[out_dtype])
        _assert_same(got, want[:n], f'{obs_shape} -> {shape} {in_dtype} -> {out_dtype}, {n} lanes')


@pytest.mark.parametrize('case', GRID_PARAMS)
def test_uint8_images(case):
  obs_shape, shape, _ = iu.GRID[case]
  lanes = iu.lanes_of(shape)
  obs = iu.uint8_lanes(obs_shape, lanes[-1], seed=case)
  want = torch.from_numpy(io.to_image(shape, obs, batched=True))
  assert want.dtype == torch.uint8
  dev = torch.from_numpy(obs).cuda()
  for n in lanes:
    got = wrappers.to_image(shape, dev[:n])                   # uint8 -> uint8 by default
    _assert_same(got, want[:n], f'{obs_shape} -> {shape}, {n} lanes')         # every lane, not only the first
  name = 'u8_' + iu.case_id(obs_shape, shape)
  if name + '__obs' in _fixture() and lanes[-1] >= 6:         # the stored lanes are the first six of this batch
    np.testing.assert_array_equal(_fixture()[name + '__obs'], obs[:6])
    np.testing.assert_array_equal(want[:6].numpy(), _fixture()[name + '__image'])


def test_reference_fixture():
  fx = _fixture()
  names = sorted({k.rsplit('__', 1)[0] for k in fx})
  assert sum(n.startswith('u8_') for n in names) >= 20 and sum(n.startswith('f16_') for n in names) >= 20
  for name in names:
    obs, image, shape = fx[name + '__obs'], fx[name + '__image'], tuple(int(s) for s in fx[name + '__shape'])
    got = wrappers.to_image(shape, torch.from_numpy(obs).cuda())
    _assert_same(got, torch.from_numpy(image), name)


def _value_inputs(in_dtype, per_lane):
  if in_dtype == 'uint8':
    return torch.from_numpy(iu.padded(iu.uint8_value_list(), per_lane))
  return _input(iu.padded(iu.value_list(), per_lane), in_dtype)


OUTS_OF = {i: iu.FLOAT_OUT + (('uint8',) if i == 'uint8' else ()) for i in iu.IN_DTYPES}


@pytest.mark.parametrize('in_dtype', iu.IN_DTYPES)
def test_value_list_in_small_mode(in_dtype):
  shape = iu.VALUE_SMALL_SHAPE
  for size in (4, 3, 2, 1):
    obs = _value_inputs(in_dtype, size)
    assert size != 4 or obs.shape[0] >= 65
    wide = obs.numpy() if in_dtype == 'uint8' else obs.float().numpy()
    want_wide = torch.from_numpy(io.small_state_to_image(shape, wide))       # copies: nothing to round but the cast
    for out_dtype in OUTS_OF[in_dtype]:
      got = wrappers.to_image(shape, obs.cuda(), dtype=TORCH[out_dtype])
      _assert_same(got, want_wide.to(TORCH[out_dtype]), f'small {size} {in_dtype} -> {out_dtype}')


@pytest.mark.parametrize('in_dtype', iu.IN_DTYPES)
def test_value_list_up_scaled(in_dtype):
  obs_shape, shape = iu.VALUE_ZOOM
  obs = _value_inputs(in_dtype, 8)
  obs = obs.reshape((obs.shape[0],) + obs_shape)
  want32 = torch.from_numpy(io.to_image(shape, obs.float().numpy(), batched=True))
  if in_dtype != 'uint8':
    nan = torch.isnan(want32)
    assert nan.any() and not nan.all(dim=(1, 2, 3)).all()     # inf * 0 and the NaN itself, and lanes that stay finite
  for out_dtype in iu.FLOAT_OUT:
    got = wrappers.to_image(shape, obs.cuda(), dtype=TORCH[out_dtype])
    _assert_same(got, want32.to(TORCH[out_dtype]), f'2x {in_dtype} -> {out_dtype}')
  if in_dtype == 'uint8':
    _assert_same(wrappers.to_image(shape, obs.cuda()), torch.from_numpy(io.to_image(shape, obs.numpy(), batched=True)), '2x uint8')


def test_subnormal_inputs_come_back():
  """A narrow subnormal observation widens to a float32 subnormal (bfloat16) or a small normal (float16): the float32
  image holds exactly these values, none flushed to zero."""
  for in_dtype, bits in (('bfloat16', iu.bf16_subnormal_bits()), ('float16', iu.f16_subnormal_bits())):
    obs = torch.from_numpy(iu.padded(bits, 4, fill=bits[0]).view(np.int16)).view(TORCH[in_dtype])
    got = wrappers.to_image(iu.VALUE_SMALL_SHAPE, obs.cuda(), dtype=torch.float32).cpu()
    assert (got > 0).all()
    assert set(got.view(torch.int32).unique().tolist()) == set(obs.float().view(torch.int32).unique().tolist())
    _assert_same(wrappers.to_image(iu.VALUE_SMALL_SHAPE, obs.cuda()), torch.from_numpy(io.small_state_to_image(
        iu.VALUE_SMALL_SHAPE, obs.view(torch.int16).numpy())).view(TORCH[in_dtype]), in_dtype)       # and in their own type
    if in_dtype == 'float16':
      fx = _fixture()
      np.testing.assert_array_equal(fx['f16_small_subnormals__obs'].view(np.int16), obs.view(torch.int16).numpy())
      np.testing.assert_array_equal(wrappers.to_image(iu.VALUE_SMALL_SHAPE, obs.cuda()).cpu().view(torch.int16).numpy(),
                                    fx['f16_small_subnormals__image'].view(np.int16))


@pytest.mark.parametrize('obs_shape,shape', [((3, 9), (2, 27, 4)), ((9, 9), (4, 4, 5)), ((5, 7), (1, 2))])
def test_one_nan_stays_local(obs_shape, shape):
  """skimage clips to [nanmin, nanmax] when the range is NaN, so a NaN spreads as far as scipy's filter and zoom carry it
  and no further; the kernel's float path does not clip at all."""
  obs = iu.float_lanes(obs_shape, 3, seed=11, finite=True)
  obs[0] = np.abs(obs[0]) + 1
  obs[1, :, obs_shape[1] // 2] = np.nan
  obs[0, 0, 0] = np.nan
  want32 = torch.from_numpy(io.to_image(shape, obs, batched=True))
  nan = torch.isnan(want32)
  assert nan[0].any() and nan[1].any() and not nan[2].any()
  if obs_shape == (3, 9):
    assert not nan[0].all() and not nan[1].all()              # up-scaling: localised, not an image of NaN
  for out_dtype in iu.FLOAT_OUT:
    got = wrappers.to_image(shape, torch.from_numpy(obs).cuda(), dtype=TORCH[out_dtype])
    _assert_same(got, want32.to(TORCH[out_dtype]), f'{obs_shape} -> {shape} {out_dtype}')


@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
@pytest.mark.parametrize('obs_shape,shape', [pytest.param(o, s, id=iu.case_id(o, s)) for o, s in iu.BIG])
def test_megabyte_images(obs_shape, shape, dtype):
  p = iu.path_of(obs_shape, shape, dtype, dtype)
  assert p['lds'] == (73708 if dtype == 'float32' else 106476) and p['blocks_per_lane'] > 1
  obs = iu.uint8_lanes(obs_shape, 1, seed=3) if dtype == 'uint8' else iu.float_lanes(obs_shape, 1, seed=3)
  want = torch.from_numpy(io.to_image(shape, obs, batched=True))
  got = wrappers.to_image(shape, torch.from_numpy(obs).cuda())
  _assert_same(got, want, f'{obs_shape} -> {shape} {dtype}')


def test_refusals():
  dev = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device='cuda')
  for obs_shape, shape in (((1, 133), (3, 4)), ((133,), (3, 4)), ((133, 2), (4, 3))):
    with pytest.raises(ValueError, match='radius 65'):
      wrappers.to_image(shape, dev(2, *obs_shape))
  assert wrappers.to_image((3, 4), dev(2, 1, 132)).shape == (2, 3, 4)          # radius 64: accepted
  for dtype in (torch.float32, torch.uint8, torch.float16, torch.bfloat16):
    for obs_shape, shape in (((4097,), (8, 1024)), ((17, 241), (8, 241)), ((2, 4), (1025, 8)), ((2, 4), (8, 1025)),
                             ((2, 4), (8, 8, 4097)), ((2, 4), (1024, 1024)), ((2, 4), (1024, 256, 4))):
      with pytest.raises(RuntimeError, match='to_image failed'):
        wrappers.to_image(shape, dev(1, *obs_shape, dtype=dtype))
  torch.cuda.synchronize()
