"""ORACLE (test infrastructure, never imported by the product): numpy restatement of
`to_image` — bsuite/utils/wrappers.py:178-247.

`_small_state_to_image` (:178-204) is restated literally.  `_interpolate_to_image` (:207-219)
calls skimage.transform.resize, a third-party dependency that is NOT under /root/reference and not
installed (setup.py lists `scikit-image` unpinned); for scikit-image >= 0.19 that call is
scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) — preceded, when an output dimension is
smaller than the input's, by the anti-aliasing scipy.ndimage.gaussian_filter(sigma=(in/out-1)/2,
mode='mirror') — whose arithmetic `resize_bilinear` restates operation by operation in f64 (ni_interpolation.c
NI_ZoomShift: cc = (k+0.5)*zoom-0.5, map_coordinate mirror, weights (1-f, f), 4-term sum in C
order).  Pinned: bit for bit against scipy.ndimage.zoom (tests/test_image_oracle.py) and against
fixtures written by the reference's own to_image running over that scipy call
(tests/golden/image_*.npz, oracle/make_golden.py).  Parity against a real skimage: UNPINNED.

A uint8 observation takes the reference's integer path (`resize_bilinear_uint8`): skimage widens it to float64, the
Gaussian passes and the zoom stay in float64 with scipy's own weights (1 - t, 1 - (1 - t)), the result is clipped to the
image's [min, max] and truncated by numpy's assignment into the uint8 result.  Pinned against scipy.ndimage run in
float64 and against the reference's uint8 images (tests/test_image_edges_host.py, tests/golden/.tools/image_*.npz).
The clip follows skimage's rule for an image that holds a NaN (`clip_bounds`) and one image's scalar bounds (`clip`).
"""
import warnings

import numpy as np


def _mirror_index(i, n):
  if n <= 1:
    return 0
  s2 = 2 * n - 2
  if i < 0:
    i = s2 * (-i // s2) + i
    return i + s2 if i <= 1 - n else -i
  if i >= n:
    i -= s2 * (i // s2)
    if i >= n:
      i = s2 - i
  return i


def _mirror_indices(i, n):
  """_mirror_index over an integer array (C's truncating division is numpy's floor division here: every dividend is
  made non-negative first)."""
  i = np.asarray(i, np.int64)
  if n <= 1:
    return np.zeros_like(i)
  s2 = 2 * n - 2
  lo = s2 * (-i // s2) + i                          # the i < 0 branch
  lo = np.where(lo <= 1 - n, lo + s2, -lo)
  hi = i - s2 * (i // s2)                           # the i >= n branch
  hi = np.where(hi >= n, s2 - hi, hi)
  return np.where(i < 0, lo, np.where(i >= n, hi, i))


def _mirror_coord(c, n):
  if c < 0:
    if n <= 1:
      return 0.0
    s2 = 2 * n - 2
    c = s2 * int(-c / s2) + c
    return c + s2 if c <= 1 - n else -c
  if c > n - 1:
    if n <= 1:
      return 0.0
    s2 = 2 * n - 2
    c -= s2 * int(c / s2)
    if c >= n:
      c = s2 - c
  return c


def axis_table(n_in, n_out, exact1=False):
  """Source index pair and weight pair of every output coordinate along one axis.  exact1: scipy's own second weight
  1 - (1 - t) (ni_splines.c: the last spline weight is one minus the others) instead of t; the two differ in the last
  bit of t, which a float32 result never shows and a truncated float64 one does."""
  zoom = np.float64(n_in) / np.float64(n_out)
  i0 = np.zeros(n_out, np.int64)
  i1 = np.zeros(n_out, np.int64)
  w0 = np.zeros(n_out)
  w1 = np.zeros(n_out)
  for k in range(n_out):
    cc = np.float64(k)
    cc = cc + 0.5
    cc = cc * zoom
    cc = cc - 0.5
    cc = np.float64(_mirror_coord(cc, n_in))
    fl = np.floor(cc)
    t = cc - fl
    w0[k] = 1.0 - t
    w1[k] = 1.0 - w0[k] if exact1 else t
    i0[k] = _mirror_index(int(fl), n_in)
    i1[k] = _mirror_index(int(fl) + 1, n_in)
  return i0, i1, w0, w1


def gaussian_half_kernel(n_in, n_out):
  """skimage's anti-aliasing Gaussian along one axis as scipy builds it: sigma = max(0, (in/out-1)/2)
  (skimage/transform/_warps.py resize), radius = int(4*sigma + 0.5) and normalised weights
  exp(-0.5/sigma^2 * x^2) / sum (scipy.ndimage._filters._gaussian_kernel1d).  Returns the weights at
  distance 0..radius, or None when the axis is not filtered (sigma <= 1e-15, or a 1-tap kernel)."""
  sigma = max(0.0, (np.float64(n_in) / np.float64(n_out) - 1) / 2)
  if not sigma > 1e-15:
    return None
  radius = int(4.0 * float(sigma) + 0.5)
  if radius == 0:
    return None                                     # weights [1.0]: exact identity
  sigma2 = sigma * sigma
  x = np.arange(-radius, radius + 1)
  phi = np.exp(-0.5 / sigma2 * x ** 2)
  phi = phi / phi.sum()
  return phi[radius:]


def gaussian_prefilter_axis(a, half, axis, dtype=np.float32):
  """scipy NI_Correlate1D, symmetric branch, mode 'mirror', on a float32 array: per output element
  t = in[0]*w[0]; for j = radius .. 1: t += (in[-j] + in[+j]) * w[j]  (f64), rounded to f32.  dtype=np.float64: the
  array skimage filters a uint8 image in, every pass kept in f64."""
  a = np.moveaxis(np.asarray(a, dtype), axis, -1)
  n = a.shape[-1]
  r = len(half) - 1
  idx = _mirror_indices(np.arange(n)[None, :] + np.arange(-r, r + 1)[:, None], n)          # [2r+1, n]
  d = a.astype(np.float64)
  t = d * half[0]
  for j in range(r, 0, -1):
    t = t + (np.take(d, idx[r - j], axis=-1) + np.take(d, idx[r + j], axis=-1)) * half[j]
  return np.moveaxis(t.astype(dtype), -1, axis)


def clip_bounds(obs):
  """skimage's clip=True bounds per image of [..., h, w] (skimage/transform/_warps.py _clip_warp_output): the range of
  the ORIGINAL image, and its nanmin / nanmax when that range is NaN — one NaN pixel must not turn the whole image into
  NaN (an image of nothing but NaN keeps NaN bounds, and stays NaN)."""
  lo = obs.min(axis=(-2, -1), keepdims=True)
  hi = obs.max(axis=(-2, -1), keepdims=True)
  if obs.dtype.kind == 'f' and (np.isnan(lo).any() or np.isnan(hi).any()):
    with warnings.catch_warnings():
      warnings.simplefilter('ignore', RuntimeWarning)                # "All-NaN slice encountered"
      lo = np.where(np.isnan(lo), np.nanmin(obs, axis=(-2, -1), keepdims=True), lo)
      hi = np.where(np.isnan(hi), np.nanmax(obs, axis=(-2, -1), keepdims=True), hi)
  return lo, hi


def clip(out, lo, hi):
  """np.clip(image, min, max) as the reference calls it, with the SCALAR bounds of one image: a value inside [lo, hi]
  comes back untouched, a NaN stays a NaN, NaN bounds clip nothing.  Written out because numpy's clip with broadcast
  per-lane bounds returns the bound where it compares equal: +0.0 clipped to [-0.0, hi] would come back as -0.0, which
  the scalar form never does."""
  with np.errstate(invalid='ignore'):
    return np.where(out < lo, lo, np.where(out > hi, hi, out)).astype(out.dtype, copy=False)


def _filter_and_zoom(obs, out_shape, dtype):
  """The f64 four-term sum of the order-1 zoom of [..., h, w] planes of `dtype`, after the anti-aliasing passes."""
  H, W = out_shape
  exact1 = dtype == np.float64
  if H < obs.shape[-2] or W < obs.shape[-1]:
    for axis, n_out in ((-2, H), (-1, W)):
      half = gaussian_half_kernel(obs.shape[axis], n_out)
      if half is not None:
        obs = gaussian_prefilter_axis(obs, half, axis, dtype)
  y0, y1, wy0, wy1 = axis_table(obs.shape[-2], H, exact1)
  x0, x1, wx0, wx1 = axis_table(obs.shape[-1], W, exact1)
  a = obs.astype(np.float64)
  wy0, wy1 = wy0[:, None], wy1[:, None]
  t = np.zeros(obs.shape[:-2] + (H, W))
  t = t + (a[..., y0[:, None], x0[None, :]] * wy0) * wx0
  t = t + (a[..., y0[:, None], x1[None, :]] * wy0) * wx1
  t = t + (a[..., y1[:, None], x0[None, :]] * wy1) * wx0
  t = t + (a[..., y1[:, None], x1[None, :]] * wy1) * wx1
  return t


def resize_bilinear(obs, out_shape):
  """[..., h, w] -> [..., H, W]; leading dimensions are independent images.  When an axis shrinks,
  skimage >= 0.19 first applies its anti-aliasing Gaussian (scipy.ndimage.gaussian_filter, axis by
  axis, each pass rounded to the float32 input dtype), then the same order-1 zoom."""
  obs = np.asarray(obs)
  lo, hi = clip_bounds(obs)
  with np.errstate(invalid='ignore', over='ignore'):             # inf * 0 and inf - inf are NaN here as in scipy
    out = _filter_and_zoom(obs, out_shape, np.float32).astype(obs.dtype)
  return clip(out, lo, hi)                       # skimage's clip=True (range of the ORIGINAL image); a no-op for finite
                                                 # images: every stage is a convex combination rounded to nearest


def resize_bilinear_uint8(obs, out_shape):
  """The reference's integer path, [..., h, w] uint8 -> [..., H, W] uint8.  skimage widens a uint8 image to float64
  and nothing is rounded before the end: the Gaussian passes stay in f64, the zoom takes scipy's weights
  (1 - t, 1 - (1 - t)) and its four-term sum in f64, the sum is clipped to the image's [min, max], and numpy's
  assignment into the uint8 result truncates toward zero (bsuite/utils/wrappers.py:210-218).  Restated operation for
  operation as csrc/image.hip documents its IMG_U8 instantiation."""
  obs = np.asarray(obs)
  assert obs.dtype == np.uint8
  a = obs.astype(np.float64)
  lo, hi = clip_bounds(a)
  t = _filter_and_zoom(a, out_shape, np.float64)
  return clip(t, lo, hi).astype(np.uint8)


def small_state_to_image(shape, obs):
  """wrappers.py:178-204; obs [..., size] with size <= 4 -> [..., *shape]."""
  obs = np.asarray(obs)
  size = obs.shape[-1]
  lead = obs.shape[:-1]
  result = np.empty(lead + tuple(shape), dtype=obs.dtype)
  r = result.reshape((-1,) + tuple(shape))                     # view: [lanes, *shape]
  f = obs.reshape((-1, size))
  v = lambda j: f[:, j].reshape((-1,) + (1,) * len(shape))
  if size == 1:
    r[:] = v(0)
  elif size == 2:
    r[:, :, :shape[1] // 2] = v(0)
    r[:, :, shape[1] // 2:] = v(1)
  elif size in (3, 4):
    r[:, :shape[0] // 2, :shape[1] // 2] = v(0)               # "top-left"
    r[:, shape[0] // 2:, :shape[1] // 2] = v(1)               # labelled top-right, is bottom-left (:193-194)
    r[:, :shape[0] // 2, shape[1] // 2:] = v(2)
    r[:, shape[0] // 2:, shape[1] // 2:] = v(size - 1)        # flattened[-1]
  else:
    raise ValueError('Hand-crafted rule only for small state observation.')
  return result


def to_image(shape, obs, batched=False):
  """wrappers.py:222-247.  batched=True: obs carries one leading lane dimension.  A uint8 observation takes the
  float64 path and returns uint8 (resize_bilinear_uint8); every other dtype is resized as it stands."""
  shape = tuple(shape)
  assert len(shape) >= 2
  obs = np.asarray(obs)
  one = obs[0] if batched else obs
  if one.size <= 4:
    flat = obs.reshape((obs.shape[0], -1)) if batched else obs.reshape(-1)
    return small_state_to_image(shape, flat)
  if one.ndim <= 2:
    if one.ndim == 1:
      obs = np.expand_dims(obs, -2)
    plane = (resize_bilinear_uint8 if obs.dtype == np.uint8 else resize_bilinear)(obs, shape[:2])
    while plane.ndim - (1 if batched else 0) < len(shape):
      plane = np.expand_dims(plane, -1)
    return np.broadcast_to(plane, ((obs.shape[0],) if batched else ()) + shape).copy()
  raise ValueError('Cannot convert observation shape {} to desired shape {}'.format(one.shape, shape))
