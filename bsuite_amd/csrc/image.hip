// ImageObservation adapter: bsuite/utils/wrappers.py:150-247 `to_image` for a whole
// batch as one store stream.  Output per lane is an [H, W, tail] f32 image (84x84x4 = 110 KiB for
// the Atari-like format), so the kernel is bound by HBM stores exactly like the deep_sea
// observation stream; the source observation of a lane (<= 16 KiB) is staged in LDS.
//
// Element types (bsx_image_observation_typed): the float images (f32, f16, bf16) read any of the four observation types
// widened to f32 and round the f32 pixel to the output type; uint8 -> uint8 is the reference's integer path in f64
// (img_out below).  A 16-byte store holds 16 / sizeof(T) elements: narrow images are the same store stream with fewer
// bytes and more pixels per store.
//
// Work split: a workgroup owns one run of IMG_K * BSX_BLOCK 16-byte chunks of ONE lane's image, so the
// per-axis interpolation tables (source indices + f64 weights, identical for every lane) and the
// lane's observation are built once per workgroup in LDS; each thread then issues IMG_K
// lane-interleaved 16-byte stores.
//
// Arithmetic of the bilinear rule restates scipy.ndimage.zoom(order=1, mode='mirror',
// grid_mode=True) — what skimage.transform.resize(order=1, mode='reflect') calls, after its
// anti-aliasing Gaussian along the axes that shrink (img_gauss_pass) — operation for operation in
// f64 without FMA:
//   zoom = in / out;  cc = ((k + 0.5) * zoom) - 0.5;  cc = mirror(cc);  f = floor(cc);
//   weights (1 - (cc - f), cc - f) on source indices mirror(f), mirror(f + 1);
//   t = 0 + (v00*wy0)*wx0 + (v01*wy0)*wx1 + (v10*wy1)*wx0 + (v11*wy1)*wx1;  out = (float)t
// (the f64 uint8 path takes scipy's own second weight 1 - (1 - (cc - f)), see img_axis_entry)
// (pinned bit for bit against scipy in tests/test_image_oracle.py, tests/test_gpu_adapters.py and tests/test_gpu_image_dtype.py;
// tests/test_gpu_image_edges.py holds the edges: filters wider than their axis, more than 64 KiB of LDS, every store
// branch of every output type over several workgroups, ties, overflow, subnormals, signed zeros, inf and NaN).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bsuite_amd.h"
#include "bsx_device.h"
#include "bsx_host.h"

// The anti-aliasing half kernels travel BY VALUE in the kernel arguments (2 x 65 doubles = 1040 B) and are copied to
// LDS by the workgroups that filter: no device buffer owned by the library, so no allocation or synchronous upload
// inside the entry point (capturable from the first call) and nothing tied to the device that happened to be current
// when a configuration was first seen (a process-global cache of device pointers faulted on a second GPU).
struct image_gauss { double w[2][BSX_IMAGE_MAX_RADIUS + 1]; };   // [0] rows (y), [1] columns (x)

struct image_args {
  const void* obs; void* image; int64_t n_lanes;
  int32_t mode, in_rows, in_cols, out_rows, out_cols, tail;
  int32_t radius_y, radius_x;                     // anti-aliasing Gaussian (down-scaling), 0 = none
  int32_t in_code;                                // element code of obs (BSX_CALL_OBS_* >> BSX_CALL_OBS_SHIFT)
  uint32_t numel;                                 // out_rows*out_cols*tail (< 2^20)
  uint32_t tail_magic, cols_magic;                // bsx_div_magic(tail), bsx_div_magic(out_cols)
  uint32_t blocks_per_lane;
};

// Element codes: the observation numbering of bsx_call_t.flags (BSX_CALL_OBS_* >> BSX_CALL_OBS_SHIFT).
enum { IMG_F32 = 0, IMG_U8 = 1, IMG_F16 = 2, IMG_BF16 = 3 };

// Output element OUT: its type, and the staged plane type S.  The float outputs stage f32 and round the f32 pixel to
// nearest-even (plain casts: v_cvt_f16_f32 / v_cvt_pk_bf16_f32, which keep NaNs); uint8 -> uint8 follows the
// reference's integer path (skimage widens to f64 and never rounds until numpy's assignment truncates the clipped
// value), so it stages f64 planes.
template <int OUT> struct img_out;
template <> struct img_out<IMG_F32> { typedef float T; typedef float S; };
template <> struct img_out<IMG_F16> { typedef _Float16 T; typedef float S; };
template <> struct img_out<IMG_BF16> { typedef __bf16 T; typedef float S; };
template <> struct img_out<IMG_U8> { typedef uint8_t T; typedef double S; };

// scipy ni_interpolation.c map_coordinate(), NI_EXTEND_MIRROR, for the (-0.5, len-0.5) range the
// grid-mode zoom produces (one reflection suffices; the general fold is kept for safety).
__device__ __forceinline__ double img_mirror_coord(double c, int len) {
  BSX_NO_CONTRACT
  if (len <= 1) return (c < 0.0 || c > (double)(len - 1)) ? 0.0 : c;
  const int s2 = 2 * len - 2;
  if (c < 0.0) {
    c = (double)(s2 * (int)(-c / (double)s2)) + c;
    return c <= (double)(1 - len) ? c + (double)s2 : -c;
  }
  if (c > (double)(len - 1)) {
    c -= (double)(s2 * (int)(c / (double)s2));
    if (c >= (double)len) c = (double)s2 - c;
  }
  return c;
}

__device__ __forceinline__ int img_mirror_index(int i, int len) {
  if (len <= 1) return 0;
  const int s2 = 2 * len - 2;
  if (i < 0) {
    i = s2 * (-i / s2) + i;
    return i <= 1 - len ? i + s2 : -i;
  }
  if (i >= len) {
    i -= s2 * (i / s2);
    if (i >= len) i = s2 - i;
  }
  return i;
}

// One axis-table entry: source index pair (packed 16+16) and the two weights.  scipy's order-1 spline weights are
// (1 - t, 1 - (1 - t)) (ni_splines.c: the last weight is 1 minus the others); the f32 path keeps (1 - t, t), which is
// pinned to scipy's f32 output after rounding, the f64 path (exact1 = true) needs scipy's own second weight.
__device__ __forceinline__ void img_axis_entry(int k, int n_in, int n_out, bool exact1, int* idx, double* w0, double* w1) {
  BSX_NO_CONTRACT
  const double zoom = (double)n_in / (double)n_out;
  double cc = (double)k;
  cc = cc + 0.5;
  cc = cc * zoom;
  cc = cc - 0.5;
  cc = img_mirror_coord(cc, n_in);
  const double fl = floor(cc);
  const int start = (int)fl;
  const double t = cc - fl;
  *w0 = 1.0 - t;
  *w1 = exact1 ? 1.0 - *w0 : t;
  *idx = img_mirror_index(start, n_in) | (img_mirror_index(start + 1, n_in) << 16);
}

template <class S>
struct img_tables {
  const S* s_obs; const int* s_yi; const int* s_xi;
  const double* s_yw; const double* s_xw;          // [2*k], [2*k+1]
};

// Pixel p of the plane: f32 (the f32 path, rounded from the f64 sum exactly as scipy's f32 output) or the f64 sum
// itself (the uint8 path, clipped and truncated by the caller).
template <class S>
__device__ __forceinline__ S img_pixel(const image_args& a, const img_tables<S>& tb, uint32_t p) {
  BSX_NO_CONTRACT
  const uint32_t y = bsx_div_cells(p, (uint32_t)a.out_cols, a.cols_magic);
  const uint32_t x = p - y * (uint32_t)a.out_cols;
  if (a.mode == BSX_IMAGE_SMALL) {                 // wrappers.py:178-204
    const int size = a.in_rows * a.in_cols;
    const bool right = (int)x >= (a.out_cols >> 1), lower = (int)y >= (a.out_rows >> 1);
    int j;
    if (size == 1) j = 0;
    else if (size == 2) j = right ? 1 : 0;
    else j = right ? (lower ? size - 1 : 2) : (lower ? 1 : 0);
    return tb.s_obs[j];
  }
  const int yi = tb.s_yi[y], xi = tb.s_xi[x];
  const int y0 = (yi & 0xFFFF) * a.in_cols, y1 = (yi >> 16) * a.in_cols;
  const int x0 = xi & 0xFFFF, x1 = xi >> 16;
  const double wy0 = tb.s_yw[2 * y], wy1 = tb.s_yw[2 * y + 1];
  const double wx0 = tb.s_xw[2 * x], wx1 = tb.s_xw[2 * x + 1];
  double t = 0.0;
  t = t + ((double)tb.s_obs[y0 + x0] * wy0) * wx0;
  t = t + ((double)tb.s_obs[y0 + x1] * wy0) * wx1;
  t = t + ((double)tb.s_obs[y1 + x0] * wy1) * wx0;
  t = t + ((double)tb.s_obs[y1 + x1] * wy1) * wx1;
  return (S)t;
}

// skimage's anti-aliasing pre-filter = scipy.ndimage.gaussian_filter(mode='mirror') on the observation staged in
// LDS: one pass per filtered axis (rows, then columns), each element
//   t = in[0]*w[0];  for j = radius..1: t += (in[-j] + in[+j]) * w[j]        (f64, NI_Correlate1D's
// symmetric branch), stored as S: rounded to f32 like scipy's float32 output array, or kept in f64 like the float64
// array skimage filters a uint8 image in.  src -> dst, both [rows x cols].
template <class S>
__device__ __forceinline__ void img_gauss_pass(const S* src, S* dst, int rows, int cols, int axis,
                                               int radius, const double* __restrict__ w) {
  BSX_NO_CONTRACT
  const int n = rows * cols, len = axis == 0 ? rows : cols, stride = axis == 0 ? cols : 1;
  for (int e = threadIdx.x; e < n; e += BSX_BLOCK) {
    const int y = e / cols, x = e - y * cols;
    const int pos = axis == 0 ? y : x;
    const int base = e - pos * stride;               // element 0 of this line
    double t = (double)src[e] * w[0];
    for (int j = radius; j >= 1; --j) {
      const double lo = (double)src[base + img_mirror_index(pos - j, len) * stride];
      const double hi = (double)src[base + img_mirror_index(pos + j, len) * stride];
      t = t + (lo + hi) * w[j];
    }
    dst[e] = (S)t;
  }
}

// One input element widened to f32 (exact for all four codes); `code` is uniform.
__device__ __forceinline__ float img_load_f32(const void* lane_obs, int code, int j) {
  if (code == IMG_U8) return (float)static_cast<const uint8_t*>(lane_obs)[j];
  if (code == IMG_F16) return (float)static_cast<const _Float16*>(lane_obs)[j];
  if (code == IMG_BF16) return __uint_as_float((uint32_t)static_cast<const uint16_t*>(lane_obs)[j] << 16);
  return static_cast<const float*>(lane_obs)[j];
}

// Pixel value -> output bits (low sizeof(T) bytes).  uint8: clip to the lane's [lo, hi] (skimage's clip=True) and
// truncate toward zero (numpy's float64 -> uint8 assignment).
template <int OUT>
__device__ __forceinline__ uint32_t img_bits(typename img_out<OUT>::S v, double lo, double hi) {
  typedef typename img_out<OUT>::T T;
  if constexpr (OUT == IMG_U8) {
    v = v < lo ? lo : (v > hi ? hi : v);
    return (uint32_t)v;
  } else {
    (void)lo; (void)hi;
    const T t = (T)v;
    if constexpr (sizeof(T) == 4) return __float_as_uint(t);
    else { uint16_t u; __builtin_memcpy(&u, &t, 2); return u; }
  }
}

// Workgroup: IMG_K 16-byte chunks per thread of ONE lane's image, i.e. a run of IMG_K * BSX_BLOCK * (16 / sizeof(T))
// elements.  OUT = output element code; the float outputs take the input code at run time (a.in_code), the uint8
// output reads uint8 only.
template <int OUT, int IMG_K>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_image_kernel(const image_args a, const image_gauss gw) {
  typedef typename img_out<OUT>::T T;
  typedef typename img_out<OUT>::S S;
  constexpr uint32_t C = 16 / sizeof(T);           // elements per 16-byte chunk
  constexpr uint32_t IMG_RUN = IMG_K * BSX_BLOCK * C;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_gauss[2][BSX_IMAGE_MAX_RADIUS + 1];
  __shared__ int s_range[2];                       // uint8 path: the lane's [min, max]
  if (a.radius_y > 0 || a.radius_x > 0) {         // uniform
    for (int j = threadIdx.x; j < 2 * (BSX_IMAGE_MAX_RADIUS + 1); j += BSX_BLOCK)
      s_gauss[j / (BSX_IMAGE_MAX_RADIUS + 1)][j % (BSX_IMAGE_MAX_RADIUS + 1)] = gw.w[j / (BSX_IMAGE_MAX_RADIUS + 1)][j % (BSX_IMAGE_MAX_RADIUS + 1)];
  }
  // LDS layout: y weights f64 [2*H] | x weights f64 [2*W] | obs S [in] | (filter: second plane S [in]) | y idx i32 [H]
  // | x idx i32 [W]  (the planes follow the f64 tables, so an f64 plane is 8-byte aligned)
  const int in_numel = a.in_rows * a.in_cols;
  const bool filtered = a.radius_y > 0 || a.radius_x > 0;
  double* s_yw = reinterpret_cast<double*>(s_raw);
  double* s_xw = s_yw + 2 * a.out_rows;
  S* s_obs = reinterpret_cast<S*>(s_xw + 2 * a.out_cols);
  S* s_tmp = s_obs + in_numel;                     // second plane: only allocated when a filter runs
  int* s_yi = reinterpret_cast<int*>(s_tmp + (filtered ? in_numel : 0));
  int* s_xi = s_yi + a.out_rows;

  const uint32_t lane = blockIdx.x / a.blocks_per_lane;
  const uint32_t run = blockIdx.x - lane * a.blocks_per_lane;
  if constexpr (OUT == IMG_U8) {
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.obs) + (int64_t)lane * in_numel;
    if (threadIdx.x == 0) { s_range[0] = 255; s_range[1] = 0; }
    __syncthreads();
    int lo = 255, hi = 0;
    for (int j = threadIdx.x; j < in_numel; j += BSX_BLOCK) {
      const int v = src[j];
      s_obs[j] = (double)v;
      lo = v < lo ? v : lo; hi = v > hi ? v : hi;
    }
    if (lo <= hi) { atomicMin(&s_range[0], lo); atomicMax(&s_range[1], hi); }
  } else {
    const void* src = static_cast<const unsigned char*>(a.obs) + (int64_t)lane * in_numel * (a.in_code == IMG_F32 ? 4 : a.in_code == IMG_U8 ? 1 : 2);
    for (int j = threadIdx.x; j < in_numel; j += BSX_BLOCK) s_obs[j] = img_load_f32(src, a.in_code, j);
  }
  if (a.mode == BSX_IMAGE_BILINEAR) {
    for (int k = threadIdx.x; k < a.out_rows + a.out_cols; k += BSX_BLOCK) {
      int idx; double w0, w1;
      if (k < a.out_rows) {
        img_axis_entry(k, a.in_rows, a.out_rows, OUT == IMG_U8, &idx, &w0, &w1);
        s_yi[k] = idx; s_yw[2 * k] = w0; s_yw[2 * k + 1] = w1;
      } else {
        const int kx = k - a.out_rows;
        img_axis_entry(kx, a.in_cols, a.out_cols, OUT == IMG_U8, &idx, &w0, &w1);
        s_xi[kx] = idx; s_xw[2 * kx] = w0; s_xw[2 * kx + 1] = w1;
      }
    }
  }
  __syncthreads();
  if (a.radius_y > 0) {                            // uniform branches: the barriers are safe
    img_gauss_pass<S>(s_obs, s_tmp, a.in_rows, a.in_cols, 0, a.radius_y, s_gauss[0]);
    __syncthreads();
    S* t = s_obs; s_obs = s_tmp; s_tmp = t;
  }
  if (a.radius_x > 0) {
    img_gauss_pass<S>(s_obs, s_tmp, a.in_rows, a.in_cols, 1, a.radius_x, s_gauss[1]);
    __syncthreads();
    S* t = s_obs; s_obs = s_tmp; s_tmp = t;
  }
  img_tables<S> tb; tb.s_obs = s_obs; tb.s_yi = s_yi; tb.s_xi = s_xi; tb.s_yw = s_yw; tb.s_xw = s_xw;
  double lo = 0.0, hi = 0.0;
  if constexpr (OUT == IMG_U8) { lo = (double)s_range[0]; hi = (double)s_range[1]; }

  T* __restrict__ dst = static_cast<T*>(a.image) + (int64_t)lane * a.numel;
  const uint32_t tail = (uint32_t)a.tail;
  const uint32_t f_begin = run * IMG_RUN;
  if ((a.numel & (C - 1)) == 0u) {
    // 16-byte stores (every lane's image starts on a 16-byte boundary); each wave owns IMG_K consecutive KiB (same
    // order as the observation stream)
    const uint32_t wave = threadIdx.x >> 6, wl = threadIdx.x & 63u;
    const bool same = (tail & (C - 1)) == 0;       // the C elements of a chunk share their pixel
    constexpr int RUN_UNROLL = C == 4 ? IMG_K : 1;  // narrow chunks unroll up to 16 guarded pixel evaluations each
#pragma unroll RUN_UNROLL
    for (int j = 0; j < IMG_K; ++j) {
      const uint32_t f = f_begin + ((wave * IMG_K + j) * 64u + wl) * C;
      if (f < a.numel) {
        uint32_t p0 = bsx_div_cells(f, tail, a.tail_magic);
        uint32_t w[4];
        if (same) {
          uint32_t b = img_bits<OUT>(img_pixel<S>(a, tb, p0), lo, hi);
          if constexpr (C >= 8) b |= b << (128 / C);
          if constexpr (C == 16) b |= b << 16;
          w[0] = b; w[1] = b; w[2] = b; w[3] = b;
        } else {
          // each distinct pixel is computed once and repeated over the part of its tail inside this chunk; element q
          // lands at byte 4 * (q / (4 / sizeof(T))) + sizeof(T) * q % 4 (statically placed: the loop is unrolled)
          uint32_t rem = f - p0 * tail;            // position inside pixel p0's tail
          uint32_t b = img_bits<OUT>(img_pixel<S>(a, tb, p0), lo, hi);
          w[0] = 0; w[1] = 0; w[2] = 0; w[3] = 0;
#pragma unroll
          for (uint32_t q = 0; q < C; ++q) {
            w[q * sizeof(T) / 4] |= b << (8 * ((q * sizeof(T)) & 3));
            if (++rem == tail && q + 1 < C) { rem = 0; ++p0; b = img_bits<OUT>(img_pixel<S>(a, tb, p0), lo, hi); }
          }
        }
        bsx_f4 v;
        v.x = __uint_as_float(w[0]); v.y = __uint_as_float(w[1]); v.z = __uint_as_float(w[2]); v.w = __uint_as_float(w[3]);
        *reinterpret_cast<bsx_f4*>(dst + f) = v;
      }
    }
  } else {
    // images whose byte size is not a multiple of 16 do not start every lane on a 16-byte boundary: element stores
    const uint32_t f_end = f_begin + IMG_RUN < a.numel ? f_begin + IMG_RUN : a.numel;
    for (uint32_t f = f_begin + threadIdx.x; f < f_end; f += BSX_BLOCK) {
      const uint32_t b = img_bits<OUT>(img_pixel<S>(a, tb, bsx_div_cells(f, tail, a.tail_magic)), lo, hi);
      if constexpr (sizeof(T) == 4) reinterpret_cast<uint32_t*>(dst)[f] = b;
      else if constexpr (sizeof(T) == 2) reinterpret_cast<uint16_t*>(dst)[f] = (uint16_t)b;
      else reinterpret_cast<uint8_t*>(dst)[f] = (uint8_t)b;
    }
  }
}

template <int OUT>
static void img_launch(int k, dim3 grid, dim3 block, size_t lds, hipStream_t st, const image_args& a, const image_gauss& gw) {
  switch (k) {
    case 8: bsx_image_kernel<OUT, 8><<<grid, block, lds, st>>>(a, gw); break;
    case 16: bsx_image_kernel<OUT, 16><<<grid, block, lds, st>>>(a, gw); break;
    default: bsx_image_kernel<OUT, 4><<<grid, block, lds, st>>>(a, gw); break;
  }
}

extern "C" int bsx_image_observation_typed(const bsx_image_t* cfg, int64_t n_lanes, const void* obs, int32_t obs_code,
                                           void* image, int32_t image_code, void* hip_stream) {
  if (obs_code < IMG_F32 || obs_code > IMG_BF16 || image_code < IMG_F32 || image_code > IMG_BF16) return BSX_EINVAL;
  if (image_code == IMG_U8 && obs_code != IMG_U8) return BSX_EMODE;   // no quantisation is invented
  if (cfg == nullptr) return BSX_ENULL;
  if (n_lanes < 0) return BSX_EINVAL;
  if (cfg->mode != BSX_IMAGE_SMALL && cfg->mode != BSX_IMAGE_BILINEAR) return BSX_EINVAL;
  if (cfg->in_rows < 1 || cfg->in_cols < 1 || cfg->out_rows < 1 || cfg->out_cols < 1 || cfg->tail < 1)
    return BSX_ERANGE;
  const int64_t in_numel = (int64_t)cfg->in_rows * cfg->in_cols;
  const int64_t numel = (int64_t)cfg->out_rows * cfg->out_cols * cfg->tail;
  if (in_numel > 4096 || cfg->out_rows > 1024 || cfg->out_cols > 1024 || cfg->tail > 4096 || numel >= (1 << 20))
    return BSX_ERANGE;
  if (cfg->mode == BSX_IMAGE_SMALL && in_numel > 4) return BSX_ERANGE;        // wrappers.py:200-201
  if (cfg->radius_y < 0 || cfg->radius_x < 0 || cfg->radius_y > BSX_IMAGE_MAX_RADIUS || cfg->radius_x > BSX_IMAGE_MAX_RADIUS)
    return BSX_ERANGE;
  const bool filtered = cfg->mode == BSX_IMAGE_BILINEAR && (cfg->radius_y > 0 || cfg->radius_x > 0);
  if (n_lanes == 0) return 0;
  if (obs == nullptr || image == nullptr) return BSX_ENULL;
  const int in_size = obs_code == IMG_F32 ? 4 : (obs_code == IMG_U8 ? 1 : 2);
  const int out_size = image_code == IMG_F32 ? 4 : (image_code == IMG_U8 ? 1 : 2);
  if (((uintptr_t)image & 15u) != 0 || ((uintptr_t)obs & (uintptr_t)(in_size - 1)) != 0) return BSX_EALIGN;
  image_args a;
  a.obs = obs; a.image = image; a.n_lanes = n_lanes;
  a.mode = cfg->mode; a.in_rows = cfg->in_rows; a.in_cols = cfg->in_cols;
  a.out_rows = cfg->out_rows; a.out_cols = cfg->out_cols; a.tail = cfg->tail;
  a.radius_y = filtered ? cfg->radius_y : 0; a.radius_x = filtered ? cfg->radius_x : 0;
  a.in_code = obs_code;
  a.numel = (uint32_t)numel;
  a.tail_magic = bsx_div_magic((uint32_t)cfg->tail);
  a.cols_magic = bsx_div_magic((uint32_t)cfg->out_cols);
  // Run length per workgroup: every workgroup re-stages its lane's observation and rebuilds the axis
  // tables before its first store, so large observations want longer runs (measured on 84x84x4,
  // profiles/r01/ab_image_k.log: 10x5 input best at 4 KiB x 4, 30x30 at x16; images whose
  // channel count is not a multiple of 4 evaluate up to four pixels per store and prefer x8).
  // Runs are counted in 16-byte chunks, so a narrow workgroup covers the same bytes and 4 / sizeof(T) times the pixels;
  // their best runs differ (profiles/image_dtype/bench_image_k.jsonl): f16 / bf16 x16 where whole pixels of four
  // channels share a chunk, else x4; uint8 x8, x4 for one channel from a small observation.
  const bool tail4 = (cfg->tail & 3) == 0;
  const int k_best = image_code == IMG_F32 ? (in_numel > 256 && tail4 ? 16 : (in_numel > 64 ? 8 : 4))
                     : image_code == IMG_U8 ? (tail4 || in_numel > 64 ? 8 : 4) : (tail4 ? 16 : 4);
  const int k = bsx_env_int("BSX_IMAGE_K", k_best);
  const int64_t run = (int64_t)k * BSX_BLOCK * (16 / out_size);
  a.blocks_per_lane = (uint32_t)((numel + run - 1) / run);
  const int64_t blocks = n_lanes * (int64_t)a.blocks_per_lane;
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  const size_t plane = (size_t)in_numel * (image_code == IMG_U8 ? 8 : 4);
  const size_t lds = (size_t)(cfg->out_rows + cfg->out_cols) * (16 + 4) + plane * (filtered ? 2 : 1);
  const dim3 grid((unsigned)blocks), block(BSX_BLOCK);
  hipStream_t st = (hipStream_t)hip_stream;
  image_gauss gw;
  memset(&gw, 0, sizeof(gw));
  if (filtered) {
    for (int j = 0; j <= cfg->radius_y; ++j) gw.w[0][j] = cfg->gauss_y[j];
    for (int j = 0; j <= cfg->radius_x; ++j) gw.w[1][j] = cfg->gauss_x[j];
  }
  switch (image_code) {
    case IMG_U8: img_launch<IMG_U8>(k, grid, block, lds, st, a, gw); break;
    case IMG_F16: img_launch<IMG_F16>(k, grid, block, lds, st, a, gw); break;
    case IMG_BF16: img_launch<IMG_BF16>(k, grid, block, lds, st, a, gw); break;
    default: img_launch<IMG_F32>(k, grid, block, lds, st, a, gw); break;
  }
  return bsx_launch_status();
}

extern "C" int bsx_image_observation(const bsx_image_t* cfg, int64_t n_lanes, const float* obs, float* image,
                                     void* hip_stream) {
  return bsx_image_observation_typed(cfg, n_lanes, obs, IMG_F32, image, IMG_F32, hip_stream);
}
