// misc.hip — ABI version / error strings, the pure-store calibration kernel and the draw-stream
// dump used by the tests to pin the device Philox / normal transform against the oracle.
#include <algorithm>

#include "bsx_host.h"
#include "bsx_lane_reset.h"
#include "bsx_pair_host.h"
#include "bsx_tab_eval.h"
#include "pair_mixed.h"

extern "C" int bsx_abi_version(void) { return BSX_ABI_VERSION; }

extern "C" int bsx_observation_dtypes(int32_t family) {
  if (family == BSX_FAM_DEEP_SEA || family == BSX_FAM_CATCH) return 0xF;   // float32, uint8, float16, bfloat16
  return (family >= 0 && family <= BSX_FAM_SWEEP_MIXED) ? 0x1 : 0;
}

extern "C" int bsx_observation_index_width(int32_t family) {
  return family == BSX_FAM_DEEP_SEA ? deep_sea_hot::INDEX_K : family == BSX_FAM_CATCH ? catch_hot::INDEX_K : 0;
}

// Index observations of a call that is not lean (BSX_CALL_OBS_INDEX under Logging / RewardNoise / MT19937-exact draws /
// reward_f64): the unchanged lane advance has written the packed state column, this decodes it into the index rows —
// one lane per thread, a wave writes one contiguous 256-byte (deep_sea) or 512-byte (catch) range.  The family is a
// uniform switch; p0 / p1 are the decoder's geometry (deep_sea: N; catch: rows, columns).  `rollout`: slice t of a
// [T,B,K] array (BSX_OUT_INDEX.rollout), else an eager step's rows (BSX_OUT_INDEX.eager).
__global__ void __launch_bounds__(BSX_BLOCK) bsx_index_decode_kernel(int32_t* __restrict__ rows, const int32_t* __restrict__ state,
                                                                     int64_t n_lanes, int32_t family, int32_t p0, int32_t p1,
                                                                     int32_t rollout) {
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (i >= n_lanes) return;
  const int32_t st = state[i];
  if (family == BSX_FAM_DEEP_SEA) {
    if (rollout) bsx_index_store<BSX_OUT_INDEX.rollout>(rows, i, st, deep_sea_hot{p0});
    else bsx_index_store<BSX_OUT_INDEX.eager>(rows, i, st, deep_sea_hot{p0});
  } else {
    if (rollout) bsx_index_store<BSX_OUT_INDEX.rollout>(rows, i, st, catch_hot{p0, p1});
    else bsx_index_store<BSX_OUT_INDEX.eager>(rows, i, st, catch_hot{p0, p1});
  }
}

int bsx_launch_index_decode(int32_t* rows, const int32_t* state, int64_t n_lanes, int32_t family, int32_t p0, int32_t p1,
                            bool rollout, hipStream_t st) {
  const int64_t blocks = bsx_blocks_of(n_lanes);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  bsx_index_decode_kernel<<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(rows, state, n_lanes, family, p0, p1, rollout ? 1 : 0);
  return 0;
}

// The dense observation of a degenerate board (fewer than 4 cells) or at an address off the 16-byte grid
// (bsx_launch_hot_stream): ONE kernel for deep_sea and catch, off every measured path.  The arguments are a tagged struct —
// `family` says which decoder of `fn` is set — and the family is a uniform switch.
struct bsx_hot_cells_args {
  float* obs;
  const int32_t* state;
  int64_t n_lanes;
  uint32_t cells;
  int32_t family;
  union {
    deep_sea_hot deep_sea;
    catch_hot catch_;
  } fn;
};

__global__ void __launch_bounds__(BSX_BLOCK) bsx_hot_cells_kernel(const bsx_hot_cells_args a) {
  if (a.family == BSX_FAM_DEEP_SEA) bsx_hot_cells_body(a.obs, a.state, a.n_lanes, a.cells, a.fn.deep_sea);
  else bsx_hot_cells_body(a.obs, a.state, a.n_lanes, a.cells, a.fn.catch_);
}

int bsx_launch_hot_cells(float* obs, const int32_t* state, int64_t n_lanes, uint32_t cells, int32_t family, int32_t p0, int32_t p1,
                         hipStream_t st) {
  const uint64_t blocks = (uint64_t)bsx_blocks_of((int64_t)((uint64_t)n_lanes * cells));
  if (blocks > 0x7FFFFFFFull) return BSX_EINVAL;
  bsx_hot_cells_args a;
  a.obs = obs; a.state = state; a.n_lanes = n_lanes; a.cells = cells; a.family = family;
  if (family == BSX_FAM_DEEP_SEA) a.fn.deep_sea = deep_sea_hot{p0};
  else a.fn.catch_ = catch_hot{p0, p1};
  bsx_hot_cells_kernel<<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(a);
  return 0;
}

// evaluate_policy (bsx_<family>_policy_evaluate): ONE kernel for deep_sea and catch — the family is a uniform switch, as in
// the two kernels around it, and each branch is bsx_tab_eval_body (bsx_pair_device.h) instantiated for its family.  The LDS
// holds the shared table and both families' own staging (deep_sea's action mapping; catch has none).
__global__ void __launch_bounds__(BSX_BLOCK) bsx_tab_eval_kernel(const bsx_tab_eval_args a) {
  __shared__ deep_sea_fam::shared s_deep_sea;
  __shared__ catch_fam::shared s_catch;
  __shared__ unsigned int s_cnt[2];
  __shared__ uint8_t s_tab[BSX_POLICY_LDS_BYTES];
  if (a.family == BSX_FAM_DEEP_SEA)
    bsx_tab_eval_body<deep_sea_fam, deep_sea_hot>(a.fam.deep_sea, a.n_steps, deep_sea_hot{a.fam.deep_sea.size}, a.p, a.out,
                                                  s_deep_sea, s_cnt, s_tab);
  else
    bsx_tab_eval_body<catch_fam, catch_hot>(a.fam.catch_, a.n_steps, catch_hot{a.fam.catch_.rows, a.fam.catch_.columns}, a.p,
                                            a.out, s_catch, s_cnt, s_tab);
}

int bsx_launch_tab_eval(const bsx_tab_eval_args& a, hipStream_t st) {
  const int64_t n_lanes = a.family == BSX_FAM_DEEP_SEA ? a.fam.deep_sea.ctl.n_lanes : a.fam.catch_.ctl.n_lanes;
  bsx_tab_eval_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), 0, st>>>(a);
  return bsx_launch_status();
}

// The lane advance of a single-family group (bsx_group_set_deep_sea / bsx_group_set_catch on a group of that family;
// bsx_group_launch_pair, phase 0): ONE kernel for deep_sea and catch, off every measured path.  The family is a uniform switch
// — `table` is the device array of that family's args, one per segment — and each branch is bsx_advance_body<Fam>
// (bsx_pair_device.h) on the segment and the block bsx_group_find names.
struct bsx_pair_advance_group_args {
  const void* table;
  bsx_group_index gi;
  int32_t family;
};

__global__ void __launch_bounds__(BSX_BLOCK) bsx_pair_advance_group_kernel(const bsx_pair_advance_group_args a) {
  __shared__ deep_sea_fam::shared s_deep_sea;
  __shared__ catch_fam::shared s_catch;
  __shared__ unsigned int s_cnt[2];
  const bsx_group_slot w = bsx_group_find(a.gi, (int)blockIdx.x);
  if (a.family == BSX_FAM_DEEP_SEA)
    bsx_advance_body<deep_sea_fam>(static_cast<const deep_sea_fam::args*>(a.table)[w.seg], w.block, s_deep_sea, s_cnt);
  else
    bsx_advance_body<catch_fam>(static_cast<const catch_fam::args*>(a.table)[w.seg], w.block, s_catch, s_cnt);
}

void bsx_launch_pair_advance_group(int32_t family, const void* table, const bsx_group_index& gi, int64_t total_blocks, hipStream_t st) {
  bsx_pair_advance_group_args a;
  a.table = table; a.gi = gi; a.family = family;
  bsx_pair_advance_group_kernel<<<dim3((unsigned)total_blocks), dim3(BSX_BLOCK), 0, st>>>(a);
}

// The lane advance of the delta observation mode (bsx_call_t.obs_paint; bsx_launch_advance_delta): ONE kernel for deep_sea
// and catch, off every measured path.  The arguments are a tagged struct — `family` says which member of `fam` and of `fn`
// is set — the family is a uniform switch, and each branch is bsx_advance_delta_body<Fam, HotFn> (bsx_pair_device.h).
struct bsx_pair_advance_delta_args {
  int32_t family;
  uint32_t cells;
  int32_t* paint;
  union {
    deep_sea_hot deep_sea;
    catch_hot catch_;
  } fn;
  union {
    deep_sea_fam::args deep_sea;
    catch_fam::args catch_;
  } fam;
};

__global__ void __launch_bounds__(BSX_BLOCK) bsx_pair_advance_delta_kernel(const bsx_pair_advance_delta_args a) {
  __shared__ union {
    deep_sea_fam::shared deep_sea;
    catch_fam::shared catch_;
  } s_fam;
  __shared__ unsigned int s_cnt[2];
  if (a.family == BSX_FAM_DEEP_SEA)
    bsx_advance_delta_body<deep_sea_fam, deep_sea_hot>(a.fam.deep_sea, a.fn.deep_sea, a.paint, a.cells, s_fam.deep_sea, s_cnt);
  else
    bsx_advance_delta_body<catch_fam, catch_hot>(a.fam.catch_, a.fn.catch_, a.paint, a.cells, s_fam.catch_, s_cnt);
}

void bsx_launch_pair_advance_delta(int32_t family, const void* args, const void* fn, int32_t* paint, uint32_t cells, int64_t blocks,
                                   hipStream_t st) {
  bsx_pair_advance_delta_args a;
  a.family = family; a.cells = cells; a.paint = paint;
  if (family == BSX_FAM_DEEP_SEA) {
    a.fn.deep_sea = *static_cast<const deep_sea_hot*>(fn);
    a.fam.deep_sea = *static_cast<const deep_sea_fam::args*>(args);
  } else {
    a.fn.catch_ = *static_cast<const catch_hot*>(fn);
    a.fam.catch_ = *static_cast<const catch_fam::args*>(args);
  }
  bsx_pair_advance_delta_kernel<<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(a);
}

extern "C" const char* bsx_strerror(int code) {
  switch (code) {
    case 0: return "ok";
    case BSX_EINVAL: return "invalid scalar argument";
    case BSX_ENULL: return "required pointer is NULL";
    case BSX_EALIGN: return "observation buffer (or row scratch) is not 16-byte aligned";
    case BSX_ERANGE: return "parameter outside the supported range of this family";
    case BSX_EMODE: return "combination not available (randn in MT19937-exact mode; obs_paint with a rollout, a group or a family without a board; a narrow observation type or index observations outside a single deep_sea / catch call or with obs_paint)";
    case BSX_ENOMEM: return "host allocation failed";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown bsx error";
  }
}

// Pure-store calibration: one 16-byte store per thread, block b writes the 4 KiB run b, no loop —
// the fastest plain fill shape found on MI355X (it matches torch's fill kernel at ~6.8-6.9 TB/s on
// boxes where a 4-stores-per-thread grid-stride fill reaches 5.8-6.0; profiles/r01/
// store_calibration4_noloop.log).  What this reaches is the practical ceiling for a dense
// observation stream on the box it runs on.
// (NT = false is the only instantiation: the non-temporal fill, which nothing in the project measures against, is a mode of
// calib_copy_n_kernel below — a kernel that can hardly ever launch still counts against the library's kernel budget.)
template <bool NT>
__global__ void __launch_bounds__(BSX_BLOCK) calib_fill_kernel(bsx_f4* __restrict__ p, int64_t n16) {
  const bsx_f4 z = {0.f, 0.f, 0.f, 0.f};
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (i < n16) { if (NT) __builtin_nontemporal_store(z, &p[i]); else p[i] = z; }
}

__global__ void calib_copy_n_kernel(const bsx_f4* __restrict__ src, bsx_f4* __restrict__ dst, int64_t n16, int n_writes);

extern "C" int bsx_calib_fill(void* dst, int64_t n_bytes, int32_t nontemporal, void* hip_stream) {
  if (dst == nullptr) return BSX_ENULL;
  if (n_bytes < 0 || (n_bytes & 15) != 0) return BSX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) != 0) return BSX_EALIGN;
  if (n_bytes == 0) return 0;
  const int64_t n16 = n_bytes / 16;
  const int64_t blocks = bsx_blocks_of(n16);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  if (nontemporal) calib_copy_n_kernel<<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(nullptr, (bsx_f4*)dst, n16, 0);
  else calib_fill_kernel<false><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>((bsx_f4*)dst, n16);
  return bsx_launch_status();
}

// Copy calibration: the access mix of the small-observation families' eager step — it reads a third of what it writes
// (state in; state, TimeStep scalars and the row out).  One 16-byte load per thread, W 16-byte stores (to W regions n_bytes
// apart), no loop, blocks in address order: the rate (R + W bytes per second) such a mix reaches on this box is the
// ceiling for a kernel that mixes reads into its writes, as the fill rate is for a pure store stream.
// W = 2 is the mix the project measures against (bench.py's COPY ceiling): its stores are unrolled.
template <int W>
__global__ void __launch_bounds__(BSX_BLOCK) calib_copy_kernel(const bsx_f4* __restrict__ src, bsx_f4* __restrict__ dst, int64_t n16) {
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (i < n16) {
    const bsx_f4 v = src[i];
#pragma unroll
    for (int w = 0; w < W; ++w) dst[(int64_t)w * n16 + i] = v;
  }
}
// ... and every other mix (one store or three per load) from ONE kernel whose store count is an argument: the same
// addresses, the same bytes, a rolled loop.  n_writes == 0 is bsx_calib_fill's non-temporal mode: nothing is read and the
// thread's one 16-byte store of zeros is non-temporal — the shape of calib_fill_kernel.
__global__ void __launch_bounds__(BSX_BLOCK) calib_copy_n_kernel(const bsx_f4* __restrict__ src, bsx_f4* __restrict__ dst, int64_t n16,
                                                                 int n_writes) {
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (n_writes == 0) {                                                    // uniform
    const bsx_f4 z = {0.f, 0.f, 0.f, 0.f};
    if (i < n16) __builtin_nontemporal_store(z, &dst[i]);
    return;
  }
  if (i < n16) {
    const bsx_f4 v = src[i];
#pragma unroll 1
    for (int w = 0; w < n_writes; ++w) dst[(int64_t)w * n16 + i] = v;
  }
}

extern "C" int bsx_calib_copy(void* dst, const void* src, int64_t n_bytes, int32_t writes_per_read, void* hip_stream) {
  if (dst == nullptr || src == nullptr) return BSX_ENULL;
  if (n_bytes < 0 || (n_bytes & 15) != 0 || writes_per_read < 1 || writes_per_read > 3) return BSX_EINVAL;
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) != 0) return BSX_EALIGN;
  if (n_bytes == 0) return 0;
  const int64_t n16 = n_bytes / 16;
  const int64_t blocks = bsx_blocks_of(n16);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 g((unsigned)blocks), b(BSX_BLOCK);
  if (writes_per_read == 2) calib_copy_kernel<2><<<g, b, 0, st>>>((const bsx_f4*)src, (bsx_f4*)dst, n16);
  else calib_copy_n_kernel<<<g, b, 0, st>>>((const bsx_f4*)src, (bsx_f4*)dst, n16, writes_per_read);
  return bsx_launch_status();
}

__global__ void counter_add_kernel(uint64_t* counter, uint64_t delta) { *counter += delta; }

extern "C" int bsx_counter_add(uint64_t* counter, uint64_t delta, void* hip_stream) {
  if (counter == nullptr) return BSX_ENULL;
  counter_add_kernel<<<dim3(1), dim3(1), 0, (hipStream_t)hip_stream>>>(counter, delta);
  return bsx_launch_status();
}

// bsuite_info() for callers of the C ABI: the columns as the reference would report them right now.  catch counts its
// misses in spare bits of the packed state word and cartpole / mountain_car fold exact per-episode sums into their columns
// only when an episode ends (include/bsuite_amd.h, each family's "Accounting" note): this adds the part that is still
// pending in the lane's state — what the Python classes' bsuite_info() does on the host side of the boundary.
//   bsuite/environments/catch.py:116-117, cartpole.py:179-181, mountain_car.py:99-100
__device__ __forceinline__ void bsuite_info_body(int64_t i, int32_t family, int32_t variant, int64_t n_lanes,
                                                 const int32_t* __restrict__ state, const double* __restrict__ info,
                                                 int32_t n_info, int32_t folded, double* __restrict__ out) {
  double pend0 = 0.0, pend2 = 0.0;
  if (folded) {
    if (family == BSX_FAM_CATCH) {
      pend0 = 2.0 * (double)(((uint32_t)state[i] >> 25) & 0x7Fu);          // a miss costs regret 2 (catch.py:92-94)
    } else if ((family == BSX_FAM_CARTPOLE && variant == 0) || family == BSX_FAM_MOUNTAIN_CAR) {
      const int32_t sk = state[i];                                         // steps = k | reset_next << 30
      const double k = (sk >> 30) & 1 ? 0.0 : (double)(sk & 0x3FFFFFFF);   // the running episode has paid k rewards of +1 / -1
      pend0 = family == BSX_FAM_CARTPOLE ? k : -k;
      pend2 = family == BSX_FAM_CARTPOLE ? k : 0.0;                        // (cartpole's internal episode_return column)
    }
  }
  for (int c = 0; c < n_info; ++c)
    out[(int64_t)c * n_lanes + i] = info[(int64_t)c * n_lanes + i] + (c == 0 ? pend0 : c == 2 ? pend2 : 0.0);
}

// The draw stream of (seed, lane0 + i, step, stream_id) as the kernels consume it: n_words raw words per lane and, optionally,
// the n_words / 2 normals made from the same words (bsx_stream_dump; the tests hold both against the oracle).
__device__ __forceinline__ void stream_dump_body(int64_t i, uint64_t seed, uint64_t lane0, uint64_t step, uint32_t stream_id,
                                                 int n_words, uint32_t* words, double* normals) {
  bsx_draws d;
  bsx_draws_init(&d, seed, lane0 + (uint64_t)i, step, stream_id);
  for (int w = 0; w < n_words; ++w) words[i * n_words + w] = bsx_word(&d);
  if (normals != nullptr) {
    bsx_draws_init(&d, seed, lane0 + (uint64_t)i, step, stream_id);
    for (int w = 0; w < n_words / 2; ++w) normals[i * (n_words / 2) + w] = bsx_normal(&d);
  }
}

// bsx_bsuite_info and bsx_stream_dump: ONE kernel for the two cold one-lane-per-thread tools, off every timed path.  The
// arguments are a tagged struct — `tool` says which member of `u` is set — and the tool is a uniform switch (the idiom of
// bsx_hot_cells_kernel above); the bodies stay separate functions.
enum { BSX_LANE_TOOL_INFO = 0, BSX_LANE_TOOL_DUMP = 1 };
struct bsx_lane_tool_args {
  int32_t tool;
  int64_t n_lanes;
  union {
    struct { const int32_t* state; const double* info; double* out; int32_t family, variant, n_info, folded; } info;
    struct { uint64_t seed, lane0, step; uint32_t* words; double* normals; uint32_t stream_id; int32_t n_words; } dump;
  } u;
};

__global__ void __launch_bounds__(BSX_BLOCK) bsx_lane_tool_kernel(const bsx_lane_tool_args a) {
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (i >= a.n_lanes) return;
  if (a.tool == BSX_LANE_TOOL_INFO)
    bsuite_info_body(i, a.u.info.family, a.u.info.variant, a.n_lanes, a.u.info.state, a.u.info.info, a.u.info.n_info, a.u.info.folded,
                     a.u.info.out);
  else
    stream_dump_body(i, a.u.dump.seed, a.u.dump.lane0, a.u.dump.step, a.u.dump.stream_id, a.u.dump.n_words, a.u.dump.words,
                     a.u.dump.normals);
}

extern "C" int bsx_bsuite_info(int32_t family, int32_t variant, int64_t n_lanes, const int32_t* state, const double* info,
                               int32_t n_info, int32_t folded, double* info_out, void* hip_stream) {
  if (family < BSX_FAM_DEEP_SEA || family > BSX_FAM_MNIST || n_lanes < 0 || n_info < 0 || n_info > 8) return BSX_EINVAL;
  if (n_lanes == 0 || n_info == 0) return 0;
  if (info == nullptr || info_out == nullptr) return BSX_ENULL;
  const bool pending = folded && (family == BSX_FAM_CATCH || (family == BSX_FAM_CARTPOLE && variant == 0) || family == BSX_FAM_MOUNTAIN_CAR);
  if (pending && state == nullptr) return BSX_ENULL;
  const int64_t blocks = bsx_blocks_of(n_lanes);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  bsx_lane_tool_args a;
  a.tool = BSX_LANE_TOOL_INFO; a.n_lanes = n_lanes;
  a.u.info = {state, info, info_out, family, variant, n_info, pending ? 1 : 0};
  bsx_lane_tool_kernel<<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, (hipStream_t)hip_stream>>>(a);
  return bsx_launch_status();
}

// Per-lane reset (step(actions, reset_mask=) of the Python classes): marks the lanes whose mask byte is non-zero so that
// their next call — a step, or the first step of a rollout — takes the path of an explicit reset().  One lane per thread,
// the family a uniform switch inside bsx_lane_reset_word (bsx_lane_reset.h, which the CPU tests run through gcc): one
// coalesced byte load per lane; a masked lane whose reset bit is not set yet reads its state word, ORs the bit in and —
// classic cartpole / mountain_car with per-episode info columns — folds the abandoned episode's return into column 0,
// as the forced branch of its step does.  Unmasked lanes, and lanes that reset anyway, are not written.  Plain stores: the
// next launch on the stream reads the column from L2.  It draws nothing and reads no call index.
__global__ void __launch_bounds__(BSX_BLOCK) bsx_lane_reset_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ state,
                                                                   double* __restrict__ info, int64_t n_lanes, int32_t family,
                                                                   int32_t variant, int32_t folded) {
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (i >= n_lanes) return;
  if (mask[i] == 0) return;
  const int32_t st = state[i];
  double delta;
  const int32_t nst = bsx_lane_reset_word(st, family, variant, folded, &delta);
  if (nst == st) return;
  state[i] = nst;
  if (delta != 0.0) info[i] += delta;                 // (only where bsx_lane_reset_folds: info was checked by the host)
}

extern "C" int bsx_lane_reset_mark(int32_t family, int32_t variant, int64_t n_lanes, const uint8_t* mask, int32_t* state,
                                   double* info, int32_t folded, void* hip_stream) {
  if (family < BSX_FAM_DEEP_SEA || family > BSX_FAM_MNIST || n_lanes < 0) return BSX_EINVAL;
  if (n_lanes == 0) return 0;
  if (mask == nullptr || state == nullptr) return BSX_ENULL;
  const int folds = bsx_lane_reset_folds(family, variant, folded);
  if (folds && info == nullptr) return BSX_ENULL;
  const int64_t blocks = bsx_blocks_of(n_lanes);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  bsx_lane_reset_kernel<<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, (hipStream_t)hip_stream>>>(
      mask, state, info, n_lanes, family, variant, folds);
  return bsx_launch_status();
}

extern "C" int bsx_stream_dump(uint64_t seed, uint64_t lane0, int64_t n_lanes, uint64_t step, int32_t stream_id,
                               int32_t n_words, uint32_t* words, double* normals, void* hip_stream) {
  if (words == nullptr) return BSX_ENULL;
  if (n_lanes < 0 || n_words < 0 || n_words > 1024) return BSX_EINVAL;
  if (n_lanes == 0 || n_words == 0) return 0;
  const int64_t blocks = bsx_blocks_of(n_lanes);
  bsx_lane_tool_args a;
  a.tool = BSX_LANE_TOOL_DUMP; a.n_lanes = n_lanes;
  a.u.dump = {seed, lane0, step, words, normals, (uint32_t)stream_id, n_words};
  bsx_lane_tool_kernel<<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, (hipStream_t)hip_stream>>>(a);
  return bsx_launch_status();
}

// ------------------------------------------------------------------------------ grouped launch
extern "C" int bsx_group_create(int32_t family, int32_t n_segments, bsx_group_t** group) {
  if (group == nullptr) return BSX_ENULL;
  if (family < BSX_FAM_DEEP_SEA || family > BSX_FAM_SWEEP_MIXED || n_segments < 1 || n_segments > (1 << 20)) return BSX_EINVAL;
  bsx_group* g = nullptr;
  try {                                   // no C++ exception may cross the C boundary
    g = new bsx_group();
    g->family = family; g->n = n_segments;
    g->blocks.assign(n_segments, 0); g->blocks2.assign(n_segments, 0); g->is_set.assign(n_segments, 0);
  } catch (...) {
    delete g;
    return BSX_ENOMEM;
  }
  *group = g;
  return 0;
}

static void group_free_device(bsx_group* g) {
  void** ptrs[] = {&g->d_args, &g->d_args2, (void**)&g->d_start, (void**)&g->d_start2, (void**)&g->d_map, (void**)&g->d_map2,
                   (void**)&g->d_tags, (void**)&g->d_ticket};
  for (void** p : ptrs) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
}

static int upload(const void* src, size_t bytes, void** dst) {
  if (bytes == 0) { *dst = nullptr; return 0; }
  hipError_t e = hipMalloc(dst, bytes);
  if (e != hipSuccess) return (int)e;
  return (int)hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
}

static int group_commit(bsx_group* g);

extern "C" int bsx_group_commit(bsx_group_t* g) {
  if (g == nullptr) return BSX_ENULL;
  if (g->committed || g->launch == nullptr) return BSX_EINVAL;
  int rc;
  try {
    rc = group_commit(g);
  } catch (...) {
    rc = BSX_ENOMEM;
  }
  if (rc != 0) group_free_device(g);      // a failed commit leaves nothing behind and may be retried
  return rc;
}

static int group_commit(bsx_group* g) {
  for (int i = 0; i < g->n; ++i) if (!g->is_set[i]) return BSX_EINVAL;
  std::vector<int32_t> start(g->n + 1, 0), start2(g->n + 1, 0);
  int64_t t1 = 0, t2 = 0;
  for (int i = 0; i < g->n; ++i) {
    start[i] = (int32_t)t1; start2[i] = (int32_t)t2;
    t1 += g->blocks[i]; t2 += g->blocks2[i];
    if (t1 > 0x7FFFFFFF || t2 > 0x7FFFFFFF) return BSX_EINVAL;
  }
  start[g->n] = (int32_t)t1; start2[g->n] = (int32_t)t2;
  g->total_blocks = t1; g->total_blocks2 = t2;
  int rc = upload(g->args.data(), g->args.size(), &g->d_args);
  if (rc == 0) rc = upload(g->args2.data(), g->args2.size(), &g->d_args2);
  if (rc == 0 && !g->tags.empty()) rc = upload(g->tags.data(), g->tags.size() * 4, (void**)&g->d_tags);
  if (rc == 0 && g->family == BSX_FAM_SWEEP_MIXED) {   // two-level retirement ticket: word 0 + 64 shards, one line each
    const std::vector<uint32_t> zeros(32 * 65, 0u);
    rc = upload(zeros.data(), zeros.size() * 4, (void**)&g->d_ticket);
  }
  if (rc == 0) rc = upload(start.data(), start.size() * 4, (void**)&g->d_start);
  if (rc == 0) rc = upload(start2.data(), start2.size() * 4, (void**)&g->d_start2);
  // (segment, local block) of every workgroup: one load per workgroup instead of a binary search;
  // launches beyond 2^24 workgroups (128 MiB of map) keep the search.
  for (int pass = 0; pass < 2 && rc == 0; ++pass) {
    const int64_t total = pass == 0 ? t1 : t2;
    const std::vector<int32_t>& blocks = pass == 0 ? g->blocks : g->blocks2;
    if (total == 0 || total > (1 << 24)) continue;
    std::vector<int2> map((size_t)total);
    size_t w = 0;
    for (int i = 0; i < g->n; ++i)
      // the segment's family tag rides in the top byte of the entry (mixed groups): the workgroup then needs ONE
      // load, not map entry -> tag, before it can fetch its argument slot
      for (int32_t b = 0; b < blocks[i]; ++b) {
        map[w].x = i | ((g->tags.empty() ? 0 : ((g->tags[i] + 1) & 0x7F)) << 24);   // tag + 1; 0 = none
        map[w].y = b;
        ++w;
      }
    rc = upload(map.data(), map.size() * sizeof(int2), (void**)(pass == 0 ? &g->d_map : &g->d_map2));
  }
  if (rc != 0) return rc;
  g->stream_without_alt = false;
  for (uint8_t f : g->needs_alt) g->stream_without_alt = g->stream_without_alt || f != 0;
  // the split step needs the segments with a share of the store stream to be the tail of the phase-0 grid
  g->rows_sorted.clear();
  for (const void* p : g->row_scratch) if (p != nullptr) g->rows_sorted.push_back(reinterpret_cast<uintptr_t>(p));
  std::sort(g->rows_sorted.begin(), g->rows_sorted.end());
  g->split_block = -1;
  g->split_round = -1;
  if (g->family == BSX_FAM_SWEEP_MIXED) {
    int first = g->n;
    while (first > 0 && g->blocks2[first - 1] > 0) --first;
    bool tail_only = true;
    for (int i = 0; i < first; ++i) tail_only = tail_only && g->blocks2[i] == 0;
    if (tail_only) g->split_block = start[first];
  }
  g->committed = true;
  return 0;
}

extern "C" int bsx_group_step(bsx_group_t* g, void* hip_stream) {
  if (g == nullptr) return BSX_ENULL;
  if (!g->committed) return BSX_EINVAL;
  return g->launch(g, -1, (hipStream_t)hip_stream);
}

extern "C" int bsx_group_phases(const bsx_group_t* g) { return g == nullptr ? BSX_ENULL : g->n_phases; }

extern "C" int bsx_group_step_phase(bsx_group_t* g, int32_t phase, void* hip_stream) {
  if (g == nullptr) return BSX_ENULL;
  if (!g->committed || phase < 0 || phase >= g->n_phases) return BSX_EINVAL;
  return g->launch(g, phase, (hipStream_t)hip_stream);
}

extern "C" int bsx_group_step_split(bsx_group_t* g, void* hip_stream) {
  if (g == nullptr) return BSX_ENULL;
  if (!g->committed) return BSX_EINVAL;
  if (g->family != BSX_FAM_SWEEP_MIXED || g->split_block < 0) return BSX_EMODE;
  return bsx_sweep_launch_split(g, (hipStream_t)hip_stream);
}

extern "C" int bsx_group_step_pipelined(bsx_group_t* streams_of, bsx_group_t* advances_of, void* hip_stream) {
  if (streams_of == nullptr || advances_of == nullptr) return BSX_ENULL;
  if (!streams_of->committed || !advances_of->committed || streams_of->family != BSX_FAM_SWEEP_MIXED ||
      advances_of->family != BSX_FAM_SWEEP_MIXED || streams_of->n != advances_of->n ||
      streams_of->shared_counter != advances_of->shared_counter)
    return BSX_EINVAL;
  if (streams_of->stream_without_alt || advances_of->stream_without_alt) return BSX_EMODE;
  // a chain segment on the row path must not share its row scratch between the two groups (the stream of step s would
  // decode the rows the advance of step s+1 is writing) — checked on EVERY call and against every segment of the other
  // group (one merge over the two sorted lists frozen at commit: no cached verdict that a recycled group address could outlive)
  for (size_t i = 0, j = 0; i < streams_of->rows_sorted.size() && j < advances_of->rows_sorted.size();) {
    const uintptr_t p = streams_of->rows_sorted[i], q = advances_of->rows_sorted[j];
    if (p == q) return BSX_EMODE;
    if (p < q) ++i; else ++j;
  }
  return bsx_sweep_launch_pipelined(streams_of, advances_of, (hipStream_t)hip_stream);
}

extern "C" int bsx_group_trace(bsx_group_t* g, uint64_t* buf, int64_t capacity) {
  if (g == nullptr) return BSX_ENULL;
  if (g->family != BSX_FAM_SWEEP_MIXED) return BSX_EMODE;
  if (buf != nullptr && (!g->committed || capacity < 3 * g->total_blocks)) return BSX_EINVAL;
  g->trace = buf;
  return 0;
}

extern "C" int bsx_group_destroy(bsx_group_t* g) {
  if (g == nullptr) return 0;
  group_free_device(g);
  delete g;
  return 0;
}
