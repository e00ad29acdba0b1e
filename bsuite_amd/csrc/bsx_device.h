// bsx_device.h — device-side building blocks shared by every environment-family kernel.
//
// gfx950 (MI355X / CDNA4) only: 64-wide wavefronts, 256-thread workgroups (4 waves = one per
// SIMD), LDS for per-block constants and hot-cell indices, 16-byte cooperative stores for the
// observation stream.  No MFMA anywhere: the path is integer indexing + scalar f32/f64.
#ifndef BSX_DEVICE_H_
#define BSX_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bsuite_amd.h"
#include "../../include/bsx_stream.h"
#include "bsx_index.h"

#define BSX_BLOCK 256
#define BSX_WAVE 64

typedef float bsx_f4 __attribute__((ext_vector_type(4)));
typedef float bsx_f2 __attribute__((ext_vector_type(2)));

// Cache policy of an OUTPUT store.  PLAIN; NT = non-temporal (`nt`): the lines neither stay in L2 nor allocate in the Infinity
// Cache; WT = write-through (`sc1`): they leave L2 for the memory side at once but DO land in the Infinity Cache.
// Which one pays depends on who reads the output next (round 6, profiles/r06/ab_store_cache_policies.log,
// ab_nt_outputs_closed_loop_policy.log; cartpole at 2^20 lanes, us per step: eager alone | fused rollout | closed loop with
// a device-side linear policy reading every observation):  plain 17.6-18.1 | 9.1-9.3 | 115-116.5;  nt 15.6-16.6 | 7.5-7.8 |
// 119.5;  sc1 16.2-16.7 | 9.3-9.8 | 114.5.  A rollout's T x B outputs have no reader inside the call: NT.  An eager step()
// exists to be followed by an agent that READS the observation: its outputs must not be pushed past the Infinity Cache —
// WT keeps most of the step's gain (the step's own inputs are no longer evicted from L2) and costs the reader nothing.
enum { BSX_ST_PLAIN = 0, BSX_ST_NT = 1, BSX_ST_WT = 2 };
// (the write-through stores are inline asm — no builtin sets sc1 alone — and end with `s_nop 1`: the compiler's hazard
// recognizer does not look inside an asm string, and a VALU write of the data registers right behind a store of more than
// 8 bytes is a hazard on gfx9: without it mountain_car's 12-byte rows came out corrupted on a few lanes per wave.
// Invariant of every caller: an sc1 store only ever targets global memory — `global_store ... off` takes the generic pointer
// as a global address — and nothing in the kernel reads its bytes back: the compiler's wait-count insertion does not count
// a store it cannot see, so no later load of the same address would wait for it.)
#if defined(__HIP_DEVICE_COMPILE__)
template <int BYTES> struct bsx_wt_store;
template <> struct bsx_wt_store<1> { template <class T> __device__ static __forceinline__ void go(const void* p, T v) { uint32_t w = 0; __builtin_memcpy(&w, &v, 1); asm volatile("global_store_byte %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory"); } };
template <> struct bsx_wt_store<4> { template <class T> __device__ static __forceinline__ void go(const void* p, T v) { uint32_t w; __builtin_memcpy(&w, &v, 4); asm volatile("global_store_dword %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory"); } };
template <> struct bsx_wt_store<8> { template <class T> __device__ static __forceinline__ void go(const void* p, T v) { uint64_t w; __builtin_memcpy(&w, &v, 8); asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory"); } };
template <> struct bsx_wt_store<12> { template <class T> __device__ static __forceinline__ void go(const void* p, T v) { typedef uint32_t u3 __attribute__((ext_vector_type(3))); u3 w; __builtin_memcpy(&w, &v, 12); asm volatile("global_store_dwordx3 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory"); } };
template <> struct bsx_wt_store<16> { template <class T> __device__ static __forceinline__ void go(const void* p, T v) { bsx_f4 w; __builtin_memcpy(&w, &v, 16); asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory"); } };
#endif
template <int POLICY, class P, class V>
__device__ __forceinline__ void bsx_st(P* p, V v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (POLICY == BSX_ST_NT) __builtin_nontemporal_store((P)v, p);
  else if constexpr (POLICY == BSX_ST_WT) bsx_wt_store<sizeof(P)>::go((const void*)p, (P)v);
  else *p = (P)v;
#else
  *p = (P)v;
#endif
}
// The policy of one kind of output, in a fused rollout and in an eager step (small_obs.h has the measurements and the rule:
// a rollout's outputs have no reader inside the call, an eager step's are read by the agent next).
struct bsx_out_policy { int rollout, eager; };
constexpr int bsx_policy(bsx_out_policy p, bool rollout) { return rollout ? p.rollout : p.eager; }
constexpr bsx_out_policy BSX_OUT_SCALARS = {BSX_ST_NT, BSX_ST_WT};        // reward / discount / step_type columns (a wave's store is
                                                                          // one contiguous 256- / 64-byte range)
// Per-call values every kernel needs, flattened out of bsx_call_t on the host.
struct bsx_ctl {
  int64_t n_lanes;
  uint64_t seed;
  uint64_t lane_offset;
  uint64_t step_index;
  const uint64_t* step_base;
  uint64_t* counters;
  double wrap_param;
  double wrap_param2;       // stacked wrappers: the outer wrapper's parameter
  double wrap_mul;          // RewardScale alone: its scale; no wrapper: 1.0 (x * 1.0 == x bit for bit) — the NOISE = 0
                            // instantiations multiply unconditionally instead of branching on wrap_kind
  uint64_t wrap_seed;
  int32_t wrap_kind;
  int32_t force_reset;
  uint32_t action_ring_mask; // R - 1 for an action ring of R = 2^k rows [R, n_lanes] (bsx_call_t.action_ring), else 0
  uint32_t _pad;
  uint32_t* mt_state;       // MT19937-exact mode: [624, n_lanes] generator states, else nullptr
  int32_t* mt_pos;          // [n_lanes]
  double* mt_gauss;         // [n_lanes] cached second normal of the env generator (nullable)
  int32_t* mt_has_gauss;
  uint32_t* wrap_mt_state;  // RewardNoise's own generator in MT19937-exact mode (all four or none)
  int32_t* wrap_mt_pos;
  double* wrap_mt_gauss;
  int32_t* wrap_mt_has_gauss;
  double* reward_f64;       // optional f64 copy of the reward column (scalar dm_env view), else nullptr
  const int32_t* state_in;  // two-kernel families: the packed state column the advance READS (nullptr: `state`)
  bsx_logging_t log;        // log.steps == nullptr: logging off
};

// No Logging wrapper, no RewardNoise, counter-based draws, no f64 reward copy (the scalar dm_env view's): the call
// the lean instantiations serve.
__host__ __device__ __forceinline__ bool bsx_ctl_lean(const bsx_ctl& c) {
  return c.log.steps == nullptr && c.wrap_kind < BSX_WRAP_NOISE && c.mt_state == nullptr && c.reward_f64 == nullptr;
}

// bsuite_info accumulators (f64 columns [K, B], a lane owns its slots).  An update can be a NO-RETURN hardware atomic
// (global_atomic_add_f64) where nothing in the launch reads the column back (no fused Logging rows): the same IEEE add,
// executed at the L2, and the wave does not wait for a dependent load of a cold column from HBM before it stores.
// Measured in every family, same call (profiles/r04/ab_info_atomics.log): it pays where a few lanes of a wave update now
// and then — memory_chain with long episodes, memory_len 13.3 -> 12.0 us per step — and costs where updates are dense
// (bandit 9.6 -> 11.2, memory_size 44.1 -> 47.4, umbrella_distract 98 -> 103, deep_sea's headline 589 -> 595) or is
// neutral (cartpole, mountain_car, mnist): adopted for memory_chain at L >= 8 only.  The columns must then be ordinary
// device memory (hardware f64 atomics do not reach fine-grained host mappings): include/bsuite_amd.h says so.
// `quiet`: no Logging wrapper reads the column in this launch (bsx_track snapshots it).
__device__ __forceinline__ void bsx_info_add(bool quiet, double* p, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (quiet) { __builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double*)p, v); return; }
#endif
  *p += v;
}
template <int LOG>
__device__ __forceinline__ bool bsx_info_quiet(const bsx_ctl& c) { return LOG == 0 || (LOG == -1 && c.log.steps == nullptr); }

__device__ __forceinline__ uint64_t bsx_step_of(const bsx_ctl& c) {
  return c.step_index + (c.step_base ? *c.step_base : 0ull);
}

// The action of output element `oi` (lane i of a step() call; t*B + i inside a fused rollout) on call `step`.
// With an action ring (bsx_call_t.action_ring = R) the call reads row (step mod R) of `action` [R, B] — the
// offset is uniform per workgroup (scalar unit) and zero without a ring.
__device__ __forceinline__ int bsx_action(const bsx_ctl& c, const int32_t* __restrict__ action, int64_t oi, uint64_t step) {
  return action[oi + (int64_t)(step & (uint64_t)c.action_ring_mask) * c.n_lanes];
}

// Opens lane i's environment draw stream for this call: the counter-based stream, or — in
// MT19937-exact mode — the lane's own RandomState carried in HBM.  bsx_draws_end writes the
// generator position back (the state words are updated in place by the twist).
// MT: -1 decide at run time (c.mt_state != nullptr), 0 the MT19937 mode is compiled out.
template <int MT = -1>
__device__ __forceinline__ void bsx_draws_begin(bsx_draws* d, const bsx_ctl& c, int64_t i, uint64_t lane,
                                                uint64_t step) {
  bsx_draws_init(d, c.seed, lane, step, BSX_STREAM_ENV);
  if (MT != 0 && c.mt_state != nullptr) {
    d->mt = c.mt_state + i;
    d->mt_stride = c.n_lanes;
    d->mt_pos = c.mt_pos[i];
    if (c.mt_gauss != nullptr) { d->mt_has_gauss = c.mt_has_gauss[i]; d->mt_gauss = c.mt_gauss[i]; }
  }
}
template <int MT = -1>
__device__ __forceinline__ void bsx_draws_end(const bsx_draws* d, const bsx_ctl& c, int64_t i) {
  if (MT != 0 && c.mt_state != nullptr) {
    c.mt_pos[i] = d->mt_pos;
    if (c.mt_gauss != nullptr) { c.mt_has_gauss[i] = d->mt_has_gauss; c.mt_gauss[i] = d->mt_gauss; }
  }
}

// Reward epilogue of utils/wrappers.py:275-283 (RewardNoise) and :338-346 (RewardScale): non-FIRST
// lanes only, evaluated in f64 like the reference, result cast to f32 once.
// NOISE = 0 compiles the RewardNoise branch out: its ~100 f64 polynomial constants are otherwise
// hoisted into VGPRs ahead of the T-step rollout loop and cost two thirds of the occupancy.
// MT = 0: the call draws from the counter-based stream (bsx_make_ctl sets wrap_mt_state only in MT19937-exact mode): the
// wrapper's own generator — twist, legacy gauss, libm log — is compiled out.
template <int NOISE = -1, int MT = -1>
__device__ __forceinline__ double bsx_wrap_reward(const bsx_ctl& c, int64_t i, uint64_t lane, uint64_t step,
                                                  double reward) {
  BSX_NO_CONTRACT
  if (NOISE == 0) return reward * c.wrap_mul;        // RewardScale or nothing: no branch (bsx_ctl.wrap_mul)
  if (c.wrap_kind == BSX_WRAP_SCALE) return reward * c.wrap_param;
  if (NOISE != 0 && c.wrap_kind >= BSX_WRAP_NOISE) {
    // RewardNoise alone, or stacked with RewardScale in either order (each wrapper acts on what the one
    // inside it returned): SCALE_NOISE = r*s + sigma*z, NOISE_SCALE = (r + sigma*z)*s
    const double sigma = c.wrap_kind == BSX_WRAP_SCALE_NOISE ? c.wrap_param2 : c.wrap_param;
    if (c.wrap_kind == BSX_WRAP_SCALE_NOISE) reward = reward * c.wrap_param;
    bsx_draws w;
    bsx_draws_init(&w, c.wrap_seed, lane, step, BSX_STREAM_WRAP);
    double z;
    if (MT != 0 && c.wrap_mt_state != nullptr) {       // MT19937-exact mode: the wrapper's own RandomState (wrappers.py:267)
      w.mt = c.wrap_mt_state + i;
      w.mt_stride = c.n_lanes;
      w.mt_pos = c.wrap_mt_pos[i];
      w.mt_has_gauss = c.wrap_mt_has_gauss[i];
      w.mt_gauss = c.wrap_mt_gauss[i];
      z = bsx_normal(&w);
      c.wrap_mt_pos[i] = w.mt_pos;
      c.wrap_mt_has_gauss[i] = w.mt_has_gauss;
      c.wrap_mt_gauss[i] = w.mt_gauss;
    } else {
      z = bsx_normal(&w);
    }
    reward = reward + sigma * z;
    if (c.wrap_kind == BSX_WRAP_NOISE_SCALE) reward = reward * c.wrap_param2;
    return reward;
  }
  return reward;
}

// `Logging._track` + `_log_bsuite_data` of bsuite/utils/wrappers.py:85-125 for one lane.  `reward`
// is the f64 reward the outermost wrapper returned (0.0 on FIRST, where the reference adds
// `timestep.reward or 0.0`).  The family's step function has already applied this call's updates
// to its info columns, so the snapshot sees the same bsuite_info() the reference logs.
__device__ __forceinline__ void bsx_track(const bsx_ctl& c, int64_t i, int type, double reward) {
  BSX_NO_CONTRACT
  const bsx_logging_t& g = c.log;
  int64_t steps = g.steps[i], episode = g.episode[i], ep_len = g.episode_len[i];
  double total = g.total_return[i], ep_ret = g.episode_return[i];
  if (type != BSX_FIRST) { steps += 1; ep_len += 1; }                    // :87-89
  if (type == BSX_LAST) episode += 1;                                     // :90-91
  ep_ret += reward;                                                       // :92
  total += reward;                                                        // :93
  bool log = false;
  const int64_t key = g.log_by_step ? steps : episode;
  if (g.log_by_step || type == BSX_LAST) {                                // :96-102
    log = g.log_every != 0;
    int lo = 0, hi = g.n_log_points;                                      // _logarithmic_logging :140-147
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const int64_t v = g.log_points[mid];
      if (v == key) { log = true; break; }
      if (v < key) lo = mid + 1; else hi = mid;
    }
  }
  if (log) {                                                              // _log_bsuite_data :112-125
    const int n = g.n_rows[i];
    g.n_rows[i] = n + 1;
    if (n < g.max_rows) {
      const int w = 5 + g.n_info;
      double* row = g.rows + ((int64_t)i * g.max_rows + n) * w;
      row[0] = (double)steps; row[1] = (double)episode; row[2] = total;
      row[3] = (double)ep_len; row[4] = ep_ret;
      for (int k = 0; k < g.n_info; ++k) row[5 + k] = g.info[(int64_t)k * c.n_lanes + i];
    }
  }
  if (type == BSX_LAST) { ep_len = 0; ep_ret = 0.0; }                     // :105-107
  g.steps[i] = steps; g.episode[i] = episode; g.episode_len[i] = ep_len;
  g.total_return[i] = total; g.episode_return[i] = ep_ret;
}

// The scalar TimeStep fields of one lane: wrapper epilogue + Logging bookkeeping, values only.
// LOG: -1 decide at run time (c.log.steps != nullptr), 0 logging compiled out, 1 always track.
// `oi` is the output element (== i for step(); t*B + i inside a fused rollout).
// F64 = false: the lean instantiations (bsx_ctl_lean: reward_f64 == nullptr) compile the f64 reward copy out.
template <int LOG = -1, int NOISE = -1, bool F64 = true, int MT = -1>
__device__ __forceinline__ void bsx_emit_values(const bsx_ctl& c, int64_t i, int64_t oi, uint64_t lane, uint64_t step,
                                                int type, double reward, float& r, float& d) {
  r = 0.0f; d = 1.0f;         // FIRST: dm_env.restart has reward/discount None -> 0 / 1 in a batch
  double wrapped = 0.0;
  if (type != BSX_FIRST) {
    wrapped = bsx_wrap_reward<NOISE, MT>(c, i, lane, step, reward);
    r = (float)wrapped;
    d = (type == BSX_LAST) ? 0.0f : 1.0f;
  }
  if (F64 && c.reward_f64 != nullptr) c.reward_f64[oi] = wrapped;
  if (LOG == 1 || (LOG == -1 && c.log.steps != nullptr)) bsx_track(c, i, type, wrapped);
}

// Writes the scalar TimeStep fields of one lane (coalesced: lane i -> element oi of each column;
// oi == i for step(), oi == t*B + i inside a fused T-step rollout).
// POLICY: other than plain stores (the scalar columns' policy, small_obs.h) ONLY where every lane of a wave emits, lane by lane (the small-observation
// kernels): a wave's store is then one contiguous range.  A lone emitting thread (the writer threads of deep_sea's
// single-launch step: one lane per 225 threads) must not — 4-byte non-temporal stores scattered over the grid took that
// kernel from 81 to 125 us at 2^17 lanes.
template <int LOG = -1, int NOISE = -1, bool F64 = true, int MT = -1, int POLICY = BSX_ST_PLAIN>
__device__ __forceinline__ void bsx_emit_at(const bsx_ctl& c, const bsx_timestep_t& out, int64_t i, int64_t oi,
                                            uint64_t lane, uint64_t step, int type, double reward) {
  float r, d;
  bsx_emit_values<LOG, NOISE, F64, MT>(c, i, oi, lane, step, type, reward, r, d);
  bsx_st<POLICY>(&out.reward[oi], r);
  bsx_st<POLICY>(&out.discount[oi], d);
  bsx_st<POLICY>(&out.step_type[oi], (int8_t)type);
}
__device__ __forceinline__ void bsx_emit(const bsx_ctl& c, const bsx_timestep_t& out, int64_t i,
                                         uint64_t lane, uint64_t step, int type, double reward) {
  bsx_emit_at(c, out, i, i, lane, step, type, reward);
}

// Termination / restart masks by wavefront ballot.  Each wave popcounts its LAST / FIRST masks
// into two LDS words (s_cnt, zeroed by the caller before the phase); after the block's barrier one
// thread flushes them with one global atomic per mask into the block's shard of the counter array
// (bsx_flush_counts).  A single device-wide word would serialise ~16k same-address atomics on the
// steps where every lane terminates (~200 us measured on catch at B=2^20).  Inactive lanes (beyond
// n_lanes) must pass type = -1.
__device__ __forceinline__ void bsx_count_types(const bsx_ctl& c, int type, unsigned int* s_cnt) {
  if (c.counters == nullptr) return;
  unsigned long long last = __ballot(type == BSX_LAST);
  unsigned long long first = __ballot(type == BSX_FIRST);
  if ((threadIdx.x & (BSX_WAVE - 1)) == 0) {
    if (last) atomicAdd(&s_cnt[0], (unsigned int)__popcll(last));
    if (first) atomicAdd(&s_cnt[1], (unsigned int)__popcll(first));
  }
}

// What a wave's lanes have written to the wave's own LDS, visible to all of them: LDS serves a wave's accesses in order, so
// this orders the compiler and costs no workgroup barrier.
__device__ __forceinline__ void bsx_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The LAST barrier of a workgroup, in front of bsx_flush_counts: it has to order the waves' LDS counter updates and
// nothing else.  __syncthreads() is a fence + barrier, and on gfx9 its release half waits for vmcnt(0) — every wave
// sat through the acknowledgements of its final stores (1-3 us behind a saturated memory system) before it could
// arrive, and the workgroup's slot stayed taken for that long; the waves may simply END with their stores in flight
// (the kernel's completion covers them).
__device__ __forceinline__ void bsx_final_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#else
  __syncthreads();
#endif
}

// Call after a __syncthreads() that follows every wave's bsx_count_types.
__device__ __forceinline__ void bsx_flush_counts(const bsx_ctl& c, const unsigned int* s_cnt,
                                                 uint32_t block_id = 0xFFFFFFFFu) {
  if (c.counters == nullptr || threadIdx.x != 0) return;
  if (block_id == 0xFFFFFFFFu) block_id = blockIdx.x;
  unsigned long long* shard = (unsigned long long*)c.counters +
                              (size_t)(block_id & (BSX_COUNTER_SHARDS - 1)) * BSX_COUNTER_STRIDE;
  if (s_cnt[0]) atomicAdd(&shard[0], (unsigned long long)s_cnt[0]);
  if (s_cnt[1]) atomicAdd(&shard[1], (unsigned long long)s_cnt[1]);
}

// The epilogue of a fused rollout, whose threads count their lanes' LAST / FIRST steps in registers: pooled into s_cnt
// (zeroed before the first barrier of the kernel) once per launch, then the final barrier and the flush.
__device__ __forceinline__ void bsx_pool_counts(const bsx_ctl& c, uint32_t n_last, uint32_t n_first, unsigned int* s_cnt,
                                                uint32_t block_id) {
  if (c.counters != nullptr) {
    if (n_last) atomicAdd(&s_cnt[0], n_last);
    if (n_first) atomicAdd(&s_cnt[1], n_first);
  }
  bsx_final_barrier();
  bsx_flush_counts(c, s_cnt, block_id);
}

// Error word: the batched kernels never fault on an action outside the action_spec —
// bandit / discounting_chain clamp, catch moves the paddle by (action - 1) and clips — where the
// reference raises IndexError; every such lane-step is counted in word 2 of the lane's counter shard
// so a caller can assert `invalid_action_count() == 0` without a per-step host check.  Rare path:
// a plain global atomic.
__device__ __forceinline__ void bsx_note_invalid_action(const bsx_ctl& c, int64_t i) {
  if (c.counters == nullptr) return;
  unsigned long long* shard = (unsigned long long*)c.counters +
                              (size_t)((uint64_t)(i >> 8) & (BSX_COUNTER_SHARDS - 1)) * BSX_COUNTER_STRIDE;
  atomicAdd(&shard[2], 1ull);
}

// Grouped launch: which segment a workgroup belongs to, and its index inside that segment.
// `map` (device memory, one (segment, local block) pair per workgroup of the launch) answers with ONE
// scalar load; without it (launches too large to tabulate) the segment is the largest s with
// start[s] <= b, found by binary search over the exclusive prefix sums `start` (n+1 entries) — a
// chain of ~log2(n) dependent loads in front of every workgroup, which cost the store-stream
// kernels 10-35 % when the sweep's 16 KiB workgroups each paid it (profiles/r01/ab_sweep_modes.log).
struct bsx_group_index {
  const int32_t* start;
  const int2* map;
  int n;
};

struct bsx_group_slot { int seg; uint32_t block; int tag; };   // tag: the segment's family in a mixed group, -1 = look it up

__device__ __forceinline__ bsx_group_slot bsx_group_find(const bsx_group_index& gi, int b) {
  bsx_group_slot r;
  if (gi.map != nullptr) {
    const int2 v = gi.map[b];
    r.seg = v.x & 0x00FFFFFF; r.block = (uint32_t)v.y; r.tag = ((v.x >> 24) & 0x7F) - 1;
    return r;
  }
  r.tag = -1;
  int lo = 0, hi = gi.n;         // invariant: start[lo] <= b < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gi.start[mid] <= b) lo = mid; else hi = mid;
  }
  r.seg = lo; r.block = (uint32_t)(b - gi.start[lo]);
  return r;
}

// n / cells for n < 2^20 via the host-built magic (bsx_div_magic); cells == 1 has no 32-bit magic.
__device__ __forceinline__ uint32_t bsx_div_cells(uint32_t n, uint32_t cells, uint32_t cells_magic) {
  return cells == 1u ? n : __umulhi(n, cells_magic);
}

// Exact 64-bit magic division (bsx_make_div64, bsx_host.h): the store streams split a workgroup's first element into
// (lane, offset) with it, once per workgroup, on the scalar unit.
struct bsx_div64 {            // n / d = __umul64hi(n, m) >> s, exact for n*d < 2^(64+s), d >= 4
  uint64_t m;
  uint32_t s;
};

#endif  // BSX_DEVICE_H_
