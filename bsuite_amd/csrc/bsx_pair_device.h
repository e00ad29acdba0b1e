// bsx_pair_device.h — device code of the two-kernel ("pair") families deep_sea and catch: a lane advance that leaves a packed
// state word per lane, and a store stream that decodes the words into boards.  Fam = deep_sea_fam / catch_fam, HotFn = deep_sea_hot /
// catch_hot (deep_sea_fam.h, catch_fam.h).  What every kernel of the library shares is bsx_device.h.
#ifndef BSX_PAIR_DEVICE_H_
#define BSX_PAIR_DEVICE_H_

#include "bsx_device.h"
#include "bsx_policy.h"

// Fam::advance<LEAN> — with the family's MT19937-exact draws compiled out as well when NOMT (deep_sea's extra template
// parameter sits between the two).
template <class Fam, bool LEAN, bool NOMT>
__device__ __forceinline__ int bsx_fam_advance(const typename Fam::args& a, const typename Fam::shared& s, int64_t i, uint64_t lane,
                                               uint64_t step, int32_t st, int act, int32_t& nst, double& reward) {
  return Fam::template advance_nomt<LEAN, NOMT>(a, s, i, lane, step, st, act, nst, reward);
}

// Advance kernel of the two-kernel families (deep_sea, catch): one lane per thread, coalesced
// column loads/stores.  At B=2^20 it moves only 22 MB and sits at the ~8 us launch/latency floor of
// any 2^20-lane kernel; a 4-lanes-per-thread variant with 16-byte column accesses measured the
// same for catch and slower for deep_sea, whose per-lane Philox draw then runs 4x serially
// (profiles/r01/ab_advance_vec4.log).
//
// Fam provides: struct args { bsx_ctl ctl; const int32_t* action; int32_t* state; bsx_timestep_t out;
//                             double* info; ... };  struct shared;  static stage(args, shared&);
//   static int advance(args, shared, i, lane, step, st, act, nst&, reward&)
// LEAN: no Logging wrapper, no RewardNoise, counter-based draws — those branches are compiled out (the
// launcher picks it when the call has none of them).
// MT = 0 (with LEAN = false): a wrapped call on the counter-based stream — the MT19937-exact generators of the
// environment and of RewardNoise are compiled out (the whole-sweep group, which holds no MT19937-exact segment).
// LPT = 2: TWO lanes per thread — lanes b*512 + t and b*512 + 256 + t, the loads of both issued before the first use:
// half as many workgroups, i.e. ONE dispatch round at 2^20 lanes instead of two.
template <class Fam, bool LEAN = false, int MT = -1, int LPT = 1>
__device__ __forceinline__ void bsx_advance_body(const typename Fam::args& a, uint32_t block_id,
                                                 typename Fam::shared& s_fam, unsigned int* s_cnt,
                                                 int32_t* s_state = nullptr) {
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  __syncthreads();
  if constexpr (LPT == 2) {
    const uint64_t step = bsx_step_of(a.ctl);
    int64_t i[2];
    bool mine[2];
    int act[2], type[2] = {-1, -1};
    int32_t st[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      i[h] = (int64_t)block_id * (2 * BSX_BLOCK) + h * BSX_BLOCK + threadIdx.x;
      mine[h] = i[h] < a.ctl.n_lanes;
      act[h] = 0; st[h] = 0;
      if (mine[h]) {
        if (!a.ctl.force_reset) act[h] = bsx_action(a.ctl, a.action, i[h], step);
        st[h] = a.ctl.state_in != nullptr ? a.ctl.state_in[i[h]] : a.state[i[h]];
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (mine[h]) {
        const uint64_t lane = a.ctl.lane_offset + (uint64_t)i[h];
        int32_t nst; double reward;
        type[h] = bsx_fam_advance<Fam, LEAN, MT == 0>(a, s_fam, i[h], lane, step, st[h], act[h], nst, reward);
        a.state[i[h]] = nst;
        if (LEAN) bsx_emit_at<0, 0, false>(a.ctl, a.out, i[h], i[h], lane, step, type[h], reward);
        else bsx_emit_at<-1, -1, true, MT>(a.ctl, a.out, i[h], i[h], lane, step, type[h], reward);
      }
      bsx_count_types(a.ctl, type[h], s_cnt);
    }
    bsx_final_barrier();
    bsx_flush_counts(a.ctl, s_cnt, block_id);
    return;
  }
  const int64_t i = (int64_t)block_id * BSX_BLOCK + threadIdx.x;
  int type = -1;
  if (i < a.ctl.n_lanes) {
    const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
    const uint64_t step = bsx_step_of(a.ctl);
    int32_t nst; double reward;
    const int act = a.ctl.force_reset ? 0 : bsx_action(a.ctl, a.action, i, step);
    const int32_t st = a.ctl.state_in != nullptr ? a.ctl.state_in[i] : a.state[i];
    type = bsx_fam_advance<Fam, LEAN, MT == 0>(a, s_fam, i, lane, step, st, act, nst, reward);
    a.state[i] = nst;
    if (s_state != nullptr) s_state[threadIdx.x] = nst;     // fused small-batch step: the tile streamer reads it from LDS
    if (LEAN) bsx_emit_at<0, 0, false>(a.ctl, a.out, i, i, lane, step, type, reward);
    else bsx_emit_at<-1, -1, true, MT>(a.ctl, a.out, i, i, lane, step, type, reward);
  }
  bsx_count_types(a.ctl, type, s_cnt);
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, block_id);
}

// (A family with Fam::ADVANCE_WITHOUT_MT == false — deep_sea — has no <Fam, false, 0> kernel of its own: its wrapped kernel
// <Fam, false, -1> holds BOTH bodies and takes one uniform branch on ctl.mt_state per launch, so that a wrapped call on the
// counter-based stream runs the body with the MT19937-exact generators compiled out, as it did from its own kernel.)
template <class Fam, bool LEAN = false, int MT = -1>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_advance_kernel(const typename Fam::args a) {
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  if constexpr (!LEAN && MT == -1 && !Fam::ADVANCE_WITHOUT_MT) {
    if (a.ctl.mt_state == nullptr) bsx_advance_body<Fam, false, 0>(a, blockIdx.x, s_fam, s_cnt);
    else bsx_advance_body<Fam, false, -1>(a, blockIdx.x, s_fam, s_cnt);
  } else {
    bsx_advance_body<Fam, LEAN, MT>(a, blockIdx.x, s_fam, s_cnt);
  }
}
// (the WRAPPED call with two lanes per thread — Logging / RewardNoise instantiation — measured in round 6 and not kept:
// catch_noise/0 49.4-50.0 -> 51.4-51.7 us per step, its normal draws then run twice in series; deep_sea under Logging equal;
// profiles/r06/ab_wrapped_advance_two_lanes.log, catch_noise_kernel_stats.csv: the wrapped advance is 18.0 us, the lean one 9.1)
template <class Fam>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_advance2_kernel(const typename Fam::args a) {     // two lanes per thread, lean
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  bsx_advance_body<Fam, true, -1, 2>(a, blockIdx.x, s_fam, s_cnt);
}

// (the lane advance of a single-family GROUP — bsx_advance_body<Fam> over a table of segments — is ONE kernel for deep_sea and
// catch, the family a uniform switch: bsx_pair_advance_group_kernel, misc.hip)

// ---------------------------------------------------------------------------------------------
// Index observations (bsx_call_t.flags & BSX_CALL_OBS_INDEX): the observation of a lane is the K = HotFn::INDEX_K hot-cell
// numbers its decoder (deep_sea_hot, catch_hot) reads from the packed state word — int32 rows [B, K] — instead of the
// board.  25-29 bytes per lane-step and no store stream: a step is a lane advance whose thread also stores the K numbers
// decoded from the word it has just computed.
typedef int32_t bsx_i2 __attribute__((ext_vector_type(2)));
constexpr bsx_out_policy BSX_OUT_INDEX = {BSX_ST_NT, BSX_ST_WT};          // index observation rows (BSX_CALL_OBS_INDEX): one 4- or
                                                                          // 8-byte store per lane, a wave's 256 / 512 bytes contiguous

// Row `oi` of the index array from the packed state `st`: one store of K * 4 bytes.
template <int POLICY, class HotFn>
__device__ __forceinline__ void bsx_index_store(int32_t* __restrict__ rows, int64_t oi, int32_t st, const HotFn& fn) {
  static_assert(HotFn::INDEX_K == 1 || HotFn::INDEX_K == 2, "index rows are one or two cells");
  int ha, hb;
  fn(st, ha, hb);
  if constexpr (HotFn::INDEX_K == 1) {
    bsx_st<POLICY>(rows + oi, (int32_t)ha);
  } else {
    const bsx_i2 v = {ha, hb};
    bsx_st<POLICY>(reinterpret_cast<bsx_i2*>(rows) + oi, v);
  }
}

// The lean step() / reset() in index mode: ONE launch — bsx_advance_body<Fam, true>'s lane advance, one lane per thread,
// and the thread stores its lane's index row.  Outputs are an eager step's (write-through: the agent reads them next).
template <class Fam, class HotFn>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_index_step_kernel(const typename Fam::args a, int32_t* __restrict__ rows,
                                                                   const HotFn fn) {
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  int type = -1;
  if (i < a.ctl.n_lanes) {
    const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
    const uint64_t step = bsx_step_of(a.ctl);
    int32_t nst; double reward;
    const int act = a.ctl.force_reset ? 0 : bsx_action(a.ctl, a.action, i, step);
    type = Fam::template advance<true>(a, s_fam, i, lane, step, a.state[i], act, nst, reward);
    a.state[i] = nst;
    bsx_emit_at<0, 0, false, -1, BSX_OUT_SCALARS.eager>(a.ctl, a.out, i, i, lane, step, type, reward);
    bsx_index_store<BSX_OUT_INDEX.eager>(rows, i, nst, fn);
  }
  bsx_count_types(a.ctl, type, s_cnt);
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, blockIdx.x);
}

// The lean rollout(T) in index mode: ONE launch for all T steps.  The state word stays in a register from its load to
// its store, the family's tables are staged in LDS once, and the actions are loaded RUN steps ahead of their use: on gfx9
// loads and stores share one in-order vmcnt, so waiting for a load issued among the stores drains the stores too — one
// such wait per run instead of one per step (the loop shape of small_obs_regs_rollout, small_obs.h).  LAST / FIRST steps
// are counted per thread and pooled once per launch.  Outputs [T,B] / [T,B,K] have no reader inside the call: non-temporal.
template <class Fam, class HotFn>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_index_rollout_kernel(const typename Fam::args a, const int n_steps,
                                                                      int32_t* __restrict__ rows, const HotFn fn) {
  constexpr int RUN = 8;
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  __syncthreads();
  const int64_t B = a.ctl.n_lanes;
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  const bool mine = i < B;
  const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a.ctl);
  int32_t st = mine ? a.state[i] : 0;
  uint32_t n_last = 0, n_first = 0;
  // (the workgroup's number waits for the final flush in a VECTOR register: deep_sea's step loop — Philox and the f64 normal
  // transform of the stochastic variant — leaves no scalar pair free for it, and the compiler would spill one)
  uint32_t block_id = blockIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(block_id));
#endif
#pragma unroll 1
  for (int t0 = 0; t0 < n_steps; t0 += RUN) {
    const int run = n_steps - t0 < RUN ? n_steps - t0 : RUN;             // uniform
    int acts[RUN];
    // (rows beyond the run re-read its last row: no per-row condition mask in scalar registers;
    // and the threads beyond the batch re-read lane 0: no branch around the loads)
    const int32_t* const ap = a.action + (int64_t)t0 * B + (mine ? i : 0);
#pragma unroll
    for (int j = 0; j < RUN; ++j) acts[j] = ap[(int64_t)(j < run ? j : run - 1) * B];
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_s_waitcnt(0x0070);     // vmcnt(0) lgkmcnt(0): the run's actions have landed, nothing pends inside the run
#endif
    // (a rolled loop, the run's action picked by selects: unrolled, the scheduler interleaves the steps' Philox blocks)
#pragma unroll 1
    for (int j = 0; j < run; ++j) {
      int act = acts[0];
#pragma unroll
      for (int q = 1; q < RUN; ++q) act = j == q ? acts[q] : act;
      if (mine) {
        const int t = t0 + j;
        const int64_t oi = (int64_t)t * B + i;
        int32_t nst; double reward;
        const int type = Fam::template advance<true>(a, s_fam, i, lane, step0 + (uint64_t)t, st, act, nst, reward);
        st = nst;
        bsx_emit_at<0, 0, false, -1, BSX_OUT_SCALARS.rollout>(a.ctl, a.out, i, oi, lane, step0 + (uint64_t)t, type, reward);
        bsx_index_store<BSX_OUT_INDEX.rollout>(rows, oi, nst, fn);
        n_last += type == BSX_LAST ? 1u : 0u;
        n_first += type == BSX_FIRST ? 1u : 0u;
      }
    }
  }
  if (mine) a.state[i] = st;
  bsx_pool_counts(a.ctl, n_last, n_first, s_cnt, block_id & (BSX_COUNTER_SHARDS - 1));    // (the shard is all bsx_flush_counts takes from it)
}

// The tabular policy of a fused closed-loop rollout, flattened out of bsx_policy_t on the host.
struct bsx_policy_args {
  const uint8_t* table;          // [n_policies, n_states]
  const int32_t* policy_index;   // [n_lanes], nullptr when n_policies == 1
  int32_t* actions_out;          // [n_steps, n_lanes]
  double epsilon;
  uint64_t explore_seed;
  int32_t n_states, n_policies;
  uint32_t num_actions;
  int32_t in_lds;                // one shared table of at most BSX_POLICY_LDS_BYTES: every workgroup stages it in LDS
};

// rollout_policy(T) in index mode: bsx_index_rollout_kernel with the action SOURCE replaced — no action tensor is read; the
// lane's action is the entry of a uint8 table at the key of the observation the lane is about to leave, decoded by HotFn
// from the state word the thread holds in a register anyway (bsx_policy.h has the key and the selection rule).  A shared
// table sits in LDS next to the family's own tables; a population of tables (and a table too large for LDS) is read from
// global memory, one byte per lane-step, L2-resident.  epsilon is uniform per launch: epsilon == 0 executes no Philox.
// The chosen actions are an output column like the others: [T,B], non-temporal.  Everything else — Fam::stage once, LAST /
// FIRST counted per thread and pooled once, the output policies of a rollout — is the index rollout's.
template <class Fam, class HotFn>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_policy_rollout_kernel(const typename Fam::args a, const int n_steps,
                                                                             int32_t* __restrict__ rows, const HotFn fn,
                                                                             const bsx_policy_args p) {
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  __shared__ uint8_t s_tab[BSX_POLICY_LDS_BYTES];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  const int S = p.n_states;
  const bool in_lds = p.in_lds != 0;                                      // uniform
  if (in_lds) {
    for (int k = threadIdx.x; k < S; k += BSX_BLOCK) s_tab[k] = p.table[k];
  }
  __syncthreads();
  const int64_t B = a.ctl.n_lanes;
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  const bool mine = i < B;
  const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a.ctl);
  const bool explore = p.epsilon > 0.0;                                   // uniform
  int32_t st = mine ? a.state[i] : 0;
  // the lane's own table (a population: its row, clamped — a bad index cannot fault)
  const uint8_t* __restrict__ tab = p.table;
  if (mine && p.policy_index != nullptr) tab += (int64_t)bsx_policy_clamp(p.policy_index[i], p.n_policies) * S;
  uint32_t n_last = 0, n_first = 0;
  uint32_t block_id = blockIdx.x;                                         // (in a vector register: see bsx_index_rollout_kernel)
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(block_id));
#endif
  if (mine) {
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const uint64_t step = step0 + (uint64_t)t;
      const int64_t oi = (int64_t)t * B + i;
      const int key = bsx_policy_clamp(fn.policy_key(st), S);
      // (two loads in two branches, kept apart by the empty asm: merged into one load through a generic pointer the lookup
      // would be a flat_load, which counts against vmcnt as well — the wait for it would drain the step's stores every step)
      uint32_t entry;
      if (in_lds) {
        entry = s_tab[key];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(entry));
#endif
      } else {
        entry = tab[key];
      }
      uint32_t w0 = 0, w1 = 0, w2 = 0;
      if (explore) {
        const bsx_u32x4 w = bsx_policy_draws(p.explore_seed, lane, step);
        w0 = w.v[0]; w1 = w.v[1]; w2 = w.v[2];
      }
      const int act = bsx_policy_select(entry, Fam::resets(st), p.epsilon, w0, w1, w2, p.num_actions);
      int32_t nst; double reward;
      const int type = Fam::template advance<true>(a, s_fam, i, lane, step, st, act, nst, reward);
      st = nst;
      bsx_emit_at<0, 0, false, -1, BSX_OUT_SCALARS.rollout>(a.ctl, a.out, i, oi, lane, step, type, reward);
      bsx_index_store<BSX_OUT_INDEX.rollout>(rows, oi, nst, fn);
      bsx_st<BSX_OUT_SCALARS.rollout>(&p.actions_out[oi], (int32_t)act);
      n_last += type == BSX_LAST ? 1u : 0u;
      n_first += type == BSX_FIRST ? 1u : 0u;
    }
    a.state[i] = st;
  }
  bsx_pool_counts(a.ctl, n_last, n_first, s_cnt, block_id & (BSX_COUNTER_SHARDS - 1));
}

// evaluate_policy(T): the closed loop of bsx_policy_rollout_kernel — same key, table, draws, selection and advance, in the
// same order — with every per-step store removed.  The lane's state word, its three f64 sums and its episode count stay
// in registers for the whole call (bsx_eval_accumulate, bsx_policy.h); what the advance would add to the bsuite_info
// columns is counted in registers too (Fam::advance_deferred).  After the loop the thread stores the state word, the
// three outputs and the info columns' deltas: B * ~28 bytes per call instead of T * B * ~20, no store and no barrier
// inside the step loop.  The body of bsx_tab_eval_kernel (misc.hip), which picks the family per launch.
template <class Fam, class HotFn>
__device__ __forceinline__ void bsx_tab_eval_body(const typename Fam::args& a, const int n_steps, const HotFn& fn,
                                                  const bsx_policy_args& p, const bsx_policy_eval_t& out,
                                                  typename Fam::shared& s_fam, unsigned int* s_cnt, uint8_t* s_tab) {
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  const int S = p.n_states;
  const bool in_lds = p.in_lds != 0;                                      // uniform
  if (in_lds) {
    for (int k = threadIdx.x; k < S; k += BSX_BLOCK) s_tab[k] = p.table[k];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  const bool mine = i < a.ctl.n_lanes;
  const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a.ctl);
  const bool explore = p.epsilon > 0.0;                                   // uniform
  uint32_t n_last = 0, n_first = 0;
  if (mine) {
    int32_t st = a.state[i];
    const uint8_t* __restrict__ tab = p.table;
    if (p.policy_index != nullptr) tab += (int64_t)bsx_policy_clamp(p.policy_index[i], p.n_policies) * S;
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
    typename Fam::deferred pend = {};
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const uint64_t step = step0 + (uint64_t)t;
      const int key = bsx_policy_clamp(fn.policy_key(st), S);
      uint32_t entry;                    // (two loads kept apart, as in the rollout kernel: merged, the lookup is a flat_load)
      if (in_lds) {
        entry = s_tab[key];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(entry));
#endif
      } else {
        entry = tab[key];
      }
      uint32_t w0 = 0, w1 = 0, w2 = 0;
      if (explore) {
        const bsx_u32x4 w = bsx_policy_draws(p.explore_seed, lane, step);
        w0 = w.v[0]; w1 = w.v[1]; w2 = w.v[2];
      }
      const int act = bsx_policy_select(entry, Fam::resets(st), p.epsilon, w0, w1, w2, p.num_actions);
      int32_t nst; double reward;
      const int type = Fam::advance_deferred(a, s_fam, i, lane, step, st, act, nst, reward, pend);
      st = nst;
      bsx_eval_accumulate(&e, type, reward);
      n_first += type == BSX_FIRST ? 1u : 0u;
    }
    n_last = (uint32_t)e.n;
    a.state[i] = st;
    out.episodes[i] = e.n;
    out.return_sum[i] = e.total;
    out.episode_return_sum[i] = e.done;
    Fam::commit_deferred(a, i, pend);
  }
  bsx_pool_counts(a.ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// Observation stream kernel: a pure store stream over the whole [B x cells] observation array,
// decoupled from the lane-advance kernel.  Block b writes the K*4 KiB run of floats
// [b*K*1024, (b+1)*K*1024): K lane-interleaved 16-byte stores per thread, blocks in address order,
// no loop — the shape of the fastest fill kernels measured on MI355X (profiles/r01/
// store_calibration*.log).  The hot cells are recomputed from the packed state column the advance
// kernel has just written (4 B per lane, L2-resident).
//
// Index math: the block's first float F0 = b*K*1024 is split once per block into (lane, offset)
// with an exact 64-bit magic division on the scalar unit; per-thread offsets stay < 2^14 so a
// 32-bit magic division is exact.

template <class HotFn>
struct bsx_stream_seg {            // one segment's arguments of the observation stream kernel
  float* obs;
  const int32_t* state;
  int64_t n_lanes;
  uint32_t cells;
  uint32_t cells_magic;
  bsx_div64 dv;
  HotFn fn;
};

// NT: non-temporal stores.  Stand-alone they cost the stream 8-10 % (deep_sea 586 -> 636-652 us per step, catch 41.0 -> 42.5:
// r01, and again profiles/r06/ab_nontemporal_stores.log); inside the sweep's mixed stream they are what keeps everything ELSE —
// the state columns the stream itself reads, the small families' columns, actions and tables — in cache while 842 MB of
// observations pass: closed-loop sweep step 161-162.5 -> 157-161.5 us, open-loop 157-158 -> 150-151.6 (pair_mixed.h).
template <class HotFn, int K, int BS, bool NT = false>
__device__ __forceinline__ void bsx_hot_stream_body(float* __restrict__ obs,
                                                    const int32_t* __restrict__ state,
                                                    int64_t n_lanes, uint32_t cells,
                                                    uint32_t cells_magic, bsx_div64 dv,
                                                    const HotFn& fn, uint32_t block_id, int wave_contig = 1) {
  const uint64_t total = (uint64_t)n_lanes * cells;                      // floats in the array
  const uint64_t F0 = (uint64_t)block_id * (uint64_t)(K * 4 * BS);
  const uint64_t lane_b = __umul64hi(F0, dv.m) >> dv.s;                  // uniform
  const uint32_t r_b = (uint32_t)(F0 - lane_b * cells);                  // < cells
  const bool aligned = (cells & 3u) == 0;
  bsx_f4* __restrict__ o4 = reinterpret_cast<bsx_f4*>(obs + F0);
  const int32_t* __restrict__ st = state + lane_b;
  const uint64_t lanes_left = (uint64_t)n_lanes - lane_b;                // lanes at or after lane_b

  uint32_t dl[K];
  int r0[K];
  int32_t s0[K], s1[K];
  bool live[K];
  // (Measured in round 4, profiles/r04/ab_stream_without_state_loads.log / ab_stream_occupancy_pace.log: WITHOUT these loads
  // the stream is 9 % slower; with fewer than 8 resident workgroups per CU it is slower at every step (7: +5 %, 4: +26 %);
  // s_sleep pacing between the loads and the stores never helps.)
  // (One state load per WAVE — lane j fetches row (first row of the wave) + j — handed to the chunks through
  // ds_bpermute instead of one mostly redundant load per chunk: 7 % slower, deep_sea 593 -> 636 us; the K stores then
  // all hang on one load + a cross-lane hop.  profiles/r03/ab_stream_wave_state_load.log)
#pragma unroll
  for (int u = 0; u < K; ++u) {
    // chunk within the block: each wave owns K consecutive KiB (store u of wave w covers KiB
    // w*K + u) — measured +3 % on deep_sea over the block-interleaved order u*BS + tid
    // (profiles/r01/ab_stream_wave_contig.log)
    const uint32_t c = wave_contig ? ((threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63))
                                   : (threadIdx.x + u * BS);
    const uint32_t f = r_b + (c << 2);                                   // float offset from lane_b's row start
    dl[u] = __umulhi(f, cells_magic);
    r0[u] = (int)(f - dl[u] * cells);
    live[u] = F0 + ((uint64_t)c << 2) + 3 < total;
    s0[u] = live[u] ? st[dl[u]] : 0;
    s1[u] = (live[u] && !aligned && (uint64_t)dl[u] + 1 < lanes_left) ? st[dl[u] + 1] : 0;
  }
#pragma unroll
  for (int u = 0; u < K; ++u) {
    if (!live[u]) continue;
    int ha, hb;
    fn(s0[u], ha, hb);
    const int a0 = ha < 0 ? -1 : ha - r0[u], b0 = hb < 0 ? -1 : hb - r0[u];
    bsx_f4 v;
    v.x = (a0 == 0 || b0 == 0) ? 1.0f : 0.0f;
    v.y = (a0 == 1 || b0 == 1) ? 1.0f : 0.0f;
    v.z = (a0 == 2 || b0 == 2) ? 1.0f : 0.0f;
    v.w = (a0 == 3 || b0 == 3) ? 1.0f : 0.0f;
    const int over = (int)cells - r0[u];
    if (!aligned && over < 4) {             // elements j >= over belong to the next lane's row
      int na, nb;
      fn(s1[u], na, nb);
      const int a1 = na < 0 ? -1 : na + over, b1 = nb < 0 ? -1 : nb + over;
      if (over <= 1) v.y = (a1 == 1 || b1 == 1) ? 1.0f : 0.0f;
      if (over <= 2) v.z = (a1 == 2 || b1 == 2) ? 1.0f : 0.0f;
      v.w = (a1 == 3 || b1 == 3) ? 1.0f : 0.0f;
    }
    {
      bsx_f4* dst = &o4[wave_contig ? ((threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63)) : (threadIdx.x + u * BS)];
      if (NT) __builtin_nontemporal_store(v, dst);
      else *dst = v;
    }
  }
  // ragged tail (< 4 floats) of an odd-sized array: the block that contains the array's end
  const uint64_t tail0 = total & ~3ull;
  if (tail0 != total && tail0 >= F0 && tail0 < F0 + (uint64_t)(K * 4 * BS) && threadIdx.x < 3) {
    const uint64_t F = tail0 + threadIdx.x;
    if (F < total) {
      const uint32_t f = r_b + (uint32_t)(F - F0);
      const uint32_t d = __umulhi(f, cells_magic);
      const int r = (int)(f - d * cells);
      int ha, hb;
      fn(st[d], ha, hb);
      obs[F] = (ha == r || hb == r) ? 1.0f : 0.0f;
    }
  }
}

template <class HotFn, int K, int BS>
__global__ void __launch_bounds__(BS) bsx_hot_stream_kernel(float* __restrict__ obs,
                                                                   const int32_t* __restrict__ state,
                                                                   int64_t n_lanes, uint32_t cells,
                                                                   uint32_t cells_magic, bsx_div64 dv,
                                                                   HotFn fn, int wave_contig) {
  bsx_hot_stream_body<HotFn, K, BS>(obs, state, n_lanes, cells, cells_magic, dv, fn, blockIdx.x, wave_contig);
}

// ---------------------------------------------------------------------------------------------
// Small batches (a rank's share of a strong-scaled batch: 2^20 / 8 lanes of catch are 26 MB of boards): ONE
// launch per step.  A workgroup advances its 256 lanes, leaves their new packed states in LDS, and after one
// barrier streams exactly those 256 boards — [256 x cells] floats, contiguous in HBM — as 16-byte chunks with the
// hot cells decoded from LDS.  At 2^20 lanes the decoupled pair wins (no store waits behind a barrier: the
// barrier'd single-kernel designs lost 15-35 % there); when the whole step is a few microseconds
// the second launch and the state column's round trip through L2 are what is left to remove.
// POLICY: the chunk stores' cache policy (bsx_st).  The fused rollout's tiles are non-temporal (catch at 2^17 lanes: 7.2 -> 5.5
// us per step; 2^18 / 2^19 equal / -4 %).  The 64-lane tiles of an EAGER step of a small batch (up to 2^18 lanes) are
// write-through: catch at 2^17 lanes 7.96 -> 6.32 us per step (non-temporal: 6.77), at 2^18 12.5 -> 10.9 (11.8), and the closed
// loop with a device-side policy reading the boards 37.4 -> 35-36 / 46.2 -> 44.7 us (non-temporal: 48.1, WORSE than plain).
// The 256-lane tiles of an eager step (2^19 lanes) are write-through too: 19.4 -> 18.6 us, closed loop 78.9 -> 77.7 (non-temporal:
// 23.3).  (profiles/r06/ab_nt_wide_rows_and_small_batches.log, ab_eager_output_policy.log, ab_catch_tile256_write_through.log)
template <class HotFn, int POLICY = BSX_ST_PLAIN>
__device__ __forceinline__ void bsx_tile_stream(float* __restrict__ tile, const int32_t* s_state, int lanes_here,
                                                uint32_t cells, uint32_t cells_magic, const HotFn& fn) {
  const uint32_t total = (uint32_t)lanes_here * cells;                  // <= 256 * 4096 floats
  const uint32_t n_chunks = total >> 2;
  const bool aligned = (cells & 3u) == 0;
  bsx_f4* __restrict__ t4 = reinterpret_cast<bsx_f4*>(tile);
  for (uint32_t c = threadIdx.x; c < n_chunks; c += BSX_BLOCK) {
    const uint32_t f = c << 2;
    const uint32_t dl = bsx_div_cells(f, cells, cells_magic);
    const int r0 = (int)(f - dl * cells);
    int ha, hb;
    fn(s_state[dl], ha, hb);
    const int a0 = ha < 0 ? -1 : ha - r0, b0 = hb < 0 ? -1 : hb - r0;
    bsx_f4 v;
    v.x = (a0 == 0 || b0 == 0) ? 1.0f : 0.0f;
    v.y = (a0 == 1 || b0 == 1) ? 1.0f : 0.0f;
    v.z = (a0 == 2 || b0 == 2) ? 1.0f : 0.0f;
    v.w = (a0 == 3 || b0 == 3) ? 1.0f : 0.0f;
    const int over = (int)cells - r0;
    if (!aligned && over < 4) {               // elements j >= over belong to the next lane's row (dl + 1 < lanes_here
      int na, nb;                             // because the chunk lies inside the tile)
      fn(s_state[dl + 1], na, nb);
      const int a1 = na < 0 ? -1 : na + over, b1 = nb < 0 ? -1 : nb + over;
      if (over <= 1) v.y = (a1 == 1 || b1 == 1) ? 1.0f : 0.0f;
      if (over <= 2) v.z = (a1 == 2 || b1 == 2) ? 1.0f : 0.0f;
      v.w = (a1 == 3 || b1 == 3) ? 1.0f : 0.0f;
    }
    bsx_st<POLICY>(&t4[c], v);
  }
  // ragged tail (< 4 floats): only the last, partial workgroup of an odd-sized array can have one
  const uint32_t f = (n_chunks << 2) + threadIdx.x;
  if (threadIdx.x < 3 && f < total) {
    const uint32_t dl = bsx_div_cells(f, cells, cells_magic);
    const int r = (int)(f - dl * cells);
    int ha, hb;
    fn(s_state[dl], ha, hb);
    tile[f] = (ha == r || hb == r) ? 1.0f : 0.0f;
  }
}

template <class Fam, bool LEAN, class HotFn>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_fused_tile_kernel(const typename Fam::args a, float* __restrict__ obs,
                                                                   const uint32_t cells, const uint32_t cells_magic,
                                                                   const HotFn fn) {
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  __shared__ int32_t s_state[BSX_BLOCK];
  bsx_advance_body<Fam, LEAN>(a, blockIdx.x, s_fam, s_cnt, s_state);    // ends with a barrier: s_state is complete
  const int64_t lane0 = (int64_t)blockIdx.x * BSX_BLOCK;
  const int64_t left = a.ctl.n_lanes - lane0;
  bsx_tile_stream<HotFn, BSX_ST_WT>(obs + lane0 * (int64_t)cells, s_state, left < BSX_BLOCK ? (int)left : BSX_BLOCK, cells, cells_magic, fn);
}

// ... with 64-lane tiles: wave 0 advances the workgroup's 64 lanes, all four waves stream their [64 x cells] boards.  A
// rank's share of a strong-scaled batch (2^17 lanes of catch) is 512 workgroups of the 256-lane kernel — two per CU,
// every wave a chain of {loads, advance, barrier, 13 chunk stores}; 64-lane tiles make it 2048 workgroups (8 per CU)
// whose threads each write 3 chunks.
template <class Fam, bool LEAN, class HotFn>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_fused_tile64_kernel(const typename Fam::args a, float* __restrict__ obs,
                                                                     const uint32_t cells, const uint32_t cells_magic,
                                                                     const HotFn fn) {
  __shared__ typename Fam::shared s_fam;
  __shared__ int32_t s_state[BSX_WAVE];
  Fam::stage(a, s_fam);
  __syncthreads();
  const int64_t lane0 = (int64_t)blockIdx.x * BSX_WAVE;
  const int64_t i = lane0 + threadIdx.x;
  int type = -1;
  if (threadIdx.x < BSX_WAVE && i < a.ctl.n_lanes) {
    const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
    const uint64_t step = bsx_step_of(a.ctl);
    int32_t nst; double reward;
    const int act = a.ctl.force_reset ? 0 : bsx_action(a.ctl, a.action, i, step);
    const int32_t st = a.ctl.state_in != nullptr ? a.ctl.state_in[i] : a.state[i];
    type = Fam::template advance<LEAN>(a, s_fam, i, lane, step, st, act, nst, reward);
    a.state[i] = nst;
    s_state[threadIdx.x] = nst;
    if (LEAN) bsx_emit_at<0, 0, false>(a.ctl, a.out, i, i, lane, step, type, reward);
    else bsx_emit(a.ctl, a.out, i, lane, step, type, reward);
  }
  if (threadIdx.x < BSX_WAVE && a.ctl.counters != nullptr) {               // one wave: its ballots ARE the workgroup's counts
    const unsigned long long last = __ballot(type == BSX_LAST), first = __ballot(type == BSX_FIRST);
    if (threadIdx.x == 0 && (last | first) != 0ull) {
      unsigned long long* shard = (unsigned long long*)a.ctl.counters + (size_t)(blockIdx.x & (BSX_COUNTER_SHARDS - 1)) * BSX_COUNTER_STRIDE;
      if (last) atomicAdd(&shard[0], (unsigned long long)__popcll(last));
      if (first) atomicAdd(&shard[1], (unsigned long long)__popcll(first));
    }
  }
  __syncthreads();
  const int64_t left = a.ctl.n_lanes - lane0;
  bsx_tile_stream<HotFn, BSX_ST_WT>(obs + lane0 * (int64_t)cells, s_state, left < BSX_WAVE ? (int)left : BSX_WAVE, cells, cells_magic, fn);
}

// The same for a rollout of T steps: ONE launch.  Lanes never interact, so a workgroup can take its 256 lanes
// through all T steps on its own — packed state in a register, actions prefetched one step ahead, per step one
// barrier (the LDS state tile is double-buffered) and the [256 x cells] tile of slice t streamed while the next
// step's advance is already under way in the faster waves.  No launch boundary, no state round trip.
template <class Fam, bool LEAN, class HotFn>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_fused_rollout_kernel(const typename Fam::args a, const int n_steps,
                                                                      float* __restrict__ obs, const uint32_t cells,
                                                                      const uint32_t cells_magic, const HotFn fn) {
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  __shared__ int32_t s_state[2][BSX_BLOCK];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  __syncthreads();
  const int64_t B = a.ctl.n_lanes;
  const int64_t lane0 = (int64_t)blockIdx.x * BSX_BLOCK;
  const int64_t i = lane0 + threadIdx.x;
  const bool mine = i < B;
  const int lanes_here = B - lane0 < BSX_BLOCK ? (int)(B - lane0) : BSX_BLOCK;
  const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a.ctl);
  int32_t st = mine ? a.state[i] : 0;
  int act_next = mine ? a.action[i] : 0;
#pragma unroll 1
  for (int t = 0; t < n_steps; ++t) {
    int type = -1;
    const int act = act_next;
    if (mine) {
      if (t + 1 < n_steps) act_next = a.action[(int64_t)(t + 1) * B + i];
      int32_t nst; double reward;
      type = Fam::template advance<LEAN>(a, s_fam, i, lane, step0 + (uint64_t)t, st, act, nst, reward);
      st = nst;
      s_state[t & 1][threadIdx.x] = nst;
      if (LEAN) bsx_emit_at<0, 0, false>(a.ctl, a.out, i, (int64_t)t * B + i, lane, step0 + (uint64_t)t, type, reward);
      else bsx_emit_at(a.ctl, a.out, i, (int64_t)t * B + i, lane, step0 + (uint64_t)t, type, reward);
    }
    bsx_count_types(a.ctl, type, s_cnt);
    // one barrier per step: tile t is read from s_state[t & 1] after it; step t+1 writes the other buffer, and no
    // thread reaches step t+2 (which rewrites this one) before every thread has passed the barrier of step t+1
    __syncthreads();
    bsx_tile_stream<HotFn, BSX_ST_NT>(obs + ((int64_t)t * B + lane0) * (int64_t)cells, s_state[t & 1], lanes_here, cells, cells_magic, fn);
  }
  if (mine) a.state[i] = st;
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, blockIdx.x);
}

// Software-pipelined rollout step of a two-kernel family: ONE launch runs the observation stream of
// step t beside the lane advance of step t+1.  Nothing inside the launch depends on anything else inside
// it — both halves read the packed state column W(t) that the previous launch wrote, the advance writes
// the OTHER column (bsx_call_t.state_alt) — so, unlike a fused {advance, stream} of the same step
// (profiles/r02/ab_step1_fused_single_launch.log), no workgroup ever waits for another.  The first
// adv_blocks of the workgroups advance lanes (bsx_pipe_role_of); the rest are the store stream.
template <class Fam, bool LEAN, class HotFn, int K>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_pipelined_kernel(const typename Fam::args a, const uint32_t adv_blocks,
                                                                  const uint32_t place,
                                                                  float* __restrict__ obs, const int32_t* __restrict__ hot_state,
                                                                  uint32_t cells, uint32_t cells_magic, bsx_div64 dv, HotFn fn) {
  __shared__ typename Fam::shared s_fam;
  __shared__ unsigned int s_cnt[2];
  const bsx_pipe_role r = bsx_pipe_role_of(blockIdx.x, gridDim.x, adv_blocks, place);   // uniform per workgroup
  if (r.adv) bsx_advance_body<Fam, LEAN>(a, r.index, s_fam, s_cnt);
  else bsx_hot_stream_body<HotFn, K, BSX_BLOCK>(obs, hot_state, a.ctl.n_lanes, cells, cells_magic, dv, fn, r.index);
}

template <class HotFn, int K>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_hot_stream_group_kernel(
    const bsx_stream_seg<HotFn>* __restrict__ table, const bsx_group_index gi) {
  const bsx_group_slot w = bsx_group_find(gi, (int)blockIdx.x);
  const bsx_stream_seg<HotFn>& g = table[w.seg];
  bsx_hot_stream_body<HotFn, K, BSX_BLOCK>(g.obs, g.state, g.n_lanes, g.cells, g.cells_magic, g.dv, g.fn, w.block);
}

// Delta observation mode (bsx_call_t.obs_paint): the observation array persists between calls and
// already shows the hot cells of the packed state recorded in `paint`; the thread that advances a
// lane also clears the cells that went stale and sets the new ones — at most 4 scattered 4-byte
// stores per lane instead of the whole board, in the same launch as the advance.  The array
// afterwards is bit-identical to the dense mode's.
template <class HotFn>
__device__ __forceinline__ void bsx_patch_board(float* __restrict__ board, int32_t was, int32_t now, const HotFn& fn) {
  if (now == was) return;
  int a0 = -1, b0 = -1, a1, b1;
  if (was != -1) fn(was, a0, b0);
  fn(now, a1, b1);
  if (a0 >= 0 && a0 != a1 && a0 != b1) board[a0] = 0.0f;
  if (b0 >= 0 && b0 != a1 && b0 != b1) board[b0] = 0.0f;
  if (a1 >= 0 && a1 != a0 && a1 != b0) board[a1] = 1.0f;
  if (b1 >= 0 && b1 != a0 && b1 != b0) board[b1] = 1.0f;
}

// The body of bsx_pair_advance_delta_kernel (misc.hip), which serves both families: one lane per thread, the workgroup's
// staging in `s_fam`.
template <class Fam, class HotFn>
__device__ __forceinline__ void bsx_advance_delta_body(const typename Fam::args& a, const HotFn& fn, int32_t* __restrict__ paint,
                                                       const uint32_t cells, typename Fam::shared& s_fam, unsigned int* s_cnt) {
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  int type = -1;
  if (i < a.ctl.n_lanes) {
    const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
    const uint64_t step = bsx_step_of(a.ctl);
    int32_t nst; double reward;
    const int act = a.ctl.force_reset ? 0 : bsx_action(a.ctl, a.action, i, step);
    const int32_t was = paint[i];
    type = Fam::template advance<false>(a, s_fam, i, lane, step, a.state[i], act, nst, reward);
    a.state[i] = nst;
    bsx_patch_board(a.out.observation + i * (int64_t)cells, was, nst, fn);
    paint[i] = nst;
    bsx_emit(a.ctl, a.out, i, lane, step, type, reward);
  }
  bsx_count_types(a.ctl, type, s_cnt);
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, blockIdx.x);
}

// Degenerate boards (cells < 4: a 16-byte chunk spans several lanes): one float per thread — the body of
// bsx_hot_cells_kernel (misc.hip), which serves both families.
template <class HotFn>
__device__ __forceinline__ void bsx_hot_cells_body(float* __restrict__ obs, const int32_t* __restrict__ state, int64_t n_lanes,
                                                   uint32_t cells, const HotFn& fn) {
  const uint64_t F = (uint64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (F >= (uint64_t)n_lanes * cells) return;
  const uint64_t lane = F / cells;
  const int r = (int)(F - lane * cells);
  int ha, hb;
  fn(state[lane], ha, hb);
  obs[F] = (ha == r || hb == r) ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// Narrow observation stream (bsx_call_t.flags & BSX_CALL_OBS_MASK): the same flat run of 16-byte chunks as
// bsx_hot_stream_body, but a chunk holds N = 16 / E elements of E bytes (uint8: E = 1; float16 / bfloat16: E = 2).
// A chunk starts as four zero dwords and receives the element's "one" bit pattern (`one`: 0x01, 0x3C00 or 0x3F80) at
// the at most four positions the hot cells of its lanes fall on — two lanes once a row has at least N cells; a
// lane without hot cell (deep_sea's all-zero terminal board: -1) contributes nothing.  Every whole chunk is ONE
// 16-byte store: element stores cost many times more per byte (sub-dword stores of the MI355X).
//
// The array [n_lanes x cells] starts at `obs` (any E-aligned address: slice t of a rollout lies t*B*cells*E bytes
// into the buffer): `head` elements up to the first 16-byte boundary, then n_chunks whole chunks, then a tail of
// fewer than N elements.  Workgroup 0 writes head and tail with element stores.  Boards of fewer than N cells
// (deep_sea N <= 3, catch below 16 / 8 cells) put several lanes into one chunk and take a slow loop over them.
template <int E>
struct bsx_narrow_chunk {                 // the 16 bytes of one chunk as two 64-bit halves
  uint64_t lo = 0, hi = 0;
  // sets element p (no-op unless 0 <= p < 16 / E)
  __device__ __forceinline__ void put(int p, uint32_t one) {
    if ((unsigned)p >= (unsigned)(16 / E)) return;
    const uint32_t bit = (uint32_t)p * (8u * E);
    const uint64_t v = (uint64_t)one << (bit & 63u);
    if (bit < 64u) lo |= v; else hi |= v;
  }
};

template <class HotFn, int E, int K>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_narrow_stream_kernel(uint8_t* __restrict__ obs,
                                                                      const int32_t* __restrict__ state,
                                                                      int64_t n_lanes, uint32_t cells,
                                                                      uint32_t cells_magic, bsx_div64 dv,
                                                                      uint32_t head, uint64_t n_chunks,
                                                                      uint32_t one, HotFn fn) {
  constexpr int N = 16 / E;
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const uint64_t total = (uint64_t)n_lanes * cells;
  if (blockIdx.x == 0 && threadIdx.x < 2 * N) {        // ragged head (threads 0..N-1) and tail (N..2N-1)
    const uint64_t e = threadIdx.x < N ? (uint64_t)threadIdx.x : head + n_chunks * N + (threadIdx.x - N);
    if (threadIdx.x < N ? e < head : e < total) {
      const uint64_t l = e / cells;
      const int r = (int)(e - l * cells);
      int ha, hb;
      fn(state[l], ha, hb);
      const uint32_t v = (ha == r || hb == r) ? one : 0u;
      if constexpr (E == 1) obs[e] = (uint8_t)v;
      else reinterpret_cast<uint16_t*>(obs)[e] = (uint16_t)v;
    }
  }
  const uint64_t c_b = (uint64_t)blockIdx.x * (K * BSX_BLOCK);          // the workgroup's first chunk
  u4* __restrict__ o4 = reinterpret_cast<u4*>(obs + (uint64_t)head * E) + c_b;
  if (cells < (uint32_t)N) {                                            // several lanes per chunk: the slow path
#pragma unroll 1
    for (int u = 0; u < K; ++u) {
      const uint32_t c = (threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63);
      if (c_b + c >= n_chunks) continue;
      const uint64_t e0 = head + (c_b + c) * N;
      uint64_t l = e0 / cells;
      int base = -(int)(e0 - l * cells);                                // chunk position of lane l's cell 0
      bsx_narrow_chunk<E> v;
      for (; base < N && l < (uint64_t)n_lanes; base += (int)cells, ++l) {
        int ha, hb;
        fn(state[l], ha, hb);
        v.put(ha < 0 ? -1 : base + ha, one);
        v.put(hb < 0 ? -1 : base + hb, one);
      }
      u4 w;
      w.x = (uint32_t)v.lo; w.y = (uint32_t)(v.lo >> 32); w.z = (uint32_t)v.hi; w.w = (uint32_t)(v.hi >> 32);
      o4[c] = w;
    }
    return;
  }
  // rows of at least N cells: a chunk touches lane dl and, when it runs over the row's end, lane dl + 1
  const uint64_t E0 = head + c_b * N;                                   // the workgroup's first element (uniform)
  const uint64_t lane_b = __umul64hi(E0, dv.m) >> dv.s;
  const uint32_t r_b = (uint32_t)(E0 - lane_b * cells);
  const int32_t* __restrict__ st = state + lane_b;
  const uint64_t lanes_left = (uint64_t)n_lanes - lane_b;
  uint32_t dl[K];
  int r0[K];
  int32_t s0[K], s1[K];
  bool live[K];
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const uint32_t c = (threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63);
    const uint32_t f = r_b + c * N;                                     // < 2^20: the 32-bit magic is exact
    dl[u] = __umulhi(f, cells_magic);
    r0[u] = (int)(f - dl[u] * cells);
    live[u] = c_b + c < n_chunks;
    s0[u] = live[u] ? st[dl[u]] : 0;
    s1[u] = (live[u] && (int)cells - r0[u] < N && (uint64_t)dl[u] + 1 < lanes_left) ? st[dl[u] + 1] : 0;
  }
#pragma unroll
  for (int u = 0; u < K; ++u) {
    if (!live[u]) continue;
    bsx_narrow_chunk<E> v;
    int ha, hb;
    fn(s0[u], ha, hb);
    v.put(ha < 0 ? -1 : ha - r0[u], one);
    v.put(hb < 0 ? -1 : hb - r0[u], one);
    const int over = (int)cells - r0[u];                                // elements >= over belong to lane dl + 1
    if (over < N) {
      fn(s1[u], ha, hb);
      v.put(ha < 0 ? -1 : ha + over, one);
      v.put(hb < 0 ? -1 : hb + over, one);
    }
    u4 w;
    w.x = (uint32_t)v.lo; w.y = (uint32_t)(v.lo >> 32); w.z = (uint32_t)v.hi; w.w = (uint32_t)(v.hi >> 32);
    o4[(threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63)] = w;
  }
}
#endif  // BSX_PAIR_DEVICE_H_
