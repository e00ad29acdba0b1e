// bsx_tab_sample_device.h — bsx_<family>_policy_sample / bsx_<family>_policy_sample_evaluate (sample_policy,
// evaluate_sampled_policy): the arguments of the ONE kernel that serves deep_sea and catch, recording or returns only
// (bsx_tab_softmax_kernel, tab_sample.hip), the two bodies of its step loop, its launcher and the checks the four entry points
// share.  The closed loops of bsx_policy_rollout_kernel and bsx_tab_eval_body (bsx_pair_device.h) with another action SOURCE:
// instead of a uint8 table entry (and an epsilon coin) the lane takes a draw from softmax(logits[row, key] / temperature) by
// Gumbel-max (bsx_tab_sample.h).
#ifndef BSX_TAB_SAMPLE_DEVICE_H_
#define BSX_TAB_SAMPLE_DEVICE_H_

#include "bsx_pair_host.h"
#include "bsx_tab_sample.h"
#include "catch_fam.h"
#include "deep_sea_fam.h"

// The table of logits, flattened out of bsx_policy_logits_t on the host.
struct bsx_tab_logits_args {
  const float* logits;           // [n_policies, n_states, A]; 4-byte aligned, no more
  const int32_t* policy_index;   // [n_lanes], nullptr when n_policies == 1
  int32_t* actions_out;          // [n_steps, n_lanes] (the recording call's alone)
  double beta;                   // 1 / temperature: finite, > 0 (the entry points check)
  uint64_t sample_seed;
  int32_t n_states, n_policies;
  int32_t in_lds;                // one shared table of at most BSX_TAB_SAMPLE_LDS_BYTES: every workgroup stages it in LDS
  int32_t _pad;
};

// The family and the kind of call are uniform switches per launch, so the arguments are a tagged struct: `family` says which
// member of `fam` is set, `record` which of `rows` (with fam's TimeStep pointers and p.actions_out) and `out` is written.
struct bsx_tab_softmax_args {
  int32_t family;                // BSX_FAM_DEEP_SEA or BSX_FAM_CATCH
  int32_t n_steps;
  int32_t record;                // 1: sample_policy (TimeStep, index rows, actions); 0: evaluate_sampled_policy (returns only)
  int32_t _pad;
  bsx_tab_logits_args p;
  int32_t* rows;                 // [n_steps, n_lanes, K] index observations (record)
  bsx_policy_eval_t out;         // (returns only)
  union {
    deep_sea_fam::args deep_sea;
    catch_fam::args catch_;
  } fam;
};

// The kernel's arguments where the launch put them — the kernarg segment — through a pointer the optimiser cannot trace: what
// is read through it is loaded where it is used, by s_load, and lives in scalar registers from there to its last use only
// (bsx_linear_view, bsx_linear_score.h, has the measurements).  Read through the by-value parameter, every scalar of the call
// stays live across the step loop, next to the constants of two logarithms per action: 54 scalar registers spilled.
#if defined(__HIP_DEVICE_COMPILE__)
#define BSX_TAB_KERNARG __attribute__((address_space(4)))
#else
#define BSX_TAB_KERNARG          /* (the host pass only parses the device functions) */
#endif
typedef const BSX_TAB_KERNARG bsx_tab_softmax_args* bsx_tab_softmax_kernarg;
__device__ __forceinline__ const bsx_tab_softmax_args& bsx_tab_softmax_view(bsx_tab_softmax_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_tab_softmax_args*)ka;
}
// Which member of `fam` a family's body reads, its decoder and its number of actions.
struct bsx_tab_softmax_deep_sea {
  typedef deep_sea_fam fam;
  typedef deep_sea_hot hot;
  static constexpr int A = 2;
  __device__ static __forceinline__ const fam::args& of(const bsx_tab_softmax_args& k) { return k.fam.deep_sea; }
  __device__ static __forceinline__ hot fn(const fam::args& a) { return hot{a.size}; }
};
struct bsx_tab_softmax_catch {
  typedef catch_fam fam;
  typedef catch_hot hot;
  static constexpr int A = 3;
  __device__ static __forceinline__ const fam::args& of(const bsx_tab_softmax_args& k) { return k.fam.catch_; }
  __device__ static __forceinline__ hot fn(const fam::args& a) { return hot{a.rows, a.columns}; }
};

// A table staged in LDS, typed as such: through a generic pointer the look-up would be a FLAT load (bsx_policy_rollout_kernel
// has what that costs).
typedef const float __attribute__((address_space(3)))* bsx_tab_lds;

// The action of a lane that does not reset: key -> the A logits of the lane's row -> block 0 of stream BSX_STREAM_SAMPLE ->
// bsx_gumbel_select_n.  The two look-ups are two branches, kept apart by the empty asm — typed LDS loads from the staged
// table, typed global loads from the lane's own table (`row_off`: its first float) — and never one load through a generic
// pointer.
template <int A, class HotFn>
__device__ __forceinline__ int bsx_tab_softmax_action(const HotFn& fn, int32_t st, const bsx_tab_logits_args& p, const float* s_tab,
                                                      int64_t row_off, uint64_t lane, uint64_t step) {
  static_assert(A >= BSX_TAB_SAMPLE_MIN_ACTIONS && A <= BSX_TAB_SAMPLE_MAX_ACTIONS, "two or three actions");
  const int key = bsx_policy_clamp(fn.policy_key(st), p.n_states);
  float l[A];
  if (p.in_lds != 0) {                                                    // uniform
    bsx_tab_lds t = (bsx_tab_lds)s_tab + key * A;
#pragma unroll
    for (int c = 0; c < A; ++c) {
      l[c] = t[c];
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+v"(l[c]));
#endif
    }
  } else {
    const float* __restrict__ g = p.logits + (row_off + (int64_t)key * A);
#pragma unroll
    for (int c = 0; c < A; ++c) l[c] = g[c];
  }
  const bsx_u32x4 u = bsx_gumbel_draws(p.sample_seed, lane, step);
  return bsx_gumbel_select_n(l, A, p.beta, u.v);
}

// What both bodies do before their loop: the counters, the family's own staging, the shared table into LDS, one barrier.
template <class Fam, int A>
__device__ __forceinline__ void bsx_tab_softmax_stage(const typename Fam::args& a, const bsx_tab_logits_args& p,
                                                      typename Fam::shared& s_fam, unsigned int* s_cnt, float* s_tab) {
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  if (p.in_lds != 0) {                                                    // uniform; n_states * A <= BSX_TAB_SAMPLE_LDS_BYTES / 4
    const int n = p.n_states * A;
    for (int k = threadIdx.x; k < n; k += BSX_BLOCK) s_tab[k] = p.logits[k];
  }
  __syncthreads();
}

// The first float of lane i's own table (a population: its row, clamped — a bad index cannot fault).
template <int A>
__device__ __forceinline__ int64_t bsx_tab_softmax_row(const bsx_tab_logits_args& p, int64_t i) {
  if (p.policy_index == nullptr) return 0;
  return (int64_t)bsx_policy_clamp(p.policy_index[i], p.n_policies) * ((int64_t)p.n_states * A);
}

// sample_policy(T): the loop of bsx_policy_rollout_kernel.  State word in a register from its load to its store, LAST / FIRST
// counted per thread and pooled once, per step the scalars, the index row and the action stored non-temporally: [T,B] outputs
// have no reader inside the call.  Nothing is looked up and nothing is drawn on a step that resets.  The arguments are read
// through three views: one before the loop, one per step, one after the loop.
template <class F>
__device__ __forceinline__ void bsx_tab_softmax_record_body(bsx_tab_softmax_kernarg ka, typename F::fam::shared& s_fam,
                                                            unsigned int* s_cnt, float* s_tab) {
  typedef typename F::fam Fam;
  constexpr int A = F::A;
  const bsx_tab_softmax_args& k0 = bsx_tab_softmax_view(ka);
  const typename Fam::args& a0 = F::of(k0);
  bsx_tab_softmax_stage<Fam, A>(a0, k0.p, s_fam, s_cnt, s_tab);
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  const bool mine = i < a0.ctl.n_lanes;
  const uint64_t lane = a0.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a0.ctl);
  const int n_steps = k0.n_steps;
  uint32_t n_last = 0, n_first = 0;
  uint32_t block_id = blockIdx.x;                                         // (in a vector register: see bsx_index_rollout_kernel)
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(block_id));
#endif
  if (mine) {
    int32_t st = a0.state[i];
    const int64_t row_off = bsx_tab_softmax_row<A>(k0.p, i);
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_tab_softmax_args& kt = bsx_tab_softmax_view(ka);
      const typename Fam::args& a = F::of(kt);
      const typename F::hot fn = F::fn(a);
      const uint64_t step = step0 + (uint64_t)t;
      const int64_t oi = (int64_t)t * a.ctl.n_lanes + i;
      const bool resets = Fam::resets(st);
      int act = 0;
      if (!resets) act = bsx_tab_softmax_action<A>(fn, st, kt.p, s_tab, row_off, lane, step);
      int32_t nst; double reward;
      const int type = Fam::template advance<true>(a, s_fam, i, lane, step, st, act, nst, reward);
      st = nst;
      bsx_emit_at<0, 0, false, -1, BSX_OUT_SCALARS.rollout>(a.ctl, a.out, i, oi, lane, step, type, reward);
      bsx_index_store<BSX_OUT_INDEX.rollout>(kt.rows, oi, nst, fn);
      bsx_st<BSX_OUT_SCALARS.rollout>(&kt.p.actions_out[oi], (int32_t)act);
      n_last += type == BSX_LAST ? 1u : 0u;
      n_first += type == BSX_FIRST ? 1u : 0u;
    }
    F::of(bsx_tab_softmax_view(ka)).state[i] = st;
  }
  bsx_pool_counts(F::of(bsx_tab_softmax_view(ka)).ctl, n_last, n_first, s_cnt, block_id & (BSX_COUNTER_SHARDS - 1));
}

// evaluate_sampled_policy(T): the loop of bsx_tab_eval_body — the same steps with the same draws, every per-step store
// removed.  State word, the three f64 sums, the episode count and the info columns' deltas stay in registers
// (bsx_eval_accumulate, Fam::advance_deferred) and are stored after the loop: no store and no barrier inside it.
template <class F>
__device__ __forceinline__ void bsx_tab_softmax_returns_body(bsx_tab_softmax_kernarg ka, typename F::fam::shared& s_fam,
                                                             unsigned int* s_cnt, float* s_tab) {
  typedef typename F::fam Fam;
  constexpr int A = F::A;
  const bsx_tab_softmax_args& k0 = bsx_tab_softmax_view(ka);
  const typename Fam::args& a0 = F::of(k0);
  bsx_tab_softmax_stage<Fam, A>(a0, k0.p, s_fam, s_cnt, s_tab);
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  const bool mine = i < a0.ctl.n_lanes;
  const uint64_t lane = a0.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a0.ctl);
  const int n_steps = k0.n_steps;
  uint32_t n_last = 0, n_first = 0;
  if (mine) {
    int32_t st = a0.state[i];
    const int64_t row_off = bsx_tab_softmax_row<A>(k0.p, i);
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
    typename Fam::deferred pend = {};
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_tab_softmax_args& kt = bsx_tab_softmax_view(ka);
      const typename Fam::args& a = F::of(kt);
      const uint64_t step = step0 + (uint64_t)t;
      const bool resets = Fam::resets(st);
      int act = 0;
      if (!resets) act = bsx_tab_softmax_action<A>(F::fn(a), st, kt.p, s_tab, row_off, lane, step);
      int32_t nst; double reward;
      const int type = Fam::advance_deferred(a, s_fam, i, lane, step, st, act, nst, reward, pend);
      st = nst;
      bsx_eval_accumulate(&e, type, reward);
      n_first += type == BSX_FIRST ? 1u : 0u;
    }
    n_last = (uint32_t)e.n;
    const bsx_tab_softmax_args& k1 = bsx_tab_softmax_view(ka);
    const typename Fam::args& a1 = F::of(k1);
    a1.state[i] = st;
    k1.out.episodes[i] = e.n;
    k1.out.return_sum[i] = e.total;
    k1.out.episode_return_sum[i] = e.done;
    Fam::commit_deferred(a1, i, pend);
  }
  bsx_pool_counts(F::of(bsx_tab_softmax_view(ka)).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_tab_softmax_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_tab_softmax(const bsx_tab_softmax_args& a, hipStream_t st);

// The refusals of the four entry points that do not depend on the family: those of bsx_check_policy_call /
// bsx_check_policy_eval_call, in their order, for a bsx_policy_t that stands in for the table of logits (epsilon 0: the
// softmax explores) — and, where they refuse n_states and epsilon, BSX_EINVAL for n_actions other than the family's and
// BSX_ERANGE for an inv_temperature that is not finite or not > 0; after the pointers, BSX_EALIGN for logits off the 4-byte
// grid.
static inline bsx_policy_t bsx_tab_softmax_stand_in(const bsx_policy_logits_t* lg, int32_t n_actions) {
  bsx_policy_t q;
  q.table = reinterpret_cast<const uint8_t*>(lg->logits);
  q.n_states = lg->n_actions == n_actions ? lg->n_states : -1;
  q.n_policies = lg->n_policies;
  q.policy_index = lg->policy_index;
  q.epsilon = (__builtin_isfinite(lg->inv_temperature) && lg->inv_temperature > 0.0) ? 0.0 : 2.0;
  q.explore_seed = lg->sample_seed;
  q.actions_out = lg->actions_out;
  return q;
}
static inline int bsx_check_tab_softmax_call(const bsx_call_t* call, const bsx_policy_logits_t* lg, int32_t n_states, int32_t n_actions,
                                             const int32_t* state, const bsx_timestep_t& out, const double* info) {
  if (call == nullptr || lg == nullptr) return BSX_ENULL;
  const bsx_policy_t q = bsx_tab_softmax_stand_in(lg, n_actions);
  const int rc = bsx_check_policy_call(call, &q, n_states, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  return (reinterpret_cast<uintptr_t>(lg->logits) & 3u) != 0 ? BSX_EALIGN : 0;
}
static inline int bsx_check_tab_softmax_eval_call(const bsx_call_t* call, const bsx_policy_logits_t* lg, int32_t n_states,
                                                  int32_t n_actions, const int32_t* state, const bsx_policy_eval_t& out,
                                                  const double* info) {
  if (call == nullptr || lg == nullptr) return BSX_ENULL;
  const bsx_policy_t q = bsx_tab_softmax_stand_in(lg, n_actions);
  const int rc = bsx_check_policy_eval_call(call, &q, n_states, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  return (reinterpret_cast<uintptr_t>(lg->logits) & 3u) != 0 ? BSX_EALIGN : 0;
}

// What the entry points share once the family's args are in place (a.fam).
static inline int bsx_tab_softmax_call(bsx_tab_softmax_args& a, int32_t family, const bsx_call_t* call, const bsx_policy_logits_t* lg,
                                       bool record, int32_t* rows, const bsx_policy_eval_t& out) {
  if (bsx_blocks_of(call->n_lanes) > 0x7FFFFFFF) return BSX_EINVAL;
  a.family = family;
  a.n_steps = call->n_steps;
  a.record = record ? 1 : 0;
  a._pad = 0;
  a.p.logits = lg->logits;
  a.p.policy_index = lg->n_policies > 1 ? lg->policy_index : nullptr;
  a.p.actions_out = record ? lg->actions_out : nullptr;
  a.p.beta = lg->inv_temperature;
  a.p.sample_seed = lg->sample_seed;
  a.p.n_states = lg->n_states; a.p.n_policies = lg->n_policies;
  a.p.in_lds = (lg->n_policies == 1 && (int64_t)lg->n_states * lg->n_actions * 4 <= BSX_TAB_SAMPLE_LDS_BYTES) ? 1 : 0;
  a.p._pad = 0;
  a.rows = rows;
  a.out = out;
  return bsx_launch_tab_softmax(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_policy_sample / bsx_<family>_policy_sample_evaluate (Fam: the family's host trait, bsx_host.h).
template <class Fam>
static inline int bsx_tab_softmax_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                        int32_t* state, const bsx_timestep_t& out, double* info) {
  bsx_tab_softmax_args s;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, &out, info, Fam::of(s.fam),
      [&] { return bsx_check_tab_softmax_call(call, policy, Fam::states(cfg), Fam::actions, state, out, info); },
      [&] {
        return bsx_tab_softmax_call(s, Fam::code, call, policy, true, reinterpret_cast<int32_t*>(out.observation), bsx_policy_eval_t{});
      });
}
template <class Fam>
static inline int bsx_tab_softmax_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                        int32_t* state, const bsx_policy_eval_t& out, double* info) {
  bsx_tab_softmax_args s;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, nullptr, info, Fam::of(s.fam),
      [&] { return bsx_check_tab_softmax_eval_call(call, policy, Fam::states(cfg), Fam::actions, state, out, info); },
      [&] { return bsx_tab_softmax_call(s, Fam::code, call, policy, false, nullptr, out); });
}

#endif  // BSX_TAB_SAMPLE_DEVICE_H_
