// bsx_linear_score.h — bsx_<family>_linear_evaluate (evaluate_linear): the arguments of the ONE kernel that serves cartpole,
// swing-up and mountain_car (bsx_linear_score_kernel, linear.hip), the body of its step loop, its launcher and the checks
// the two entry points share.  The family is a uniform switch per launch, so the arguments are a tagged struct: `family`
// says which member of `fam` is set (the idiom of bsx_tab_eval.h).
#ifndef BSX_LINEAR_SCORE_H_
#define BSX_LINEAR_SCORE_H_

#include "small_obs.h"                 // (first: it brings the HIP runtime's header, which BSX_HD needs)
#include "bsx_linear.h"
#include "bsx_policy.h"
#include "cartpole_env.h"
#include "mountain_car_env.h"

// The policy side of the call, as the kernel reads it.
struct bsx_linear_args {
  const float* weights;            // [n_policies, 3, D + 1]
  const int32_t* policy_index;     // [n_lanes], or null: every lane takes row 0 (n_policies == 1)
  const float* observation_in;     // [n_lanes, D]
  double epsilon;
  uint64_t explore_seed;
  int32_t n_policies, _pad;
};

struct bsx_linear_score_args {
  int32_t family;                  // BSX_FAM_CARTPOLE (classic or swing-up: fam.cartpole.cfg.swingup) or BSX_FAM_MOUNTAIN_CAR
  int32_t n_steps;
  bsx_linear_args p;
  bsx_linear_eval_t out;
  union {
    cartpole_env::args cartpole;
    mountain_car_env::args mountain_car;
  } fam;
};

// A shared weight matrix in LDS, typed as such (bsx_lds_table: a generic pointer would make every read a FLAT load).
#define BSX_LINEAR_LDS_FLOATS 32     // >= BSX_LINEAR_ROW(BSX_LINEAR_MAX_OBS) = 27

// The kernel's arguments where the launch put them: the kernarg segment (constant memory, read through the scalar cache).
#if defined(__HIP_DEVICE_COMPILE__)
#define BSX_KERNARG __attribute__((address_space(4)))
#else
#define BSX_KERNARG              /* (the host pass only parses the device functions) */
#endif
typedef const BSX_KERNARG bsx_linear_score_args* bsx_linear_kernarg;
// The same arguments through a pointer the optimiser cannot trace (bsx_fresh, for a uniform pointer): what is read through
// it is loaded where it is used, by s_load, and lives in scalar registers from there to its last use only.  Read through the
// by-value parameter, all ~70 scalars of a cartpole call (cfg, derived parameters, column and output pointers, the policy)
// are loaded in the entry block and stay live to their last use — the step loop's parameters through the loop, the output
// pointers across it: 107 scalar registers spilled to vector lanes, a dozen reloads in every step.
__device__ __forceinline__ const bsx_linear_score_args& bsx_linear_view(bsx_linear_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_linear_score_args*)ka;
}
// Which member of `fam` a family's body reads.
struct bsx_linear_cartpole {
  typedef cartpole_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_linear_score_args& k) { return k.fam.cartpole; }
};
struct bsx_linear_mountain_car {
  typedef mountain_car_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_linear_score_args& k) { return k.fam.mountain_car; }
};

// evaluate_linear(T): the lean register loop of small_obs_regs_rollout (small_obs.h) — state in Env::regs, the info columns
// in registers (IREGS), Env::core on the registers, LAST / FIRST counted per thread and pooled once — without its action
// loads and without any of its per-step stores.  The row o[] that core() fills is the next step's input: the action is
// bsx_linear_select(w, o) fed through bsx_policy_select, the ε draws bsx_policy_draws, the sums bsx_eval_accumulate.  After
// the loop the thread stores its state, its info, the three sums, the episode count and the final row.
//   V       the family's variant (Env::numel_of(V) floats per row: cartpole 0 classic / 1 swing-up)
//   SHARED  one matrix for all lanes (n_policies == 1): staged in LDS by the workgroup and read from there every step, so
//           that it costs no vector register across the step; else the lane's own row, loaded once into registers.
// The time-fraction table is read from where core<TAB = false> reads it (cartpole: the device table, mountain_car: the
// division itself) and resets are not pooled (POOL = false): no LDS write and no barrier inside the loop.
// The arguments are read through three views (bsx_linear_view): one before the loop, one per step, one after the loop.
template <class Fam, int V, bool SHARED>
__device__ __forceinline__ void bsx_linear_score_body(bsx_linear_kernarg ka, float* s_w, unsigned int* s_cnt) {
  typedef typename Fam::env Env;
  constexpr int D = Env::numel_of(V), NW = BSX_LINEAR_ROW(D);
  static_assert(D <= BSX_LINEAR_MAX_OBS && NW <= BSX_LINEAR_LDS_FLOATS, "row length");
  const bsx_linear_score_args& k0 = bsx_linear_view(ka);
  const typename Env::args& a0 = Fam::of(k0);
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  if constexpr (SHARED) {
    if (threadIdx.x < NW) s_w[threadIdx.x] = k0.p.weights[threadIdx.x];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  const bool mine = i < a0.ctl.n_lanes;
  const uint64_t lane = a0.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a0.ctl);
  const int n_steps = k0.n_steps;
  uint32_t n_last = 0, n_first = 0;
  if (mine) {
    typename Env::regs rg;
    Env::clear(rg);
    Env::load(a0, i, rg);
    Env::template load_info<V>(a0, i, rg);
    const uint32_t pending_in = Env::reset_pending(rg) ? 1u : 0u;
    // the lane's input row: not read by a lane that resets on the first step (it takes action 0 there)
    float o[8];
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] = pending_in ? 0.0f : k0.p.observation_in[i * D + d];
    float w[NW];
    if constexpr (!SHARED) {
      const float* __restrict__ row = k0.p.weights + (int64_t)bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies) * NW;
#pragma unroll
      for (int k = 0; k < NW; ++k) w[k] = row[k];
    }
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_linear_score_args& kt = bsx_linear_view(ka);
      const typename Env::args& a = Fam::of(kt);
      const bsx_linear_args& p = kt.p;
      const uint64_t step = step0 + (uint64_t)t;
      const int resets = Env::reset_pending(rg) ? 1 : 0;
      if constexpr (SHARED) {
        // (from an offset the compiler cannot trace to the loop's outside: hoisted, the matrix is 12-27 live registers)
        bsx_lds_table tab = (bsx_lds_table)s_w + bsx_fresh(0u);
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = tab[k];
      }
      const int32_t best = bsx_linear_select(w, o, D);
      uint32_t w0 = 0, w1 = 0, w2 = 0;
      if (p.epsilon > 0.0 && !resets) {
        const bsx_u32x4 u = bsx_policy_draws(p.explore_seed, lane, step);
        w0 = u.v[0]; w1 = u.v[1]; w2 = u.v[2];
      }
      const int act = bsx_policy_select((uint32_t)best, resets, p.epsilon, w0, w1, w2, BSX_LINEAR_ACTIONS);
      double reward = 0.0;
      const int type = Env::template core<0, 0, true, false, false, V, true>(a, rg, act, i, lane, step, o, reward);
      bsx_eval_accumulate(&e, type, reward);
    }
    // every LAST is followed by a FIRST except one at the call's final step, and a lane that arrives with its reset
    // pending begins with one (small_obs_regs_rollout)
    n_last = (uint32_t)e.n;
    n_first = n_last + pending_in - (Env::reset_pending(rg) ? 1u : 0u);
    const bsx_linear_score_args& k1 = bsx_linear_view(ka);
    const typename Env::args& a1 = Fam::of(k1);
    Env::store(a1, i, rg);
    Env::template store_info<V>(a1, i, rg);
    k1.out.episodes[i] = e.n;
    k1.out.return_sum[i] = e.total;
    k1.out.episode_return_sum[i] = e.done;
    small_obs_store_row<false>(k1.out.observation_out + i * D, o, D);
  }
  bsx_pool_counts(Fam::of(bsx_linear_view(ka)).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_linear_score_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_linear_score(const bsx_linear_score_args& a, hipStream_t st);

// The refusals of bsx_<family>_linear_evaluate that do not depend on the family, in bsx_<family>_policy_evaluate's order
// (bsx_check_policy_eval_call): modes, scalars, then — for a call with lanes — pointers.  The caller has checked cfg, call
// and linear for null and the cfg's range; `extra` is a pointer only the family needs (cartpole's table) or any non-null.
// `outputs_present`: every output pointer the call writes through is non-null (the evaluation's four; a recording call's
// TimeStep and action column, bsx_trajectory.h).
static inline int bsx_check_linear_call(const bsx_call_t* call, const bsx_linear_t* lin, const float* state, const int32_t* steps,
                                        bool outputs_present, const double* info, const void* extra) {
  if ((call->flags & (BSX_CALL_OBS_MASK | BSX_CALL_OBS_INDEX)) != 0) return BSX_EMODE;       // float32 rows only
  if (call->logging != nullptr || call->wrap.kind != BSX_WRAP_NONE || call->stream.mt_state != nullptr ||
      call->stream.mt_pos != nullptr || call->reward_f64 != nullptr || call->obs_paint != nullptr ||
      call->state_alt != nullptr || call->action_ring > 1 || call->force_reset)
    return BSX_EMODE;
  if (call->n_steps < 1 || call->n_lanes < 0 || call->n_lanes > ((int64_t)1 << 40)) return BSX_EINVAL;
  if (lin->n_policies < 1) return BSX_EINVAL;
  if (!(lin->epsilon >= 0.0 && lin->epsilon <= 1.0)) return BSX_ERANGE;      // (NaN included)
  if (call->n_lanes == 0) return 0;
  if (lin->weights == nullptr || lin->observation_in == nullptr || state == nullptr || steps == nullptr || info == nullptr ||
      extra == nullptr || !outputs_present)
    return BSX_ENULL;
  if (lin->n_policies > 1 && lin->policy_index == nullptr) return BSX_ENULL;
  if (call->action_ring < 0) return BSX_EINVAL;                              // (what bsx_check_call refuses for a rollout)
  if (bsx_blocks_of(call->n_lanes) > 0x7FFFFFFF) return BSX_EINVAL;
  return 0;
}

static inline bool bsx_linear_eval_present(const bsx_linear_eval_t& out) {
  return out.episodes != nullptr && out.return_sum != nullptr && out.episode_return_sum != nullptr && out.observation_out != nullptr;
}
static inline int bsx_check_linear_call(const bsx_call_t* call, const bsx_linear_t* lin, const float* state, const int32_t* steps,
                                        const bsx_linear_eval_t& out, const double* info, const void* extra) {
  return bsx_check_linear_call(call, lin, state, steps, bsx_linear_eval_present(out), info, extra);
}

// What the two entry points share once the family's args are in place.
static inline int bsx_linear_score_call(bsx_linear_score_args& a, int32_t family, const bsx_call_t* call, const bsx_linear_t* lin,
                                        const bsx_linear_eval_t& out) {
  a.family = family;
  a.n_steps = call->n_steps;
  a.p.weights = lin->weights;
  a.p.policy_index = lin->n_policies > 1 ? lin->policy_index : nullptr;
  a.p.observation_in = lin->observation_in;
  a.p.epsilon = lin->epsilon;
  a.p.explore_seed = lin->explore_seed;
  a.p.n_policies = lin->n_policies; a.p._pad = 0;
  a.out = out;
  return bsx_launch_linear_score(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_linear_evaluate (Fam: the family's host trait, bsx_host.h).
template <class Fam>
static inline int bsx_linear_score_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_linear_t* lin, float* state,
                                         int32_t* steps, const bsx_linear_eval_t& out, double* info) {
  bsx_linear_score_args e;
  return bsx_physics_closed_loop<Fam>(
      cfg, call, lin, state, steps, info, e.fam,
      [&](const void* extra, int) { return bsx_check_linear_call(call, lin, state, steps, out, info, extra); },
      [&](int32_t family) { return bsx_linear_score_call(e, family, call, lin, out); });
}

// The rule of every drawn (softmax) physics call, stated where the greedy calls refuse an epsilon outside [0, 1] (BSX_ERANGE:
// after the modes and the scalars, before an empty call returns and before any pointer is looked at): an epsilon other than
// 0.0 (NaN included) or an inv_temperature that is not finite or not > 0 is refused there.  The greedy check is given this
// copy of the policy, whose epsilon is 0.0 when both are acceptable and out of range when either is not.
template <class Policy>
static inline Policy bsx_drawn_policy(const Policy* policy, double inv_temperature) {
  Policy q = *policy;
  const bool ok = policy->epsilon == 0.0 && __builtin_isfinite(inv_temperature) && inv_temperature > 0.0;
  q.epsilon = ok ? 0.0 : 2.0;
  return q;
}

#endif  // BSX_LINEAR_SCORE_H_
