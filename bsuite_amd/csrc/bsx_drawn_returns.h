// bsx_drawn_returns.h — bsx_<family>_linear_sample_evaluate / bsx_<family>_mlp_sample_evaluate (evaluate_sampled_linear,
// evaluate_sampled_mlp): the arguments of the ONE kernel that serves cartpole, swing-up and mountain_car under either kind of
// softmax policy (bsx_drawn_returns_kernel, drawn_returns.hip), the body of its step loop, its launcher and the checks the
// four entry points share.  The sampled closed loop of bsx_gumbel_device.h that writes only what the evaluation writes
// (bsx_linear_score.h): the lanes take the steps and the draws of sample_linear / sample_mlp, and per lane the call leaves
// the episode count, the two float64 sums and the row of its last step instead of [T,B] slabs.
#ifndef BSX_DRAWN_RETURNS_H_
#define BSX_DRAWN_RETURNS_H_

#include "bsx_gumbel_device.h"         // bsx_trajectory_policy, bsx_gumbel_hidden_logits, bsx_gumbel.h, the checks below it

// A tagged struct, as bsx_linear_score_args: `family` says which member of `fam` is set.  p.explore_seed is the sample seed;
// p.epsilon is not read.
struct bsx_drawn_returns_args {
  int32_t family;                  // BSX_FAM_CARTPOLE (classic or swing-up: fam.cartpole.cfg.swingup) or BSX_FAM_MOUNTAIN_CAR
  int32_t n_steps;
  bsx_trajectory_policy p;
  double beta;                     // 1 / temperature: finite, > 0 (the entry points check)
  bsx_linear_eval_t out;
  union {
    cartpole_env::args cartpole;
    mountain_car_env::args mountain_car;
  } fam;
};

// The arguments through the kernarg segment, read where they are used (bsx_linear_view has the reason).
typedef const BSX_KERNARG bsx_drawn_returns_args* bsx_drawn_returns_kernarg;
__device__ __forceinline__ const bsx_drawn_returns_args& bsx_drawn_returns_view(bsx_drawn_returns_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_drawn_returns_args*)ka;
}
// Which member of `fam` a family's body reads.
struct bsx_drawn_returns_cartpole {
  typedef cartpole_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_drawn_returns_args& k) { return k.fam.cartpole; }
};
struct bsx_drawn_returns_mountain_car {
  typedef mountain_car_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_drawn_returns_args& k) { return k.fam.mountain_car; }
};

// evaluate_sampled_linear(T) / evaluate_sampled_mlp(T): bsx_gumbel_body with its per-step stores replaced by
// bsx_linear_score_body's accumulation.  State in Env::regs, the info columns in registers, Env::core on the registers,
// resets computed in line.  Per step the lane computes its three logits (bsx_linear_logits, or the hidden-layer pieces of
// bsx_gumbel_hidden_logits) and — unless it resets on this step: then it takes action 0 and draws nothing — block 0 of
// stream BSX_STREAM_SAMPLE and bsx_gumbel_select; after core() the float64 reward goes into bsx_eval_accumulate.  After the
// loop the thread stores its state, its info, the three sums, the episode count and the final row; LAST / FIRST are
// derived from the episode count and pooled once.
//   V, SHARED, HIDDEN   as in bsx_trajectory_body.
// The arguments are read through three views (bsx_drawn_returns_view): one before the loop, one per step, one after the
// loop.  No store, no barrier, no atomic and no LDS write inside the loop.
template <class Fam, int V, bool SHARED, bool HIDDEN>
__device__ __forceinline__ void bsx_drawn_returns_body(bsx_drawn_returns_kernarg ka, float* s_w, unsigned int* s_cnt) {
  typedef typename Fam::env Env;
  constexpr int D = Env::numel_of(V), NW = BSX_LINEAR_ROW(D);
  static_assert(D <= BSX_LINEAR_MAX_OBS && NW <= BSX_MLP_LDS_FLOATS, "row length");
  const bsx_drawn_returns_args& k0 = bsx_drawn_returns_view(ka);
  const typename Env::args& a0 = Fam::of(k0);
  const int H = HIDDEN ? k0.p.hidden : 0;                                // 1 .. BSX_MLP_MAX_HIDDEN (the entry points check)
  const int n1 = HIDDEN ? BSX_MLP_W1(D, H) : NW;
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  if constexpr (SHARED) {
    const int n = HIDDEN ? n1 + BSX_MLP_W2(H) : NW;                      // <= BSX_MLP_LDS_FLOATS
#pragma unroll
    for (int r = 0; r < (HIDDEN ? BSX_MLP_STAGE_ROUNDS : 1); ++r) {
      const int k = r * BSX_BLOCK + (int)threadIdx.x;
      if (k < n) s_w[k] = k < n1 ? k0.p.w1[k] : k0.p.w2[k - n1];
    }
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
    int32_t row = 0;                                                     // the lane's policy
    if constexpr (!SHARED) row = bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies);
    float w[HIDDEN ? 1 : NW];
    (void)w; (void)row;
    if constexpr (!SHARED && !HIDDEN) {
      const float* __restrict__ mine_w = k0.p.w1 + (int64_t)row * NW;
#pragma unroll
      for (int k = 0; k < NW; ++k) w[k] = mine_w[k];
    }
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_drawn_returns_args& kt = bsx_drawn_returns_view(ka);
      const typename Env::args& a = Fam::of(kt);
      const bsx_trajectory_policy& p = kt.p;
      const uint64_t step = step0 + (uint64_t)t;
      const int resets = Env::reset_pending(rg) ? 1 : 0;
      int32_t act = 0;
      if (!resets) {
        float l[BSX_LINEAR_ACTIONS];
        if constexpr (HIDDEN) {
          if constexpr (SHARED) {
            // (from an offset the compiler cannot trace to the loop's outside: bsx_mlp_returns_body)
            bsx_lds_table t1 = (bsx_lds_table)s_w + bsx_fresh(0u);
            bsx_gumbel_hidden_logits<D>(t1, t1 + n1, H, o, l);
          } else {
            const float* __restrict__ g1 = p.w1 + (int64_t)row * n1;
            const float* __restrict__ g2 = p.w2 + (int64_t)row * BSX_MLP_W2(H);
            bsx_gumbel_hidden_logits<D>(g1, g2, H, o, l);
          }
        } else {
          if constexpr (SHARED) {
            bsx_lds_table tab = (bsx_lds_table)s_w + bsx_fresh(0u);
#pragma unroll
            for (int k = 0; k < NW; ++k) w[k] = tab[k];
          }
          bsx_linear_logits(w, o, D, l);
        }
        const bsx_u32x4 u = bsx_gumbel_draws(p.explore_seed, lane, step);
        // (the action pinned where it is drawn: its only reader is core(), and sunk to that use the float64 arithmetic of
        // the six logarithms leaves their ~60 constants — opaque scalar pairs, BSX_K — live at once: 854 scalar spills)
        act = (int32_t)bsx_fresh((uint32_t)bsx_gumbel_select(l, kt.beta, u.v[0], u.v[1], u.v[2]));
      }
      double reward = 0.0;
      const int type = Env::template core<0, 0, true, false, false, V, true>(a, rg, act, i, lane, step, o, reward);
      bsx_eval_accumulate(&e, type, reward);
    }
    // every LAST is followed by a FIRST except one at the call's final step, and a lane that arrives with its reset
    // pending begins with one (small_obs_regs_rollout)
    n_last = (uint32_t)e.n;
    n_first = n_last + pending_in - (Env::reset_pending(rg) ? 1u : 0u);
    const bsx_drawn_returns_args& k1 = bsx_drawn_returns_view(ka);
    const typename Env::args& a1 = Fam::of(k1);
    Env::store(a1, i, rg);
    Env::template store_info<V>(a1, i, rg);
    k1.out.episodes[i] = e.n;
    k1.out.return_sum[i] = e.total;
    k1.out.episode_return_sum[i] = e.done;
    small_obs_store_row<false>(k1.out.observation_out + i * D, o, D);
  }
  bsx_pool_counts(Fam::of(bsx_drawn_returns_view(ka)).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_drawn_returns_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_drawn_returns(const bsx_drawn_returns_args& a, hipStream_t st);

// The refusals of the four entry points that do not depend on the family: bsx_check_linear_call's / bsx_check_mlp_call's, in
// their order, for the policy under the drawn rule (bsx_drawn_policy, bsx_linear_score.h).  No slab is written, so there is
// no 4 GiB refusal.
static inline int bsx_check_drawn_returns_call(const bsx_call_t* call, const bsx_linear_t* lin, double inv_temperature,
                                               const float* state, const int32_t* steps, const bsx_linear_eval_t& out,
                                               const double* info, const void* extra) {
  const bsx_linear_t q = bsx_drawn_policy(lin, inv_temperature);
  return bsx_check_linear_call(call, &q, state, steps, out, info, extra);
}
static inline int bsx_check_drawn_returns_call(const bsx_call_t* call, const bsx_mlp_t* mlp, double inv_temperature,
                                               const float* state, const int32_t* steps, const bsx_linear_eval_t& out,
                                               const double* info, const void* extra) {
  const bsx_mlp_t q = bsx_drawn_policy(mlp, inv_temperature);
  return bsx_check_mlp_call(call, &q, state, steps, out, info, extra);
}

// What the entry points share once the family's args are in place (a.fam): policy->explore_seed is the sample seed.
template <class Policy>
static inline int bsx_drawn_returns_call(bsx_drawn_returns_args& a, int32_t family, const bsx_call_t* call, const Policy* policy,
                                         double inv_temperature, const bsx_linear_eval_t& out) {
  a.family = family;
  a.n_steps = call->n_steps;
  a.p = bsx_make_trajectory_policy(policy);
  a.p.epsilon = 0.0;
  a.beta = inv_temperature;
  a.out = out;
  return bsx_launch_drawn_returns(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_linear_sample_evaluate / bsx_<family>_mlp_sample_evaluate (Fam: the family's host trait, bsx_host.h).
template <class Fam, class Policy>
static inline int bsx_drawn_returns_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const Policy* policy,
                                          double inv_temperature, float* state, int32_t* steps, const bsx_linear_eval_t& out,
                                          double* info) {
  bsx_drawn_returns_args e;
  return bsx_physics_closed_loop<Fam>(
      cfg, call, policy, state, steps, info, e.fam,
      [&](const void* extra, int) { return bsx_check_drawn_returns_call(call, policy, inv_temperature, state, steps, out, info, extra); },
      [&](int32_t family) { return bsx_drawn_returns_call(e, family, call, policy, inv_temperature, out); });
}

#endif  // BSX_DRAWN_RETURNS_H_
