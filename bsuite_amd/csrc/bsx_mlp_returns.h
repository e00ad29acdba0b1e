// bsx_mlp_returns.h — bsx_<family>_mlp_evaluate (evaluate_mlp): the arguments of the ONE kernel that serves cartpole, swing-up
// and mountain_car (bsx_mlp_returns_kernel, mlp.hip), the body of its step loop, its launcher and the checks the two entry
// points share.  The sibling of bsx_linear_score.h: the same tagged struct, kernarg views and register loop, with one ReLU
// hidden layer (bsx_mlp.h) between the observation and the logits.
#ifndef BSX_MLP_RETURNS_H_
#define BSX_MLP_RETURNS_H_

#include "bsx_linear_score.h"          // BSX_KERNARG, bsx_check_linear_call (and small_obs.h, bsx_policy.h, the two families)
#include "bsx_mlp.h"

// The policy side of the call, as the kernel reads it.
struct bsx_mlp_args {
  const float* w1;                 // [n_policies, hidden, D + 1]
  const float* w2;                 // [n_policies, 3, hidden + 1]
  const int32_t* policy_index;     // [n_lanes], or null: every lane takes pair 0 (n_policies == 1)
  const float* observation_in;     // [n_lanes, D]
  double epsilon;
  uint64_t explore_seed;
  int32_t n_policies, hidden;
};

struct bsx_mlp_returns_args {
  int32_t family;                  // BSX_FAM_CARTPOLE (classic or swing-up: fam.cartpole.cfg.swingup) or BSX_FAM_MOUNTAIN_CAR
  int32_t n_steps;
  bsx_mlp_args p;
  bsx_linear_eval_t out;
  union {
    cartpole_env::args cartpole;
    mountain_car_env::args mountain_car;
  } fam;
};

// A shared pair of matrices in LDS: w1 then w2, as in global memory.
#define BSX_MLP_LDS_FLOATS 772       // >= BSX_MLP_W1(BSX_LINEAR_MAX_OBS, BSX_MLP_MAX_HIDDEN) + BSX_MLP_W2(BSX_MLP_MAX_HIDDEN) = 771
#define BSX_MLP_STAGE_ROUNDS ((BSX_MLP_LDS_FLOATS + BSX_BLOCK - 1) / BSX_BLOCK)

// The arguments through the kernarg segment, read where they are used (bsx_linear_view has the reason).
typedef const BSX_KERNARG bsx_mlp_returns_args* bsx_mlp_kernarg;
__device__ __forceinline__ const bsx_mlp_returns_args& bsx_mlp_view(bsx_mlp_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_mlp_returns_args*)ka;
}
// Which member of `fam` a family's body reads.
struct bsx_mlp_cartpole {
  typedef cartpole_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_mlp_returns_args& k) { return k.fam.cartpole; }
};
struct bsx_mlp_mountain_car {
  typedef mountain_car_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_mlp_returns_args& k) { return k.fam.mountain_car; }
};

// evaluate_mlp(T): bsx_linear_score_body's loop — state in Env::regs, the info columns in registers, Env::core on the
// registers, resets computed in line, LAST / FIRST counted per thread and pooled once, no store inside the loop — with
// bsx_mlp_select's pieces in place of bsx_linear_select.  Per step the thread walks the H hidden units: unit j costs the
// D + 1 floats of its row of w1 and the three w2[a][j], each consumed where it is read, so that the policy holds three logit
// accumulators across the walk and nothing across the step.
//   SHARED  one pair for all lanes (n_policies == 1): staged once in LDS by the workgroup; every lane of a wave reads the
//           same address (a broadcast), through an offset the compiler cannot trace to the loop's outside (bsx_fresh).
//           else the lane's own pair, read from global memory inside the step: its addresses depend on
//           bsx_policy_clamp(policy_index[i], P) alone, so a wave whose lanes name one pair touches one line per load and
//           a wave of 64 different pairs touches 64 (the caller's layout: lanes grouped by policy is the fast one).
// The arguments are read through three views (bsx_mlp_view): one before the loop, one per step, one after the loop.
// (bsx_torso_body, bsx_torso.h, repeats this loop's skeleton around a two-hidden-layer policy: a change to the prologue, the
// coin, the n_first rule or the epilogue here belongs there too.)
template <class Fam, int V, bool SHARED>
__device__ __forceinline__ void bsx_mlp_returns_body(bsx_mlp_kernarg ka, float* s_w, unsigned int* s_cnt) {
  typedef typename Fam::env Env;
  constexpr int D = Env::numel_of(V);
  static_assert(D <= BSX_LINEAR_MAX_OBS, "row length");
  const bsx_mlp_returns_args& k0 = bsx_mlp_view(ka);
  const typename Env::args& a0 = Fam::of(k0);
  const int H = k0.p.hidden;                                             // 1 .. BSX_MLP_MAX_HIDDEN (the entry points check)
  const int n1 = BSX_MLP_W1(D, H);
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  if constexpr (SHARED) {
    const int n = n1 + BSX_MLP_W2(H);                                    // <= BSX_MLP_LDS_FLOATS
#pragma unroll
    for (int r = 0; r < BSX_MLP_STAGE_ROUNDS; ++r) {
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
    int32_t row = 0;                                                     // the lane's pair: all of the policy that stays live
    if constexpr (!SHARED) row = bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies);
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_mlp_returns_args& kt = bsx_mlp_view(ka);
      const typename Env::args& a = Fam::of(kt);
      const bsx_mlp_args& p = kt.p;
      const uint64_t step = step0 + (uint64_t)t;
      const int resets = Env::reset_pending(rg) ? 1 : 0;
      float l[BSX_LINEAR_ACTIONS];
      if constexpr (SHARED) {
        bsx_lds_table t1 = (bsx_lds_table)s_w + bsx_fresh(0u);
        bsx_lds_table t2 = t1 + n1;
#pragma unroll
        for (int c = 0; c < BSX_LINEAR_ACTIONS; ++c) l[c] = t2[c * (H + 1) + H];
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
          float w1j[D + 1], w2j[BSX_LINEAR_ACTIONS];
#pragma unroll
          for (int d = 0; d <= D; ++d) w1j[d] = t1[j * (D + 1) + d];
#pragma unroll
          for (int c = 0; c < BSX_LINEAR_ACTIONS; ++c) w2j[c] = t2[c * (H + 1) + j];
          bsx_mlp_accumulate(l, w2j, bsx_mlp_hidden(w1j, o, D));
        }
      } else {
        const float* __restrict__ g1 = p.w1 + (int64_t)row * n1;
        const float* __restrict__ g2 = p.w2 + (int64_t)row * BSX_MLP_W2(H);
#pragma unroll
        for (int c = 0; c < BSX_LINEAR_ACTIONS; ++c) l[c] = g2[c * (H + 1) + H];
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
          float w1j[D + 1], w2j[BSX_LINEAR_ACTIONS];
#pragma unroll
          for (int d = 0; d <= D; ++d) w1j[d] = g1[j * (D + 1) + d];
#pragma unroll
          for (int c = 0; c < BSX_LINEAR_ACTIONS; ++c) w2j[c] = g2[c * (H + 1) + j];
          bsx_mlp_accumulate(l, w2j, bsx_mlp_hidden(w1j, o, D));
        }
      }
      const int32_t best = bsx_mlp_argmax(l);
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
    const bsx_mlp_returns_args& k1 = bsx_mlp_view(ka);
    const typename Env::args& a1 = Fam::of(k1);
    Env::store(a1, i, rg);
    Env::template store_info<V>(a1, i, rg);
    k1.out.episodes[i] = e.n;
    k1.out.return_sum[i] = e.total;
    k1.out.episode_return_sum[i] = e.done;
    small_obs_store_row<false>(k1.out.observation_out + i * D, o, D);
  }
  bsx_pool_counts(Fam::of(bsx_mlp_view(ka)).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_mlp_returns_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_mlp_returns(const bsx_mlp_returns_args& a, hipStream_t st);

// The refusals of bsx_<family>_mlp_evaluate that do not depend on the family: bsx_check_linear_call's, in its order — modes,
// scalars, then, for a call with lanes, pointers.  A `hidden` outside [1, BSX_MLP_MAX_HIDDEN] is reported where
// n_policies < 1 is, and w2 is one more pointer a call with lanes needs.  (`extra` as there.)
static inline int bsx_check_mlp_call(const bsx_call_t* call, const bsx_mlp_t* mlp, const float* state, const int32_t* steps,
                                     bool outputs_present, const double* info, const void* extra) {
  const bool hidden_ok = mlp->hidden >= 1 && mlp->hidden <= BSX_MLP_MAX_HIDDEN;
  const bsx_linear_t lin = {mlp->w1, hidden_ok ? mlp->n_policies : 0, mlp->policy_index, mlp->epsilon, mlp->explore_seed,
                            mlp->observation_in};
  return bsx_check_linear_call(call, &lin, state, steps, outputs_present, info, mlp->w2 != nullptr ? extra : nullptr);
}
static inline int bsx_check_mlp_call(const bsx_call_t* call, const bsx_mlp_t* mlp, const float* state, const int32_t* steps,
                                     const bsx_linear_eval_t& out, const double* info, const void* extra) {
  return bsx_check_mlp_call(call, mlp, state, steps, bsx_linear_eval_present(out), info, extra);
}

// What the two entry points share once the family's args are in place.
static inline int bsx_mlp_returns_call(bsx_mlp_returns_args& a, int32_t family, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                       const bsx_linear_eval_t& out) {
  a.family = family;
  a.n_steps = call->n_steps;
  a.p.w1 = mlp->w1;
  a.p.w2 = mlp->w2;
  a.p.policy_index = mlp->n_policies > 1 ? mlp->policy_index : nullptr;
  a.p.observation_in = mlp->observation_in;
  a.p.epsilon = mlp->epsilon;
  a.p.explore_seed = mlp->explore_seed;
  a.p.n_policies = mlp->n_policies; a.p.hidden = mlp->hidden;
  a.out = out;
  return bsx_launch_mlp_returns(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_mlp_evaluate (Fam: the family's host trait, bsx_host.h).
template <class Fam>
static inline int bsx_mlp_returns_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp, float* state,
                                        int32_t* steps, const bsx_linear_eval_t& out, double* info) {
  bsx_mlp_returns_args e;
  return bsx_physics_closed_loop<Fam>(
      cfg, call, mlp, state, steps, info, e.fam,
      [&](const void* extra, int) { return bsx_check_mlp_call(call, mlp, state, steps, out, info, extra); },
      [&](int32_t family) { return bsx_mlp_returns_call(e, family, call, mlp, out); });
}

#endif  // BSX_MLP_RETURNS_H_
