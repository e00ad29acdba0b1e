// bsx_gumbel_device.h — bsx_<family>_linear_sample / bsx_<family>_mlp_sample (sample_linear, sample_mlp): the arguments of the
// ONE kernel that serves cartpole, swing-up and mountain_car under either kind of softmax policy (bsx_gumbel_kernel,
// gumbel.hip), the body of its step loop, its launcher and the checks the four entry points share.  The recording closed loop
// of bsx_trajectory.h with another decision: instead of the greedy action (and an epsilon coin) the lane takes a draw from
// softmax(logits / temperature) by Gumbel-max (bsx_gumbel.h).
#ifndef BSX_GUMBEL_DEVICE_H_
#define BSX_GUMBEL_DEVICE_H_

#include "bsx_trajectory.h"            // bsx_trajectory_args and its family accessors, the checks; small_obs.h through it
#include "bsx_gumbel.h"

// The trajectory's arguments plus the inverse temperature.  t.p.explore_seed is the sample seed; t.p.epsilon is not read.
struct bsx_gumbel_args {
  bsx_trajectory_args t;
  double beta;                     // 1 / temperature: finite, > 0 (the entry points check)
};

// The arguments through the kernarg segment, read where they are used (bsx_linear_view has the reason).
typedef const BSX_KERNARG bsx_gumbel_args* bsx_gumbel_kernarg;
__device__ __forceinline__ const bsx_gumbel_args& bsx_gumbel_view(bsx_gumbel_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_gumbel_args*)ka;
}

// The logits of row o[] under a pair of matrices read through `Tab` — a table in LDS (a shared pair) or the lane's own pair in
// global memory: bsx_mlp_logits' walk in the kernel's pieces (bsx_mlp.h), unit j consumed where it is read, three logit
// accumulators live across the walk.
template <int D, class Tab>
__device__ __forceinline__ void bsx_gumbel_hidden_logits(Tab t1, Tab t2, const int H, const float* o, float* l) {
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
}

// sample_linear(T) / sample_mlp(T): bsx_trajectory_body with the softmax decision.  State in Env::regs, the info columns in
// registers, Env::core on the registers, resets computed in line, LAST / FIRST counted per thread and pooled once, state and
// info stored after the loop.  Per step the lane computes its three logits (bsx_linear_logits, or the hidden-layer pieces),
// and — unless it resets on this step: then it takes action 0 and draws nothing — block 0 of stream BSX_STREAM_SAMPLE and
// bsx_gumbel_select.  After core() it stores what step() would have returned and the action, each address {the step's slab
// pointer, formed on the scalar unit} + {the lane's 32-bit byte offset}: the entry points refuse a [B, D] slab of 4 GiB or
// more.  The stores follow the fused rollout's policy (small_obs.h) with ONE policy for the rows whatever their length,
// small_obs_store_row<true>: three floats leave as one non-temporal 12-byte store, six and eight as plain 8-byte pieces
// (BSX_OUT_PARTIAL) — what the trajectory kernel measured as the faster choice for its linear cases.  Nothing
// the kernel stores is read back: o[] of core() is the next step's input.
//   V, SHARED, HIDDEN   as in bsx_trajectory_body.
// The arguments are read through three views (bsx_gumbel_view): one before the loop, one per step, one after the loop.
// No barrier, no atomic and no LDS write inside the loop.
template <class Fam, int V, bool SHARED, bool HIDDEN>
__device__ __forceinline__ void bsx_gumbel_body(bsx_gumbel_kernarg ka, float* s_w, unsigned int* s_cnt) {
  typedef typename Fam::env Env;
  constexpr int D = Env::numel_of(V), NW = BSX_LINEAR_ROW(D);
  static_assert(D <= BSX_LINEAR_MAX_OBS && NW <= BSX_MLP_LDS_FLOATS, "row length");
  const bsx_trajectory_args& k0 = bsx_gumbel_view(ka).t;
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
    const uint32_t iu0 = (uint32_t)i;
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_gumbel_args& gt = bsx_gumbel_view(ka);
      const bsx_trajectory_args& kt = gt.t;
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
        act = bsx_gumbel_select(l, gt.beta, u.v[0], u.v[1], u.v[2]);
      }
      double reward = 0.0;
      const int type = Env::template core<0, 0, true, false, false, V, true>(a, rg, act, i, lane, step, o, reward);
      n_last += type == BSX_LAST ? 1u : 0u;
      // the step's outputs.  t * B on the scalar unit from a step number the optimiser cannot turn into five running
      // pointers (small_obs_regs_rollout has the reason), the lane's byte offsets from a value it cannot hoist.
      uint32_t tu = (uint32_t)t;
      asm volatile("" : "+s"(tu));
      const int64_t tb = (int64_t)tu * a.ctl.n_lanes;                    // uniform
      const uint32_t iu = bsx_fresh(iu0);
      float r, d;
      bsx_emit_values<0, 0, false, 0>(a.ctl, i, i, lane, step, type, reward, r, d);
      constexpr int NTS = small_rollout_nt_scalars<Env>::value ? BSX_OUT_SCALARS.rollout : BSX_ST_PLAIN;
      bsx_st<NTS>(bsx_at_off(kt.out.reward + tb, iu * 4u), r);
      bsx_st<NTS>(bsx_at_off(kt.out.discount + tb, iu * 4u), d);
      bsx_st<NTS>(bsx_at_off(kt.out.step_type + tb, iu), (int8_t)type);
      small_obs_store_row<true>(bsx_at_off(kt.out.observation + tb * D, iu * (uint32_t)(D * 4)), o, D);
      bsx_st<BSX_OUT_SCALARS.rollout>(bsx_at_off(kt.actions_out + tb, iu * 4u), (int32_t)act);
    }
    // every LAST is followed by a FIRST except one at the call's final step, and a lane that arrives with its reset
    // pending begins with one (small_obs_regs_rollout)
    n_first = n_last + pending_in - (Env::reset_pending(rg) ? 1u : 0u);
    const bsx_trajectory_args& k1 = bsx_gumbel_view(ka).t;
    const typename Env::args& a1 = Fam::of(k1);
    Env::store(a1, i, rg);
    Env::template store_info<V>(a1, i, rg);
  }
  bsx_pool_counts(Fam::of(bsx_gumbel_view(ka).t).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_gumbel_kernel over a.t.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_gumbel(const bsx_gumbel_args& a, hipStream_t st);

// The refusals of the four entry points that do not depend on the family: bsx_check_trajectory_call's, in its order, for
// the policy under the drawn rule (bsx_drawn_policy, bsx_linear_score.h).
template <class Policy>
static inline int bsx_check_gumbel_call(const bsx_call_t* call, const Policy* policy, double inv_temperature, const float* state,
                                        const int32_t* steps, const bsx_timestep_t& out, const int32_t* actions_out,
                                        const double* info, const void* extra, int D) {
  const Policy q = bsx_drawn_policy(policy, inv_temperature);
  return bsx_check_trajectory_call(call, &q, state, steps, out, actions_out, info, extra, D);
}

// What the entry points share once the family's args are in place (a.t.fam): policy->explore_seed is the sample seed.
template <class Policy>
static inline int bsx_gumbel_call(bsx_gumbel_args& a, int32_t family, const bsx_call_t* call, const Policy* policy,
                                  double inv_temperature, const bsx_timestep_t& out, int32_t* actions_out) {
  a.t.family = family;
  a.t.n_steps = call->n_steps;
  a.t.p = bsx_make_trajectory_policy(policy);
  a.t.p.epsilon = 0.0;
  a.t.out = out; a.t.actions_out = actions_out;
  a.beta = inv_temperature;
  return bsx_launch_gumbel(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_linear_sample / bsx_<family>_mlp_sample (Fam: the family's host trait, bsx_host.h).
template <class Fam, class Policy>
static inline int bsx_gumbel_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const Policy* policy, double inv_temperature,
                                   float* state, int32_t* steps, const bsx_timestep_t& out, int32_t* actions_out, double* info) {
  bsx_gumbel_args e;
  return bsx_physics_closed_loop<Fam>(
      cfg, call, policy, state, steps, info, e.t.fam,
      [&](const void* extra, int D) {
        return bsx_check_gumbel_call(call, policy, inv_temperature, state, steps, out, actions_out, info, extra, D);
      },
      [&](int32_t family) { return bsx_gumbel_call(e, family, call, policy, inv_temperature, out, actions_out); });
}

#endif  // BSX_GUMBEL_DEVICE_H_
