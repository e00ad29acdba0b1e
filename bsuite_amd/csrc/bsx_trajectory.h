// bsx_trajectory.h — bsx_<family>_linear_rollout / bsx_<family>_mlp_rollout (rollout_linear, rollout_mlp): the arguments of
// the ONE kernel that serves cartpole, swing-up and mountain_car under either kind of policy (bsx_trajectory_kernel,
// trajectory.hip), the body of its step loop, its launcher and the checks the four entry points share.  The closed loop of
// bsx_linear_score.h / bsx_mlp_returns.h that also WRITES what it walks through: the TimeStep of every step and the action
// taken, [T,B] each, through the per-step output path of the lean fused rollout (small_obs_regs_rollout, OFF32).
#ifndef BSX_TRAJECTORY_H_
#define BSX_TRAJECTORY_H_

#include "bsx_mlp_returns.h"           // bsx_linear_score.h, bsx_mlp.h, BSX_KERNARG, BSX_MLP_LDS_FLOATS and the two checks

// The policy side of the call, as the kernel reads it: either kind.
struct bsx_trajectory_policy {
  const float* w1;                 // linear: weights [n_policies, 3, D + 1]; hidden layer: w1 [n_policies, hidden, D + 1]
  const float* w2;                 // hidden layer: [n_policies, 3, hidden + 1]; linear: null
  const int32_t* policy_index;     // [n_lanes], or null: every lane takes policy 0 (n_policies == 1)
  const float* observation_in;     // [n_lanes, D]
  double epsilon;
  uint64_t explore_seed;
  int32_t n_policies, hidden;      // hidden == 0: a linear policy
};

struct bsx_trajectory_args {
  int32_t family;                  // BSX_FAM_CARTPOLE (classic or swing-up: fam.cartpole.cfg.swingup) or BSX_FAM_MOUNTAIN_CAR
  int32_t n_steps;
  bsx_trajectory_policy p;
  bsx_timestep_t out;              // [n_steps, n_lanes] reward / discount / step_type, [n_steps, n_lanes, D] observation
  int32_t* actions_out;            // [n_steps, n_lanes]
  union {
    cartpole_env::args cartpole;
    mountain_car_env::args mountain_car;
  } fam;
};

// The arguments through the kernarg segment, read where they are used (bsx_linear_view has the reason).
typedef const BSX_KERNARG bsx_trajectory_args* bsx_trajectory_kernarg;
__device__ __forceinline__ const bsx_trajectory_args& bsx_trajectory_view(bsx_trajectory_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_trajectory_args*)ka;
}
// Which member of `fam` a family's body reads.
struct bsx_trajectory_cartpole {
  typedef cartpole_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_trajectory_args& k) { return k.fam.cartpole; }
};
struct bsx_trajectory_mountain_car {
  typedef mountain_car_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_trajectory_args& k) { return k.fam.mountain_car; }
};

// The greedy action of row o[] under a pair of matrices read through `Tab` — a table in LDS (bsx_lds_table, a shared pair) or
// the lane's own pair in global memory: bsx_mlp_select's walk in the kernel's pieces (bsx_mlp.h), unit j consumed where it
// is read, three logit accumulators live across the walk.
template <int D, class Tab>
__device__ __forceinline__ int32_t bsx_trajectory_hidden_action(Tab t1, Tab t2, const int H, const float* o) {
  float l[BSX_LINEAR_ACTIONS];
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
  return bsx_mlp_argmax(l);
}

// A lane's row of a [T,B,D] trajectory, stored by its own thread, NON-TEMPORAL whatever its length: three floats through
// small_obs_store_row<true> (one 12-byte store), six and eight in 16- and 8-byte pieces.  This is what the call's acceptance
// pins (tests/test_trajectory_host.py: every row store inside the loops is non-temporal), not what is fastest:
// small_obs_store_row keeps rows of 6 / 8 floats plain (BSX_OUT_PARTIAL), and with it this kernel's linear cases take 7.5
// instead of 18.3 us per step (cartpole) and 9.9 instead of 27.7 (swing-up) at 2^20 lanes; under a hidden layer the two are
// equal (profiles/trajectory/README.md, "Row stores").
template <int D>
__device__ __forceinline__ void bsx_trajectory_store_row(BSX_GLOBAL float* dst, const float* o) {
  if constexpr (D == 6 || D == 8) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float row4v __attribute__((ext_vector_type(4), aligned(4)));
    typedef float row2v __attribute__((ext_vector_type(2), aligned(4)));
    row4v lo; lo.x = o[0]; lo.y = o[1]; lo.z = o[2]; lo.w = o[3];
    __builtin_nontemporal_store(lo, reinterpret_cast<BSX_GLOBAL row4v*>(dst));
    if constexpr (D == 8) {
      row4v hi; hi.x = o[4]; hi.y = o[5]; hi.z = o[6]; hi.w = o[7];
      __builtin_nontemporal_store(hi, reinterpret_cast<BSX_GLOBAL row4v*>(dst + 4));
    } else {
      row2v hi; hi.x = o[4]; hi.y = o[5];
      __builtin_nontemporal_store(hi, reinterpret_cast<BSX_GLOBAL row2v*>(dst + 4));
    }
#endif
  } else {
    small_obs_store_row<true>(dst, o, D);
  }
}

// rollout_linear(T) / rollout_mlp(T).  Before and after the loop this is the evaluate body (bsx_linear_score_body,
// bsx_mlp_returns_body): state in Env::regs, the info columns in registers, Env::core on the registers, resets computed in
// line, LAST / FIRST counted per thread and pooled once, state and info stored after the loop.  Per step, after core(), the
// lane stores what step() would have returned — reward / discount from bsx_emit_values' lean instantiation (the float32 is
// the one step() writes), step_type, the row o[] — and the action it took.  Each address is {the step's slab pointer: the
// kernarg base + t * B elements, formed on the scalar unit} + {the lane's 32-bit byte offset}: the entry points refuse a
// [B, D] slab of 4 GiB or more, so the offset never wraps.  The stores follow the fused rollout's policy (small_obs.h): rows
// non-temporal (bsx_trajectory_store_row), the action column non-temporal, the three scalar columns as
// small_rollout_nt_scalars<Env> says.  Nothing the kernel stores is read back: o[] of core() is the next step's input.
//   V       the family's variant (Env::numel_of(V) floats per row: cartpole 0 classic / 1 swing-up)
//   SHARED  one policy for all lanes (n_policies == 1): staged in LDS by the workgroup and read from there every step; else
//           the lane's own — a linear row loaded once into registers, a hidden-layer pair read per step from global memory.
//   HIDDEN  one ReLU hidden layer of p.hidden units (bsx_mlp.h), else a linear map (bsx_linear.h).
// The arguments are read through three views (bsx_trajectory_view): one before the loop, one per step, one after the loop.
// No barrier, no atomic and no LDS write inside the loop.
// (bsx_torso_body, bsx_torso.h, repeats this loop's skeleton — prologue, coin, per-step stores, the n_first rule, epilogue —
// around a two-hidden-layer policy: a change to any of them here belongs there too.)
template <class Fam, int V, bool SHARED, bool HIDDEN>
__device__ __forceinline__ void bsx_trajectory_body(bsx_trajectory_kernarg ka, float* s_w, unsigned int* s_cnt) {
  typedef typename Fam::env Env;
  constexpr int D = Env::numel_of(V), NW = BSX_LINEAR_ROW(D);
  static_assert(D <= BSX_LINEAR_MAX_OBS && NW <= BSX_MLP_LDS_FLOATS, "row length");
  const bsx_trajectory_args& k0 = bsx_trajectory_view(ka);
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
      const bsx_trajectory_args& kt = bsx_trajectory_view(ka);
      const typename Env::args& a = Fam::of(kt);
      const bsx_trajectory_policy& p = kt.p;
      const uint64_t step = step0 + (uint64_t)t;
      const int resets = Env::reset_pending(rg) ? 1 : 0;
      int32_t best;
      if constexpr (HIDDEN) {
        if constexpr (SHARED) {
          // (from an offset the compiler cannot trace to the loop's outside: bsx_mlp_returns_body)
          bsx_lds_table t1 = (bsx_lds_table)s_w + bsx_fresh(0u);
          best = bsx_trajectory_hidden_action<D>(t1, t1 + n1, H, o);
        } else {
          const float* __restrict__ g1 = p.w1 + (int64_t)row * n1;
          const float* __restrict__ g2 = p.w2 + (int64_t)row * BSX_MLP_W2(H);
          best = bsx_trajectory_hidden_action<D>(g1, g2, H, o);
        }
      } else {
        if constexpr (SHARED) {
          bsx_lds_table tab = (bsx_lds_table)s_w + bsx_fresh(0u);
#pragma unroll
          for (int k = 0; k < NW; ++k) w[k] = tab[k];
        }
        best = bsx_linear_select(w, o, D);
      }
      uint32_t w0 = 0, w1 = 0, w2 = 0;
      if (p.epsilon > 0.0 && !resets) {
        const bsx_u32x4 u = bsx_policy_draws(p.explore_seed, lane, step);
        w0 = u.v[0]; w1 = u.v[1]; w2 = u.v[2];
      }
      const int act = bsx_policy_select((uint32_t)best, resets, p.epsilon, w0, w1, w2, BSX_LINEAR_ACTIONS);
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
      bsx_trajectory_store_row<D>(bsx_at_off(kt.out.observation + tb * D, iu * (uint32_t)(D * 4)), o);
      bsx_st<BSX_OUT_SCALARS.rollout>(bsx_at_off(kt.actions_out + tb, iu * 4u), (int32_t)act);
    }
    // every LAST is followed by a FIRST except one at the call's final step, and a lane that arrives with its reset
    // pending begins with one (small_obs_regs_rollout)
    n_first = n_last + pending_in - (Env::reset_pending(rg) ? 1u : 0u);
    const bsx_trajectory_args& k1 = bsx_trajectory_view(ka);
    const typename Env::args& a1 = Fam::of(k1);
    Env::store(a1, i, rg);
    Env::template store_info<V>(a1, i, rg);
  }
  bsx_pool_counts(Fam::of(bsx_trajectory_view(ka)).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_trajectory_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_trajectory(const bsx_trajectory_args& a, hipStream_t st);

// The refusals of the four entry points that do not depend on the family: those of bsx_check_linear_call /
// bsx_check_mlp_call, in their order, with the TimeStep's four pointers and the action column as the outputs that must be
// present.  Then what only a call that writes [T,B] slabs has: a [B, D] slab of 4 GiB or more (BSX_EINVAL: the kernel adds
// the lane's 32-bit byte offset to the slab's 64-bit address).
static inline bool bsx_trajectory_outputs_present(const bsx_timestep_t& out, const int32_t* actions_out) {
  return out.reward != nullptr && out.discount != nullptr && out.step_type != nullptr && out.observation != nullptr &&
         actions_out != nullptr;
}
static inline int bsx_check_trajectory_slab(int rc, const bsx_call_t* call, int D) {
  if (rc == 0 && call->n_lanes * (int64_t)(D * 4) >= ((int64_t)1 << 32)) return BSX_EINVAL;
  return rc;
}
static inline int bsx_check_trajectory_call(const bsx_call_t* call, const bsx_linear_t* lin, const float* state, const int32_t* steps,
                                            const bsx_timestep_t& out, const int32_t* actions_out, const double* info,
                                            const void* extra, int D) {
  return bsx_check_trajectory_slab(
      bsx_check_linear_call(call, lin, state, steps, bsx_trajectory_outputs_present(out, actions_out), info, extra), call, D);
}
static inline int bsx_check_trajectory_call(const bsx_call_t* call, const bsx_mlp_t* mlp, const float* state, const int32_t* steps,
                                            const bsx_timestep_t& out, const int32_t* actions_out, const double* info,
                                            const void* extra, int D) {
  return bsx_check_trajectory_slab(
      bsx_check_mlp_call(call, mlp, state, steps, bsx_trajectory_outputs_present(out, actions_out), info, extra), call, D);
}

// The policy side of a call as the kernel reads it, from either kind of policy struct (epsilon and explore_seed as given:
// a drawn call overwrites the one and reads the other as its sample seed).
static inline bsx_trajectory_policy bsx_make_trajectory_policy(const bsx_linear_t* lin) {
  return {lin->weights, nullptr, lin->n_policies > 1 ? lin->policy_index : nullptr, lin->observation_in, lin->epsilon,
          lin->explore_seed, lin->n_policies, 0};
}
static inline bsx_trajectory_policy bsx_make_trajectory_policy(const bsx_mlp_t* mlp) {
  return {mlp->w1, mlp->w2, mlp->n_policies > 1 ? mlp->policy_index : nullptr, mlp->observation_in, mlp->epsilon,
          mlp->explore_seed, mlp->n_policies, mlp->hidden};
}

// What the entry points share once the family's args are in place.
template <class Policy>
static inline int bsx_trajectory_call(bsx_trajectory_args& a, int32_t family, const bsx_call_t* call, const Policy* policy,
                                      const bsx_timestep_t& out, int32_t* actions_out) {
  a.family = family;
  a.n_steps = call->n_steps;
  a.p = bsx_make_trajectory_policy(policy);
  a.out = out; a.actions_out = actions_out;
  return bsx_launch_trajectory(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_linear_rollout / bsx_<family>_mlp_rollout (Fam: the family's host trait, bsx_host.h).
template <class Fam, class Policy>
static inline int bsx_trajectory_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const Policy* policy, float* state,
                                       int32_t* steps, const bsx_timestep_t& out, int32_t* actions_out, double* info) {
  bsx_trajectory_args e;
  return bsx_physics_closed_loop<Fam>(
      cfg, call, policy, state, steps, info, e.fam,
      [&](const void* extra, int D) { return bsx_check_trajectory_call(call, policy, state, steps, out, actions_out, info, extra, D); },
      [&](int32_t family) { return bsx_trajectory_call(e, family, call, policy, out, actions_out); });
}

#endif  // BSX_TRAJECTORY_H_
