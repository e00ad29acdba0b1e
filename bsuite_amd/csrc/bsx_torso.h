// bsx_torso.h — bsx_<family>_mlp2_evaluate / bsx_<family>_mlp2_rollout (evaluate_mlp2, rollout_mlp2) and
// bsx_<family>_mlp2_sample_evaluate / bsx_<family>_mlp2_sample (evaluate_sampled_mlp2, sample_mlp2): the arguments of the ONE
// kernel that serves cartpole, swing-up and mountain_car under a policy with two ReLU hidden layers (bsx_torso_kernel,
// torso.hip), the body of its step loop, its launcher and the checks the eight entry points share.  The closed loop of
// bsx_mlp_returns.h (evaluate: three sums and the final row) and of bsx_trajectory.h (record: the TimeStep of every step and
// the action taken), with bsx_mlp2.h's rule between the observation and the action.
#ifndef BSX_TORSO_H_
#define BSX_TORSO_H_

#include "bsx_trajectory.h"            // bsx_mlp_returns.h, bsx_linear_score.h, BSX_KERNARG, bsx_trajectory_store_row, the checks
#include "bsx_mlp2.h"
#include "bsx_gumbel.h"

// How a lane's action comes from its logits: the greedy one (with the epsilon coin), or a draw from softmax(logits /
// temperature) by Gumbel-max (bsx_gumbel.h; bsx_<family>_mlp2_sample / bsx_<family>_mlp2_sample_evaluate, sample_mlp2 /
// evaluate_sampled_mlp2).  Uniform per launch; a compile-time parameter of the body (DRAWN) and of the walk (KEEP): twelve
// bodies for each mode.
#define BSX_TORSO_GREEDY 0
#define BSX_TORSO_DRAWN 1

// The policy side of the call, as the kernel reads it.
struct bsx_torso_policy {
  const float* w1;                 // [n_policies, hidden1, D + 1]
  const float* w2;                 // [n_policies, hidden2, hidden1 + 1]
  const float* w3;                 // [n_policies, 3, hidden2 + 1]
  const int32_t* policy_index;     // [n_lanes], or null: every lane takes triple 0 (n_policies == 1)
  const float* observation_in;     // [n_lanes, D]
  double epsilon;                  // BSX_TORSO_GREEDY; not read by BSX_TORSO_DRAWN
  uint64_t explore_seed;           // BSX_TORSO_DRAWN: the sample seed
  int32_t n_policies, hidden1, hidden2;
  int32_t width;                   // layer-2 accumulators a lane keeps: the smallest of 16, 32, 64 that is >= hidden2
};

struct bsx_torso_args {
  int32_t family;                  // BSX_FAM_CARTPOLE (classic or swing-up: fam.cartpole.cfg.swingup) or BSX_FAM_MOUNTAIN_CAR
  int32_t n_steps;
  int32_t mode;                    // BSX_TORSO_GREEDY or BSX_TORSO_DRAWN
  int32_t record;                  // 0: evaluate (writes `ev` after the loop); 1: record (writes `out`, `actions_out` per step)
  bsx_torso_policy p;
  bsx_linear_eval_t ev;
  bsx_timestep_t out;              // [n_steps, n_lanes] reward / discount / step_type, [n_steps, n_lanes, D] observation
  int32_t* actions_out;            // [n_steps, n_lanes]
  union {
    cartpole_env::args cartpole;
    mountain_car_env::args mountain_car;
  } fam;
  // (after everything the greedy bodies read: their kernarg offsets stay what they were)
  double beta;                     // BSX_TORSO_DRAWN: 1 / temperature, finite and > 0 (the entry points check)
};

// A shared triple in the workgroup's dynamic LDS, staged once per launch (bsx_torso_stage), W = p.width:
//   [0, (H1 + 1) * W)              w2 TRANSPOSED and zero-padded: row j holds w2[0 .. H2-1][j], then zeros to W; row H1 is the
//                                  bias.  For a fixed j the k-run is contiguous and 16-byte aligned: one broadcast 16-byte read
//                                  per four weights.
//   then (H2 + 1) * 4              w3 transposed: row k holds w3[0][k], w3[1][k], w3[2][k], 0; row H2 is the bias
//   then H1 * (D + 1)              w1, as in global memory
// At most 65 * 64 + 65 * 4 + 64 * 9 = 4996 floats (19,984 bytes): the launch sizes the segment.
#define BSX_TORSO_W2T(H1, W) (((H1) + 1) * (W))
#define BSX_TORSO_W3T(H2) (((H2) + 1) * 4)
#define BSX_TORSO_LDS_FLOATS(D, H1, H2, W) (BSX_TORSO_W2T(H1, W) + BSX_TORSO_W3T(H2) + BSX_MLP2_W1(D, H1))
#define BSX_TORSO_ROUNDS(n) (((n) + BSX_BLOCK - 1) / BSX_BLOCK)
static inline int bsx_torso_width(int hidden2) { return hidden2 <= 16 ? 16 : hidden2 <= 32 ? 32 : 64; }

// The arguments through the kernarg segment, read where they are used (bsx_linear_view has the reason).
typedef const BSX_KERNARG bsx_torso_args* bsx_torso_kernarg;
__device__ __forceinline__ const bsx_torso_args& bsx_torso_view(bsx_torso_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_torso_args*)ka;
}
// Which member of `fam` a family's body reads.
struct bsx_torso_cartpole {
  typedef cartpole_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_torso_args& k) { return k.fam.cartpole; }
};
struct bsx_torso_mountain_car {
  typedef mountain_car_env env;
  __device__ static __forceinline__ const env::args& of(const bsx_torso_args& k) { return k.fam.mountain_car; }
};

typedef float bsx_torso_quad __attribute__((ext_vector_type(4)));

// The staged triple as the walk reads it: every lane of a wave reads the same address (a broadcast).
template <int D>
struct bsx_torso_lds {
  bsx_lds_table s;                 // the segment, from an offset the compiler cannot trace to the step loop's outside
  int W, off3, off1;
  __device__ __forceinline__ void unit(int) {}
  __device__ __forceinline__ float w1(int j, int d) const { return s[off1 + j * (D + 1) + d]; }
  // w2[4q .. 4q+3][j] (j == H1: the biases)
  __device__ __forceinline__ bsx_torso_quad w2(int j, int q) {
    return *(const bsx_torso_quad __attribute__((address_space(3)))*)(s + j * W + q * 4);
  }
  // w3[0..2][k] (k == H2: the biases)
  __device__ __forceinline__ bsx_torso_quad w3(int k) const {
    return *(const bsx_torso_quad __attribute__((address_space(3)))*)(s + off3 + k * 4);
  }
};
// ... and a lane's own triple in global memory, as the caller laid it out: the same walk, a load per weight.  The k-run of a
// fixed j has stride H1 + 1: the walk calls w2(j, 0), w2(j, 1), ... in this order after unit(j), and the element index runs
// along with it in a vector register, clamped to k = H2 - 1 — an accumulator k >= H2 (never read) takes that row's weights,
// so that every load is inside the matrix.  (Stride and clamp are refreshed per hidden unit: traced to the walk's outside,
// the W uniform offsets k * (H1 + 1) would be live across it, more scalar registers than the step loop leaves.)
template <int D>
struct bsx_torso_global {
  const float* __restrict__ g1;
  const float* __restrict__ g2;
  const float* __restrict__ g3;
  int H2, stride, k_max;           // stride = H1 + 1, k_max = H2 - 1
  uint32_t at, at_max;             // the element of w2 the next load reads, and the last one of this j
  __device__ __forceinline__ void unit(int j) {
    asm volatile("" : "+s"(stride), "+s"(k_max));
    at = bsx_fresh((uint32_t)j);
    at_max = at + (uint32_t)(k_max * stride);
  }
  __device__ __forceinline__ float w1(int j, int d) const { return g1[j * (D + 1) + d]; }
  __device__ __forceinline__ bsx_torso_quad w2(int, int) {
    bsx_torso_quad v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = g2[at];
      at = at + (uint32_t)stride < at_max ? at + (uint32_t)stride : at_max;
    }
    return v;
  }
  __device__ __forceinline__ bsx_torso_quad w3(int k) const {
    bsx_torso_quad v;
#pragma unroll
    for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) v[a] = g3[a * (H2 + 1) + k];
    v[3] = 0.0f;
    return v;
  }
};

// The greedy action of row o[] under a triple read through `Tab`: bsx_mlp2_select's walk in the kernel's pieces (bsx_mlp2.h).
// j runs outside: hidden unit j of layer 1 is consumed where it is produced, by W layer-2 accumulators that stay in
// registers across the walk — every index into acc[] is a compile-time constant.  Accumulators k >= H2 see zero weights and
// are never read.  Layer 3 consumes accumulator k where its ReLU is taken: three logit accumulators.
//   KEEP   the drawn mode: the three logits (bsx_mlp2_logits' values, bit for bit) are copied to keep[]; the greedy bodies
//          instantiate the walk without it, as it was before that mode.
template <int D, int W, bool KEEP = false, class Tab>
__device__ __forceinline__ int32_t bsx_torso_action(Tab& t, const int H1, const int H2, const float* o, float* keep = nullptr) {
  float acc[W];
  t.unit(H1);
#pragma unroll
  for (int q = 0; q < W / 4; ++q) {
    const bsx_torso_quad b = t.w2(H1, q);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[q * 4 + c] = b[c];
  }
#pragma unroll 1
  for (int j = 0; j < H1; ++j) {
    float w1j[D + 1];
    t.unit(j);
#pragma unroll
    for (int d = 0; d <= D; ++d) w1j[d] = t.w1(j, d);
    const float h = bsx_mlp_hidden(w1j, o, D);
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      const bsx_torso_quad v = t.w2(j, q);
      const float w2j[4] = {v[0], v[1], v[2], v[3]};
      bsx_mlp2_accumulate(acc + q * 4, w2j, h, 4);
    }
  }
  float l[BSX_LINEAR_ACTIONS];
  {
    const bsx_torso_quad b = t.w3(H2);
#pragma unroll
    for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) l[a] = b[a];
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (k < H2) {                                                          // uniform (a `break` keeps the loop rolled: acc[] in scratch)
      const bsx_torso_quad v = t.w3(k);
      const float w3k[BSX_LINEAR_ACTIONS] = {v[0], v[1], v[2]};
      bsx_mlp_accumulate(l, w3k, bsx_mlp_relu(acc[k]));
    }
  }
  if constexpr (KEEP) {
#pragma unroll
    for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) keep[a] = l[a];
  }
  return bsx_mlp_argmax(l);
}

// ... at the launch's width: a uniform switch, taken per step.
template <int D, bool KEEP = false, class Tab>
__device__ __forceinline__ int32_t bsx_torso_action_of(Tab& t, const int W, const int H1, const int H2, const float* o,
                                                       float* keep = nullptr) {
  if (W == 16) return bsx_torso_action<D, 16, KEEP>(t, H1, H2, o, keep);
  if (W == 32) return bsx_torso_action<D, 32, KEEP>(t, H1, H2, o, keep);
  return bsx_torso_action<D, 64, KEEP>(t, H1, H2, o, keep);
}

// Stages a shared triple (bsx_torso_lds's layout) for a row length D that is uniform but not a compile-time constant here:
// the kernel stages once, before it takes its switch.  Straight-line rounds of one element per thread, no loop.
__device__ __forceinline__ void bsx_torso_stage(const bsx_torso_args& k, const int D, float* s_w) {
  const int H1 = k.p.hidden1, H2 = k.p.hidden2, W = k.p.width;
  const int shift = W == 16 ? 4 : W == 32 ? 5 : 6;
  const int n2 = BSX_TORSO_W2T(H1, W), n3 = BSX_TORSO_W3T(H2), n1 = BSX_MLP2_W1(D, H1);
#pragma unroll
  for (int r = 0; r < BSX_TORSO_ROUNDS(BSX_TORSO_W2T(BSX_MLP_MAX_HIDDEN, BSX_MLP_MAX_HIDDEN)); ++r) {
    const int e = r * BSX_BLOCK + (int)threadIdx.x;
    const int j = e >> shift, c = e & (W - 1);
    if (e < n2) s_w[e] = c < H2 ? k.p.w2[c * (H1 + 1) + j] : 0.0f;
  }
#pragma unroll
  for (int r = 0; r < BSX_TORSO_ROUNDS(BSX_TORSO_W3T(BSX_MLP_MAX_HIDDEN)); ++r) {
    const int e = r * BSX_BLOCK + (int)threadIdx.x;
    const int c = e >> 2, a = e & 3;
    if (e < n3) s_w[n2 + e] = a < BSX_LINEAR_ACTIONS ? k.p.w3[a * (H2 + 1) + c] : 0.0f;
  }
#pragma unroll
  for (int r = 0; r < BSX_TORSO_ROUNDS(BSX_MLP2_W1(BSX_LINEAR_MAX_OBS, BSX_MLP_MAX_HIDDEN)); ++r) {
    const int e = r * BSX_BLOCK + (int)threadIdx.x;
    if (e < n1) s_w[n2 + n3 + e] = k.p.w1[e];
  }
}

// evaluate_mlp2(T) / rollout_mlp2(T), and with DRAWN evaluate_sampled_mlp2(T) / sample_mlp2(T).
// Around the policy this is bsx_mlp_returns_body (RECORD = false) and
// bsx_trajectory_body (RECORD = true): state in Env::regs, the info columns in registers, Env::core on the registers, resets
// computed in line, LAST / FIRST counted per thread and pooled once, state and info stored after the loop; per step either
// bsx_eval_accumulate or the trajectory's stores — reward / discount from bsx_emit_values' lean instantiation, step_type, the
// row (bsx_trajectory_store_row) and the action, each at {the step's slab: kernarg base + t * B elements, on the scalar
// unit} + {the lane's 32-bit byte offset} (the entry points refuse a [B, D] slab of 4 GiB or more).  Nothing the kernel
// stores is read back.
//   V       the family's variant (Env::numel_of(V) floats per row: cartpole 0 classic / 1 swing-up)
//   SHARED  one triple for all lanes (n_policies == 1): staged in LDS by the kernel before this body and read from there
//           every step; else the lane's own, read from global memory inside the step (lanes grouped by policy share loads).
//   DRAWN   the action is a draw from softmax(logits * beta) by Gumbel-max over the walk's three logits (bsx_gumbel.h), as in
//           bsx_gumbel_body: block 0 of stream BSX_STREAM_SAMPLE of (p.explore_seed, lane, step), nothing drawn and action
//           0 on a step that resets; no epsilon coin.  A compile-time mode: the greedy bodies' instruction streams are what
//           they were without it.
// The arguments are read through three views (bsx_torso_view): one before the loop, one per step, one after the loop.
// No barrier, no atomic and no LDS write inside the loop.
// (The skeleton — prologue, coin, per-step stores, the n_first rule, epilogue — is the third copy of those two bodies': keep
// the three alike.)
template <class Fam, int V, bool SHARED, bool RECORD, bool DRAWN = false>
__device__ __forceinline__ void bsx_torso_body(bsx_torso_kernarg ka, float* s_w, unsigned int* s_cnt) {
  typedef typename Fam::env Env;
  constexpr int D = Env::numel_of(V);
  static_assert(D <= BSX_LINEAR_MAX_OBS, "row length");
  const bsx_torso_args& k0 = bsx_torso_view(ka);
  const typename Env::args& a0 = Fam::of(k0);
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
    int32_t row = 0;                                                     // the lane's triple: all of the policy that stays live
    if constexpr (!SHARED) row = bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies);
    (void)row;
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
    (void)e;
    const uint32_t iu0 = (uint32_t)i;
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_torso_args& kt = bsx_torso_view(ka);
      const typename Env::args& a = Fam::of(kt);
      const bsx_torso_policy& p = kt.p;
      const uint64_t step = step0 + (uint64_t)t;
      const int resets = Env::reset_pending(rg) ? 1 : 0;
      const int H1 = p.hidden1, H2 = p.hidden2, W = p.width;               // 1 .. BSX_MLP_MAX_HIDDEN (the entry points check)
      int32_t best;
      float l[BSX_LINEAR_ACTIONS];                                         // DRAWN: the walk's logits
      (void)l;
      if constexpr (SHARED) {
        // (from an offset the compiler cannot trace to the loop's outside: bsx_mlp_returns_body; in units of 16 bytes, so
        // that the alignment of the rows stays visible)
        bsx_torso_lds<D> tab;
        tab.s = (bsx_lds_table)s_w + bsx_fresh(0u) * 4u;
        tab.W = W; tab.off3 = BSX_TORSO_W2T(H1, W); tab.off1 = tab.off3 + BSX_TORSO_W3T(H2);
        if constexpr (DRAWN) best = bsx_torso_action_of<D, true>(tab, W, H1, H2, o, l);
        else best = bsx_torso_action_of<D>(tab, W, H1, H2, o);
      } else {
        bsx_torso_global<D> tab;
        tab.g1 = p.w1 + (int64_t)row * BSX_MLP2_W1(D, H1);
        tab.g2 = p.w2 + (int64_t)row * BSX_MLP2_W2(H1, H2);
        tab.g3 = p.w3 + (int64_t)row * BSX_MLP2_W3(H2);
        tab.H2 = H2; tab.stride = H1 + 1; tab.k_max = H2 - 1;
        if constexpr (DRAWN) best = bsx_torso_action_of<D, true>(tab, W, H1, H2, o, l);
        else best = bsx_torso_action_of<D>(tab, W, H1, H2, o);
      }
      (void)best;
      int act = 0;
      if constexpr (DRAWN) {
        // bsx_gumbel_body's decision: a lane that resets on this step takes action 0 and draws nothing.  (The action pinned
        // where it is drawn: bsx_drawn_returns_body has the reason.)
        if (!resets) {
          const bsx_u32x4 u = bsx_gumbel_draws(p.explore_seed, lane, step);
          act = (int32_t)bsx_fresh((uint32_t)bsx_gumbel_select(l, kt.beta, u.v[0], u.v[1], u.v[2]));
        }
      } else {
        uint32_t w0 = 0, w1 = 0, w2 = 0;
        if (p.epsilon > 0.0 && !resets) {
          const bsx_u32x4 u = bsx_policy_draws(p.explore_seed, lane, step);
          w0 = u.v[0]; w1 = u.v[1]; w2 = u.v[2];
        }
        act = bsx_policy_select((uint32_t)best, resets, p.epsilon, w0, w1, w2, BSX_LINEAR_ACTIONS);
      }
      double reward = 0.0;
      const int type = Env::template core<0, 0, true, false, false, V, true>(a, rg, act, i, lane, step, o, reward);
      if constexpr (!RECORD) {
        bsx_eval_accumulate(&e, type, reward);
      } else {
        n_last += type == BSX_LAST ? 1u : 0u;
        // the step's outputs, as bsx_trajectory_body stores them: t * B on the scalar unit, the lane's byte offsets from a
        // value the optimiser cannot hoist
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
    }
    // every LAST is followed by a FIRST except one at the call's final step, and a lane that arrives with its reset
    // pending begins with one (small_obs_regs_rollout)
    if constexpr (!RECORD) n_last = (uint32_t)e.n;
    n_first = n_last + pending_in - (Env::reset_pending(rg) ? 1u : 0u);
    const bsx_torso_args& k1 = bsx_torso_view(ka);
    const typename Env::args& a1 = Fam::of(k1);
    Env::store(a1, i, rg);
    Env::template store_info<V>(a1, i, rg);
    if constexpr (!RECORD) {
      k1.ev.episodes[i] = e.n;
      k1.ev.return_sum[i] = e.total;
      k1.ev.episode_return_sum[i] = e.done;
      small_obs_store_row<false>(k1.ev.observation_out + i * D, o, D);
    }
  }
  bsx_pool_counts(Fam::of(bsx_torso_view(ka)).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_torso_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_torso(const bsx_torso_args& a, hipStream_t st);

// The refusals of the four entry points that do not depend on the family: bsx_check_mlp_call's, in its order — modes,
// scalars, then, for a call with lanes, pointers.  A hidden1 or hidden2 outside [1, BSX_MLP_MAX_HIDDEN] is reported where
// `hidden` is there, and w3 is one more pointer a call with lanes needs.  (`extra` as there.)
static inline int bsx_check_mlp2_call(const bsx_call_t* call, const bsx_mlp2_t* m, const float* state, const int32_t* steps,
                                      bool outputs_present, const double* info, const void* extra) {
  const bool hidden_ok = m->hidden1 >= 1 && m->hidden1 <= BSX_MLP_MAX_HIDDEN && m->hidden2 >= 1 && m->hidden2 <= BSX_MLP_MAX_HIDDEN;
  const bsx_mlp_t one = {m->w1, m->w2, hidden_ok ? 1 : 0, m->n_policies, m->policy_index, m->epsilon, m->explore_seed,
                         m->observation_in};
  return bsx_check_mlp_call(call, &one, state, steps, outputs_present, info, m->w3 != nullptr ? extra : nullptr);
}

// ... and of the four sampled entry points (bsx_<family>_mlp2_sample, bsx_<family>_mlp2_sample_evaluate): the same, for the
// policy under the drawn rule (bsx_drawn_policy, bsx_linear_score.h).
static inline int bsx_check_mlp2_sample_call(const bsx_call_t* call, const bsx_mlp2_t* m, double inv_temperature, const float* state,
                                             const int32_t* steps, bool outputs_present, const double* info, const void* extra) {
  const bsx_mlp2_t q = bsx_drawn_policy(m, inv_temperature);
  return bsx_check_mlp2_call(call, &q, state, steps, outputs_present, info, extra);
}

// What the entry points share once the family's args are in place: `ev` for an evaluation (out / actions_out unused),
// `out` and `actions_out` for a recording call; `mode` BSX_TORSO_GREEDY (inv_temperature unused) or BSX_TORSO_DRAWN
// (m->explore_seed is the sample seed, m->epsilon is 0.0).
static inline int bsx_torso_call(bsx_torso_args& a, int32_t family, const bsx_call_t* call, const bsx_mlp2_t* m, int32_t mode,
                                 double inv_temperature, bool record, const bsx_linear_eval_t& ev, const bsx_timestep_t& out,
                                 int32_t* actions_out) {
  a.family = family;
  a.n_steps = call->n_steps;
  a.mode = mode;
  a.record = record ? 1 : 0;
  a.p.w1 = m->w1; a.p.w2 = m->w2; a.p.w3 = m->w3;
  a.p.policy_index = m->n_policies > 1 ? m->policy_index : nullptr;
  a.p.observation_in = m->observation_in;
  a.p.epsilon = mode == BSX_TORSO_DRAWN ? 0.0 : m->epsilon;
  a.p.explore_seed = m->explore_seed;
  a.p.n_policies = m->n_policies; a.p.hidden1 = m->hidden1; a.p.hidden2 = m->hidden2;
  a.p.width = bsx_torso_width(m->hidden2);
  a.ev = ev; a.out = out; a.actions_out = actions_out;
  a.beta = mode == BSX_TORSO_DRAWN ? inv_temperature : 1.0;
  return bsx_launch_torso(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_mlp2_evaluate / _mlp2_rollout (BSX_TORSO_GREEDY) and _mlp2_sample_evaluate / _mlp2_sample (BSX_TORSO_DRAWN), returns
// only or recorded (Fam: the family's host trait, bsx_host.h).  A recording call refuses last what bsx_check_trajectory_call
// refuses last: the 4 GiB slab.
template <class Fam>
static inline int bsx_torso_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2, int32_t mode,
                                  double inv_temperature, float* state, int32_t* steps, bool record, const bsx_linear_eval_t& ev,
                                  const bsx_timestep_t& out, int32_t* actions_out, double* info) {
  bsx_torso_args e;
  return bsx_physics_closed_loop<Fam>(
      cfg, call, mlp2, state, steps, info, e.fam,
      [&](const void* extra, int D) {
        const bool present = record ? bsx_trajectory_outputs_present(out, actions_out) : bsx_linear_eval_present(ev);
        const int rc = mode == BSX_TORSO_DRAWN ? bsx_check_mlp2_sample_call(call, mlp2, inv_temperature, state, steps, present, info, extra)
                                               : bsx_check_mlp2_call(call, mlp2, state, steps, present, info, extra);
        return record ? bsx_check_trajectory_slab(rc, call, D) : rc;
      },
      [&](int32_t family) { return bsx_torso_call(e, family, call, mlp2, mode, inv_temperature, record, ev, out, actions_out); });
}

#endif  // BSX_TORSO_H_
