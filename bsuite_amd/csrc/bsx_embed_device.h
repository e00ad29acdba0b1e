// bsx_embed_device.h — bsx_<family>_embedding_rollout / bsx_<family>_embedding_evaluate (rollout_embedding,
// evaluate_embedding): the arguments of the ONE kernel that serves deep_sea and catch, recording or returns only
// (bsx_embed_kernel, embed.hip), the two bodies of its step loop, its launcher and the checks the four entry points share.
// The closed loops of bsx_policy_rollout_kernel and bsx_tab_eval_body (bsx_pair_device.h) with another action SOURCE: instead
// of a uint8 table entry the lane takes the greedy action of a one-hidden-layer network on its index row (bsx_embed.h); the
// epsilon coin behind it is bsx_policy_select's, unchanged.  bsx_<family>_embedding_sample / _embedding_sample_evaluate
// (sample_embedding, evaluate_sampled_embedding) are the same kernel with a third uniform switch: the lane takes a draw from
// softmax(logits / temperature) of the same network by Gumbel-max (bsx_embed_sample.h) — no epsilon there.
#ifndef BSX_EMBED_DEVICE_H_
#define BSX_EMBED_DEVICE_H_

#include "bsx_pair_host.h"
#include "bsx_embed_sample.h"         // bsx_embed.h, bsx_tab_sample.h (bsx_gumbel_draws, bsx_gumbel_select_n)
#include "catch_fam.h"
#include "deep_sea_fam.h"

// The pair of matrices, flattened out of bsx_policy_embedding_t on the host.
struct bsx_embed_net_args {
  const float* w1;               // [n_policies, n_cells + 2, n_hidden]; 4-byte aligned, no more
  const float* w2;               // [n_policies, A, n_hidden + 1]; 4-byte aligned, no more
  const int32_t* policy_index;   // [n_lanes], nullptr when n_policies == 1
  int32_t* actions_out;          // [n_steps, n_lanes] (the recording call's alone)
  double epsilon;                // (greedy)
  uint64_t explore_seed;         // (greedy)
  double beta;                   // (drawn) 1 / temperature: finite, > 0 (the entry points check)
  uint64_t sample_seed;          // (drawn)
  int32_t n_cells, n_hidden, n_policies;
  int32_t in_lds;                // one shared pair whose copy fits BSX_EMBED_LDS_BYTES: every workgroup stages it in LDS
};

// The family and the kind of call are uniform switches per launch, so the arguments are a tagged struct: `family` says which
// member of `fam` is set, `record` which of `rows` (with fam's TimeStep pointers and p.actions_out) and `out` is written,
// `drawn` which of p's (epsilon, explore_seed) and (beta, sample_seed) is read.
struct bsx_embed_args {
  int32_t family;                // BSX_FAM_DEEP_SEA or BSX_FAM_CATCH
  int32_t n_steps;
  int32_t record;                // 1: rollout_embedding (TimeStep, index rows, actions); 0: evaluate_embedding (returns only)
  int32_t drawn;                 // 1: sample_embedding / evaluate_sampled_embedding (Gumbel-max); 0: greedy with an epsilon coin
  bsx_embed_net_args p;
  int32_t* rows;                 // [n_steps, n_lanes, K] index observations (record)
  bsx_policy_eval_t out;         // (returns only)
  union {
    deep_sea_fam::args deep_sea;
    catch_fam::args catch_;
  } fam;
};

// The kernel's arguments where the launch put them — the kernarg segment — through a pointer the optimiser cannot trace: what
// is read through it is loaded where it is used, by s_load, and lives in scalar registers from there to its last use only
// (bsx_tab_softmax_view, bsx_tab_sample_device.h, and bsx_linear_view, bsx_linear_score.h, have the measurements).
#if defined(__HIP_DEVICE_COMPILE__)
#define BSX_EMBED_KERNARG __attribute__((address_space(4)))
#else
#define BSX_EMBED_KERNARG          /* (the host pass only parses the device functions) */
#endif
typedef const BSX_EMBED_KERNARG bsx_embed_args* bsx_embed_kernarg;
__device__ __forceinline__ const bsx_embed_args& bsx_embed_view(bsx_embed_kernarg ka) {
  asm volatile("" : "+s"(ka));
  return *(const bsx_embed_args*)ka;
}
// Which member of `fam` a family's body reads, its decoder, the entries of its index row and its number of actions.
struct bsx_embed_deep_sea {
  typedef deep_sea_fam fam;
  typedef deep_sea_hot hot;
  static constexpr int K = 1, A = 2;
  __device__ static __forceinline__ const fam::args& of(const bsx_embed_args& k) { return k.fam.deep_sea; }
  __device__ static __forceinline__ hot fn(const fam::args& a) { return hot{a.size}; }
};
struct bsx_embed_catch {
  typedef catch_fam fam;
  typedef catch_hot hot;
  static constexpr int K = 2, A = 3;
  __device__ static __forceinline__ const fam::args& of(const bsx_embed_args& k) { return k.fam.catch_; }
  __device__ static __forceinline__ hot fn(const fam::args& a) { return hot{a.rows, a.columns}; }
};
// The action source of a body: the greedy action behind an epsilon coin, or — bsx_embed_drawn<family> — a draw from the softmax.
struct bsx_embed_greedy {};
struct bsx_embed_gumbel {};
template <class F>
struct bsx_embed_drawn : F {};
template <class F>
struct bsx_embed_source_of { typedef bsx_embed_greedy type; };
template <class F>
struct bsx_embed_source_of<bsx_embed_drawn<F>> { typedef bsx_embed_gumbel type; };

// The pair staged in LDS, typed as such and read in 16-byte chunks: through a generic pointer the look-up would be a FLAT
// load (bsx_policy_rollout_kernel has what that costs).
typedef const bsx_f4 __attribute__((address_space(3)))* bsx_embed_lds4;

// The greedy action of a lane that does not reset: cells -> rows of w1 -> the hidden units, consumed as they are produced ->
// argmax — or, for Source = bsx_embed_gumbel, the lane's draw: the same logits -> block 0 of stream BSX_STREAM_SAMPLE ->
// bsx_gumbel_select_n (the float64 scores come after the hidden-unit loop, when only the A logits are live).  The two
// look-ups are two branches, kept apart by the empty asm, and never one load through a generic pointer:
//   LDS     16-byte typed loads from the staged copy (bsx_embed.h has its layout): per four hidden units one chunk of each of
//           the lane's K rows, one of the bias row (the same address in every lane: a broadcast) and four of the transposed
//           w2 (broadcasts too).  The floats of a chunk beyond H are padding that is never looked at.
//   global  typed 4-byte loads from the lane's own pair (`prow`: its row of a population, 0 for a shared pair) — no wider
//           alignment than a float's is assumed.
template <int K, int A, class Source = bsx_embed_greedy, class HotFn>
__device__ __forceinline__ int bsx_embed_best(const HotFn& fn, int32_t st, const bsx_embed_net_args& p, const float* s_net, int prow,
                                              uint64_t lane = 0, uint64_t step = 0) {
  static_assert(K >= 1 && K <= BSX_EMBED_MAX_K && A >= 2 && A <= BSX_EMBED_MAX_ACTIONS, "deep_sea or catch");
  const int C = p.n_cells, H = p.n_hidden;
  int cell[2];
  fn(st, cell[0], cell[1]);
  int row[K];
#pragma unroll
  for (int k = 0; k < K; ++k) row[k] = bsx_embed_row(cell[k], C);
  float l[A];
  if (p.in_lds != 0) {                                                    // uniform
    const int S4 = BSX_EMBED_STRIDE(H) >> 2;                              // chunks of a staged row
    bsx_embed_lds4 base = (bsx_embed_lds4)s_net;
    bsx_embed_lds4 bias = base + (C + 1) * S4;
    bsx_embed_lds4 t = base + (C + 2) * S4;                               // t[j] = {w2[0][j], w2[1][j], w2[2][j], -}
    bsx_embed_lds4 e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = base + row[k] * S4;
    const bsx_f4 lb = t[H];
#pragma unroll
    for (int a = 0; a < A; ++a) l[a] = lb[a];
#pragma unroll 1
    for (int j = 0; j < H; j += 4) {
      const bsx_f4 b = bias[j >> 2];
      bsx_f4 ev[K];
#pragma unroll
      for (int k = 0; k < K; ++k) ev[k] = e[k][j >> 2];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (j + c < H) {                                                  // uniform
          const bsx_f4 w = t[j + c];
          float ek[K], w2j[A];
#pragma unroll
          for (int k = 0; k < K; ++k) ek[k] = ev[k][c];
#pragma unroll
          for (int a = 0; a < A; ++a) w2j[a] = w[a];
          bsx_embed_accumulate(l, w2j, bsx_mlp_relu(bsx_embed_preactivation(b[c], ek, K)), A);
        }
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int a = 0; a < A; ++a) asm volatile("" : "+v"(l[a]));
#endif
  } else {
    const float* __restrict__ g1 = p.w1 + (int64_t)prow * BSX_EMBED_W1(C, H);
    const float* __restrict__ g2 = p.w2 + (int64_t)prow * BSX_EMBED_W2(A, H);
    const float* __restrict__ gb = g1 + (int64_t)(C + 1) * H;
    const float* __restrict__ ge[K];
#pragma unroll
    for (int k = 0; k < K; ++k) ge[k] = g1 + (int64_t)row[k] * H;
#pragma unroll
    for (int a = 0; a < A; ++a) l[a] = g2[a * (H + 1) + H];
#pragma unroll 4
    for (int j = 0; j < H; ++j) {
      float ek[K], w2j[A];
#pragma unroll
      for (int k = 0; k < K; ++k) ek[k] = ge[k][j];
#pragma unroll
      for (int a = 0; a < A; ++a) w2j[a] = g2[a * (H + 1) + j];
      bsx_embed_accumulate(l, w2j, bsx_mlp_relu(bsx_embed_preactivation(gb[j], ek, K)), A);
    }
  }
  if constexpr (__is_same(Source, bsx_embed_gumbel)) {
    const bsx_u32x4 u = bsx_gumbel_draws(p.sample_seed, lane, step);
    return bsx_gumbel_select_n(l, A, p.beta, u.v);
  }
  return bsx_embed_argmax(l, A);
}

// The action of a lane that does not reset: the greedy action, then rollout_policy's epsilon coin on block 0 of stream
// BSX_STREAM_POLICY — with epsilon == 0 (uniform per launch) no Philox is executed.
template <int K, int A, class HotFn>
__device__ __forceinline__ int bsx_embed_action(bsx_embed_greedy, const HotFn& fn, int32_t st, const bsx_embed_net_args& p, const float* s_net,
                                                int prow, uint64_t lane, uint64_t step) {
  const int best = bsx_embed_best<K, A>(fn, st, p, s_net, prow);
  uint32_t w0 = 0, w1 = 0, w2 = 0;
  if (p.epsilon > 0.0) {
    const bsx_u32x4 w = bsx_policy_draws(p.explore_seed, lane, step);
    w0 = w.v[0]; w1 = w.v[1]; w2 = w.v[2];
  }
  return bsx_policy_select((uint32_t)best, /*resets=*/0, p.epsilon, w0, w1, w2, (uint32_t)A);
}
// ... and of a drawn call: the draw itself, no coin.  The action is NOT pinned behind an opaque asm as bsx_drawn_returns_body
// pins its own: no scalar spills here without it, and an opaque action is one the compiler can no longer prove inside
// [0, A) — deep_sea's count of invalid actions (a global atomic) would come back into the step loop.
template <int K, int A, class HotFn>
__device__ __forceinline__ int bsx_embed_action(bsx_embed_gumbel, const HotFn& fn, int32_t st, const bsx_embed_net_args& p, const float* s_net,
                                                int prow, uint64_t lane, uint64_t step) {
  return bsx_embed_best<K, A, bsx_embed_gumbel>(fn, st, p, s_net, prow, lane, step);
}

// What both bodies do before their loop: the counters, the family's own staging, the shared pair into LDS, one barrier.
template <class Fam, int A>
__device__ __forceinline__ void bsx_embed_stage(const typename Fam::args& a, const bsx_embed_net_args& p, typename Fam::shared& s_fam,
                                                unsigned int* s_cnt, float* s_net) {
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  Fam::stage(a, s_fam);
  if (p.in_lds != 0) {                                  // uniform; BSX_EMBED_STAGED_BYTES(C, H) <= BSX_EMBED_LDS_BYTES
    const int H = p.n_hidden, S = BSX_EMBED_STRIDE(H), R = p.n_cells + 2;
    for (int k = threadIdx.x; k < R * H; k += BSX_BLOCK) {
      const int r = k / H;
      s_net[r * S + (k - r * H)] = p.w1[k];
    }
    float* t = s_net + R * S;
    for (int k = threadIdx.x; k < A * (H + 1); k += BSX_BLOCK) {
      const int r = k / (H + 1);
      t[(k - r * (H + 1)) * 4 + r] = p.w2[k];
    }
  }
  __syncthreads();
}

// Lane i's row of a population, clamped — a bad index cannot fault; 0 for a shared pair.
__device__ __forceinline__ int bsx_embed_prow(const bsx_embed_net_args& p, int64_t i) {
  if (p.policy_index == nullptr) return 0;
  return bsx_policy_clamp(p.policy_index[i], p.n_policies);
}

// rollout_embedding(T): the loop of bsx_policy_rollout_kernel.  State word in a register from its load to its store, LAST /
// FIRST counted per thread and pooled once, per step the scalars, the index row and the action stored non-temporally: [T,B]
// outputs have no reader inside the call.  Nothing is computed and nothing is drawn on a step that resets.  The arguments are
// read through three views: one before the loop, one per step, one after the loop.
template <class F>
__device__ __forceinline__ void bsx_embed_record_body(bsx_embed_kernarg ka, typename F::fam::shared& s_fam, unsigned int* s_cnt,
                                                      float* s_net) {
  typedef typename F::fam Fam;
  typedef typename bsx_embed_source_of<F>::type Source;
  const bsx_embed_args& k0 = bsx_embed_view(ka);
  const typename Fam::args& a0 = F::of(k0);
  bsx_embed_stage<Fam, F::A>(a0, k0.p, s_fam, s_cnt, s_net);
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
    const int prow = bsx_embed_prow(k0.p, i);
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_embed_args& kt = bsx_embed_view(ka);
      const typename Fam::args& a = F::of(kt);
      const typename F::hot fn = F::fn(a);
      const uint64_t step = step0 + (uint64_t)t;
      const int64_t oi = (int64_t)t * a.ctl.n_lanes + i;
      const bool resets = Fam::resets(st);
      int act = 0;
      if (!resets) act = bsx_embed_action<F::K, F::A>(Source(), fn, st, kt.p, s_net, prow, lane, step);
      int32_t nst; double reward;
      const int type = Fam::template advance<true>(a, s_fam, i, lane, step, st, act, nst, reward);
      st = nst;
      bsx_emit_at<0, 0, false, -1, BSX_OUT_SCALARS.rollout>(a.ctl, a.out, i, oi, lane, step, type, reward);
      bsx_index_store<BSX_OUT_INDEX.rollout>(kt.rows, oi, nst, fn);
      bsx_st<BSX_OUT_SCALARS.rollout>(&kt.p.actions_out[oi], (int32_t)act);
      n_last += type == BSX_LAST ? 1u : 0u;
      n_first += type == BSX_FIRST ? 1u : 0u;
    }
    F::of(bsx_embed_view(ka)).state[i] = st;
  }
  bsx_pool_counts(F::of(bsx_embed_view(ka)).ctl, n_last, n_first, s_cnt, block_id & (BSX_COUNTER_SHARDS - 1));
}

// evaluate_embedding(T): the loop of bsx_tab_eval_body — the same steps with the same draws, every per-step store removed.
// State word, the three f64 sums, the episode count and the info columns' deltas stay in registers (bsx_eval_accumulate,
// Fam::advance_deferred) and are stored after the loop: no store and no barrier inside it.
template <class F>
__device__ __forceinline__ void bsx_embed_returns_body(bsx_embed_kernarg ka, typename F::fam::shared& s_fam, unsigned int* s_cnt,
                                                       float* s_net) {
  typedef typename F::fam Fam;
  typedef typename bsx_embed_source_of<F>::type Source;
  const bsx_embed_args& k0 = bsx_embed_view(ka);
  const typename Fam::args& a0 = F::of(k0);
  bsx_embed_stage<Fam, F::A>(a0, k0.p, s_fam, s_cnt, s_net);
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  const bool mine = i < a0.ctl.n_lanes;
  const uint64_t lane = a0.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a0.ctl);
  const int n_steps = k0.n_steps;
  uint32_t n_last = 0, n_first = 0;
  if (mine) {
    int32_t st = a0.state[i];
    const int prow = bsx_embed_prow(k0.p, i);
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
    typename Fam::deferred pend = {};
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
      const bsx_embed_args& kt = bsx_embed_view(ka);
      const typename Fam::args& a = F::of(kt);
      const uint64_t step = step0 + (uint64_t)t;
      const bool resets = Fam::resets(st);
      int act = 0;
      if (!resets) act = bsx_embed_action<F::K, F::A>(Source(), F::fn(a), st, kt.p, s_net, prow, lane, step);
      int32_t nst; double reward;
      const int type = Fam::advance_deferred(a, s_fam, i, lane, step, st, act, nst, reward, pend);
      st = nst;
      bsx_eval_accumulate(&e, type, reward);
      n_first += type == BSX_FIRST ? 1u : 0u;
    }
    n_last = (uint32_t)e.n;
    const bsx_embed_args& k1 = bsx_embed_view(ka);
    const typename Fam::args& a1 = F::of(k1);
    a1.state[i] = st;
    k1.out.episodes[i] = e.n;
    k1.out.return_sum[i] = e.total;
    k1.out.episode_return_sum[i] = e.done;
    Fam::commit_deferred(a1, i, pend);
  }
  bsx_pool_counts(F::of(bsx_embed_view(ka)).ctl, n_last, n_first, s_cnt, blockIdx.x);
}

// Launches bsx_embed_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_embed(const bsx_embed_args& a, hipStream_t st);

// The refusals of the four entry points that do not depend on the family: those of bsx_check_policy_call /
// bsx_check_policy_eval_call, in their order, for a bsx_policy_t that stands in for the pair of matrices — where they refuse
// n_states, BSX_EINVAL for n_cells or n_actions other than the family's and for n_hidden outside [1, BSX_MLP_MAX_HIDDEN]; the
// epsilon is the struct's own; after the pointers, BSX_EALIGN for w1 or w2 off the 4-byte grid.
static inline bsx_policy_t bsx_embed_stand_in(const bsx_policy_embedding_t* em, int32_t n_cells, int32_t n_actions) {
  bsx_policy_t q;
  q.table = reinterpret_cast<const uint8_t*>(em->w2 != nullptr ? em->w1 : nullptr);
  q.n_states = (em->n_cells == n_cells && em->n_actions == n_actions && em->n_hidden >= 1 && em->n_hidden <= BSX_MLP_MAX_HIDDEN) ? n_cells : -1;
  q.n_policies = em->n_policies;
  q.policy_index = em->policy_index;
  q.epsilon = em->epsilon;
  q.explore_seed = em->explore_seed;
  q.actions_out = em->actions_out;
  return q;
}
static inline int bsx_embed_aligned(const bsx_policy_embedding_t* em) {
  return ((reinterpret_cast<uintptr_t>(em->w1) | reinterpret_cast<uintptr_t>(em->w2)) & 3u) != 0 ? BSX_EALIGN : 0;
}
static inline int bsx_check_embed_call(const bsx_call_t* call, const bsx_policy_embedding_t* em, int32_t n_cells, int32_t n_actions,
                                       const int32_t* state, const bsx_timestep_t& out, const double* info) {
  if (call == nullptr || em == nullptr) return BSX_ENULL;
  const bsx_policy_t q = bsx_embed_stand_in(em, n_cells, n_actions);
  const int rc = bsx_check_policy_call(call, &q, n_cells, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  return bsx_embed_aligned(em);
}
static inline int bsx_check_embed_eval_call(const bsx_call_t* call, const bsx_policy_embedding_t* em, int32_t n_cells, int32_t n_actions,
                                            const int32_t* state, const bsx_policy_eval_t& out, const double* info) {
  if (call == nullptr || em == nullptr) return BSX_ENULL;
  const bsx_policy_t q = bsx_embed_stand_in(em, n_cells, n_actions);
  const int rc = bsx_check_policy_eval_call(call, &q, n_cells, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  return bsx_embed_aligned(em);
}

// The same refusals for the drawn calls (bsx_<family>_embedding_sample / _embedding_sample_evaluate): the sampled struct as a
// greedy one whose epsilon is 0.0 for an inv_temperature that is finite and > 0 and out of range for any other — BSX_ERANGE
// where the epsilon is refused, as in bsx_tab_softmax_stand_in.
static inline bsx_policy_embedding_t bsx_embed_sample_stand_in(const bsx_policy_embedding_sample_t* sm) {
  bsx_policy_embedding_t em;
  em.w1 = sm->w1; em.w2 = sm->w2;
  em.n_cells = sm->n_cells; em.n_hidden = sm->n_hidden; em.n_actions = sm->n_actions; em.n_policies = sm->n_policies;
  em.policy_index = sm->policy_index;
  em.epsilon = (__builtin_isfinite(sm->inv_temperature) && sm->inv_temperature > 0.0) ? 0.0 : 2.0;
  em.explore_seed = sm->sample_seed;
  em.actions_out = sm->actions_out;
  return em;
}
static inline int bsx_check_embed_sample_call(const bsx_call_t* call, const bsx_policy_embedding_sample_t* sm, int32_t n_cells,
                                              int32_t n_actions, const int32_t* state, const bsx_timestep_t& out, const double* info) {
  if (call == nullptr || sm == nullptr) return BSX_ENULL;
  const bsx_policy_embedding_t em = bsx_embed_sample_stand_in(sm);
  return bsx_check_embed_call(call, &em, n_cells, n_actions, state, out, info);
}
static inline int bsx_check_embed_sample_eval_call(const bsx_call_t* call, const bsx_policy_embedding_sample_t* sm, int32_t n_cells,
                                                   int32_t n_actions, const int32_t* state, const bsx_policy_eval_t& out,
                                                   const double* info) {
  if (call == nullptr || sm == nullptr) return BSX_ENULL;
  const bsx_policy_embedding_t em = bsx_embed_sample_stand_in(sm);
  return bsx_check_embed_eval_call(call, &em, n_cells, n_actions, state, out, info);
}

// What the entry points share once the family's args are in place (a.fam).
static inline int bsx_embed_fill_and_launch(bsx_embed_args& a, int32_t family, const bsx_call_t* call, const bsx_policy_embedding_t* em,
                                            bool record, bool drawn, double beta, int32_t* rows, const bsx_policy_eval_t& out) {
  if (bsx_blocks_of(call->n_lanes) > 0x7FFFFFFF) return BSX_EINVAL;
  a.family = family;
  a.n_steps = call->n_steps;
  a.record = record ? 1 : 0;
  a.drawn = drawn ? 1 : 0;
  a.p.w1 = em->w1;
  a.p.w2 = em->w2;
  a.p.policy_index = em->n_policies > 1 ? em->policy_index : nullptr;
  a.p.actions_out = record ? em->actions_out : nullptr;
  a.p.epsilon = drawn ? 0.0 : em->epsilon;
  a.p.explore_seed = drawn ? 0 : em->explore_seed;
  a.p.beta = beta;
  a.p.sample_seed = drawn ? em->explore_seed : 0;
  a.p.n_cells = em->n_cells; a.p.n_hidden = em->n_hidden; a.p.n_policies = em->n_policies;
  a.p.in_lds = (em->n_policies == 1 && BSX_EMBED_STAGED_BYTES(em->n_cells, em->n_hidden) <= BSX_EMBED_LDS_BYTES) ? 1 : 0;
  a.rows = rows;
  a.out = out;
  return bsx_launch_embed(a, (hipStream_t)call->hip_stream);
}
static inline int bsx_embed_call(bsx_embed_args& a, int32_t family, const bsx_call_t* call, const bsx_policy_embedding_t* em, bool record,
                                 int32_t* rows, const bsx_policy_eval_t& out) {
  return bsx_embed_fill_and_launch(a, family, call, em, record, false, 1.0, rows, out);
}
static inline int bsx_embed_sample_call(bsx_embed_args& a, int32_t family, const bsx_call_t* call, const bsx_policy_embedding_sample_t* sm,
                                        bool record, int32_t* rows, const bsx_policy_eval_t& out) {
  const bsx_policy_embedding_t em = bsx_embed_sample_stand_in(sm);
  return bsx_embed_fill_and_launch(a, family, call, &em, record, true, sm->inv_temperature, rows, out);
}

// bsx_<family>_embedding_rollout / _embedding_evaluate and _embedding_sample / _embedding_sample_evaluate: a recording call by
// its TimeStep, an evaluation by its three columns (Fam: the family's host trait, bsx_host.h).
template <class Fam>
static inline int bsx_embed_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                  int32_t* state, const bsx_timestep_t& out, double* info) {
  bsx_embed_args s;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, &out, info, Fam::of(s.fam),
      [&] { return bsx_check_embed_call(call, policy, Fam::cells(cfg), Fam::actions, state, out, info); },
      [&] { return bsx_embed_call(s, Fam::code, call, policy, true, reinterpret_cast<int32_t*>(out.observation), bsx_policy_eval_t{}); });
}
template <class Fam>
static inline int bsx_embed_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                  int32_t* state, const bsx_policy_eval_t& out, double* info) {
  bsx_embed_args s;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, nullptr, info, Fam::of(s.fam),
      [&] { return bsx_check_embed_eval_call(call, policy, Fam::cells(cfg), Fam::actions, state, out, info); },
      [&] { return bsx_embed_call(s, Fam::code, call, policy, false, nullptr, out); });
}
template <class Fam>
static inline int bsx_embed_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_sample_t* policy,
                                  int32_t* state, const bsx_timestep_t& out, double* info) {
  bsx_embed_args s;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, &out, info, Fam::of(s.fam),
      [&] { return bsx_check_embed_sample_call(call, policy, Fam::cells(cfg), Fam::actions, state, out, info); },
      [&] {
        return bsx_embed_sample_call(s, Fam::code, call, policy, true, reinterpret_cast<int32_t*>(out.observation), bsx_policy_eval_t{});
      });
}
template <class Fam>
static inline int bsx_embed_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_sample_t* policy,
                                  int32_t* state, const bsx_policy_eval_t& out, double* info) {
  bsx_embed_args s;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, nullptr, info, Fam::of(s.fam),
      [&] { return bsx_check_embed_sample_eval_call(call, policy, Fam::cells(cfg), Fam::actions, state, out, info); },
      [&] { return bsx_embed_sample_call(s, Fam::code, call, policy, false, nullptr, out); });
}

#endif  // BSX_EMBED_DEVICE_H_
