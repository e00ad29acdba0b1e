// deep_sea.hip — batched DeepSea for gfx950.  Replaces bsuite/environments/deep_sea.py:103-144
// (`_get_observation`, `_reset`, `_step`) plus the auto-reset of bsuite/environments/base.py:54-65.
//
// Shape of the work at the headline config (N=30, B=2^20): 21 B of scalar traffic and 3600 B of
// observation stores per lane per call — a pure store stream.  Two launches per call:
//   advance  bsx_advance_kernel<deep_sea_fam>: the N*N-bit action mapping goes kernarg -> LDS once
//            per block (lane-divergent `mapping[row,col]` lookup); every thread advances one
//            lane (coalesced column loads/stores of action / packed state / reward / discount /
//            step_type), LAST/FIRST masks by wavefront ballot;
//   observe  bsx_hot_stream_kernel<deep_sea_hot,4,256>: a pure store stream over [B x N*N] f32 —
//            block b writes floats [b*4096,(b+1)*4096) as 4 lane-interleaved 16-byte stores per
//            thread, hot cells recomputed from the packed state column (4 B/lane, L2-resident).
// (With bsx_call_t.obs_paint — the delta observation mode — the call is ONE launch instead,
//  bsx_pair_advance_delta_kernel (misc.hip): the advancing thread patches its lane's persistent board in place.)
// Decoupling the two is what makes the store stream fast: single-kernel variants that advance
// lanes, synchronise and then store (per-block 230 KB tiles, or flat 16 KiB runs with ping-pong
// state) measured 5.1-5.5 TB/s against 6.2-6.4 TB/s for this pair (profiles/r01/ab_*.log).
// Host code, below the kernels: the family's host trait (deep_sea_host: cfg check, fill, make), the step entries, the group
// setter, and the eight fused closed-loop entry points as one-statement delegations ("Host glue of the closed-loop calls").
#include "bsx_embed_device.h"
#include "bsx_pair_host.h"
#include "bsx_tab_eval.h"
#include "bsx_tab_sample_device.h"
#include "deep_sea_fam.h"
#include "deep_sea_hint.h"
#include "pair_mixed.h"

// ---------------------------------------------------------------------------------------------
// ONE launch per step (ABI v11, bsx_call_t.flags & BSX_CALL_STATE_TAGGED; deterministic, no wrapper, no Logging).
// The observation store stream, unchanged in shape — workgroup b writes floats [b*K*1024, (b+1)*K*1024) as K
// lane-interleaved 16-byte stores per thread — but nobody has advanced the lanes beforehand: every thread loads the
// packed state AND the action of the lane whose row its chunk belongs to and recomputes that lane's transition itself
// (deterministic deep_sea: ~25 vector instructions and one look-up in the action mapping, which every WAVE keeps as its
// own copy in LDS — no workgroup barrier anywhere).  The thread whose chunk holds the first float of a lane's row is
// that lane's WRITER: it alone stores the new state word, reward / discount / step_type and the bsuite_info updates.
// A reader may find the word already advanced by its writer; bit 18 (the parity of the next call's index, written by
// every advance: deep_sea_fam.h) says which, and both cases end in the same new state.  No second launch, no launch gap,
// no state column round trip: the 12.5 us lane advance of the two-launch step and the gap behind it are gone.
// (The same for catch would put a Philox block — its reset draw — into most waves of the stream: r01 measured 100 vs
// 42 us.  Stochastic deep_sea draws per step and keeps the two launches.)
// (cells: a multiple of 4 — a 16-byte chunk then never straddles two lanes — and at least 768; other boards keep the two launches)
// (hint_out != nullptr: the launch is the HINTED step instead — deep_sea_hint_advance / deep_sea_hint_stream below, one uniform
// branch per workgroup.  It is a mode of this kernel and not a kernel of its own because the library's kernel count is held
// where it is by the features' host tests; the two bodies share nothing but the LDS copy of the mapping.)
__device__ __forceinline__ void deep_sea_hint_advance(const deep_sea_fam::args& a, uint32_t block_id, uint32_t* __restrict__ hint_out,
                                                      deep_sea_fam::shared& s_fam, unsigned int* s_cnt);
template <int K>
__device__ __forceinline__ void deep_sea_hint_stream(float* __restrict__ obs, const uint32_t* __restrict__ hint_in,
                                                     const int32_t* __restrict__ action, int64_t n_lanes, uint32_t cells,
                                                     uint32_t cells_magic, bsx_div64 dv, uint32_t block_id);

template <int K>
__global__ void __launch_bounds__(BSX_BLOCK) deep_sea_step1_kernel(const deep_sea_fam::args a, const uint32_t cells,
                                                                   const uint32_t cells_magic, const bsx_div64 dv,
                                                                   const uint32_t adv_blocks, const uint32_t* __restrict__ hint_in,
                                                                   uint32_t* __restrict__ hint_out) {
  __shared__ deep_sea_fam::shared s_map[BSX_BLOCK / BSX_WAVE];           // one copy per wave: in-order LDS, no s_barrier
  if (hint_out != nullptr) {                                             // uniform: the hinted step (bsx_deep_sea_step_hinted)
    __shared__ unsigned int s_cnt[2];
    const bsx_pipe_role r = bsx_pipe_role_of(blockIdx.x, gridDim.x, adv_blocks, 0u);   // uniform per workgroup
    if (r.adv) deep_sea_hint_advance(a, r.index, hint_out, s_map[0], s_cnt);
    else deep_sea_hint_stream<K>(a.out.observation, hint_in, a.action, a.ctl.n_lanes, cells, cells_magic, dv, r.index);
    return;
  }
  const int wl = (int)(threadIdx.x & 63u);
  deep_sea_fam::shared& map = s_map[threadIdx.x >> 6];
  const int64_t n_lanes = a.ctl.n_lanes;
  const uint64_t step = bsx_step_of(a.ctl);
  const int32_t tag_new = (int32_t)(((uint32_t)(step + 1) & 1u) << DS_TAG_SHIFT);
  const bool forced = a.ctl.force_reset != 0;
  const deep_sea_hot fn{a.size};
  const uint64_t total = (uint64_t)n_lanes * cells;
  const uint64_t F0 = (uint64_t)blockIdx.x * (uint64_t)(K * 4 * BSX_BLOCK);
  const uint64_t lane_b = __umul64hi(F0, dv.m) >> dv.s;                  // uniform: the lane of the workgroup's first float
  const uint32_t r_b = (uint32_t)(F0 - lane_b * cells);
  bsx_f4* __restrict__ o4 = reinterpret_cast<bsx_f4*>(a.out.observation + F0);
  // everything per lane is addressed {uniform pointer at lane_b} + {32-bit lane offset}
  const int32_t* __restrict__ st_b = a.state + lane_b;
  const int32_t* __restrict__ act_b = a.action + (forced ? 0 : lane_b);

  // The K chunks of a thread lie 256 floats apart (each wave owns K consecutive KiB), the first and the last one
  // (K - 1) * 256 = 768 floats: with rows of at least that many floats (the launcher's condition: N >= 28) they touch
  // at most TWO lanes, the first chunk's and the last chunk's — two transitions per thread, not one per chunk.
  uint32_t dl[K];
  int r0[K];
  bool live[K];
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const uint32_t c = (threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63);
    const uint32_t f = r_b + (c << 2);
    dl[u] = __umulhi(f, cells_magic);
    r0[u] = (int)(f - dl[u] * cells);
    live[u] = F0 + ((uint64_t)c << 2) + 3 < total;
  }
  // lanes A = the first chunk's, B = the last live chunk's (B == A or A + 1 when cells >= (K - 1) * 256)
  const uint32_t dA = dl[0];
  uint32_t dB = dA;
  bool wrA = false, wrB = false;                                         // is some chunk of mine the first of lane A's / B's row?
#pragma unroll
  for (int u = 0; u < K; ++u) {
    if (live[u]) dB = dl[u];
  }
#pragma unroll
  for (int u = 0; u < K; ++u) {
    wrA |= live[u] && r0[u] == 0 && dl[u] == dA;
    wrB |= live[u] && r0[u] == 0 && dl[u] == dB && dB != dA;
  }
  const bool any = live[0];
  const int32_t wA = any ? st_b[dA] : 0, wB = any ? st_b[dB] : 0;
  const int aA = (any && !forced) ? act_b[dA] : 0, aB = (any && !forced) ? act_b[dB] : 0;

  // (the wave's copy of the action mapping: its loads go out BEHIND the state / action loads above — one round trip for all)
  const int map_words = (a.size * a.size + 31) >> 5;                    // <= DS_MAP_WORDS = 128: two words per lane at most
  static_assert(DS_MAP_WORDS <= 2 * BSX_WAVE, "the per-wave copy of the action mapping is two passes at most");
  if (wl < map_words) map.map[wl] = a.mapping_bits[wl];
  if (wl + BSX_WAVE < map_words) map.map[wl + BSX_WAVE] = a.mapping_bits[wl + BSX_WAVE];
  bsx_wave_sync();


  // The new packed state of lane lane_b + d given its state word w and action; `writer` publishes it.
  auto resolve = [&](uint32_t d, int32_t w, int act, bool writer, int& type) -> int32_t {
    type = -1;
    if (!writer && (w & DS_TAG_BIT) == tag_new) return w;                // the lane's writer has been here already
    const int64_t L = (int64_t)lane_b + d;
    int32_t nst; double reward;
    const int ty = deep_sea_fam::advance<true, 1>(a, map, L, a.ctl.lane_offset + (uint64_t)L, step, w, act, nst, reward, writer);
    if (writer) {
      type = ty;
      a.state[L] = nst;
      bsx_emit_at<0, 0, false>(a.ctl, a.out, L, L, a.ctl.lane_offset + (uint64_t)L, step, ty, reward);
    }
    return nst;
  };
  int tA = -1, tB = -1;
  int32_t nA = 0, nB = 0;
  if (any) {
    nA = resolve(dA, wA, aA, wrA, tA);
    nB = dB != dA ? resolve(dB, wB, aB, wrB, tB) : nA;
  }
  int hA, hB, unused;
  fn(nA, hA, unused);
  fn(nB, hB, unused);
#pragma unroll
  for (int u = 0; u < K; ++u) {
    if (!live[u]) continue;
    int hot = dl[u] == dA ? hA : hB;
    const int p0 = hot < 0 ? -1 : hot - r0[u];
    bsx_f4 v;
    v.x = p0 == 0 ? 1.0f : 0.0f;
    v.y = p0 == 1 ? 1.0f : 0.0f;
    v.z = p0 == 2 ? 1.0f : 0.0f;
    v.w = p0 == 3 ? 1.0f : 0.0f;
    // (non-temporal here: 79 -> 83.5 us per step at 2^17 lanes, 157 -> 166 at 2^18: profiles/r06/ab_deep_sea_step1_nt.log)
    o4[(threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63)] = v;
  }
  const unsigned int n_last = (unsigned int)__popcll(__ballot(tA == BSX_LAST)) + (unsigned int)__popcll(__ballot(tB == BSX_LAST));
  const unsigned int n_first = (unsigned int)__popcll(__ballot(tA == BSX_FIRST)) + (unsigned int)__popcll(__ballot(tB == BSX_FIRST));
  // one pair of sharded atomics per WAVE that saw an episode end or begin (a 1/31 of the lanes each on a steady-state call)
  if (a.ctl.counters != nullptr && wl == 0 && (n_last | n_first) != 0u) {
    unsigned long long* shard = (unsigned long long*)a.ctl.counters +
                                (size_t)((blockIdx.x * (BSX_BLOCK / BSX_WAVE) + (threadIdx.x >> 6)) & (BSX_COUNTER_SHARDS - 1)) * BSX_COUNTER_STRIDE;
    if (n_last) atomicAdd(&shard[0], (unsigned long long)n_last);
    if (n_first) atomicAdd(&shard[1], (unsigned long long)n_first);
  }
}

// ---------------------------------------------------------------------------------------------
// ONE launch per step at LARGE batches (bsx_deep_sea_step_hinted; the hint mode of deep_sea_step1_kernel), with
// bsx_pipelined_kernel's wait-free shape: the
// first adv_blocks workgroups advance the lanes (bsx_pipe_role_of, place 0), the rest are the observation store stream,
// and nothing in the launch depends on anything else in it.  Deterministic deep_sea has two outcomes per lane and call
// — which one is `action == mapping[row, col]` — so the lane advance of the PREVIOUS call has left both hot cells of
// this call's board in the lane's hint word (deep_sea_hint.h); a chunk of the stream loads hint_in[lane] and
// action[lane] where bsx_hot_stream_body loads state[lane], and selects.  It reads no byte this launch writes: the
// advance workgroups write `state`, the TimeStep columns and hint_out, the other half of the hint ping-pong pair.
// Against deep_sea_step1_kernel: no transition, no LDS and no tag test in the stream, whose body stays that of
// bsx_hot_stream_kernel<deep_sea_hot, 4, 256> plus one coalesced 4-byte load per chunk.
// With no stream workgroups the same launch is the PRIMING advance (no valid hint_in yet): it leaves hint_out and is followed
// by the unchanged store stream over the state column.
//
// The advance workgroups: the lean two-lanes-per-thread body of bsx_advance2_kernel (bsx_advance_body<Fam, true, -1, 2>:
// the same loads, state store, TimeStep stores and counter flush; the transition with the draws compiled out, as in
// deep_sea_step1_kernel) + the hint of the NEW word, one more look-up in the LDS copy of the mapping per lane.
__device__ __forceinline__ void deep_sea_hint_advance(const deep_sea_fam::args& a, uint32_t block_id, uint32_t* __restrict__ hint_out,
                                                      deep_sea_fam::shared& s_fam, unsigned int* s_cnt) {
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  deep_sea_fam::stage(a, s_fam);
  __syncthreads();
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
      act[h] = a.action[i[h]];                              // (no ring, no forced reset: the launcher's conditions)
      st[h] = a.state[i[h]];
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (mine[h]) {
      const uint64_t lane = a.ctl.lane_offset + (uint64_t)i[h];
      int32_t nst; double reward;
      type[h] = deep_sea_fam::advance<true, 1>(a, s_fam, i[h], lane, step, st[h], act[h], nst, reward);
      a.state[i[h]] = nst;
      hint_out[i[h]] = ds_hint_pack(nst & 0xFF, (nst >> 8) & 0xFF, nst & DS_RESET_BIT, a.size, s_fam.map);
      bsx_emit_at<0, 0, false>(a.ctl, a.out, i[h], i[h], lane, step, type[h], reward);
    }
    bsx_count_types(a.ctl, type[h], s_cnt);
  }
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, block_id);
}

// The stream workgroups: bsx_hot_stream_body<deep_sea_hot, K, BSX_BLOCK> for rows of a multiple of 4 floats (a chunk never
// straddles two lanes, the array has no ragged tail) — the same chunk -> address map, guards and plain 16-byte stores.
template <int K>
__device__ __forceinline__ void deep_sea_hint_stream(float* __restrict__ obs, const uint32_t* __restrict__ hint_in,
                                                     const int32_t* __restrict__ action, int64_t n_lanes, uint32_t cells,
                                                     uint32_t cells_magic, bsx_div64 dv, uint32_t block_id) {
  const uint64_t total = (uint64_t)n_lanes * cells;                      // floats in the array
  const uint64_t F0 = (uint64_t)block_id * (uint64_t)(K * 4 * BSX_BLOCK);
  const uint64_t lane_b = __umul64hi(F0, dv.m) >> dv.s;                  // uniform
  const uint32_t r_b = (uint32_t)(F0 - lane_b * cells);                  // < cells
  bsx_f4* __restrict__ o4 = reinterpret_cast<bsx_f4*>(obs + F0);
  const uint32_t* __restrict__ hi = hint_in + lane_b;
  const int32_t* __restrict__ ac = action + lane_b;

  int r0[K];
  uint32_t h0[K];
  int32_t a0[K];
  bool live[K];
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const uint32_t c = (threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63);   // each wave owns K consecutive KiB
    const uint32_t f = r_b + (c << 2);                                   // float offset from lane_b's row start
    const uint32_t dl = __umulhi(f, cells_magic);
    r0[u] = (int)(f - dl * cells);
    live[u] = F0 + ((uint64_t)c << 2) + 3 < total;                       // (then lane_b + dl < n_lanes: cells % 4 == 0)
    h0[u] = live[u] ? hi[dl] : 0u;
    a0[u] = live[u] ? ac[dl] : 0;
  }
#pragma unroll
  for (int u = 0; u < K; ++u) {
    if (!live[u]) continue;
    const int hot = ds_hint_hot(h0[u], a0[u]);
    const int p0 = hot < 0 ? -1 : hot - r0[u];
    bsx_f4 v;
    v.x = p0 == 0 ? 1.0f : 0.0f;
    v.y = p0 == 1 ? 1.0f : 0.0f;
    v.z = p0 == 2 ? 1.0f : 0.0f;
    v.w = p0 == 3 ? 1.0f : 0.0f;
    o4[(threadIdx.x >> 6) * (K * 64) + u * 64 + (threadIdx.x & 63)] = v;
  }
}

// What differs between the grid families on the host: the trait of bsx_grid_closed_loop (bsx_host.h).
namespace {                                 // (internal linkage: the library exports its C ABI and nothing else)
struct deep_sea_host {
  typedef bsx_deep_sea_t cfg_t;
  typedef deep_sea_fam fam;
  typedef deep_sea_hot hot_t;
  static constexpr int32_t code = BSX_FAM_DEEP_SEA, actions = 2;
  // The cfg's range check, the same for every entry point.
  static int check_cfg(const cfg_t* cfg) { return (cfg->size < 1 || cfg->size > BSX_DEEP_SEA_MAX_SIZE) ? BSX_ERANGE : 0; }
  static int32_t states(const cfg_t* cfg) { return bsx_policy_states_deep_sea(cfg->size); }
  static int32_t cells(const cfg_t* cfg) { return cfg->size * cfg->size; }
  static hot_t hot(const cfg_t* cfg) { return deep_sea_hot{cfg->size}; }
  // The kernel argument struct of a checked call.
  static void fill(const cfg_t* cfg, const bsx_call_t* call, const int32_t* action, int32_t* state, bsx_timestep_t out, double* info,
                   fam::args* a) {
    a->ctl = bsx_make_ctl(call);
    a->action = action; a->state = state; a->out = out; a->info = info;
    a->move_cost = cfg->move_cost; a->inv_size = cfg->inv_size;
    a->size = cfg->size; a->deterministic = cfg->deterministic;
    for (int w = 0; w < DS_MAP_WORDS; ++w) a->mapping_bits[w] = cfg->mapping_bits[w];
  }
  // Validates one call's arguments and fills the kernel argument struct (step, the groups and the recording closed loops).
  static int make(const cfg_t* cfg, const bsx_call_t* call, const int32_t* action, int32_t* state, bsx_timestep_t out, double* info,
                  fam::args* a) {
    if (cfg == nullptr) return BSX_ENULL;
    int rc = bsx_check_call(call, action, out, /*delta_ok=*/true, /*narrow_ok=*/true);
    if (rc != 0) return rc;
    if ((rc = check_cfg(cfg)) != 0) return rc;
    if (call->stream.mt_state != nullptr && !cfg->deterministic && call->stream.mt_gauss == nullptr)
      return BSX_ENULL;                      // the stochastic variant draws randn: needs the gauss cache columns
    if (call->n_lanes > 0 && (state == nullptr || info == nullptr)) return BSX_ENULL;
    fill(cfg, call, action, state, out, info, a);
    return 0;
  }
  template <class Union>
  static fam::args* of(Union& u) { return &u.deep_sea; }
};
}  // namespace

extern "C" int bsx_deep_sea_step(const bsx_deep_sea_t* cfg, const bsx_call_t* call,
                                 const int32_t* action, int32_t* state, bsx_timestep_t out,
                                 double* info) {
  deep_sea_fam::args a;
  int rc = deep_sea_host::make(cfg, call, action, state, out, info, &a);
  if (rc != 0) return rc;
  if (call->n_lanes == 0) return 0;
  const uint32_t cells = (uint32_t)(cfg->size * cfg->size);
  // ONE launch (deep_sea_step1_kernel) where the caller vouches for the state words' parity tags and nothing but the
  // deterministic transition itself has to be recomputed per thread; small boards in small batches keep their fused
  // tile step (bsx_pair_call), which is one launch already.
  // ... up to 2^18 lanes of N = 30 (at most 1 GiB of observations per step): there the 12.5 us lane advance and
  // the launch gap it removes outweigh the transitions recomputed in every wave of the stream; at 2^20 lanes the
  // recomputation costs the stream 25-50 us (597 -> 622-648 us, profiles/r04/ab_deep_sea_single_launch.log) and the
  // two launches stay.  (The kernel reads `action` as a plain [B] column: a call that walks an action ring takes the
  // two-launch path, whose lane advance goes through bsx_action().)
  static const int step1_env = bsx_env_int("BSX_DEEP_SEA_STEP1", 1);
  if (step1_env != 0 && (int64_t)call->n_lanes * cells * 4 <= ((int64_t)1 << 30) && (call->flags & BSX_CALL_STATE_TAGGED) && call->n_steps <= 1 && call->action_ring <= 1 && cfg->deterministic && bsx_ctl_lean(a.ctl) &&
      call->obs_paint == nullptr && bsx_call_obs(call) == 0 && !bsx_call_index(call) && (cells & 3u) == 0 && cells >= 3u * 256u) {
    constexpr int K = 4;
    const uint64_t total = (uint64_t)call->n_lanes * cells;
    const uint64_t blocks = (total + (uint64_t)K * 4 * BSX_BLOCK - 1) / ((uint64_t)K * 4 * BSX_BLOCK);
    if (blocks > 0x7FFFFFFFull) return BSX_EINVAL;
    deep_sea_step1_kernel<K><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, (hipStream_t)call->hip_stream>>>(
        a, cells, bsx_div_magic(cells), bsx_make_div64(cells), 0u, nullptr, nullptr);
    return bsx_launch_status();
  }
  return bsx_pair_call<deep_sea_fam, deep_sea_hot, 4>(a, call, action, state, out, cells, deep_sea_hot{cfg->size});
}

extern "C" int bsx_deep_sea_step_hinted(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const int32_t* action, int32_t* state,
                                        bsx_timestep_t out, double* info, const uint32_t* const hint_in, uint32_t* const hint_out) {
  if (cfg == nullptr || call == nullptr) return BSX_ENULL;
  // (the 16-byte alignment of the boards is one of this entry's modes: BSX_EMODE, ahead of the common checks' BSX_EALIGN)
  if ((reinterpret_cast<uintptr_t>(out.observation) & 15u) != 0) return BSX_EMODE;
  deep_sea_fam::args a;
  int rc = deep_sea_host::make(cfg, call, action, state, out, info, &a);
  if (rc != 0) return rc;
  const uint32_t cells = (uint32_t)(cfg->size * cfg->size);
  if (!cfg->deterministic || !bsx_ctl_lean(a.ctl) || bsx_call_obs(call) != 0 || bsx_call_index(call) || call->obs_paint != nullptr ||
      call->n_steps > 1 || call->action_ring > 1 || call->force_reset != 0 || !(call->flags & BSX_CALL_STATE_TAGGED) || (cells & 3u) != 0)
    return BSX_EMODE;
  if (call->n_lanes == 0) return 0;
  if (hint_out == nullptr || hint_out == hint_in) return BSX_ENULL;
  hipStream_t st = (hipStream_t)call->hip_stream;
  const uint64_t adv_blocks = (uint64_t)((bsx_blocks_of(call->n_lanes) + 1) / 2);          // two lanes per thread
  const uint64_t str_blocks = hint_in == nullptr ? 0 : bsx_flat_blocks((uint64_t)call->n_lanes * cells, PAIR_DEEP_SEA_K);
  if (adv_blocks + str_blocks > 0x7FFFFFFFull) return BSX_EINVAL;
  const uint32_t magic = bsx_div_magic(cells);
  deep_sea_step1_kernel<PAIR_DEEP_SEA_K><<<dim3((unsigned)(adv_blocks + str_blocks)), dim3(BSX_BLOCK), 0, st>>>(
      a, cells, magic, bsx_make_div64(cells), (uint32_t)adv_blocks, hint_in, hint_out);
  // priming: no hint of this call exists yet — the boards come from the state column the advance has just written
  if (hint_in == nullptr) {
    rc = bsx_launch_hot_stream<deep_sea_hot, PAIR_DEEP_SEA_K>(out.observation, state, call->n_lanes, cells, magic, deep_sea_hot{cfg->size}, st);
    if (rc != 0) return rc;
  }
  return bsx_launch_status();
}

// The eight fused closed-loop entry points: each body is stated once for both families, beside its kind's checks
// (bsx_policy_rollout_entry, bsx_pair_host.h; bsx_tab_eval_entry; bsx_tab_softmax_entry; bsx_embed_entry), over the one
// prologue of bsx_host.h.  A recording call is told from an evaluation by its output struct.
extern "C" int bsx_deep_sea_policy_rollout(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy,
                                           int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_policy_rollout_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_deep_sea_policy_evaluate(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy,
                                            int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_tab_eval_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_deep_sea_policy_sample(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                          int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_tab_softmax_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_deep_sea_policy_sample_evaluate(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                                   int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_tab_softmax_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_deep_sea_embedding_rollout(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                              int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_embed_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_deep_sea_embedding_evaluate(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                               int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_embed_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_deep_sea_embedding_sample(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_sample_t* policy,
                                             int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_embed_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_deep_sea_embedding_sample_evaluate(const bsx_deep_sea_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_sample_t* policy,
                                                      int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_embed_entry<deep_sea_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_group_set_deep_sea(bsx_group_t* g, int32_t index, const bsx_deep_sea_t* cfg,
                                      const bsx_call_t* call, const int32_t* action, int32_t* state,
                                      bsx_timestep_t out, double* info) {
  if (g == nullptr) return BSX_ENULL;
  if (call != nullptr && (bsx_call_obs(call) != 0 || bsx_call_index(call))) return BSX_EMODE;   // groups write float32 boards
  int rc;
  deep_sea_fam::args a;
  if (bsx_is_mixed_pair_group(g)) {            // one segment of the mixed two-kernel group
    rc = deep_sea_host::make(cfg, call, action, state, out, info, &a);
    if (rc != 0) return rc;
    a.ctl.state_in = call->state_alt;            // pipelined sweeps: the advance reads the other column
    const uint32_t cells = (uint32_t)(cfg->size * cfg->size);
    if (cells < 4u) return BSX_ERANGE;
    const bsx_stream_seg<deep_sea_hot> sg = bsx_make_stream_seg(out.observation, state, a.ctl.n_lanes, cells, deep_sea_hot{cfg->size});
    return bsx_mixed_put(g, BSX_FAM_DEEP_SEA, index, call, &a, sizeof(a), &sg, sizeof(sg),
                              (uint64_t)bsx_blocks_of(a.ctl.n_lanes),
                              bsx_flat_blocks((uint64_t)a.ctl.n_lanes * cells, PAIR_DEEP_SEA_K), 0);
  }
  rc = bsx_group_check_set(g, BSX_FAM_DEEP_SEA, index, call, sizeof(deep_sea_fam::args),
                           sizeof(bsx_stream_seg<deep_sea_hot>), 0);
  if (rc != 0) return rc;
  rc = deep_sea_host::make(cfg, call, action, state, out, info, &a);
  if (rc != 0) return rc;
  g->launch = bsx_group_launch_pair<deep_sea_fam, deep_sea_hot, 4>;
  g->n_phases = 2;
  return bsx_group_put_pair<deep_sea_fam, deep_sea_hot>(g, index, a, out.observation, state,
                                                        (uint32_t)(cfg->size * cfg->size), deep_sea_hot{cfg->size}, 4);
}
