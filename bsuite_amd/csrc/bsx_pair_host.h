// bsx_pair_host.h — host side of the two-kernel ("pair") families deep_sea and catch: the launchers of bsx_pair_device.h's
// kernels, their grouped launch, and the one call that picks among them (bsx_pair_call).
#ifndef BSX_PAIR_HOST_H_
#define BSX_PAIR_HOST_H_

#include "bsx_host.h"
#include "bsx_pair_device.h"

// Launches the lane-per-thread advance kernel of a two-kernel family.
template <class Fam>
static inline int bsx_launch_advance(const typename Fam::args& a, hipStream_t st) {
  const int64_t blocks = bsx_blocks_of(a.ctl.n_lanes);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  const bool lean = bsx_ctl_lean(a.ctl);
  // From two dispatch rounds of one-lane workgroups up (2^20 lanes): two lanes per thread, both lanes' loads issued up
  // front — ONE round.  Same call (profiles/r04/ab_advance_two_lanes.log): catch/0 42.5 -> 41.6 us per step, deep_sea -0.5 us;
  // equal at 2^19 lanes, 79.8 -> 78.8 at 2^21.  (0 = never)
  static const int lpt2_min_blocks = bsx_env_int("BSX_ADVANCE_LPT2_MIN_BLOCKS", 4096);
  if (lean && lpt2_min_blocks > 0 && blocks >= lpt2_min_blocks) {
    bsx_advance2_kernel<Fam><<<dim3((unsigned)((blocks + 1) / 2)), dim3(BSX_BLOCK), 0, st>>>(a);
    return 0;
  }
  if (lean) bsx_advance_kernel<Fam, true><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(a);
  // the wrapped call on the counter-based stream (the common one): the MT19937-exact generators compiled out — in a
  // kernel of its own for a family that keeps that instantiation (Fam::ADVANCE_WITHOUT_MT: catch), else (deep_sea) as one of
  // the two bodies of the wrapped kernel, which switches on ctl.mt_state itself (bsx_advance_kernel).
  else if constexpr (Fam::ADVANCE_WITHOUT_MT) {
    if (a.ctl.mt_state == nullptr) bsx_advance_kernel<Fam, false, 0><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(a);
    else bsx_advance_kernel<Fam, false><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(a);
  } else {
    bsx_advance_kernel<Fam, false><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(a);
  }
  return 0;
}

// ... and of the delta observation mode: bsx_pair_advance_delta_kernel (misc.hip), ONE kernel for deep_sea and catch.
// `args` is the family's args and `fn` its decoder (BSX_FAM_DEEP_SEA: deep_sea_fam::args, deep_sea_hot; BSX_FAM_CATCH:
// catch_fam::args, catch_hot), both copied into the launch.
void bsx_launch_pair_advance_delta(int32_t family, const void* args, const void* fn, int32_t* paint, uint32_t cells, int64_t blocks,
                                   hipStream_t st);

template <class Fam, class HotFn>
static inline int bsx_launch_advance_delta(const typename Fam::args& a, const HotFn& fn, int32_t* paint,
                                           uint32_t cells, hipStream_t st) {
  const int64_t blocks = bsx_blocks_of(a.ctl.n_lanes);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  bsx_launch_pair_advance_delta(HotFn::FAMILY, &a, &fn, paint, cells, blocks, st);
  return 0;
}

// Launches bsx_hot_cells_kernel (misc.hip): the one-float-per-thread writer of a dense observation [n_lanes x cells] of
// `family` (BSX_FAM_DEEP_SEA: p0 = N; BSX_FAM_CATCH: p0 = rows, p1 = columns), at any 4-byte aligned address.
int bsx_launch_hot_cells(float* obs, const int32_t* state, int64_t n_lanes, uint32_t cells, int32_t family, int32_t p0, int32_t p1,
                         hipStream_t st);

// Launches the split-phase observation writer: K stores per thread, 256 threads per workgroup — each family's measured
// optimum (profiles/r01/sweep_stream_*.log) — in the wave-contiguous order.  (That order is a run-time argument that is
// always 1: folded into the kernel at compile time, the compiler schedules the headline's stream differently and it ran
// 0.2 % slower, deep_sea/10 at 2^20 lanes 0.5913 -> 0.5926 ms per step, A/B/B/A in one call.)
template <class HotFn, int K>
static inline int bsx_launch_hot_stream(float* obs, const int32_t* state, int64_t n_lanes, uint32_t cells,
                                        uint32_t cells_magic, HotFn fn, hipStream_t st) {
  const uint64_t total = (uint64_t)n_lanes * cells;
  // 4-byte stores for degenerate boards and for an observation slice that does not start on a 16-byte
  // boundary (rollout slice t of an odd B x cells: t*B*cells*4 bytes into the [T,B,cells] array)
  if (cells < 4u || (reinterpret_cast<uintptr_t>(obs) & 15u) != 0)
    return bsx_launch_hot_cells(obs, state, n_lanes, cells, HotFn::FAMILY, fn.geom0(), fn.geom1(), st);
  const bsx_div64 dv = bsx_make_div64(cells);
  const uint64_t per_block = (uint64_t)K * 4 * BSX_BLOCK;
  const uint64_t blocks = (total + per_block - 1) / per_block;
  if (blocks > 0x7FFFFFFFull) return BSX_EINVAL;
  bsx_hot_stream_kernel<HotFn, K, BSX_BLOCK><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, st>>>(obs, state, n_lanes, cells, cells_magic, dv, fn, 1);
  return 0;
}

// Launches the narrow observation stream (bsx_narrow_stream_kernel) of one step: `obs` -> [n_lanes x cells] elements of
// observation code `code` (1..3), at any element-aligned address.
template <class HotFn, int K>
static inline int bsx_launch_narrow_stream(void* obs, const int32_t* state, int64_t n_lanes, uint32_t cells, int code,
                                           HotFn fn, hipStream_t st) {
  static const uint32_t one[4] = {0u, 0x01u, 0x3C00u, 0x3F80u};      // the element's 1.0 (index: observation code)
  const int E = code == 1 ? 1 : 2, N = 16 / E;
  const uint64_t total = (uint64_t)n_lanes * cells;
  uint64_t head = ((16u - (reinterpret_cast<uintptr_t>(obs) & 15u)) & 15u) / (uint64_t)E;
  if (head > total) head = total;
  const uint64_t n_chunks = (total - head) / (uint64_t)N;
  const uint64_t per_block = (uint64_t)K * BSX_BLOCK;
  const uint64_t blocks = n_chunks == 0 ? 1 : (n_chunks + per_block - 1) / per_block;   // workgroup 0 writes head and tail
  if (blocks > 0x7FFFFFFFull) return BSX_EINVAL;
  const bool wide = cells >= (uint32_t)N;                   // the kernel's fast path (bsx_make_div64 needs cells >= 4)
  const uint32_t magic = wide ? bsx_div_magic(cells) : 0u;
  const bsx_div64 dv = wide ? bsx_make_div64(cells) : bsx_div64{0, 0};
  const dim3 grid((unsigned)blocks), block(BSX_BLOCK);
  if (E == 1)
    bsx_narrow_stream_kernel<HotFn, 1, K><<<grid, block, 0, st>>>((uint8_t*)obs, state, n_lanes, cells, magic, dv,
                                                                   (uint32_t)head, n_chunks, one[code], fn);
  else
    bsx_narrow_stream_kernel<HotFn, 2, K><<<grid, block, 0, st>>>((uint8_t*)obs, state, n_lanes, cells, magic, dv,
                                                                   (uint32_t)head, n_chunks, one[code], fn);
  return 0;
}

// One segment's arguments of the observation stream kernel (cells >= 4: bsx_make_div64).
template <class HotFn>
static inline bsx_stream_seg<HotFn> bsx_make_stream_seg(float* obs, const int32_t* state, int64_t n_lanes, uint32_t cells, const HotFn& fn) {
  bsx_stream_seg<HotFn> sg;
  sg.obs = obs; sg.state = state; sg.n_lanes = n_lanes; sg.cells = cells;
  sg.cells_magic = bsx_div_magic(cells); sg.dv = bsx_make_div64(cells); sg.fn = fn;
  return sg;
}

// Records one segment of a two-kernel family (advance args + stream-kernel segment).
template <class Fam, class HotFn>
static inline int bsx_group_put_pair(bsx_group* g, int32_t index, const typename Fam::args& a, float* obs,
                                     int32_t* state, uint32_t cells, const HotFn& fn, int k) {
  if (cells < 4u) return BSX_ERANGE;                        // degenerate boards: step them singly
  memcpy(&g->args[(size_t)index * sizeof(typename Fam::args)], &a, sizeof(a));
  const bsx_stream_seg<HotFn> sg = bsx_make_stream_seg(obs, state, a.ctl.n_lanes, cells, fn);
  memcpy(&g->args2[(size_t)index * sizeof(sg)], &sg, sizeof(sg));
  const uint64_t b1 = (uint64_t)bsx_blocks_of(a.ctl.n_lanes);
  const uint64_t b2 = bsx_flat_blocks((uint64_t)a.ctl.n_lanes * cells, k);
  if (b1 > 0x3FFFFFFFull || b2 > 0x3FFFFFFFull) return BSX_EINVAL;
  g->blocks[index] = (int32_t)b1; g->blocks2[index] = (int32_t)b2;
  g->is_set[index] = 1;
  return 0;
}

// Launches bsx_pair_advance_group_kernel (misc.hip): the lane advance of every segment of a single-family group of `family`
// (BSX_FAM_DEEP_SEA / BSX_FAM_CATCH), `table` the device array of the family's args, one workgroup per 256 lanes.
void bsx_launch_pair_advance_group(int32_t family, const void* table, const bsx_group_index& gi, int64_t total_blocks, hipStream_t st);

template <class Fam, class HotFn, int K>
static int bsx_group_launch_pair(bsx_group* g, int phase, hipStream_t st) {
  if (phase != 1) bsx_launch_pair_advance_group(HotFn::FAMILY, g->d_args, g->index1(), g->total_blocks, st);
  if (phase != 0)
    bsx_hot_stream_group_kernel<HotFn, K><<<dim3((unsigned)g->total_blocks2), dim3(BSX_BLOCK), 0, st>>>(
        (const bsx_stream_seg<HotFn>*)g->d_args2, g->index2());
  return (int)hipGetLastError();
}

// Launches bsx_index_decode_kernel (misc.hip): packed state column -> index rows [n_lanes, K] of `family` (BSX_FAM_DEEP_SEA:
// p0 = N; BSX_FAM_CATCH: p0 = rows, p1 = columns).  `rollout`: the rows are a slice of a rollout's [T,B,K] output.
int bsx_launch_index_decode(int32_t* rows, const int32_t* state, int64_t n_lanes, int32_t family, int32_t p0, int32_t p1,
                            bool rollout, hipStream_t st);

// The refusals of bsx_<family>_policy_rollout / _policy_evaluate that do not depend on the family, in the documented order
// (include/bsuite_amd.h): modes, then scalars.  `n_states`: the family's table length for this cfg.
static inline int bsx_check_policy_scalars(const bsx_call_t* call, const bsx_policy_t* pol, int32_t n_states) {
  if (call == nullptr || pol == nullptr) return BSX_ENULL;
  if ((call->flags & (BSX_CALL_OBS_MASK | BSX_CALL_OBS_INDEX)) != BSX_CALL_OBS_INDEX) return BSX_EMODE;
  if (call->logging != nullptr || call->wrap.kind != BSX_WRAP_NONE || call->stream.mt_state != nullptr ||
      call->stream.mt_pos != nullptr || call->reward_f64 != nullptr || call->obs_paint != nullptr ||
      call->state_alt != nullptr || call->action_ring > 1 || call->force_reset)
    return BSX_EMODE;
  if (call->n_steps < 1 || call->n_lanes < 0 || call->n_lanes > ((int64_t)1 << 40)) return BSX_EINVAL;
  if (pol->n_states != n_states || pol->n_policies < 1) return BSX_EINVAL;
  if (!(pol->epsilon >= 0.0 && pol->epsilon <= 1.0)) return BSX_ERANGE;      // (NaN included)
  return 0;
}

// ... then, for a call with lanes, the pointers of a policy rollout.
static inline int bsx_check_policy_call(const bsx_call_t* call, const bsx_policy_t* pol, int32_t n_states, const int32_t* state,
                                        const bsx_timestep_t& out, const double* info) {
  const int rc = bsx_check_policy_scalars(call, pol, n_states);
  if (rc != 0 || call->n_lanes == 0) return rc;
  if (pol->table == nullptr || pol->actions_out == nullptr || state == nullptr || info == nullptr ||
      out.reward == nullptr || out.discount == nullptr || out.step_type == nullptr || out.observation == nullptr)
    return BSX_ENULL;
  if (pol->n_policies > 1 && pol->policy_index == nullptr) return BSX_ENULL;
  if ((reinterpret_cast<uintptr_t>(out.observation) & 15u) != 0) return BSX_EALIGN;
  return 0;
}

// ... and those of a policy evaluation: no TimeStep buffers, actions_out is not looked at, three output columns.
static inline int bsx_check_policy_eval_call(const bsx_call_t* call, const bsx_policy_t* pol, int32_t n_states,
                                             const int32_t* state, const bsx_policy_eval_t& out, const double* info) {
  const int rc = bsx_check_policy_scalars(call, pol, n_states);
  if (rc != 0 || call->n_lanes == 0) return rc;
  if (pol->table == nullptr || state == nullptr || info == nullptr || out.episodes == nullptr || out.return_sum == nullptr ||
      out.episode_return_sum == nullptr)
    return BSX_ENULL;
  if (pol->n_policies > 1 && pol->policy_index == nullptr) return BSX_ENULL;
  if (call->action_ring < 0) return BSX_EINVAL;                              // (what bsx_check_call refuses for a rollout)
  if (bsx_blocks_of(call->n_lanes) > 0x7FFFFFFF) return BSX_EINVAL;
  return 0;
}

// bsx_policy_args of a call (`actions_out` is the rollout's alone).
static inline bsx_policy_args bsx_make_policy_args(const bsx_policy_t* pol, uint32_t num_actions) {
  bsx_policy_args p;
  p.table = pol->table;
  p.policy_index = pol->n_policies > 1 ? pol->policy_index : nullptr;
  p.actions_out = pol->actions_out;
  p.epsilon = pol->epsilon;
  p.explore_seed = pol->explore_seed;
  p.n_states = pol->n_states; p.n_policies = pol->n_policies;
  p.num_actions = num_actions;
  p.in_lds = (pol->n_policies == 1 && pol->n_states <= BSX_POLICY_LDS_BYTES) ? 1 : 0;
  return p;
}

// Launches bsx_policy_rollout_kernel: `a` from the family's make() (its action pointer is never read).
template <class Fam, class HotFn>
static int bsx_policy_rollout_call(const typename Fam::args& a, const bsx_call_t* call, const bsx_policy_t* pol,
                                   uint32_t num_actions, bsx_timestep_t out, const HotFn& fn) {
  const int64_t blocks = bsx_blocks_of(call->n_lanes);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  const bsx_policy_args p = bsx_make_policy_args(pol, num_actions);
  bsx_policy_rollout_kernel<Fam, HotFn><<<dim3((unsigned)blocks), dim3(BSX_BLOCK), 0, (hipStream_t)call->hip_stream>>>(
      a, call->n_steps, reinterpret_cast<int32_t*>(out.observation), fn, p);
  return bsx_launch_status();
}

// bsx_<family>_policy_rollout (Fam: the family's host trait, bsx_host.h).
template <class Fam>
static int bsx_policy_rollout_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy, int32_t* state,
                                    const bsx_timestep_t& out, double* info) {
  typename Fam::fam::args a;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, &out, info, &a,
      [&] { return bsx_check_policy_call(call, policy, Fam::states(cfg), state, out, info); },
      [&] { return bsx_policy_rollout_call<typename Fam::fam, typename Fam::hot_t>(a, call, policy, Fam::actions, out, Fam::hot(cfg)); });
}

// One call of a two-kernel family (deep_sea, catch): step() / reset() / a rollout of T steps with outputs
// [T,B,...].  `a` comes from the family's make(); K = stores per thread of its observation stream.
//   delta mode (obs_paint)          one launch per step: advance + in-place patch
//   dense                           advance + observation stream per step
//   dense rollout with state_alt    software-pipelined: advance(0); {stream(t), advance(t+1)} for t < T-1;
//                                   stream(T-1) — T+1 launches.  The advances alternate between `state`
//                                   and `state_alt` so that the column stream(t) reads is not the one
//                                   advance(t+1) writes; the parity is chosen so that the last advance
//                                   writes `state`.
template <class Fam, class HotFn, int K>
static int bsx_pair_call(const typename Fam::args& a0, const bsx_call_t* call, const int32_t* action, int32_t* state,
                         bsx_timestep_t out, uint32_t cells, const HotFn& fn) {
  hipStream_t st = (hipStream_t)call->hip_stream;
  const int T = bsx_n_steps(call);
  const int64_t B = call->n_lanes;
  auto at = [&](int t) {                      // the arguments of step t: slice [t] of every [T,B,...] array
    typename Fam::args s = a0;
    const int64_t off = (int64_t)t * B;
    s.ctl.step_index = call->stream.step_index + (uint64_t)t;
    s.ctl.reward_f64 = call->reward_f64 ? call->reward_f64 + off : nullptr;
    s.action = action ? action + off : action;
    s.out.reward = out.reward + off; s.out.discount = out.discount + off; s.out.step_type = out.step_type + off;
    s.out.observation = out.observation + off * (int64_t)cells;
    return s;
  };
  // Index observations (BSX_CALL_OBS_INDEX): no board is written, so none of the size rules below applies.  A lean call is
  // ONE launch — step() / reset(): bsx_index_step_kernel; rollout(T): bsx_index_rollout_kernel for all T steps — and any
  // other call (Logging, RewardNoise, MT19937-exact draws, reward_f64) is the unchanged lane advance followed by the
  // decode kernel state column -> index rows, per step.
  if (bsx_call_index(call)) {
    constexpr int IK = HotFn::INDEX_K;
    int32_t* const rows = reinterpret_cast<int32_t*>(out.observation);
    const int64_t blocks = bsx_blocks_of(B);
    if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
    const dim3 grid((unsigned)blocks), block(BSX_BLOCK);
    if (bsx_ctl_lean(a0.ctl)) {
      if (T > 1) bsx_index_rollout_kernel<Fam, HotFn><<<grid, block, 0, st>>>(a0, T, rows, fn);
      else bsx_index_step_kernel<Fam, HotFn><<<grid, block, 0, st>>>(a0, rows, fn);
      return bsx_launch_status();
    }
    int rc = 0;
    for (int t = 0; t < T && rc == 0; ++t) {
      typename Fam::args s = at(t);                        // (the advance never touches the observation)
      rc = bsx_launch_advance<Fam>(s, st);
      if (rc == 0) rc = bsx_launch_index_decode(rows + (int64_t)t * B * IK, state, B, HotFn::FAMILY, fn.geom0(), fn.geom1(), T > 1, st);
    }
    return rc != 0 ? rc : bsx_launch_status();
  }
  // Narrow observations (BSX_CALL_OBS_*): lane advance + narrow store stream per step, at every batch size.  Taken before
  // every size rule below: the fused tiles, the pipelined rollout and their byte thresholds are float32-only.
  const int obs_code = bsx_call_obs(call);
  if (obs_code != 0) {
    const int64_t slice_bytes = B * (int64_t)cells * (obs_code == 1 ? 1 : 2);
    int rc = 0;
    for (int t = 0; t < T && rc == 0; ++t) {
      typename Fam::args s = at(t);
      void* obs_t = (uint8_t*)out.observation + (int64_t)t * slice_bytes;
      s.out.observation = (float*)obs_t;                  // (the advance never touches the observation)
      rc = bsx_launch_advance<Fam>(s, st);
      if (rc == 0) rc = bsx_launch_narrow_stream<HotFn, K>(obs_t, state, B, cells, obs_code, fn, st);
    }
    return rc != 0 ? rc : bsx_launch_status();
  }
  const uint32_t magic = bsx_div_magic(cells);
  static const int place = bsx_env_int("BSX_PIPELINED_PLACE", 0);     // bsx_pipe_role_of: first (measured best)
  // the fused launch uses the 16-byte store stream: every [t] slice must start on a 16-byte boundary
  const bool pipelined = T > 1 && call->state_alt != nullptr && call->obs_paint == nullptr &&
                         cells >= 4u && (((uint64_t)B * cells) & 3ull) == 0;
  int rc = 0;
  // Boards of at most BSX_FUSED_TILE_MAX_CELLS floats (catch's 50; a workgroup's [256 x cells] tile is then <= 128 KiB):
  // ONE fused launch per step (bsx_fused_tile_kernel) and ONE per rollout (bsx_fused_rollout_kernel) while the
  // observation array of a step is at most fused_step_mib / BSX_FUSED_ROLLOUT_MAX_MIB = 128 MiB: catch up to
  // 2^19 lanes (105 MB: 20 vs 23 us eager, 20 vs 22 us per rollout step; 2^17: 9.4 vs 11 and 7.1 vs 9.0).  At 2^20
  // lanes (210 MB) the winner depends on the box — fused 41.9 vs 43.5 on one, 44.4-45.2 vs 43.2-43.6 on another; a
  // rollout 36.9 vs 39.6 and 43.4-45.5 vs 39.7-40.9 (its T slices lie 210 MB apart: page-mapping luck) — so the
  // decoupled pair / the pipelined rollout, steady within 2 % everywhere, keep that size (profiles/r03/
  // ab_fused_tile*.log, ab_fused_crossover.log); deep_sea N=30 (900 cells, 0.9 MiB tiles) never fuses.  The tile start
  // block*256*cells*4 is always 16-byte aligned when the slice is.  (A barrier-free variant — every wave its own
  // 64 lanes, neighbour states through ds_bpermute — measured 1-9 % slower: profiles/r03/ab_fused_wave.log; two tiles
  // per workgroup with both tiles' inputs loaded up front, i.e. one dispatch round at 2^20 lanes: 42.7-45.2 vs
  // 41.1-41.7 us for the pair, profiles/r03/ab_fused_tiles_per_wg.log.)
  static const int fused_cells = bsx_env_int("BSX_FUSED_TILE_MAX_CELLS", 128);
  constexpr int fused_step_mib = 128;
  static const int fused_roll_mib = bsx_env_int("BSX_FUSED_ROLLOUT_MAX_MIB", 128);
  // (64-lane tiles up to 2^18 lanes: catch 2^15 7.3 -> 5.6 us, 2^16 8.1 -> 6.0, 2^17 9.1 -> 8.0 (r04, ordinary stores:
  // profiles/r04/ab_catch_fused_tile64.log; 2^18 was 12.3 -> 12.7 then); re-measured in round 6 with non-temporal chunks, 2^17
  // 8.0 -> 6.8, 2^18 12.2 -> 11.55, 2^19 19.3 -> 19.8 (profiles/r06/ab_catch_tile64_nt_larger_batches.log): the limit stayed.
  // The chunks the product stores are write-through (bsx_fused_tile64_kernel, bsx_tile_stream has the measurements).)
  static const int64_t tile64_max_lanes = bsx_env_int("BSX_FUSED_TILE64_MAX_LANES", 1 << 18);
  const int64_t step_bytes = B * (int64_t)cells * 4;
  const bool fusable = call->obs_paint == nullptr && cells >= 4u && (int)cells <= fused_cells &&
                       (((uint64_t)B * cells) & 3ull) == 0 && (reinterpret_cast<uintptr_t>(out.observation) & 15u) == 0;
  // A WRAPPED step (RewardNoise / Logging / MT19937-exact draws: catch_noise's lane advance is 18 us against the lean 9) fuses at
  // EVERY batch size: inside the one launch the heavy advance of a tile hides among the other workgroups' tile stores, in front
  // of a stand-alone stream it does not — catch_noise/0 at 2^20 lanes 48.3-48.6 -> 42.8-43.2 us per step, rollout r32 49.0-49.5
  // -> 44.6-45.6, r8 48.9-49.8 -> 41.7-42.4 (profiles/r06/ab_catch_noise_fused_at_2p20.log; the lean step in the same call:
  // 41.0 -> 43.8, ab_catch_fused_at_2p20.log); 1.5 * 2^20 lanes 69.1-70.5 -> 63.5-64.1, 2^21 91.6-92.7 -> 82.9-83.5, 2^22
  // 200.6-202.1 -> 170.8-171.3 (ab_catch_wrapped_fused_larger.log).  (MiB; 2^20 = no limit in practice)
  static const int fused_wrapped_mib = bsx_env_int("BSX_FUSED_WRAPPED_MAX_MIB", 1 << 20);
  const bool lean_f = bsx_ctl_lean(a0.ctl);
  int fused_mib = T > 1 ? fused_roll_mib : fused_step_mib;
  if (!lean_f && fused_wrapped_mib > fused_mib) fused_mib = fused_wrapped_mib;
  const bool fused = fusable && step_bytes <= ((int64_t)fused_mib << 20);
  if (fused && T > 1) {
    const dim3 grid((unsigned)bsx_blocks_of(B)), block(BSX_BLOCK);
    if (lean_f) bsx_fused_rollout_kernel<Fam, true, HotFn><<<grid, block, 0, st>>>(a0, T, out.observation, cells, magic, fn);
    else bsx_fused_rollout_kernel<Fam, false, HotFn><<<grid, block, 0, st>>>(a0, T, out.observation, cells, magic, fn);
    return bsx_launch_status();
  }
  if (!pipelined || fused) {
    for (int t = 0; t < T && rc == 0; ++t) {
      const typename Fam::args s = at(t);
      if (call->obs_paint != nullptr) {
        rc = bsx_launch_advance_delta<Fam, HotFn>(s, fn, call->obs_paint, cells, st);
      } else if (fused && lean_f && B <= tile64_max_lanes) {
        // (64-lane tiles while the 256-lane grid would leave the chip under-filled: bsx_fused_tile64_kernel)
        const dim3 grid((unsigned)((B + BSX_WAVE - 1) / BSX_WAVE)), block(BSX_BLOCK);
        bsx_fused_tile64_kernel<Fam, true, HotFn><<<grid, block, 0, st>>>(s, s.out.observation, cells, magic, fn);
      } else if (fused) {
        const dim3 grid((unsigned)bsx_blocks_of(B)), block(BSX_BLOCK);
        if (lean_f) bsx_fused_tile_kernel<Fam, true, HotFn><<<grid, block, 0, st>>>(s, s.out.observation, cells, magic, fn);
        else bsx_fused_tile_kernel<Fam, false, HotFn><<<grid, block, 0, st>>>(s, s.out.observation, cells, magic, fn);
      } else {
        rc = bsx_launch_advance<Fam>(s, st);
        // stores/thread x 256 threads: a sharp optimum per family (profiles/r01/sweep_stream_*.log)
        if (rc == 0) rc = bsx_launch_hot_stream<HotFn, K>(s.out.observation, state, B, cells, magic, fn, st);
      }
    }
    return rc != 0 ? rc : bsx_launch_status();
  }
  int32_t* const col[2] = {state, call->state_alt};
  auto W = [&](int t) { return col[(T - 1 - t) & 1]; };      // the column advance(t) writes; W(T-1) = state
  const uint64_t adv_blocks = (uint64_t)bsx_blocks_of(B);
  const uint64_t str_blocks = ((uint64_t)B * cells + (uint64_t)K * 4 * BSX_BLOCK - 1) / ((uint64_t)K * 4 * BSX_BLOCK);
  if (adv_blocks + str_blocks > 0x7FFFFFFFull) return BSX_EINVAL;
  const bsx_div64 dv = bsx_make_div64(cells);
  const bool lean = bsx_ctl_lean(a0.ctl);
  typename Fam::args s = at(0);
  s.ctl.state_in = state; s.state = W(0);
  rc = bsx_launch_advance<Fam>(s, st);
  for (int t = 0; t + 1 < T && rc == 0; ++t) {
    s = at(t + 1);
    s.ctl.state_in = W(t); s.state = W(t + 1);
    float* obs_t = out.observation + (int64_t)t * B * (int64_t)cells;
    const dim3 grid((unsigned)(adv_blocks + str_blocks)), block(BSX_BLOCK);
    if (lean) bsx_pipelined_kernel<Fam, true, HotFn, K><<<grid, block, 0, st>>>(s, (uint32_t)adv_blocks, (uint32_t)place, obs_t, W(t), cells, magic, dv, fn);
    else bsx_pipelined_kernel<Fam, false, HotFn, K><<<grid, block, 0, st>>>(s, (uint32_t)adv_blocks, (uint32_t)place, obs_t, W(t), cells, magic, dv, fn);
  }
  if (rc == 0) rc = bsx_launch_hot_stream<HotFn, K>(out.observation + (int64_t)(T - 1) * B * (int64_t)cells, state, B, cells, magic, fn, st);
  return rc != 0 ? rc : bsx_launch_status();
}

#endif  // BSX_PAIR_HOST_H_
