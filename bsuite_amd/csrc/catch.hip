// catch.hip — batched Catch for gfx950.  Replaces bsuite/environments/catch.py:68-114
// (`_reset`, `_step`, `_observation`) including its private auto-reset (:80-81).
//
// 221 B per lane per call at 10x5: 21 B of scalar columns + a 200 B board with at most two ones.
// The board is never materialised anywhere but in the output: a lane is its two hot cell indices
// (ball, paddle), decoded from the packed state.  Two launches per call:
//   advance  bsx_advance_kernel<catch_fam>: one lane per thread (paddle moves before the ball
//            drops, action ignored on the auto-reset call, `randint(columns)` on reset);
//   observe  bsx_hot_stream_kernel<catch_hot,2,256>: pure store stream over [B x rows*cols] f32.
//            rows*cols = 50 is not a multiple of 4, so a 16-byte chunk may straddle two lanes'
//            boards (one division per chunk, spill-over elements patched from lane l+1's state).
// Host code: the family's host trait (catch_host: cfg check, fill, make), step, the group setter, and the eight fused
// closed-loop entry points as one-statement delegations ("Host glue of the closed-loop calls").
#include "bsx_embed_device.h"
#include "bsx_pair_host.h"
#include "bsx_tab_eval.h"
#include "bsx_tab_sample_device.h"
#include "catch_fam.h"
#include "pair_mixed.h"

// What differs between the grid families on the host: the trait of bsx_grid_closed_loop (bsx_host.h).
namespace {                                 // (internal linkage: the library exports its C ABI and nothing else)
struct catch_host {
  typedef bsx_catch_t cfg_t;
  typedef catch_fam fam;
  typedef catch_hot hot_t;
  static constexpr int32_t code = BSX_FAM_CATCH, actions = 3;
  // The cfg's range check, the same for every entry point.
  static int check_cfg(const cfg_t* cfg) {
    return (cfg->rows < 2 || cfg->rows > 64 || cfg->columns < 1 || cfg->columns > 64) ? BSX_ERANGE : 0;
  }
  static int32_t states(const cfg_t* cfg) { return bsx_policy_states_catch(cfg->rows, cfg->columns); }
  static int32_t cells(const cfg_t* cfg) { return cfg->rows * cfg->columns; }
  static hot_t hot(const cfg_t* cfg) { return catch_hot{cfg->rows, cfg->columns}; }
  // The kernel argument struct of a checked call.
  static void fill(const cfg_t* cfg, const bsx_call_t* call, const int32_t* action, int32_t* state, bsx_timestep_t out, double* info,
                   fam::args* a) {
    a->ctl = bsx_make_ctl(call);
    a->action = action; a->state = state; a->out = out; a->info = info;
    a->rows = cfg->rows; a->columns = cfg->columns;
    a->tile_cells_magic = 0; a->_pad = 0;
  }
  // Validates one call's arguments and fills the kernel argument struct (step, the groups and the recording closed loops).
  static int make(const cfg_t* cfg, const bsx_call_t* call, const int32_t* action, int32_t* state, bsx_timestep_t out, double* info,
                  fam::args* a) {
    if (cfg == nullptr) return BSX_ENULL;
    int rc = bsx_check_call(call, action, out, /*delta_ok=*/true, /*narrow_ok=*/true);
    if (rc != 0) return rc;
    if ((rc = check_cfg(cfg)) != 0) return rc;
    if (call->n_lanes > 0 && (state == nullptr || info == nullptr)) return BSX_ENULL;
    fill(cfg, call, action, state, out, info, a);
    return 0;
  }
  template <class Union>
  static fam::args* of(Union& u) { return &u.catch_; }
};
}  // namespace

extern "C" int bsx_catch_step(const bsx_catch_t* cfg, const bsx_call_t* call, const int32_t* action,
                              int32_t* state, bsx_timestep_t out, double* info) {
  catch_fam::args a;
  int rc = catch_host::make(cfg, call, action, state, out, info, &a);
  if (rc != 0) return rc;
  if (call->n_lanes == 0) return 0;
  const uint32_t cells = (uint32_t)(cfg->rows * cfg->columns);
  return bsx_pair_call<catch_fam, catch_hot, 2>(a, call, action, state, out, cells, catch_hot{cfg->rows, cfg->columns});
}

// The eight fused closed-loop entry points: each body is stated once for both families, beside its kind's checks
// (bsx_policy_rollout_entry, bsx_pair_host.h; bsx_tab_eval_entry; bsx_tab_softmax_entry; bsx_embed_entry), over the one
// prologue of bsx_host.h.  A recording call is told from an evaluation by its output struct.
extern "C" int bsx_catch_policy_rollout(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy,
                                        int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_policy_rollout_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_catch_policy_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy,
                                         int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_tab_eval_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_catch_policy_sample(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                       int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_tab_softmax_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_catch_policy_sample_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                                int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_tab_softmax_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_catch_embedding_rollout(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                           int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_embed_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_catch_embedding_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                            int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_embed_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_catch_embedding_sample(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_sample_t* policy,
                                          int32_t* state, bsx_timestep_t out, double* info) {
  return bsx_embed_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_catch_embedding_sample_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_sample_t* policy,
                                                   int32_t* state, bsx_policy_eval_t out, double* info) {
  return bsx_embed_entry<catch_host>(cfg, call, policy, state, out, info);
}

extern "C" int bsx_group_set_catch(bsx_group_t* g, int32_t index, const bsx_catch_t* cfg, const bsx_call_t* call,
                                   const int32_t* action, int32_t* state, bsx_timestep_t out, double* info) {
  if (g == nullptr) return BSX_ENULL;
  if (call != nullptr && (bsx_call_obs(call) != 0 || bsx_call_index(call))) return BSX_EMODE;   // groups write float32 boards
  int rc;
  catch_fam::args a;
  if (bsx_is_mixed_pair_group(g)) {            // one segment of the mixed two-kernel group
    rc = catch_host::make(cfg, call, action, state, out, info, &a);
    if (rc != 0) return rc;
    a.ctl.state_in = call->state_alt;            // pipelined sweeps: the advance reads the other column
    const uint32_t cells = (uint32_t)(cfg->rows * cfg->columns);
    if (cells < 4u) return BSX_ERANGE;
    const bsx_stream_seg<catch_hot> sg = bsx_make_stream_seg(out.observation, state, a.ctl.n_lanes, cells, catch_hot{cfg->rows, cfg->columns});
    // Whole-sweep group, small boards, one state column (no state_alt): phase 0 — latency-bound, its memory pipe
    // idle — writes the segment's boards itself as fused tiles; the segment leaves the phase-1 store stream, where
    // its 8 KiB runs went at 3.7 TB/s (tools/sweep_stream_parts.py: 27 MB in 7.3 us of a 145 us stream).
    // (any lane count: the tile of workgroup b starts b*256*cells floats into the 16-byte-aligned array, and
    // bsx_tile_stream writes the < 4 floats behind the last whole chunk one by one.  The predicate is the one
    // sweep_batch.prepare_groups uses to decide whether the segment gets a second state column: BSX_FUSED_CATCH_MAX_CELLS.)
    const bool fused = g->family == BSX_FAM_SWEEP_MIXED && call->state_alt == nullptr && cells <= BSX_FUSED_CATCH_MAX_CELLS;
    if (fused) a.tile_cells_magic = sg.cells_magic;
    return bsx_mixed_put(g, BSX_FAM_CATCH, index, call, &a, sizeof(a), &sg, sizeof(sg),
                              (uint64_t)bsx_blocks_of(a.ctl.n_lanes),
                              fused ? 0 : bsx_flat_blocks((uint64_t)a.ctl.n_lanes * cells, PAIR_CATCH_K), 0);
  }
  rc = bsx_group_check_set(g, BSX_FAM_CATCH, index, call, sizeof(catch_fam::args),
                           sizeof(bsx_stream_seg<catch_hot>), 0);
  if (rc != 0) return rc;
  rc = catch_host::make(cfg, call, action, state, out, info, &a);
  if (rc != 0) return rc;
  g->launch = bsx_group_launch_pair<catch_fam, catch_hot, 2>;
  g->n_phases = 2;
  return bsx_group_put_pair<catch_fam, catch_hot>(g, index, a, out.observation, state,
                                                  (uint32_t)(cfg->rows * cfg->columns),
                                                  catch_hot{cfg->rows, cfg->columns}, 2);
}
