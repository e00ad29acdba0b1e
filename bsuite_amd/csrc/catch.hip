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
#include "bsx_embed_device.h"
#include "bsx_pair_host.h"
#include "bsx_tab_eval.h"
#include "bsx_tab_sample_device.h"
#include "catch_fam.h"
#include "pair_mixed.h"

// The cfg's range check, the same for every entry point.
static int catch_check_cfg(const bsx_catch_t* cfg) {
  return (cfg->rows < 2 || cfg->rows > 64 || cfg->columns < 1 || cfg->columns > 64) ? BSX_ERANGE : 0;
}

// The kernel argument struct of a checked call.
static void catch_fill(const bsx_catch_t* cfg, const bsx_call_t* call, const int32_t* action, int32_t* state, bsx_timestep_t out,
                       double* info, catch_fam::args* a) {
  a->ctl = bsx_make_ctl(call);
  a->action = action; a->state = state; a->out = out; a->info = info;
  a->rows = cfg->rows; a->columns = cfg->columns;
  a->tile_cells_magic = 0; a->_pad = 0;
}

static int catch_make(const bsx_catch_t* cfg, const bsx_call_t* call, const int32_t* action, int32_t* state,
                      bsx_timestep_t out, double* info, catch_fam::args* a) {
  if (cfg == nullptr) return BSX_ENULL;
  int rc = bsx_check_call(call, action, out, /*delta_ok=*/true, /*narrow_ok=*/true);
  if (rc != 0) return rc;
  if ((rc = catch_check_cfg(cfg)) != 0) return rc;
  if (call->n_lanes > 0 && (state == nullptr || info == nullptr)) return BSX_ENULL;
  catch_fill(cfg, call, action, state, out, info, a);
  return 0;
}

extern "C" int bsx_catch_step(const bsx_catch_t* cfg, const bsx_call_t* call, const int32_t* action,
                              int32_t* state, bsx_timestep_t out, double* info) {
  catch_fam::args a;
  int rc = catch_make(cfg, call, action, state, out, info, &a);
  if (rc != 0) return rc;
  if (call->n_lanes == 0) return 0;
  const uint32_t cells = (uint32_t)(cfg->rows * cfg->columns);
  return bsx_pair_call<catch_fam, catch_hot, 2>(a, call, action, state, out, cells, catch_hot{cfg->rows, cfg->columns});
}

extern "C" int bsx_catch_policy_rollout(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy,
                                        int32_t* state, bsx_timestep_t out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_policy_call(call, policy, bsx_policy_states_catch(cfg->rows, cfg->columns), state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  catch_fam::args a;
  // (the action pointer of a policy rollout is never read: actions_out stands in for it in the common checks)
  rc = catch_make(cfg, call, policy->actions_out, state, out, info, &a);
  if (rc != 0) return rc;
  a.action = nullptr;
  return bsx_policy_rollout_call<catch_fam, catch_hot>(a, call, policy, 3u, out, catch_hot{cfg->rows, cfg->columns});
}

extern "C" int bsx_catch_policy_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy, int32_t* state,
                                          bsx_policy_eval_t out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_policy_eval_call(call, policy, bsx_policy_states_catch(cfg->rows, cfg->columns), state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_tab_eval_args e;
  catch_fill(cfg, call, nullptr, state, bsx_timestep_t{}, info, &e.fam.catch_);          // (no action column, no TimeStep)
  return bsx_tab_eval_call(e, BSX_FAM_CATCH, call, policy, 3u, out);
}

extern "C" int bsx_catch_policy_sample(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                       int32_t* state, bsx_timestep_t out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_tab_softmax_call(call, policy, bsx_policy_states_catch(cfg->rows, cfg->columns), 3, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_tab_softmax_args s;
  // (no action column is read: actions_out stands in for it in the common checks, as in bsx_catch_policy_rollout)
  rc = catch_make(cfg, call, policy->actions_out, state, out, info, &s.fam.catch_);
  if (rc != 0) return rc;
  s.fam.catch_.action = nullptr;
  return bsx_tab_softmax_call(s, BSX_FAM_CATCH, call, policy, true, reinterpret_cast<int32_t*>(out.observation), bsx_policy_eval_t{});
}

extern "C" int bsx_catch_policy_sample_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_logits_t* policy,
                                                int32_t* state, bsx_policy_eval_t out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_tab_softmax_eval_call(call, policy, bsx_policy_states_catch(cfg->rows, cfg->columns), 3, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_tab_softmax_args s;
  catch_fill(cfg, call, nullptr, state, bsx_timestep_t{}, info, &s.fam.catch_);          // (no action column, no TimeStep)
  return bsx_tab_softmax_call(s, BSX_FAM_CATCH, call, policy, false, nullptr, out);
}

extern "C" int bsx_catch_embedding_rollout(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                        int32_t* state, bsx_timestep_t out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_embed_call(call, policy, cfg->rows * cfg->columns, 3, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_embed_args s;
  // (no action column is read: actions_out stands in for it in the common checks, as in bsx_catch_policy_rollout)
  rc = catch_make(cfg, call, policy->actions_out, state, out, info, &s.fam.catch_);
  if (rc != 0) return rc;
  s.fam.catch_.action = nullptr;
  return bsx_embed_call(s, BSX_FAM_CATCH, call, policy, true, reinterpret_cast<int32_t*>(out.observation), bsx_policy_eval_t{});
}

extern "C" int bsx_catch_embedding_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_t* policy,
                                         int32_t* state, bsx_policy_eval_t out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_embed_eval_call(call, policy, cfg->rows * cfg->columns, 3, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_embed_args s;
  catch_fill(cfg, call, nullptr, state, bsx_timestep_t{}, info, &s.fam.catch_);          // (no action column, no TimeStep)
  return bsx_embed_call(s, BSX_FAM_CATCH, call, policy, false, nullptr, out);
}

extern "C" int bsx_catch_embedding_sample(const bsx_catch_t* cfg, const bsx_call_t* call, const bsx_policy_embedding_sample_t* policy,
                                       int32_t* state, bsx_timestep_t out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_embed_sample_call(call, policy, cfg->rows * cfg->columns, 3, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_embed_args s;
  // (no action column is read: actions_out stands in for it in the common checks, as in bsx_catch_policy_rollout)
  rc = catch_make(cfg, call, policy->actions_out, state, out, info, &s.fam.catch_);
  if (rc != 0) return rc;
  s.fam.catch_.action = nullptr;
  return bsx_embed_sample_call(s, BSX_FAM_CATCH, call, policy, true, reinterpret_cast<int32_t*>(out.observation), bsx_policy_eval_t{});
}

extern "C" int bsx_catch_embedding_sample_evaluate(const bsx_catch_t* cfg, const bsx_call_t* call,
                                                const bsx_policy_embedding_sample_t* policy, int32_t* state, bsx_policy_eval_t out,
                                                double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = catch_check_cfg(cfg);
  if (rc == 0) rc = bsx_check_embed_sample_eval_call(call, policy, cfg->rows * cfg->columns, 3, state, out, info);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_embed_args s;
  catch_fill(cfg, call, nullptr, state, bsx_timestep_t{}, info, &s.fam.catch_);          // (no action column, no TimeStep)
  return bsx_embed_sample_call(s, BSX_FAM_CATCH, call, policy, false, nullptr, out);
}

extern "C" int bsx_group_set_catch(bsx_group_t* g, int32_t index, const bsx_catch_t* cfg, const bsx_call_t* call,
                                   const int32_t* action, int32_t* state, bsx_timestep_t out, double* info) {
  if (g == nullptr) return BSX_ENULL;
  if (call != nullptr && (bsx_call_obs(call) != 0 || bsx_call_index(call))) return BSX_EMODE;   // groups write float32 boards
  int rc;
  catch_fam::args a;
  if (bsx_is_mixed_pair_group(g)) {            // one segment of the mixed two-kernel group
    rc = catch_make(cfg, call, action, state, out, info, &a);
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
  rc = catch_make(cfg, call, action, state, out, info, &a);
  if (rc != 0) return rc;
  g->launch = bsx_group_launch_pair<catch_fam, catch_hot, 2>;
  g->n_phases = 2;
  return bsx_group_put_pair<catch_fam, catch_hot>(g, index, a, out.observation, state,
                                                  (uint32_t)(cfg->rows * cfg->columns),
                                                  catch_hot{cfg->rows, cfg->columns}, 2);
}
