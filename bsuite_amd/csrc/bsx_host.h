// bsx_host.h — host-side glue shared by the C-ABI entry points (argument checks, launch math, the grouped launch, the one
// prologue of the fused closed-loop calls).
#ifndef BSX_HOST_H_
#define BSX_HOST_H_

#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bsx_device.h"

// Observation element code of a call (bsx_call_t.flags, BSX_CALL_OBS_*): 0 float32, 1 uint8, 2 float16, 3 bfloat16.
static inline int bsx_call_obs(const bsx_call_t* call) { return (call->flags & BSX_CALL_OBS_MASK) >> BSX_CALL_OBS_SHIFT; }

// Index observations (BSX_CALL_OBS_INDEX): out.observation is int32 [n_lanes, K] hot-cell numbers instead of a board.
static inline bool bsx_call_index(const bsx_call_t* call) { return (call->flags & BSX_CALL_OBS_INDEX) != 0; }

// delta_ok / narrow_ok: the family has the delta observation mode (obs_paint) / the narrow observation codes and the
// index observations (deep_sea and catch have all of them, nobody else any).
static inline int bsx_check_call(const bsx_call_t* call, const void* action, const bsx_timestep_t& out,
                                 bool delta_ok = false, bool narrow_ok = false) {
  if (call == nullptr) return BSX_ENULL;
  if (call->obs_paint != nullptr && (!delta_ok || call->n_steps > 1)) return BSX_EMODE;
  if (bsx_call_obs(call) != 0 && (!narrow_ok || call->obs_paint != nullptr)) return BSX_EMODE;
  if (bsx_call_index(call) && (!narrow_ok || call->obs_paint != nullptr || bsx_call_obs(call) != 0)) return BSX_EMODE;
  if (call->n_lanes < 0 || call->n_lanes > ((int64_t)1 << 40)) return BSX_EINVAL;
  if (call->n_lanes == 0) return 0;
  if (out.reward == nullptr || out.discount == nullptr || out.step_type == nullptr ||
      out.observation == nullptr)
    return BSX_ENULL;
  if (action == nullptr && !call->force_reset) return BSX_ENULL;
  if ((reinterpret_cast<uintptr_t>(out.observation) & 15u) != 0) return BSX_EALIGN;
  if (call->wrap.kind < BSX_WRAP_NONE || call->wrap.kind > BSX_WRAP_NOISE_SCALE) return BSX_EINVAL;
  if (call->n_steps < 0 || (call->n_steps > 1 && call->force_reset)) return BSX_EINVAL;
  // action ring: a power of two of rows, for single-step calls only (a rollout already takes [T,B] actions)
  if (call->action_ring < 0 || (call->action_ring & (call->action_ring - 1)) != 0) return BSX_EINVAL;
  if (call->action_ring > 1 && (call->n_steps > 1 || call->obs_paint != nullptr)) return BSX_EMODE;
  if ((call->stream.mt_state == nullptr) != (call->stream.mt_pos == nullptr)) return BSX_ENULL;
  if ((call->stream.mt_gauss == nullptr) != (call->stream.mt_has_gauss == nullptr)) return BSX_ENULL;
  if (call->stream.mt_state != nullptr && call->wrap.kind >= BSX_WRAP_NOISE &&
      (call->wrap.mt_state == nullptr || call->wrap.mt_pos == nullptr || call->wrap.mt_gauss == nullptr ||
       call->wrap.mt_has_gauss == nullptr))
    return BSX_ENULL;                      // MT19937-exact RewardNoise needs the wrapper's own generator
  if (call->logging != nullptr) {
    const bsx_logging_t* g = call->logging;
    if (g->steps == nullptr || g->episode == nullptr || g->total_return == nullptr || g->episode_len == nullptr ||
        g->episode_return == nullptr || g->rows == nullptr || g->n_rows == nullptr)
      return BSX_ENULL;
    if (g->n_info < 0 || g->max_rows < 0 || g->n_log_points < 0) return BSX_EINVAL;
    if (g->n_info > 0 && g->info == nullptr) return BSX_ENULL;
    if (g->n_log_points > 0 && g->log_points == nullptr) return BSX_ENULL;
  }
  return 0;
}

static inline bsx_ctl bsx_make_ctl(const bsx_call_t* call) {
  bsx_ctl c;
  c.n_lanes = call->n_lanes;
  c.seed = call->stream.seed;
  c.lane_offset = call->stream.lane_offset;
  c.step_index = call->stream.step_index;
  c.step_base = call->stream.step_base;
  c.counters = call->counters;
  c.wrap_param = call->wrap.param;
  c.wrap_param2 = call->wrap.param2;
  c.wrap_seed = call->wrap.seed;
  c.wrap_kind = call->wrap.kind;
  c.wrap_mul = call->wrap.kind == BSX_WRAP_SCALE ? call->wrap.param : 1.0;
  c.force_reset = call->force_reset;
  c.action_ring_mask = call->action_ring > 1 ? (uint32_t)call->action_ring - 1u : 0u;
  c._pad = 0;
  c.mt_state = call->stream.mt_state;
  c.mt_pos = call->stream.mt_pos;
  c.mt_gauss = call->stream.mt_gauss;
  c.mt_has_gauss = call->stream.mt_has_gauss;
  const bool wrap_mt = call->stream.mt_state != nullptr && call->wrap.kind >= BSX_WRAP_NOISE;
  c.wrap_mt_state = wrap_mt ? call->wrap.mt_state : nullptr;
  c.wrap_mt_pos = wrap_mt ? call->wrap.mt_pos : nullptr;
  c.wrap_mt_gauss = wrap_mt ? call->wrap.mt_gauss : nullptr;
  c.wrap_mt_has_gauss = wrap_mt ? call->wrap.mt_has_gauss : nullptr;
  c.reward_f64 = call->reward_f64;
  c.state_in = nullptr;
  if (call->logging != nullptr) c.log = *call->logging;
  else c.log = bsx_logging_t{};
  return c;
}

static inline int bsx_n_steps(const bsx_call_t* call) { return call->n_steps > 1 ? call->n_steps : 1; }

// workgroups of BSX_BLOCK threads for n lanes (or other items), one each
static inline int64_t bsx_blocks_of(int64_t n) { return (n + BSX_BLOCK - 1) / BSX_BLOCK; }

// magic for q = n / d via __umulhi(n, magic): exact for n < 2^20, d <= 4096
static inline uint32_t bsx_div_magic(uint32_t d) { return (uint32_t)((0x100000000ull / d) + 1ull); }

// A/B knobs.  The product library never reads the environment: the knobs exist only in the
// tuning build (`python -m bsuite_amd.build --tuning` -> libbsuite_amd_tuning.so, compiled with -DBSX_TUNING and
// loaded through BSX_NATIVE_LIB by the A/B scripts under tools/ and by the tests that cover the non-default
// settings); everywhere else every knob is its measured-best default, fixed at compile time.
static inline int bsx_env_int(const char* name, int dflt) {
#ifdef BSX_TUNING
  const char* v = getenv(name);
  return (v != nullptr && *v != '\0') ? atoi(v) : dflt;
#else
  (void)name;
  return dflt;
#endif
}

// Exact 64-bit magic for n / d (4 <= d <= 4096, n < 2^52): s = floor(log2 d) - 1.
static inline bsx_div64 bsx_make_div64(uint32_t d) {
  bsx_div64 r;
  uint32_t lg = 0;
  while ((2u << lg) <= d) ++lg;             // lg = floor(log2 d)
  r.s = lg - 1;
  const unsigned __int128 num = (unsigned __int128)1 << (64 + r.s);
  r.m = (uint64_t)(num / d) + 1;
  return r;
}

// ---------------------------------------------------------------------------------------------
// Grouped launch (bsx_group_t): host-side container.  Each family file fills `args`/`args2` (its
// kernel argument structs, one per segment) and the per-segment block counts, and installs `launch`.
struct bsx_group {
  int32_t family = -1;
  int32_t n = 0;
  int32_t klass = -1;                   // family-specific launch class (lanes per workgroup of small_obs), -1 unset
  size_t arg_size = 0, arg2_size = 0;
  std::vector<uint8_t> args, args2;     // n * arg_size  /  n * arg2_size (second kernel of a pair)
  std::vector<int32_t> blocks, blocks2; // workgroups of each segment in kernel 1 / kernel 2
  std::vector<uint8_t> is_set;
  std::vector<int32_t> tags;            // BSX_FAM_PAIR_MIXED: family of each segment (empty otherwise)
  int32_t* d_tags = nullptr;
  uint64_t* shared_counter = nullptr;   // BSX_FAM_SWEEP_MIXED: the call counter every segment reads; phase 0 bumps it
  uint32_t* d_ticket = nullptr;         //   ... when its last workgroup retires (device word, zero between launches)
  size_t lds_bytes = 0;                 // max dynamic LDS over segments (kernel 1)
  uint64_t* trace = nullptr;            // diagnostics (bsx_group_trace): per-workgroup [start, end, tag] of phase 0
  void* d_args = nullptr;
  void* d_args2 = nullptr;
  int32_t* d_start = nullptr;           // [n+1] exclusive prefix of blocks
  int32_t* d_start2 = nullptr;
  int2* d_map = nullptr;                // [total_blocks] (segment, local block) per workgroup, or null
  int2* d_map2 = nullptr;
  bsx_group_index index1() const { bsx_group_index gi; gi.start = d_start; gi.map = d_map; gi.n = n; return gi; }
  bsx_group_index index2() const { bsx_group_index gi; gi.start = d_start2; gi.map = d_map2; gi.n = n; return gi; }
  int64_t total_blocks = 0, total_blocks2 = 0;
  bool committed = false;
  // a two-kernel segment that has store-stream workgroups but one state column only: fine for {advance, stream} in
  // order, a race in the pipelined launch (the stream of step s would read the column the advance of s+1 writes)
  bool stream_without_alt = false;      // = any(needs_alt), evaluated at commit
  std::vector<uint8_t> needs_alt;       // per segment (mixed groups)
  std::vector<const void*> row_scratch; // per segment: the row scratch of a chain segment on the row path, else null
  std::vector<uintptr_t> rows_sorted;   // the non-null ones, sorted (frozen at commit: bsx_group_step_pipelined's aliasing check)
  int64_t split_block = -1;             // whole-sweep groups: first phase-0 workgroup of the segments that have a share of
                                        // the store stream, when those segments are the tail of the group (else -1)
  int64_t split_round = -1;             // workgroups of the split step's first launch (sweep_mixed.hip), derived on first use
  // launch(g, phase, stream): phase 0 = the first kernel (the lane advance of a two-kernel family, or the
  // whole step of a small-observation group), phase 1 = the observation stream kernel of a two-kernel
  // family (depends on phase 0 of the same group only), phase < 0 = both in order.
  int (*launch)(bsx_group*, int, hipStream_t) = nullptr;
  int n_phases = 1;
};

static inline uint64_t bsx_flat_blocks(uint64_t total_floats, int k) {
  const uint64_t per_block = (uint64_t)k * 4 * BSX_BLOCK;
  return (total_floats + per_block - 1) / per_block;
}

// Common validation + bookkeeping of bsx_group_set_<family>.
static inline int bsx_group_check_set(bsx_group* g, int32_t family, int32_t index, const bsx_call_t* call,
                                      size_t arg_size, size_t arg2_size, int klass) {
  if (g == nullptr || call == nullptr) return BSX_ENULL;
  if (bsx_call_index(call)) return BSX_EMODE;                                    // groups write dense boards
  if (g->committed || g->family != family || index < 0 || index >= g->n) return BSX_EINVAL;
  if (call->stream.step_base == nullptr || call->force_reset || call->n_steps > 1 || call->n_lanes < 1)
    return BSX_EINVAL;                 // static arguments need a device-resident call counter
  if (call->obs_paint != nullptr) return BSX_EMODE;
  if (g->klass >= 0 && g->klass != klass) return BSX_EINVAL;
  g->klass = klass;
  if (g->args.empty()) {
    g->arg_size = arg_size; g->arg2_size = arg2_size;
    g->args.assign((size_t)g->n * arg_size, 0);
    g->args2.assign((size_t)g->n * arg2_size, 0);
  }
  if (g->arg_size != arg_size || g->arg2_size != arg2_size) return BSX_EINVAL;
  return 0;
}

static inline int bsx_launch_status() { return (int)hipGetLastError(); }

// ---------------------------------------------------------------------------------------------
// The host-side prologue of the forty fused closed-loop entry points bsx_<family>_<kind>_<verb>, once per group of
// families.  A family's .hip defines a host trait `Fam` with what differs between the families; a kind's header gives its
// family-free refusals (`check`) and its fill-and-launch (`launch`) and states each entry's body once, as a template over
// Fam; the extern "C" definitions in the family's .hip are one-statement delegations.  The order of the refusals is the
// documented one (include/bsuite_amd.h): null structs, the cfg's range, the kind's modes / scalars / pointers, an empty
// call (code 0), and only then the kernel's arguments and whatever the launch itself refuses (the grid bound).
//
// cartpole, mountain_car (linear, mlp, mlp2).  Fam:
//   cfg_t, env, code    the cfg struct, the device-side family (env::args), BSX_FAM_*
//   range(cfg, a)       the cfg's range check — 0 or BSX_ERANGE — leaving what it derives from the cfg in *a
//   obs_numel(cfg)      floats per observation row;  extra(cfg): a pointer only the family needs, or any non-null
//   fill(cfg, call, action, state, steps, out, info, a)   the rest of *a (the family's make() fills through it too)
//   of(fam)             the family's member of a kernel's `fam` union
// `fam` is that union in the kind's argument struct; check(extra, D) and launch(family code) are the kind's.
template <class Fam, class Union, class Policy, class Check, class Launch>
static inline int bsx_physics_closed_loop(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const Policy* policy, float* state,
                                          int32_t* steps, double* info, Union& fam, Check check, Launch launch) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  typename Fam::env::args* a = Fam::of(fam);
  int rc = Fam::range(cfg, a);
  if (rc == 0) rc = check(Fam::extra(cfg), Fam::obs_numel(cfg));
  if (rc != 0 || call->n_lanes == 0) return rc;
  // (no action column; no TimeStep: a recording kernel reads its own struct's)
  Fam::fill(cfg, call, nullptr, state, steps, bsx_timestep_t{}, info, a);
  return launch(Fam::code);
}

// deep_sea, catch (policy, embedding).  Fam:
//   cfg_t, fam, hot_t, code, actions    the cfg struct, the device-side family (fam::args), its hot-cell functor, BSX_FAM_*, |A|
//   check_cfg(cfg), states(cfg), cells(cfg), hot(cfg)    the cfg's range check, the table length, the board's cells, the functor
//   make(...) / fill(...)               the family's checked / unchecked kernel arguments (step and the groups use make too)
//   of(fam)                             the family's member of a kernel's `fam` union
// `record`: the [T,B] TimeStep of a recording call — its *a comes from make() with actions_out standing in for the action
// column in the common checks, and no action column is read — or null: an evaluation has no action column and no TimeStep.
template <class Fam, class Policy, class Check, class Launch>
static inline int bsx_grid_closed_loop(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const Policy* policy, int32_t* state,
                                       const bsx_timestep_t* record, double* info, typename Fam::fam::args* a, Check check,
                                       Launch launch) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = Fam::check_cfg(cfg);
  if (rc == 0) rc = check();
  if (rc != 0 || call->n_lanes == 0) return rc;
  if (record != nullptr) {
    rc = Fam::make(cfg, call, policy->actions_out, state, *record, info, a);
    if (rc != 0) return rc;
    a->action = nullptr;
  } else {
    Fam::fill(cfg, call, nullptr, state, bsx_timestep_t{}, info, a);
  }
  return launch();
}

#endif  // BSX_HOST_H_
