// bsx_policy.h — the tabular policy of a fused closed-loop rollout (bsx_<family>_policy_rollout): which table entry a lane's
// observation selects, and which action the lane takes.  Plain C99 + BSX_HD so that the CPU tests compile the very same
// code with gcc (tests/csrc/policy_shim.c) and hold it against trajectories of the unmodified reference: a wrong key here
// is a silently different policy on the device.
#ifndef BSX_POLICY_H_
#define BSX_POLICY_H_

#include <stdint.h>

#include "../../include/bsx_stream.h"   // BSX_HD, Philox, BSX_STREAM_POLICY

// Bytes of a shared table (n_policies == 1) a workgroup keeps in LDS: every deep_sea (64 * 64 states at most) and catch
// boards up to rows * columns^2 = 4096 (the default 10 x 5 has 250).  Larger tables, and every population of tables, are
// read from global memory.
#define BSX_POLICY_LDS_BYTES 4096

// Observation keys: the row of the table a lane's index observation (BSX_CALL_OBS_INDEX) selects.
//   deep_sea  the observation itself, row * N + column (never looked up on the terminal observation -1: the lane resets
//             on the call that follows a LAST, and a resetting lane takes action 0);
//   catch     ball_cell * columns + paddle_x with paddle_x = paddle_cell - (rows - 1) * columns.
BSX_HD int32_t bsx_policy_key_deep_sea(int32_t cell) { return cell; }
BSX_HD int32_t bsx_policy_key_catch(int32_t ball_cell, int32_t paddle_cell, int32_t rows, int32_t columns) {
  return ball_cell * columns + (paddle_cell - (rows - 1) * columns);
}
// Entries of one table: deep_sea N * N, catch rows * columns * columns.
BSX_HD int32_t bsx_policy_states_deep_sea(int32_t size) { return size * size; }
BSX_HD int32_t bsx_policy_states_catch(int32_t rows, int32_t columns) { return rows * columns * columns; }

// What the kernels index with: a key outside the table (a state word the library did not write) reads an end of it
// instead of faulting, and a lane's policy_index is clamped to [0, n_policies - 1] the same way.
BSX_HD int32_t bsx_policy_clamp(int32_t v, int32_t n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// The exploration draws of (explore_seed, global lane id, call index): block 0 of stream BSX_STREAM_POLICY.
// Words 0, 1 are U() and word 2 is RandInt(num_actions) (include/bsx_stream.h); word 3 is unused.
BSX_HD bsx_u32x4 bsx_policy_draws(uint64_t explore_seed, uint64_t lane, uint64_t step) {
  bsx_draws d;
  bsx_draws_init(&d, explore_seed, lane, step, BSX_STREAM_POLICY);
  return bsx_philox4x32_10(d.c0, d.c1, d.c2, d.c3hi, d.k0, d.k1);
}

// The selection rule.  A lane that resets on this call takes action 0 (the step ignores it; nothing is looked up and
// nothing is drawn).  Otherwise, with epsilon > 0: U() < epsilon (f64 compare) takes RandInt(num_actions), else the table
// entry; with epsilon == 0 the words are not looked at.  The table entry is returned as it is: one outside the
// action_spec reaches the step like the same value passed to step().
BSX_HD int32_t bsx_policy_select(uint32_t table_byte, int resets, double epsilon, uint32_t w0, uint32_t w1, uint32_t w2,
                                 uint32_t num_actions) {
  if (resets) return 0;
  if (epsilon > 0.0) {
    const uint64_t k = ((uint64_t)(w0 >> 5) << 26) | (uint64_t)(w1 >> 6);
    const double u = (double)k * 0x1p-53;
    if (u < epsilon) return (int32_t)(((uint64_t)w2 * (uint64_t)num_actions) >> 32);
  }
  return (int32_t)table_byte;
}

// What bsx_<family>_policy_evaluate keeps of a lane's steps instead of writing them (evaluate_policy): the episodes that
// ended inside the call, the sum of all rewards, and the sum of the returns of the episodes that ended — the running
// episode's return so far is `acc`.  `reward` is the f64 reward of the lane advance, before any rounding to float32;
// step types are dm_env's (FIRST 0, MID 1, LAST 2: a FIRST step carries no reward).  Sums in step order, plain IEEE adds.
typedef struct { double acc, done, total; int32_t n; } bsx_eval_acc;
BSX_HD void bsx_eval_accumulate(bsx_eval_acc* e, int step_type, double reward) {
  if (step_type != 0) { e->acc += reward; e->total += reward; }
  if (step_type == 2) { e->done += e->acc; e->acc = 0.0; e->n += 1; }
}

#endif  // BSX_POLICY_H_
