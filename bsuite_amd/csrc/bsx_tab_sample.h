// bsx_tab_sample.h — the softmax policy of a fused sampled rollout from a TABLE of logits (bsx_<family>_policy_sample /
// bsx_<family>_policy_sample_evaluate, sample_policy / evaluate_sampled_policy; deep_sea and catch): which action a lane
// draws from softmax(logits[row, key] / temperature).  The key of the lane's observation and its clamps are bsx_policy.h's,
// the draws, the noise and the score are bsx_gumbel.h's; what is added is the Gumbel-max over 2 or 3 actions.  Plain C99 +
// BSX_HD so that the CPU tests compile the very same code with gcc (tests/csrc/tab_sample_shim.c).
#ifndef BSX_TAB_SAMPLE_H_
#define BSX_TAB_SAMPLE_H_

#include <stdint.h>

#include "bsx_policy.h"
#include "bsx_gumbel.h"

// Actions of a table of logits: deep_sea 2, catch 3.
#define BSX_TAB_SAMPLE_MIN_ACTIONS 2
#define BSX_TAB_SAMPLE_MAX_ACTIONS 3

// Bytes of a shared table of logits (n_policies == 1) a workgroup keeps in LDS: [n_states, n_actions] float32 — every
// catch up to rows * columns^2 = 1024 and deep_sea up to N = 39.  Larger tables, and every population, are read from
// global memory.
#define BSX_TAB_SAMPLE_LDS_BYTES 12288

// Gumbel-max over n actions (n = 2 or 3): argmax_a z_a with z_a = bsx_gumbel_score(l[a], beta, w[a]) is a draw from
// softmax(beta * l).  The z_a are computed one after another; best = 0, and a >= 1 wins only with z_a > z_best.  For n == 3
// this is bsx_gumbel_select(l, beta, w[0], w[1], w[2]) for every input.  What follows from the rule:
//   a -inf logit masks its action: the noise is finite, so z_a = -inf never exceeds a finite z_best (all -inf: action 0);
//   a NaN z_a never wins: `NaN > z_best` is false;
//   a NaN z_0 is never beaten: `z_a > NaN` is false.
BSX_HD int32_t bsx_gumbel_select_n(const float* l, int n, double beta, const uint32_t* w) {
  int32_t best = 0;
  double z_best = bsx_gumbel_score(l[0], beta, w[0]);
  for (int a = 1; a < n; ++a) {
    const double z = bsx_gumbel_score(l[a], beta, w[a]);
    if (z > z_best) { best = a; z_best = z; }
  }
  return best;
}

#endif  // BSX_TAB_SAMPLE_H_
