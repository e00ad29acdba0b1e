// bsx_linear.h — the linear policy of a fused linear evaluation (bsx_<family>_linear_evaluate, evaluate_linear): which
// action a lane's float observation selects.  Plain C99 + BSX_HD, in the idiom of bsx_policy.h, so that the CPU tests
// compile the very same code with gcc (tests/csrc/linear_shim.c) and hold it against a numpy float32 restatement: a
// different rounding here is a silently different policy on the device.
#ifndef BSX_LINEAR_H_
#define BSX_LINEAR_H_

#include <stdint.h>

#include "../../include/bsx_stream.h"   // BSX_HD, BSX_NO_CONTRACT

// The three physics families have three actions; their observation rows have 3 (mountain_car), 6 (cartpole) or 8
// (swing-up) floats.
#define BSX_LINEAR_ACTIONS 3
#define BSX_LINEAR_MAX_OBS 8
// floats of one weight matrix [A, D + 1]: row a holds the D weights of action a and, in column D, its bias
#define BSX_LINEAR_ROW(D) (BSX_LINEAR_ACTIONS * ((D) + 1))

// The greedy action of observation o[0..D-1] under the matrix w[A][D + 1]:
//     l_a = w[a][D]; for d = 0 .. D-1: l_a = l_a + w[a][d] * o[d]          (float32; every multiply and every add is
//                                                                           rounded on its own — no FMA)
//     best = 0; for a = 1 .. A-1: if (l_a > l_best) best = a                (the lowest index wins a tie; a NaN logit
//                                                                           never wins, and a NaN l_0 is never beaten)
// (gcc has no pragma for the contraction: the shim is compiled with -ffp-contract=off, as the library is.)
BSX_HD int32_t bsx_linear_select(const float* w, const float* o, int D) {
  BSX_NO_CONTRACT
  int32_t best = 0;
  float l_best = 0.0f;
  for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) {
    const float* wa = w + a * (D + 1);
    float l = wa[D];
    for (int d = 0; d < D; ++d) {
      const float prod = wa[d] * o[d];
      l = l + prod;
    }
    if (a == 0) l_best = l;
    else if (l > l_best) { best = a; l_best = l; }
  }
  return best;
}

#endif  // BSX_LINEAR_H_
