// bsx_mlp.h — the hidden-layer policy of a fused evaluation (bsx_<family>_mlp_evaluate, evaluate_mlp): which action a
// lane's float observation selects through one ReLU hidden layer.  Plain C99 + BSX_HD, in the idiom of bsx_linear.h, so
// that the CPU tests compile the very same code with gcc (tests/csrc/mlp_shim.c) and hold it against a numpy float32
// restatement: a different rounding here is a silently different policy on the device.
#ifndef BSX_MLP_H_
#define BSX_MLP_H_

#include <stdint.h>

#include "bsx_linear.h"                 // BSX_LINEAR_ACTIONS, BSX_LINEAR_MAX_OBS (and BSX_HD, BSX_NO_CONTRACT)

// Hidden units of one policy: a run-time value in [1, BSX_MLP_MAX_HIDDEN].  The cap is a design choice: a shared pair of
// matrices is then at most 64 * 9 + 3 * 65 = 771 floats, which a workgroup keeps in 3084 B of LDS.
#define BSX_MLP_MAX_HIDDEN 64
// floats of the two matrices of one policy: w1[H][D + 1] and w2[3][H + 1], the bias in the last column of each
#define BSX_MLP_W1(D, H) ((H) * ((D) + 1))
#define BSX_MLP_W2(H) (BSX_LINEAR_ACTIONS * ((H) + 1))

// The rule, in the pieces the kernel calls (it consumes a hidden activation as it is produced: three logit accumulators
// and the row o[], never H registers).  float32 throughout; every multiply and every add is rounded on its own — no FMA
// (gcc has no pragma for the contraction: the shim is compiled with -ffp-contract=off, as the library is).
//
// Hidden unit j from its row w1j[0..D] of w1 (w1j[D] the bias):
//     s = w1j[D]; for d = 0 .. D-1: s = s + w1j[d] * o[d];   h = (s > 0.0f) ? s : 0.0f
// The ReLU is a compare and a select, not a maximum: a NaN and a -0.0 pre-activation give +0.0, -inf gives +0.0, +inf inf.
BSX_HD float bsx_mlp_preactivation(const float* w1j, const float* o, int D) {
  BSX_NO_CONTRACT
  float s = w1j[D];
  for (int d = 0; d < D; ++d) {
    const float prod = w1j[d] * o[d];
    s = s + prod;
  }
  return s;
}
BSX_HD float bsx_mlp_relu(float s) { return (s > 0.0f) ? s : 0.0f; }
BSX_HD float bsx_mlp_hidden(const float* w1j, const float* o, int D) { return bsx_mlp_relu(bsx_mlp_preactivation(w1j, o, D)); }

// ... its contribution to the three logits, w2j[a] = w2[a][j]:   l_a = l_a + w2j[a] * h     (inf * 0 is a NaN logit)
BSX_HD void bsx_mlp_accumulate(float* l, const float* w2j, float h) {
  BSX_NO_CONTRACT
  for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) {
    const float prod = w2j[a] * h;
    l[a] = l[a] + prod;
  }
}

// ... and the winner — bsx_linear_select's rule: the lowest index wins a tie; a NaN logit never wins, and a NaN l_0 is never
// beaten.
BSX_HD int32_t bsx_mlp_argmax(const float* l) {
  int32_t best = 0;
  float l_best = l[0];
  for (int a = 1; a < BSX_LINEAR_ACTIONS; ++a)
    if (l[a] > l_best) { best = a; l_best = l[a]; }
  return best;
}

// The greedy action of observation o[0..D-1] under w1[H][D + 1] and w2[3][H + 1]:
//     l_a = w2[a][H]                                           a = 0..2
//     for j = 0 .. H-1:  h = hidden unit j;  for a = 0..2: l_a = l_a + w2[a][j] * h
//     best = argmax, as above
BSX_HD int32_t bsx_mlp_select(const float* w1, const float* w2, const float* o, int D, int H) {
  float l[BSX_LINEAR_ACTIONS];
  for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) l[a] = w2[a * (H + 1) + H];
  for (int j = 0; j < H; ++j) {
    float w2j[BSX_LINEAR_ACTIONS];
    for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) w2j[a] = w2[a * (H + 1) + j];
    bsx_mlp_accumulate(l, w2j, bsx_mlp_hidden(w1 + j * (D + 1), o, D));
  }
  return bsx_mlp_argmax(l);
}

#endif  // BSX_MLP_H_
