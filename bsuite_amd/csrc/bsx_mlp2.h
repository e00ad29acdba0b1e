// bsx_mlp2.h — the two-hidden-layer policy of a fused closed loop (bsx_<family>_mlp2_evaluate / _mlp2_rollout, evaluate_mlp2 /
// rollout_mlp2): which action a lane's float observation selects through two ReLU hidden layers.  Plain C99 + BSX_HD, built
// from bsx_mlp.h's pieces, so that the CPU tests compile the very same code with gcc (tests/csrc/mlp2_shim.c) and hold it
// against a numpy float32 restatement: a different rounding here is a silently different policy on the device.
#ifndef BSX_MLP2_H_
#define BSX_MLP2_H_

#include <stdint.h>

#include "bsx_mlp.h"                    // bsx_mlp_hidden / _relu / _accumulate / _argmax, BSX_MLP_MAX_HIDDEN

// floats of the three matrices of one policy: w1[H1][D + 1], w2[H2][H1 + 1] and w3[3][H2 + 1], the bias in the last column
// of each; 1 <= H1, H2 <= BSX_MLP_MAX_HIDDEN.
#define BSX_MLP2_W1(D, H1) ((H1) * ((D) + 1))
#define BSX_MLP2_W2(H1, H2) ((H2) * ((H1) + 1))
#define BSX_MLP2_W3(H2) (BSX_LINEAR_ACTIONS * ((H2) + 1))

// The rule.  float32 throughout; every multiply and every add is rounded on its own — no FMA (the shim is compiled with
// -ffp-contract=off, as the library is).
//     h1_j = bsx_mlp_hidden(w1[j], o, D)                                          j = 0 .. H1-1
//     s2_k = w2[k][H1];  for j = 0 .. H1-1: s2_k = s2_k + w2[k][j] * h1_j         k = 0 .. H2-1
//     h2_k = bsx_mlp_relu(s2_k)
//     l_a  = w3[a][H2];  for k = 0 .. H2-1: l_a = l_a + w3[a][k] * h2_k           a = 0 .. 2
//     best = bsx_mlp_argmax(l)
// For a fixed k the sum runs over j ascending, whichever way the two loops are nested: the kernel walks j outside and keeps
// the s2_k in registers, in the piece below.
//
// One hidden unit's contribution to n layer-2 accumulators, w2j[k] = w2[k][j]:   s2_k = s2_k + w2j[k] * h   (inf * 0 is a NaN)
BSX_HD void bsx_mlp2_accumulate(float* s2, const float* w2j, float h, int n) {
  BSX_NO_CONTRACT
  for (int k = 0; k < n; ++k) {
    const float prod = w2j[k] * h;
    s2[k] = s2[k] + prod;
  }
}

// Layer 2's pre-activations s2[0 .. H2-1] of row o[0 .. D-1], j outside as the kernel walks it.
BSX_HD void bsx_mlp2_preactivations(const float* w1, const float* w2, const float* o, int D, int H1, int H2, float* s2) {
  for (int k = 0; k < H2; ++k) s2[k] = w2[k * (H1 + 1) + H1];
  for (int j = 0; j < H1; ++j) {
    float w2j[BSX_MLP_MAX_HIDDEN];
    for (int k = 0; k < H2; ++k) w2j[k] = w2[k * (H1 + 1) + j];
    bsx_mlp2_accumulate(s2, w2j, bsx_mlp_hidden(w1 + j * (D + 1), o, D), H2);
  }
}

// The three logits of row o[] under w1[H1][D + 1], w2[H2][H1 + 1] and w3[3][H2 + 1].
BSX_HD void bsx_mlp2_logits(const float* w1, const float* w2, const float* w3, const float* o, int D, int H1, int H2, float* l) {
  float s2[BSX_MLP_MAX_HIDDEN];
  bsx_mlp2_preactivations(w1, w2, o, D, H1, H2, s2);
  for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) l[a] = w3[a * (H2 + 1) + H2];
  for (int k = 0; k < H2; ++k) {
    float w3k[BSX_LINEAR_ACTIONS];
    for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) w3k[a] = w3[a * (H2 + 1) + k];
    bsx_mlp_accumulate(l, w3k, bsx_mlp_relu(s2[k]));
  }
}

// ... and the greedy action: the lowest index wins a tie, a NaN never wins (bsx_mlp_argmax).
BSX_HD int32_t bsx_mlp2_select(const float* w1, const float* w2, const float* w3, const float* o, int D, int H1, int H2) {
  float l[BSX_LINEAR_ACTIONS];
  bsx_mlp2_logits(w1, w2, w3, o, D, H1, H2, l);
  return bsx_mlp_argmax(l);
}

#endif  // BSX_MLP2_H_
