// bsx_embed.h — the hidden-layer policy of a fused closed loop on the grid families (bsx_<family>_embedding_rollout /
// bsx_<family>_embedding_evaluate, rollout_embedding / evaluate_embedding; deep_sea and catch): which action a lane's index
// observation selects through one ReLU hidden layer whose first layer is a row gather.  Plain C99 + BSX_HD, in the idiom of
// bsx_mlp.h, so that the CPU tests compile the very same code with gcc (tests/csrc/embed_shim.c) and hold it against a
// numpy float32 restatement: a different rounding here is a silently different policy on the device.
#ifndef BSX_EMBED_H_
#define BSX_EMBED_H_

#include <stdint.h>

#include "bsx_mlp.h"                    // bsx_mlp_relu, BSX_MLP_MAX_HIDDEN (and BSX_HD, BSX_NO_CONTRACT)

// Entries of an index row (deep_sea 1, catch 2) and actions (deep_sea 2, catch 3).
#define BSX_EMBED_MAX_K 2
#define BSX_EMBED_MAX_ACTIONS 3

// One policy is w1[C + 2][H] and w2[A][H + 1], C the cells of the board: row c + 1 of w1 is the embedding of cell c, row 0 the
// row a -1 entry selects (utils.observations.index_embedding's layout), row C + 1 the hidden bias; column H of w2 is the bias.
#define BSX_EMBED_W1(C, H) (((C) + 2) * (H))
#define BSX_EMBED_W2(A, H) ((A) * ((H) + 1))

// The LDS copy of a shared pair (n_policies == 1) is the kernel's own layout: the rows of w1 at a stride of
// BSX_EMBED_STRIDE(H) floats — H rounded up to whole 16-byte chunks plus one chunk of padding, so that a lane's row starts on
// a 16-byte boundary and 16 lanes reading 16 rows touch 16 different groups of four banks (a stride of 64 floats puts every
// row on bank 0) — and w2 transposed, [H + 1][4].  A pair whose copy needs more than BSX_EMBED_LDS_BYTES is read from global
// memory, as every population is.  catch/0 (C = 50) with H = 64 needs 52 * 68 * 4 + 65 * 16 = 15184 bytes.
#define BSX_EMBED_STRIDE(H) ((((H) + 3) & ~3) + 4)
#define BSX_EMBED_LDS_BYTES 15360
#define BSX_EMBED_STAGED_BYTES(C, H) (4 * ((int64_t)((C) + 2) * BSX_EMBED_STRIDE(H) + 4 * ((H) + 1)))

// The rule, in the pieces the kernel calls (it consumes a hidden activation as it is produced: A logit accumulators, never H
// registers).  float32 throughout; every multiply and every add is rounded on its own — no FMA (the shim is compiled with
// -ffp-contract=off, as the library is).
//
// The row of w1 an entry of the index row selects: the cell clamped to [-1, C - 1] — no state word can fault — plus one.
BSX_HD int32_t bsx_embed_row(int32_t cell, int32_t n_cells) {
  return (cell < -1 ? -1 : (cell > n_cells - 1 ? n_cells - 1 : cell)) + 1;
}

// Hidden unit j from the hidden bias and the K embedding entries e[k] = w1[row_k][j], in the order of the index row (catch:
// ball, then paddle; the same cell twice is added twice, as index_embedding does):
//     s = bias; for k = 0 .. K-1: s = s + e[k];   h = bsx_mlp_relu(s): compare and select, NaN and -0.0 give +0.0
BSX_HD float bsx_embed_preactivation(float bias, const float* e, int K) {
  BSX_NO_CONTRACT
  float s = bias;
  for (int k = 0; k < K; ++k) s = s + e[k];
  return s;
}

// ... its contribution to the A logits, w2j[a] = w2[a][j]:   l_a = l_a + w2j[a] * h     (inf * 0 is a NaN logit)
BSX_HD void bsx_embed_accumulate(float* l, const float* w2j, float h, int A) {
  BSX_NO_CONTRACT
  for (int a = 0; a < A; ++a) {
    const float prod = w2j[a] * h;
    l[a] = l[a] + prod;
  }
}

// ... and the winner: the lowest index wins a tie; a NaN logit never wins, and a NaN l_0 is never beaten.
BSX_HD int32_t bsx_embed_argmax(const float* l, int A) {
  int32_t best = 0;
  float l_best = l[0];
  for (int a = 1; a < A; ++a)
    if (l[a] > l_best) { best = a; l_best = l[a]; }
  return best;
}

// The logits of the index row cells[0..K-1] under w1[C + 2][H] and w2[A][H + 1]:
//     l_a = w2[a][H]                                                       a = 0..A-1
//     for j = 0 .. H-1:  h = hidden unit j;  for a = 0..A-1: l_a = l_a + w2[a][j] * h
BSX_HD void bsx_embed_logits(const float* w1, const float* w2, const int32_t* cells, int K, int C, int H, int A, float* l) {
  int32_t row[BSX_EMBED_MAX_K];
  for (int k = 0; k < K; ++k) row[k] = bsx_embed_row(cells[k], C);
  for (int a = 0; a < A; ++a) l[a] = w2[a * (H + 1) + H];
  for (int j = 0; j < H; ++j) {
    float e[BSX_EMBED_MAX_K], w2j[BSX_EMBED_MAX_ACTIONS];
    for (int k = 0; k < K; ++k) e[k] = w1[row[k] * H + j];
    for (int a = 0; a < A; ++a) w2j[a] = w2[a * (H + 1) + j];
    bsx_embed_accumulate(l, w2j, bsx_mlp_relu(bsx_embed_preactivation(w1[(C + 1) * H + j], e, K)), A);
  }
}

// ... and its greedy action.
BSX_HD int32_t bsx_embed_select(const float* w1, const float* w2, const int32_t* cells, int K, int C, int H, int A) {
  float l[BSX_EMBED_MAX_ACTIONS];
  bsx_embed_logits(w1, w2, cells, K, C, H, A, l);
  return bsx_embed_argmax(l, A);
}

#endif  // BSX_EMBED_H_
