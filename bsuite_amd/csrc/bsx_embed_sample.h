// bsx_embed_sample.h — the softmax policy of a fused sampled closed loop from a hidden-layer network on the index row
// (bsx_<family>_embedding_sample / bsx_<family>_embedding_sample_evaluate, sample_embedding / evaluate_sampled_embedding;
// deep_sea and catch): which action a lane draws from softmax(logits / temperature).  The logits are bsx_embed.h's, the draws,
// the noise, the score and the Gumbel-max over 2 or 3 actions are bsx_gumbel.h's and bsx_tab_sample.h's; what is added is
// their composition.  Plain C99 + BSX_HD so that the CPU tests compile the very same code with gcc
// (tests/csrc/embed_sample_shim.c).
#ifndef BSX_EMBED_SAMPLE_H_
#define BSX_EMBED_SAMPLE_H_

#include <stdint.h>

#include "bsx_embed.h"
#include "bsx_tab_sample.h"

// The action drawn for the index row cells[0..K-1] under w1[C + 2][H] and w2[A][H + 1] from the words w[0..A-1] (word a
// belongs to action a): bsx_embed_logits, then bsx_gumbel_select_n with beta = 1 / temperature.  The lowest index wins a tie,
// a NaN score never wins, a -inf logit masks its action (all -inf: action 0).
BSX_HD int32_t bsx_embed_sample_select(const float* w1, const float* w2, const int32_t* cells, int K, int C, int H, int A, double beta,
                                       const uint32_t* w) {
  float l[BSX_EMBED_MAX_ACTIONS];
  bsx_embed_logits(w1, w2, cells, K, C, H, A, l);
  return bsx_gumbel_select_n(l, A, beta, w);
}

// ... for (sample_seed, global lane id, call index): the words are block 0 of stream BSX_STREAM_SAMPLE.
BSX_HD int32_t bsx_embed_sample_action(const float* w1, const float* w2, const int32_t* cells, int K, int C, int H, int A, double beta,
                                       uint64_t sample_seed, uint64_t lane, uint64_t step) {
  const bsx_u32x4 u = bsx_gumbel_draws(sample_seed, lane, step);
  return bsx_embed_sample_select(w1, w2, cells, K, C, H, A, beta, u.v);
}

#endif  // BSX_EMBED_SAMPLE_H_
