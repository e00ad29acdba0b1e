// bsx_gumbel.h — the softmax policy of a fused sampled trajectory (bsx_<family>_linear_sample / bsx_<family>_mlp_sample,
// sample_linear / sample_mlp): which action a lane draws from softmax(logits / temperature).  Plain C99 + BSX_HD, in the
// idiom of bsx_linear.h / bsx_mlp.h, so that the CPU tests compile the very same code with gcc (tests/csrc/gumbel_shim.c)
// and hold it against a numpy float64 restatement: a different rounding here is a silently different sample on the device.
#ifndef BSX_GUMBEL_H_
#define BSX_GUMBEL_H_

#include <stdint.h>

#include "bsx_mlp.h"                    // bsx_linear.h, the hidden-layer pieces (and BSX_HD, BSX_NO_CONTRACT, bsx_log, Philox)

// The logits of observation o[0..D-1] under the matrix w[A][D + 1] — exactly the accumulations of bsx_linear_select:
//     l_a = w[a][D]; for d = 0 .. D-1: l_a = l_a + w[a][d] * o[d]          (float32; every multiply and every add is
//                                                                           rounded on its own — no FMA)
// so argmax(l) under bsx_mlp_argmax's rule is bsx_linear_select(w, o, D).  (The hidden-layer logits are bsx_mlp.h's pieces:
// l_a = w2[a][H], then bsx_mlp_accumulate(l, w2j, bsx_mlp_hidden(w1j, o, D)) for j = 0 .. H-1.)
BSX_HD void bsx_linear_logits(const float* w, const float* o, int D, float* l) {
  BSX_NO_CONTRACT
  for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) {
    const float* wa = w + a * (D + 1);
    float acc = wa[D];
    for (int d = 0; d < D; ++d) {
      const float prod = wa[d] * o[d];
      acc = acc + prod;
    }
    l[a] = acc;
  }
}

// The Gumbel draws of (sample_seed, global lane id, call index): block 0 of stream BSX_STREAM_SAMPLE.  Word a belongs to
// action a (include/bsx_stream.h); word 3 is unused.
BSX_HD bsx_u32x4 bsx_gumbel_draws(uint64_t sample_seed, uint64_t lane, uint64_t step) {
  bsx_draws d;
  bsx_draws_init(&d, sample_seed, lane, step, BSX_STREAM_SAMPLE);
  return bsx_philox4x32_10(d.c0, d.c1, d.c2, d.c3hi, d.k0, d.k1);
}

// A standard Gumbel variate from one word, float64:
//     u = ((double)word + 0.5) * 2^-32        exact, in (0, 1): [2^-33, 1 - 2^-33]
//     e = -bsx_log(u)                          in [1.16e-10, 22.9]
//     g = -bsx_log(e)                          finite for every word
// bsx_log (include/bsx_stream.h) is the project's bit-reproducible logarithm; its algorithm holds for every positive normal
// double, not only for the (0, 1] its comment names.
BSX_HD double bsx_gumbel_noise(uint32_t word) {
  BSX_NO_CONTRACT
  const double u = ((double)word + 0.5) * 0x1p-32;
  const double e = -bsx_log(u);
  return -bsx_log(e);
}

// The perturbed logit of one action: z = (double)l * beta + g, the multiply and the add rounded on their own (beta is
// 1 / temperature, computed by the caller: nothing here divides by it).
BSX_HD double bsx_gumbel_score(float l, double beta, uint32_t word) {
  BSX_NO_CONTRACT
  const double scaled = (double)l * beta;
  return scaled + bsx_gumbel_noise(word);
}

// Gumbel-max over the three actions: argmax_a z_a is a draw from softmax(beta * l).  The z_a are computed one after another;
// best = 0, and a = 1, 2 wins only with z_a > z_best — the rule of bsx_linear_select: the lowest index wins a tie, a NaN z_a
// never wins, and a NaN z_0 is never beaten.
BSX_HD int32_t bsx_gumbel_select(const float* l, double beta, uint32_t w0, uint32_t w1, uint32_t w2) {
  int32_t best = 0;
  double z_best = bsx_gumbel_score(l[0], beta, w0);
  const double z1 = bsx_gumbel_score(l[1], beta, w1);
  if (z1 > z_best) { best = 1; z_best = z1; }
  const double z2 = bsx_gumbel_score(l[2], beta, w2);
  if (z2 > z_best) { best = 2; z_best = z2; }
  return best;
}

// The hidden-layer logits as one call — bsx_mlp_select's walk over bsx_mlp.h's pieces, without its argmax (the kernel walks
// the same pieces itself, unit by unit from where its matrices lie: bsx_gumbel_hidden_logits, bsx_gumbel_device.h).
BSX_HD void bsx_mlp_logits(const float* w1, const float* w2, const float* o, int D, int H, float* l) {
  for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) l[a] = w2[a * (H + 1) + H];
  for (int j = 0; j < H; ++j) {
    float w2j[BSX_LINEAR_ACTIONS];
    for (int a = 0; a < BSX_LINEAR_ACTIONS; ++a) w2j[a] = w2[a * (H + 1) + j];
    bsx_mlp_accumulate(l, w2j, bsx_mlp_hidden(w1 + j * (D + 1), o, D));
  }
}

#endif  // BSX_GUMBEL_H_
