/* Test shim: the softmax decision of a fused sampled trajectory (bsx_linear_logits, bsx_mlp_logits, bsx_gumbel_noise,
 * bsx_gumbel_score, bsx_gumbel_select and bsx_gumbel_draws, bsuite_amd/csrc/bsx_gumbel.h — the header the HIP kernel
 * compiles), evaluated on the host by gcc with -ffp-contract=off.  Case c has its own weights, row o[c] = [D], words
 * w[c] = [3] and inverse temperature beta[c]. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_gumbel.h"

/* logits [n, 3], the sampled action [n] and the greedy action of the existing rule [n] */
void shim_linear(int64_t n_cases, int32_t D, const float* w, const float* o, const uint32_t* words, const double* beta,
                 float* logits, int32_t* action, int32_t* greedy) {
  for (int64_t c = 0; c < n_cases; ++c) {
    bsx_linear_logits(w + c * BSX_LINEAR_ROW(D), o + c * D, D, logits + 3 * c);
    action[c] = bsx_gumbel_select(logits + 3 * c, beta[c], words[3 * c], words[3 * c + 1], words[3 * c + 2]);
    greedy[c] = bsx_linear_select(w + c * BSX_LINEAR_ROW(D), o + c * D, D);
  }
}

void shim_mlp(int64_t n_cases, int32_t D, int32_t H, const float* w1, const float* w2, const float* o, const uint32_t* words,
              const double* beta, float* logits, int32_t* action, int32_t* greedy) {
  for (int64_t c = 0; c < n_cases; ++c) {
    bsx_mlp_logits(w1 + c * BSX_MLP_W1(D, H), w2 + c * BSX_MLP_W2(H), o + c * D, D, H, logits + 3 * c);
    action[c] = bsx_gumbel_select(logits + 3 * c, beta[c], words[3 * c], words[3 * c + 1], words[3 * c + 2]);
    greedy[c] = bsx_mlp_select(w1 + c * BSX_MLP_W1(D, H), w2 + c * BSX_MLP_W2(H), o + c * D, D, H);
  }
}

/* the decision alone: logits [n, 3], words [n, 3], beta [n] -> z [n, 3], action [n] */
void shim_select(int64_t n_cases, const float* logits, const uint32_t* words, const double* beta, double* z, int32_t* action) {
  for (int64_t c = 0; c < n_cases; ++c) {
    for (int a = 0; a < 3; ++a) z[3 * c + a] = bsx_gumbel_score(logits[3 * c + a], beta[c], words[3 * c + a]);
    action[c] = bsx_gumbel_select(logits + 3 * c, beta[c], words[3 * c], words[3 * c + 1], words[3 * c + 2]);
  }
}

void shim_noise(int64_t n, const uint32_t* words, double* g) {
  for (int64_t k = 0; k < n; ++k) g[k] = bsx_gumbel_noise(words[k]);
}

void shim_log(int64_t n, const double* x, double* y) {
  for (int64_t k = 0; k < n; ++k) y[k] = bsx_log(x[k]);
}

/* words 0..3 of block 0 of the sample stream of lanes lane0 .. lane0 + n - 1 */
void shim_draws(uint64_t seed, uint64_t lane0, int64_t n, uint64_t step, uint32_t* words) {
  for (int64_t k = 0; k < n; ++k) {
    const bsx_u32x4 u = bsx_gumbel_draws(seed, lane0 + (uint64_t)k, step);
    for (int a = 0; a < 4; ++a) words[4 * k + a] = u.v[a];
  }
}

uint32_t shim_stream_sample(void) { return BSX_STREAM_SAMPLE; }

#ifdef GUMBEL_SHIM_MAIN
/* Stand-alone run for the sanitizers (gcc -fsanitize=address,undefined -DGUMBEL_SHIM_MAIN): the largest pair and the widest
 * linear matrix on a fixed row, the extreme words, and a short run of the draw stream. */
#include <stdio.h>
int main(void) {
  enum { D = 8, H = BSX_MLP_MAX_HIDDEN, N = 64 };
  static float w1[H * (D + 1)], w2[3 * (H + 1)], w[3 * (D + 1)], o[D];
  for (int k = 0; k < H * (D + 1); ++k) w1[k] = (float)((k * 37) % 19 - 9) * 0.125f;
  for (int k = 0; k < 3 * (H + 1); ++k) w2[k] = (float)((k * 53) % 23 - 11) * 0.0625f;
  for (int k = 0; k < 3 * (D + 1); ++k) w[k] = (float)((k * 29) % 17 - 8) * 0.25f;
  for (int d = 0; d < D; ++d) o[d] = (float)(d - 3) * 0.5f;
  static uint32_t words[4 * N];
  shim_draws(0x8000000000000005ull, 0xFFFFFFEFull, N, ((uint64_t)1 << 34) + 3, words);
  words[0] = 0u; words[1] = 0xFFFFFFFFu;
  int bad = 0, seen[3] = {0, 0, 0};
  for (int k = 0; k < N; ++k) {
    const double beta = k % 3 == 0 ? 0.25 : k % 3 == 1 ? 1.0 : 4.0;
    float l[3];
    int32_t a, g;
    shim_linear(1, D, w, o, words + 4 * k, &beta, l, &a, &g);
    bad |= a < 0 || a > 2 || g < 0 || g > 2;
    shim_mlp(1, D, H, w1, w2, o, words + 4 * k, &beta, l, &a, &g);
    bad |= a < 0 || a > 2 || g < 0 || g > 2;
    seen[a] += 1;
  }
  printf("%d %d %d\n", seen[0], seen[1], seen[2]);
  return bad;
}
#endif
