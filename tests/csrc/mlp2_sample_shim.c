/* Test shim: the decision of a fused sampled two-hidden-layer call — bsx_gumbel_select over bsx_mlp2_logits
 * (bsuite_amd/csrc/bsx_mlp2.h and bsuite_amd/csrc/bsx_gumbel.h, the headers the HIP kernel compiles), evaluated on the host by
 * gcc: case c has its own triple w1[c] = [H1, D + 1], w2[c] = [H2, H1 + 1], w3[c] = [3, H2 + 1], row o[c] = [D], words[c] = [3]
 * and beta[c] = 1 / temperature. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_mlp2.h"
#include "../../bsuite_amd/csrc/bsx_gumbel.h"

/* action = [n_cases], logits = [n_cases, 3] */
void shim_mlp2_sample(int64_t n_cases, int32_t D, int32_t H1, int32_t H2, const float* w1, const float* w2, const float* w3,
                      const float* o, const uint32_t* words, const double* beta, int32_t* action, float* logits) {
  for (int64_t c = 0; c < n_cases; ++c) {
    float* l = logits + c * BSX_LINEAR_ACTIONS;
    const uint32_t* u = words + c * BSX_LINEAR_ACTIONS;
    bsx_mlp2_logits(w1 + c * BSX_MLP2_W1(D, H1), w2 + c * BSX_MLP2_W2(H1, H2), w3 + c * BSX_MLP2_W3(H2), o + c * D, D, H1, H2, l);
    action[c] = bsx_gumbel_select(l, beta[c], u[0], u[1], u[2]);
  }
}

uint32_t shim_stream_sample(void) { return BSX_STREAM_SAMPLE; }

#ifdef MLP2_SAMPLE_SHIM_MAIN
/* Stand-alone run for the sanitizers (gcc -fsanitize=address,undefined -DMLP2_SAMPLE_SHIM_MAIN): the largest triple on a fixed
 * row, at three temperatures with the draws of three (seed, lane, step). */
#include <stdio.h>
int main(void) {
  enum { D = 8, H = BSX_MLP_MAX_HIDDEN, N = 3 };
  static float w1[N][H * (D + 1)], w2[N][H * (H + 1)], w3[N][3 * (H + 1)], o[N][D], l[N][3];
  static uint32_t words[N][3];
  static const double beta[N] = {4.0, 1.0, 0.25};
  int32_t action[N] = {-1, -1, -1};
  for (int c = 0; c < N; ++c) {
    for (int k = 0; k < H * (D + 1); ++k) w1[c][k] = (float)((k * 37 + c) % 19 - 9) * 0.125f;
    for (int k = 0; k < H * (H + 1); ++k) w2[c][k] = (float)((k * 41 + c) % 17 - 8) * 0.03125f;
    for (int k = 0; k < 3 * (H + 1); ++k) w3[c][k] = (float)((k * 53 + c) % 23 - 11) * 0.0625f;
    for (int d = 0; d < D; ++d) o[c][d] = (float)(d - 3) * 0.5f;
    const bsx_u32x4 u = bsx_gumbel_draws(((uint64_t)1 << 63) + 5, ((uint64_t)1 << 32) - 1 + (uint64_t)c, (uint64_t)c);
    words[c][0] = u.v[0]; words[c][1] = u.v[1]; words[c][2] = u.v[2];
  }
  shim_mlp2_sample(N, D, H, H, &w1[0][0], &w2[0][0], &w3[0][0], &o[0][0], &words[0][0], beta, action, &l[0][0]);
  int bad = 0;
  for (int c = 0; c < N; ++c) {
    printf("%d\n", (int)action[c]);
    bad |= action[c] < 0 || action[c] > 2;
  }
  return bad;
}
#endif
