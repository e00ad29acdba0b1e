/* Test shim: the selection rule of a fused two-hidden-layer call (bsx_mlp2_select and its pieces, bsuite_amd/csrc/bsx_mlp2.h —
 * the header the HIP kernel compiles), evaluated on the host by gcc: case c has its own triple w1[c] = [H1, D + 1],
 * w2[c] = [H2, H1 + 1], w3[c] = [3, H2 + 1] and row o[c] = [D]. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_mlp2.h"

/* best = [n_cases], logits = [n_cases, 3], s2 = [n_cases, H2] (layer 2's pre-activations) */
void shim_mlp2(int64_t n_cases, int32_t D, int32_t H1, int32_t H2, const float* w1, const float* w2, const float* w3, const float* o,
               int32_t* best, float* logits, float* s2) {
  for (int64_t c = 0; c < n_cases; ++c) {
    const float* a1 = w1 + c * BSX_MLP2_W1(D, H1);
    const float* a2 = w2 + c * BSX_MLP2_W2(H1, H2);
    const float* a3 = w3 + c * BSX_MLP2_W3(H2);
    best[c] = bsx_mlp2_select(a1, a2, a3, o + c * D, D, H1, H2);
    bsx_mlp2_logits(a1, a2, a3, o + c * D, D, H1, H2, logits + c * BSX_LINEAR_ACTIONS);
    bsx_mlp2_preactivations(a1, a2, o + c * D, D, H1, H2, s2 + c * H2);
  }
}

int32_t shim_mlp2_triple_floats(int32_t D, int32_t H1, int32_t H2) { return BSX_MLP2_W1(D, H1) + BSX_MLP2_W2(H1, H2) + BSX_MLP2_W3(H2); }

#ifdef MLP2_SHIM_MAIN
/* Stand-alone run for the sanitizers (gcc -fsanitize=address,undefined -DMLP2_SHIM_MAIN): the largest triple on a fixed row. */
#include <stdio.h>
int main(void) {
  enum { D = 8, H = BSX_MLP_MAX_HIDDEN };
  static float w1[H * (D + 1)], w2[H * (H + 1)], w3[3 * (H + 1)], o[D], l[3], s2[H];
  for (int k = 0; k < H * (D + 1); ++k) w1[k] = (float)((k * 37) % 19 - 9) * 0.125f;
  for (int k = 0; k < H * (H + 1); ++k) w2[k] = (float)((k * 41) % 17 - 8) * 0.03125f;
  for (int k = 0; k < 3 * (H + 1); ++k) w3[k] = (float)((k * 53) % 23 - 11) * 0.0625f;
  for (int d = 0; d < D; ++d) o[d] = (float)(d - 3) * 0.5f;
  int32_t best = -1;
  shim_mlp2(1, D, H, H, w1, w2, w3, o, &best, l, s2);
  printf("%d\n", (int)best);
  return best < 0 || best > 2;
}
#endif
