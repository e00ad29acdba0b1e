/* Test shim: the selection rule of a fused hidden-layer evaluation (bsx_mlp_select and its pieces, bsuite_amd/csrc/bsx_mlp.h —
 * the header the HIP kernel compiles), evaluated on the host by gcc: case c has its own pair w1[c] = [H, D + 1],
 * w2[c] = [3, H + 1] and row o[c] = [D]. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_mlp.h"

void shim_mlp_select(int64_t n_cases, int32_t D, int32_t H, const float* w1, const float* w2, const float* o, int32_t* best) {
  for (int64_t c = 0; c < n_cases; ++c)
    best[c] = bsx_mlp_select(w1 + c * BSX_MLP_W1(D, H), w2 + c * BSX_MLP_W2(H), o + c * D, D, H);
}

/* pre-activation and activation of every hidden unit: s, h = [n_cases, H] */
void shim_mlp_hidden(int64_t n_cases, int32_t D, int32_t H, const float* w1, const float* o, float* s, float* h) {
  for (int64_t c = 0; c < n_cases; ++c)
    for (int32_t j = 0; j < H; ++j) {
      const float* w1j = w1 + c * BSX_MLP_W1(D, H) + j * (D + 1);
      s[c * H + j] = bsx_mlp_preactivation(w1j, o + c * D, D);
      h[c * H + j] = bsx_mlp_hidden(w1j, o + c * D, D);
    }
}

void shim_mlp_relu(int64_t n, const float* s, float* h) {
  for (int64_t k = 0; k < n; ++k) h[k] = bsx_mlp_relu(s[k]);
}

int32_t shim_mlp_max_hidden(void) { return BSX_MLP_MAX_HIDDEN; }
int32_t shim_mlp_pair_floats(int32_t D, int32_t H) { return BSX_MLP_W1(D, H) + BSX_MLP_W2(H); }

#ifdef MLP_SHIM_MAIN
/* Stand-alone run for the sanitizers (gcc -fsanitize=address,undefined -DMLP_SHIM_MAIN): the largest pair on a fixed row. */
#include <stdio.h>
int main(void) {
  enum { D = 8, H = BSX_MLP_MAX_HIDDEN };
  static float w1[H * (D + 1)], w2[3 * (H + 1)], o[D];
  for (int k = 0; k < H * (D + 1); ++k) w1[k] = (float)((k * 37) % 19 - 9) * 0.125f;
  for (int k = 0; k < 3 * (H + 1); ++k) w2[k] = (float)((k * 53) % 23 - 11) * 0.0625f;
  for (int d = 0; d < D; ++d) o[d] = (float)(d - 3) * 0.5f;
  int32_t best = -1;
  shim_mlp_select(1, D, H, w1, w2, o, &best);
  printf("%d\n", (int)best);
  return best < 0 || best > 2;
}
#endif
