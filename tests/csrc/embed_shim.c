/* Test shim: the hidden-layer policy of a fused closed loop on the grid families (bsuite_amd/csrc/bsx_embed.h — the header the
 * HIP kernel compiles), evaluated on the host by gcc with -ffp-contract=off.  One pair w1 [C + 2, H], w2 [A, H + 1] for all
 * cases; case c has its own index row cells[c] = [K]. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_embed.h"

/* cells [cases, K] (any int32: clamped) -> logits [cases, A], action [cases] */
void shim_embed(int64_t n_cases, int32_t K, int32_t C, int32_t H, int32_t A, const float* w1, const float* w2, const int32_t* cells,
                float* logits, int32_t* action) {
  for (int64_t c = 0; c < n_cases; ++c) {
    bsx_embed_logits(w1, w2, cells + K * c, K, C, H, A, logits + A * c);
    action[c] = bsx_embed_select(w1, w2, cells + K * c, K, C, H, A);
  }
}

/* the pieces on their own */
int32_t shim_embed_row(int32_t cell, int32_t C) { return bsx_embed_row(cell, C); }
float shim_embed_preactivation(float bias, const float* e, int32_t K) { return bsx_embed_preactivation(bias, e, K); }
int32_t shim_embed_argmax(const float* l, int32_t A) { return bsx_embed_argmax(l, A); }

int32_t shim_embed_lds_bytes(void) { return BSX_EMBED_LDS_BYTES; }
int32_t shim_embed_stride(int32_t H) { return BSX_EMBED_STRIDE(H); }
int64_t shim_embed_staged_bytes(int32_t C, int32_t H) { return BSX_EMBED_STAGED_BYTES(C, H); }
int32_t shim_embed_max_hidden(void) { return BSX_MLP_MAX_HIDDEN; }

#ifdef EMBED_SHIM_MAIN
/* Stand-alone run for the sanitizers (gcc -fsanitize=address,undefined -DEMBED_SHIM_MAIN): both families' widths on heap
 * matrices whose last row ends the allocation, cells outside the board, infinities and NaNs. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
int main(void) {
  enum { C = 13, N = 64 };
  int bad = 0, seen[3] = {0, 0, 0};
  const int hs[3] = {1, 5, 64};
  for (int f = 0; f < 2; ++f) {
    const int K = f + 1, A = f + 2;
    for (int q = 0; q < 3; ++q) {
      const int H = hs[q];
      float* w1 = (float*)malloc(sizeof(float) * BSX_EMBED_W1(C, H));   /* heap: a read past the end is an error */
      float* w2 = (float*)malloc(sizeof(float) * BSX_EMBED_W2(A, H));
      int32_t cells[2 * N], action[N];
      float logits[3 * N];
      for (int k = 0; k < BSX_EMBED_W1(C, H); ++k) w1[k] = (float)((k * 37) % 19 - 9) * 0.25f;
      for (int k = 0; k < BSX_EMBED_W2(A, H); ++k) w2[k] = (float)((k * 29) % 17 - 8) * 0.5f;
      if (H > 1) { w1[3] = NAN; w2[1] = INFINITY; }
      for (int k = 0; k < K * N; ++k) cells[k] = k == 0 ? -5 : k == 1 ? 1 << 30 : k == 2 ? -1 : (k * 7) % C;
      shim_embed(N, K, C, H, A, w1, w2, cells, logits, action);
      for (int k = 0; k < N; ++k) { bad |= action[k] < 0 || action[k] >= A; if (!bad) seen[action[k]] += 1; }
      free(w1); free(w2);
    }
  }
  printf("%d %d %d\n", seen[0], seen[1], seen[2]);
  return bad;
}
#endif
