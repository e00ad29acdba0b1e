/* Test shim: the softmax policy of a fused sampled closed loop from a hidden-layer network on the index row
 * (bsuite_amd/csrc/bsx_embed_sample.h — the header the HIP kernel compiles), evaluated on the host by gcc with
 * -ffp-contract=off.  One pair w1 [C + 2, H], w2 [A, H + 1] for all cases; case c has its own index row cells[c] = [K], its
 * own words[c] = [A] and its own beta[c]. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_embed_sample.h"

/* cells [cases, K] (any int32: clamped), words [cases, A], beta [cases] -> action [cases] */
void shim_embed_sample(int64_t n_cases, int32_t K, int32_t C, int32_t H, int32_t A, const float* w1, const float* w2,
                       const int32_t* cells, const uint32_t* words, const double* beta, int32_t* action) {
  for (int64_t c = 0; c < n_cases; ++c)
    action[c] = bsx_embed_sample_select(w1, w2, cells + K * c, K, C, H, A, beta[c], words + A * c);
}

/* ... with the words drawn here: block 0 of stream BSX_STREAM_SAMPLE of (sample_seed, lane[c], step) */
void shim_embed_sample_action(int64_t n_cases, int32_t K, int32_t C, int32_t H, int32_t A, const float* w1, const float* w2,
                              const int32_t* cells, double beta, uint64_t sample_seed, const uint64_t* lane, uint64_t step,
                              int32_t* action) {
  for (int64_t c = 0; c < n_cases; ++c)
    action[c] = bsx_embed_sample_action(w1, w2, cells + K * c, K, C, H, A, beta, sample_seed, lane[c], step);
}

int32_t shim_embed_sample_stream(void) { return BSX_STREAM_SAMPLE; }

#ifdef EMBED_SAMPLE_SHIM_MAIN
/* Stand-alone run for the sanitizers (gcc -fsanitize=address,undefined -DEMBED_SAMPLE_SHIM_MAIN): both families' widths on
 * heap matrices and heap words whose last element ends the allocation, cells outside the board, infinities and NaNs, a hot
 * and a cold temperature. */
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
      uint32_t* words = (uint32_t*)malloc(sizeof(uint32_t) * A * N);
      double* beta = (double*)malloc(sizeof(double) * N);
      uint64_t* lane = (uint64_t*)malloc(sizeof(uint64_t) * N);
      int32_t cells[2 * N], action[N];
      for (int k = 0; k < BSX_EMBED_W1(C, H); ++k) w1[k] = (float)((k * 37) % 19 - 9) * 0.25f;
      for (int k = 0; k < BSX_EMBED_W2(A, H); ++k) w2[k] = (float)((k * 29) % 17 - 8) * 0.5f;
      if (H > 1) { w1[3] = NAN; w2[1] = INFINITY; }
      if (H == 5) w2[A * (H + 1) - 1] = -INFINITY;                       /* the last action masked */
      for (int k = 0; k < K * N; ++k) cells[k] = k == 0 ? -5 : k == 1 ? 1 << 30 : k == 2 ? -1 : (k * 7) % C;
      for (int k = 0; k < A * N; ++k) words[k] = k == 0 ? 0u : k == 1 ? 0xFFFFFFFFu : (uint32_t)k * 2654435761u;
      for (int k = 0; k < N; ++k) { beta[k] = (k & 1) ? 4.0 : 0.25; lane[k] = 0xFFFFFFF0ull + (uint64_t)k; }
      shim_embed_sample(N, K, C, H, A, w1, w2, cells, words, beta, action);
      for (int k = 0; k < N; ++k) { bad |= action[k] < 0 || action[k] >= A; if (!bad) seen[action[k]] += 1; }
      shim_embed_sample_action(N, K, C, H, A, w1, w2, cells, 1.0, 0xFFFFFFFFFFFFFFFFull, lane, 1ull << 40, action);
      for (int k = 0; k < N; ++k) { bad |= action[k] < 0 || action[k] >= A; if (!bad) seen[action[k]] += 1; }
      free(w1); free(w2); free(words); free(beta); free(lane);
    }
  }
  printf("%d %d %d\n", seen[0], seen[1], seen[2]);
  return bad;
}
#endif
