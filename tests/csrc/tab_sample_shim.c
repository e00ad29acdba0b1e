/* Test shim: the softmax decision of a fused sampled rollout from a table of logits (bsx_gumbel_select_n,
 * bsuite_amd/csrc/bsx_tab_sample.h — the header the HIP kernel compiles — over bsx_gumbel.h's score and draws and
 * bsx_policy.h's keys), evaluated on the host by gcc with -ffp-contract=off.  Case c has its own logits l[c] = [n], words
 * w[c] = [n] and inverse temperature beta[c]. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_tab_sample.h"

/* logits [cases, n], words [cases, n], beta [cases] -> z [cases, n], action [cases] */
void shim_select_n(int64_t n_cases, int32_t n, const float* logits, const uint32_t* words, const double* beta, double* z,
                   int32_t* action) {
  for (int64_t c = 0; c < n_cases; ++c) {
    for (int a = 0; a < n; ++a) z[n * c + a] = bsx_gumbel_score(logits[n * c + a], beta[c], words[n * c + a]);
    action[c] = bsx_gumbel_select_n(logits + n * c, n, beta[c], words + n * c);
  }
}

/* the three-action rule of the physics families on the same inputs: logits [cases, 3], words [cases, 3] */
void shim_select_3(int64_t n_cases, const float* logits, const uint32_t* words, const double* beta, int32_t* action) {
  for (int64_t c = 0; c < n_cases; ++c)
    action[c] = bsx_gumbel_select(logits + 3 * c, beta[c], words[3 * c], words[3 * c + 1], words[3 * c + 2]);
}

/* a whole lane-step of the kernel's action source: key -> clamp -> the row's logits -> the draws -> the rule.
 * table [n_states, n]; keys [cases] (any int32: clamped); lanes lane0 + c */
void shim_table_actions(int64_t n_cases, int32_t n, int32_t n_states, const float* table, const int32_t* keys, uint64_t seed,
                        uint64_t lane0, uint64_t step, double beta, int32_t* action) {
  for (int64_t c = 0; c < n_cases; ++c) {
    const int32_t key = bsx_policy_clamp(keys[c], n_states);
    const bsx_u32x4 u = bsx_gumbel_draws(seed, lane0 + (uint64_t)c, step);
    action[c] = bsx_gumbel_select_n(table + (int64_t)key * n, n, beta, u.v);
  }
}

int32_t shim_lds_bytes(void) { return BSX_TAB_SAMPLE_LDS_BYTES; }
uint32_t shim_stream_sample(void) { return BSX_STREAM_SAMPLE; }

#ifdef TAB_SAMPLE_SHIM_MAIN
/* Stand-alone run for the sanitizers (gcc -fsanitize=address,undefined -DTAB_SAMPLE_SHIM_MAIN): both widths on tables whose
 * last row ends the allocation, keys outside the table, the extreme words, infinities and NaNs. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
int main(void) {
  enum { S = 37, N = 64 };
  int bad = 0, seen[3] = {0, 0, 0};
  for (int n = 2; n <= 3; ++n) {
    float* table = (float*)malloc(sizeof(float) * S * n);           /* heap: a read past a row's end is an error */
    int32_t keys[N], action[N];
    for (int k = 0; k < S * n; ++k) table[k] = (float)((k * 37) % 19 - 9) * 0.25f;
    table[0] = -INFINITY; table[n] = NAN; table[2 * n + 1] = INFINITY;
    for (int k = 0; k < N; ++k) keys[k] = k == 0 ? -5 : k == 1 ? 1 << 30 : (k * 7) % S;
    for (int b = 0; b < 3; ++b) {
      shim_table_actions(N, n, S, table, keys, 0x8000000000000005ull, 0xFFFFFFEFull, ((uint64_t)1 << 34) + 3,
                         b == 0 ? 0.25 : b == 1 ? 1.0 : 4.0, action);
      for (int k = 0; k < N; ++k) { bad |= action[k] < 0 || action[k] >= n; if (!bad) seen[action[k]] += 1; }
    }
    const uint32_t ends[6] = {0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu};
    const double beta = 1.0;
    double z[3];
    int32_t a;
    shim_select_n(1, n, table + (S - 1) * n, ends, &beta, z, &a);   /* the table's last row */
    bad |= a < 0 || a >= n;
    free(table);
  }
  printf("%d %d %d\n", seen[0], seen[1], seen[2]);
  return bad;
}
#endif
