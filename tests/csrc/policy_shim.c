/* Test shim: the key arithmetic and the selection rule of a fused policy rollout (bsuite_amd/csrc/bsx_policy.h, the header
 * the HIP kernels compile), evaluated on the host by gcc. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_policy.h"

int32_t shim_key_deep_sea(int32_t cell) { return bsx_policy_key_deep_sea(cell); }
int32_t shim_key_catch(int32_t ball, int32_t paddle, int32_t rows, int32_t columns) {
  return bsx_policy_key_catch(ball, paddle, rows, columns);
}
int32_t shim_states_deep_sea(int32_t size) { return bsx_policy_states_deep_sea(size); }
int32_t shim_states_catch(int32_t rows, int32_t columns) { return bsx_policy_states_catch(rows, columns); }
int32_t shim_clamp(int32_t v, int32_t n) { return bsx_policy_clamp(v, n); }
int32_t shim_lds_bytes(void) { return BSX_POLICY_LDS_BYTES; }
uint32_t shim_stream_id(void) { return BSX_STREAM_POLICY; }

void shim_draws(uint64_t explore_seed, uint64_t lane, uint64_t step, uint32_t* out4) {
  const bsx_u32x4 w = bsx_policy_draws(explore_seed, lane, step);
  for (int k = 0; k < 4; ++k) out4[k] = w.v[k];
}

int32_t shim_select(uint32_t table_byte, int32_t resets, double epsilon, uint32_t w0, uint32_t w1, uint32_t w2,
                    uint32_t num_actions) {
  return bsx_policy_select(table_byte, resets, epsilon, w0, w1, w2, num_actions);
}

/* One call of the rollout kernel's action source for n lanes, in the kernel's own order: the key of the index row the lane
 * is about to leave (K = 1 deep_sea, K = 2 catch), clamped; the lane's table; the draws of (explore_seed, lane, step); the
 * selection.  keys_out holds the UNCLAMPED key. */
void shim_actions(int32_t K, int32_t rows, int32_t columns, int64_t n, const int32_t* index_rows, const uint8_t* resets,
                  const uint8_t* table, int32_t n_states, int32_t n_policies, const int32_t* policy_index, double epsilon,
                  uint64_t explore_seed, const uint64_t* lanes, uint64_t step, uint32_t num_actions, int32_t* keys_out,
                  int32_t* actions_out) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t key = K == 1 ? bsx_policy_key_deep_sea(index_rows[i])
                               : bsx_policy_key_catch(index_rows[2 * i], index_rows[2 * i + 1], rows, columns);
    keys_out[i] = key;
    const uint8_t* tab = table + (int64_t)(policy_index ? bsx_policy_clamp(policy_index[i], n_policies) : 0) * n_states;
    const uint32_t entry = tab[bsx_policy_clamp(key, n_states)];
    uint32_t w0 = 0, w1 = 0, w2 = 0;
    if (epsilon > 0.0) {
      const bsx_u32x4 w = bsx_policy_draws(explore_seed, lanes[i], step);
      w0 = w.v[0]; w1 = w.v[1]; w2 = w.v[2];
    }
    actions_out[i] = bsx_policy_select(entry, resets[i], epsilon, w0, w1, w2, num_actions);
  }
}
