/* Test shim: the hint word of the one-launch deep_sea step (bsuite_amd/csrc/deep_sea_hint.h, the header the HIP
 * kernel compiles), evaluated on the host by gcc. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/deep_sea_hint.h"

/* hot[i] = ds_hint_hot(ds_hint_pack(row[i], col[i], reset[i], N, mapping_bits), action[i]); hint[i] = the packed word */
void shim_hint_hot(int n, int N, const uint32_t* mapping_bits, const int32_t* row, const int32_t* col, const int32_t* reset,
                   const int32_t* action, uint32_t* hint, int32_t* hot) {
  for (int i = 0; i < n; ++i) {
    hint[i] = ds_hint_pack(row[i], col[i], reset[i], N, mapping_bits);
    hot[i] = ds_hint_hot(hint[i], action[i]);
  }
}

int shim_hint_field_bits(void) { return DS_HINT_FIELD_BITS; }
int shim_hint_l_shift(void) { return DS_HINT_L_SHIFT; }
int shim_hint_m_shift(void) { return DS_HINT_M_SHIFT; }
int shim_max_size(void) { return BSX_DEEP_SEA_MAX_SIZE; }
