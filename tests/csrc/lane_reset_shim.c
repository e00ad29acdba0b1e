/* Test shim: the per-word arithmetic of a per-lane reset mark, bsuite_amd/csrc/bsx_lane_reset.h (the header
 * bsx_lane_reset_kernel compiles), evaluated on the host by gcc. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_lane_reset.h"

int32_t shim_reset_bit(int32_t family) { return bsx_lane_reset_bit(family); }

int shim_folds(int32_t family, int32_t variant, int32_t folded) { return bsx_lane_reset_folds(family, variant, folded); }

int32_t shim_reset_word(int32_t word, int32_t family, int32_t variant, int32_t folded, double* info_delta) {
  return bsx_lane_reset_word(word, family, variant, folded, info_delta);
}

/* What the kernel does to its columns, lane by lane: masked lanes only, a lane whose word does not change is not written. */
void shim_mark(int32_t family, int32_t variant, int64_t n, const uint8_t* mask, int32_t* state, double* info, int32_t folded,
               int32_t* written) {
  for (int64_t i = 0; i < n; ++i) {
    written[i] = 0;
    if (mask[i] == 0) continue;
    double delta;
    const int32_t nst = bsx_lane_reset_word(state[i], family, variant, folded, &delta);
    if (nst == state[i]) continue;
    state[i] = nst;
    written[i] = 1;
    if (delta != 0.0) info[i] += delta;
  }
}
