/* Test shim: the selection rule of a fused linear evaluation (bsx_linear_select, bsuite_amd/csrc/bsx_linear.h — the header
 * the HIP kernel compiles), evaluated on the host by gcc: case c has its own matrix w[c] = [3, D + 1] and row o[c] = [D]. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_linear.h"

void shim_linear_select(int64_t n_cases, int32_t D, const float* w, const float* o, int32_t* best) {
  for (int64_t c = 0; c < n_cases; ++c) best[c] = bsx_linear_select(w + c * BSX_LINEAR_ROW(D), o + c * D, D);
}

int32_t shim_linear_actions(void) { return BSX_LINEAR_ACTIONS; }
int32_t shim_linear_max_obs(void) { return BSX_LINEAR_MAX_OBS; }
