/* Test shim: the accumulation rule of a fused policy evaluation (bsx_eval_accumulate, bsuite_amd/csrc/bsx_policy.h — the
 * header the HIP kernel compiles), evaluated on the host by gcc over [T, B] step types and f64 rewards. */
#include <stdint.h>
#include "../../bsuite_amd/csrc/bsx_policy.h"

void shim_evaluate(int64_t n_steps, int64_t n_lanes, const int8_t* step_type, const double* reward, int32_t* episodes,
                   double* return_sum, double* episode_return_sum) {
  for (int64_t i = 0; i < n_lanes; ++i) {
    bsx_eval_acc e = {0.0, 0.0, 0.0, 0};
    for (int64_t t = 0; t < n_steps; ++t) bsx_eval_accumulate(&e, step_type[t * n_lanes + i], reward[t * n_lanes + i]);
    episodes[i] = e.n;
    return_sum[i] = e.total;
    episode_return_sum[i] = e.done;
  }
}
