// linear.hip — evaluate_linear (bsx_cartpole_linear_evaluate, bsx_mountain_car_linear_evaluate): ONE kernel for cartpole,
// swing-up and mountain_car.  The family, its variant and whether the weight matrix is shared are uniform switches, taken
// once per launch; each branch is bsx_linear_score_body (bsx_linear_score.h) instantiated for its case.  The entry points
// are in cartpole.hip and mountain_car.hip; their one body is bsx_linear_score_entry (bsx_linear_score.h).
#include "bsx_linear_score.h"

__global__ void __launch_bounds__(BSX_BLOCK) bsx_linear_score_kernel(const bsx_linear_score_args a) {
  __shared__ float s_w[BSX_LINEAR_LDS_FLOATS];
  __shared__ unsigned int s_cnt[2];
  const bsx_linear_kernarg ka = (bsx_linear_kernarg)__builtin_amdgcn_kernarg_segment_ptr();     // = &a, in constant memory
  const bool shared = a.p.n_policies == 1;                                // uniform
  if (a.family == BSX_FAM_MOUNTAIN_CAR) {
    if (shared) bsx_linear_score_body<bsx_linear_mountain_car, 0, true>(ka, s_w, s_cnt);
    else bsx_linear_score_body<bsx_linear_mountain_car, 0, false>(ka, s_w, s_cnt);
  } else if (a.fam.cartpole.cfg.swingup) {
    if (shared) bsx_linear_score_body<bsx_linear_cartpole, 1, true>(ka, s_w, s_cnt);
    else bsx_linear_score_body<bsx_linear_cartpole, 1, false>(ka, s_w, s_cnt);
  } else {
    if (shared) bsx_linear_score_body<bsx_linear_cartpole, 0, true>(ka, s_w, s_cnt);
    else bsx_linear_score_body<bsx_linear_cartpole, 0, false>(ka, s_w, s_cnt);
  }
}

int bsx_launch_linear_score(const bsx_linear_score_args& a, hipStream_t st) {
  const int64_t n_lanes = a.family == BSX_FAM_MOUNTAIN_CAR ? a.fam.mountain_car.ctl.n_lanes : a.fam.cartpole.ctl.n_lanes;
  bsx_linear_score_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), 0, st>>>(a);
  return bsx_launch_status();
}
