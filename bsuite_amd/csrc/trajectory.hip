// trajectory.hip — rollout_linear / rollout_mlp (bsx_<family>_linear_rollout, bsx_<family>_mlp_rollout): ONE kernel for
// cartpole, swing-up and mountain_car under a linear or a hidden-layer policy.  The family, its variant, whether the policy
// is shared and its kind are uniform switches, taken once per launch; each of the twelve branches is bsx_trajectory_body
// (bsx_trajectory.h) instantiated for its case.  The entry points are in cartpole.hip and mountain_car.hip;
// their one body is bsx_trajectory_entry (bsx_trajectory.h).
#include "bsx_trajectory.h"

template <class Fam, int V>
__device__ __forceinline__ void bsx_trajectory_switch(bsx_trajectory_kernarg ka, bool shared, bool hidden, float* s_w, unsigned int* s_cnt) {
  if (hidden) {
    if (shared) bsx_trajectory_body<Fam, V, true, true>(ka, s_w, s_cnt);
    else bsx_trajectory_body<Fam, V, false, true>(ka, s_w, s_cnt);
  } else {
    if (shared) bsx_trajectory_body<Fam, V, true, false>(ka, s_w, s_cnt);
    else bsx_trajectory_body<Fam, V, false, false>(ka, s_w, s_cnt);
  }
}

__global__ void __launch_bounds__(BSX_BLOCK) bsx_trajectory_kernel(const bsx_trajectory_args a) {
  __shared__ float s_w[BSX_MLP_LDS_FLOATS];
  __shared__ unsigned int s_cnt[2];
  const bsx_trajectory_kernarg ka = (bsx_trajectory_kernarg)__builtin_amdgcn_kernarg_segment_ptr();   // = &a, in constant memory
  const bool shared = a.p.n_policies == 1, hidden = a.p.hidden != 0;      // uniform
  if (a.family == BSX_FAM_MOUNTAIN_CAR) bsx_trajectory_switch<bsx_trajectory_mountain_car, 0>(ka, shared, hidden, s_w, s_cnt);
  else if (a.fam.cartpole.cfg.swingup) bsx_trajectory_switch<bsx_trajectory_cartpole, 1>(ka, shared, hidden, s_w, s_cnt);
  else bsx_trajectory_switch<bsx_trajectory_cartpole, 0>(ka, shared, hidden, s_w, s_cnt);
}

int bsx_launch_trajectory(const bsx_trajectory_args& a, hipStream_t st) {
  const int64_t n_lanes = a.family == BSX_FAM_MOUNTAIN_CAR ? a.fam.mountain_car.ctl.n_lanes : a.fam.cartpole.ctl.n_lanes;
  bsx_trajectory_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), 0, st>>>(a);
  return bsx_launch_status();
}
