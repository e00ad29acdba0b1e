// gumbel.hip — sample_linear / sample_mlp (bsx_<family>_linear_sample, bsx_<family>_mlp_sample): ONE kernel for cartpole,
// swing-up and mountain_car under a linear or a hidden-layer softmax policy.  The family, its variant, whether the policy is
// shared and its kind are uniform switches, taken once per launch; each of the twelve branches is bsx_gumbel_body
// (bsx_gumbel_device.h) instantiated for its case.  The entry points are in cartpole.hip and mountain_car.hip;
// their one body is bsx_gumbel_entry (bsx_gumbel_device.h).
#include "bsx_gumbel_device.h"

template <class Fam, int V>
__device__ __forceinline__ void bsx_gumbel_switch(bsx_gumbel_kernarg ka, bool shared, bool hidden, float* s_w, unsigned int* s_cnt) {
  if (hidden) {
    if (shared) bsx_gumbel_body<Fam, V, true, true>(ka, s_w, s_cnt);
    else bsx_gumbel_body<Fam, V, false, true>(ka, s_w, s_cnt);
  } else {
    if (shared) bsx_gumbel_body<Fam, V, true, false>(ka, s_w, s_cnt);
    else bsx_gumbel_body<Fam, V, false, false>(ka, s_w, s_cnt);
  }
}

__global__ void __launch_bounds__(BSX_BLOCK) bsx_gumbel_kernel(const bsx_gumbel_args a) {
  __shared__ float s_w[BSX_MLP_LDS_FLOATS];
  __shared__ unsigned int s_cnt[2];
  const bsx_gumbel_kernarg ka = (bsx_gumbel_kernarg)__builtin_amdgcn_kernarg_segment_ptr();   // = &a, in constant memory
  const bool shared = a.t.p.n_policies == 1, hidden = a.t.p.hidden != 0;  // uniform
  if (a.t.family == BSX_FAM_MOUNTAIN_CAR) bsx_gumbel_switch<bsx_trajectory_mountain_car, 0>(ka, shared, hidden, s_w, s_cnt);
  else if (a.t.fam.cartpole.cfg.swingup) bsx_gumbel_switch<bsx_trajectory_cartpole, 1>(ka, shared, hidden, s_w, s_cnt);
  else bsx_gumbel_switch<bsx_trajectory_cartpole, 0>(ka, shared, hidden, s_w, s_cnt);
}

int bsx_launch_gumbel(const bsx_gumbel_args& a, hipStream_t st) {
  const int64_t n_lanes = a.t.family == BSX_FAM_MOUNTAIN_CAR ? a.t.fam.mountain_car.ctl.n_lanes : a.t.fam.cartpole.ctl.n_lanes;
  bsx_gumbel_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), 0, st>>>(a);
  return bsx_launch_status();
}
