// drawn_returns.hip — evaluate_sampled_linear / evaluate_sampled_mlp (bsx_<family>_linear_sample_evaluate,
// bsx_<family>_mlp_sample_evaluate): ONE kernel for cartpole, swing-up and mountain_car under a linear or a hidden-layer
// softmax policy.  The family, its variant, whether the policy is shared and its kind are uniform switches, taken once per
// launch; each of the twelve branches is bsx_drawn_returns_body (bsx_drawn_returns.h) instantiated for its case.  The entry
// points are in cartpole.hip and mountain_car.hip; their one body is bsx_drawn_returns_entry (bsx_drawn_returns.h).
#include "bsx_drawn_returns.h"

template <class Fam, int V>
__device__ __forceinline__ void bsx_drawn_returns_switch(bsx_drawn_returns_kernarg ka, bool shared, bool hidden, float* s_w,
                                                         unsigned int* s_cnt) {
  if (hidden) {
    if (shared) bsx_drawn_returns_body<Fam, V, true, true>(ka, s_w, s_cnt);
    else bsx_drawn_returns_body<Fam, V, false, true>(ka, s_w, s_cnt);
  } else {
    if (shared) bsx_drawn_returns_body<Fam, V, true, false>(ka, s_w, s_cnt);
    else bsx_drawn_returns_body<Fam, V, false, false>(ka, s_w, s_cnt);
  }
}

__global__ void __launch_bounds__(BSX_BLOCK) bsx_drawn_returns_kernel(const bsx_drawn_returns_args a) {
  __shared__ float s_w[BSX_MLP_LDS_FLOATS];
  __shared__ unsigned int s_cnt[2];
  const bsx_drawn_returns_kernarg ka = (bsx_drawn_returns_kernarg)__builtin_amdgcn_kernarg_segment_ptr();   // = &a, in constant memory
  const bool shared = a.p.n_policies == 1, hidden = a.p.hidden != 0;     // uniform
  if (a.family == BSX_FAM_MOUNTAIN_CAR) bsx_drawn_returns_switch<bsx_drawn_returns_mountain_car, 0>(ka, shared, hidden, s_w, s_cnt);
  else if (a.fam.cartpole.cfg.swingup) bsx_drawn_returns_switch<bsx_drawn_returns_cartpole, 1>(ka, shared, hidden, s_w, s_cnt);
  else bsx_drawn_returns_switch<bsx_drawn_returns_cartpole, 0>(ka, shared, hidden, s_w, s_cnt);
}

int bsx_launch_drawn_returns(const bsx_drawn_returns_args& a, hipStream_t st) {
  const int64_t n_lanes = a.family == BSX_FAM_MOUNTAIN_CAR ? a.fam.mountain_car.ctl.n_lanes : a.fam.cartpole.ctl.n_lanes;
  bsx_drawn_returns_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), 0, st>>>(a);
  return bsx_launch_status();
}
