// tab_sample.hip — sample_policy / evaluate_sampled_policy (bsx_<family>_policy_sample, bsx_<family>_policy_sample_evaluate):
// ONE kernel for deep_sea and catch, recording or returns only.  The family and the kind of call are uniform switches, taken
// once per launch; each of the four branches is a body of bsx_tab_sample_device.h instantiated for its family.  The LDS holds
// the shared table of logits and both families' own staging (deep_sea's action mapping; catch has none).  The entry points
// are in deep_sea.hip and catch.hip; their bodies are the two bsx_tab_softmax_entry (bsx_tab_sample_device.h).
#include "bsx_tab_sample_device.h"

__global__ void __launch_bounds__(BSX_BLOCK) bsx_tab_softmax_kernel(const bsx_tab_softmax_args a) {
  __shared__ deep_sea_fam::shared s_deep_sea;
  __shared__ catch_fam::shared s_catch;
  __shared__ unsigned int s_cnt[2];
  __shared__ float s_tab[BSX_TAB_SAMPLE_LDS_BYTES / 4];
  const bsx_tab_softmax_kernarg ka = (bsx_tab_softmax_kernarg)__builtin_amdgcn_kernarg_segment_ptr();   // = &a, in constant memory
  if (a.family == BSX_FAM_DEEP_SEA) {
    if (a.record) bsx_tab_softmax_record_body<bsx_tab_softmax_deep_sea>(ka, s_deep_sea, s_cnt, s_tab);
    else bsx_tab_softmax_returns_body<bsx_tab_softmax_deep_sea>(ka, s_deep_sea, s_cnt, s_tab);
  } else {
    if (a.record) bsx_tab_softmax_record_body<bsx_tab_softmax_catch>(ka, s_catch, s_cnt, s_tab);
    else bsx_tab_softmax_returns_body<bsx_tab_softmax_catch>(ka, s_catch, s_cnt, s_tab);
  }
}

int bsx_launch_tab_softmax(const bsx_tab_softmax_args& a, hipStream_t st) {
  const int64_t n_lanes = a.family == BSX_FAM_DEEP_SEA ? a.fam.deep_sea.ctl.n_lanes : a.fam.catch_.ctl.n_lanes;
  bsx_tab_softmax_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), 0, st>>>(a);
  return bsx_launch_status();
}
