// embed.hip — rollout_embedding / evaluate_embedding (bsx_<family>_embedding_rollout, bsx_<family>_embedding_evaluate) and
// sample_embedding / evaluate_sampled_embedding (bsx_<family>_embedding_sample, bsx_<family>_embedding_sample_evaluate): ONE
// kernel for deep_sea and catch, recording or returns only, greedy or drawn.  The family, the kind of call and the action
// source are uniform switches, taken once per launch; each of the eight branches is a body of bsx_embed_device.h instantiated
// for its family and its source.  The LDS holds the staged copy of a shared pair of matrices and both families' own staging
// (deep_sea's action mapping; catch has none).  The entry points are in deep_sea.hip and catch.hip;
// their bodies are the four bsx_embed_entry (bsx_embed_device.h).
#include "bsx_embed_device.h"

// Six waves per SIMD (80 vector registers) is the occupancy every branch has on its own (the largest, catch returns only,
// needs 78).  With eight branches in one function the scheduler, left to itself, relaxes to five waves (84 registers) in the
// unrolled global look-up of one drawn branch; told the target it allocates 78 with no spill and no scratch.
__attribute__((amdgpu_waves_per_eu(6)))
__global__ void __launch_bounds__(BSX_BLOCK) bsx_embed_kernel(const bsx_embed_args a) {
  __shared__ deep_sea_fam::shared s_deep_sea;
  __shared__ catch_fam::shared s_catch;
  __shared__ unsigned int s_cnt[2];
  __shared__ __attribute__((aligned(16))) float s_net[BSX_EMBED_LDS_BYTES / 4];
  const bsx_embed_kernarg ka = (bsx_embed_kernarg)__builtin_amdgcn_kernarg_segment_ptr();   // = &a, in constant memory
  if (a.drawn == 0) {
    if (a.family == BSX_FAM_DEEP_SEA) {
      if (a.record) bsx_embed_record_body<bsx_embed_deep_sea>(ka, s_deep_sea, s_cnt, s_net);
      else bsx_embed_returns_body<bsx_embed_deep_sea>(ka, s_deep_sea, s_cnt, s_net);
    } else {
      if (a.record) bsx_embed_record_body<bsx_embed_catch>(ka, s_catch, s_cnt, s_net);
      else bsx_embed_returns_body<bsx_embed_catch>(ka, s_catch, s_cnt, s_net);
    }
  } else if (a.family == BSX_FAM_DEEP_SEA) {
    if (a.record) bsx_embed_record_body<bsx_embed_drawn<bsx_embed_deep_sea>>(ka, s_deep_sea, s_cnt, s_net);
    else bsx_embed_returns_body<bsx_embed_drawn<bsx_embed_deep_sea>>(ka, s_deep_sea, s_cnt, s_net);
  } else {
    if (a.record) bsx_embed_record_body<bsx_embed_drawn<bsx_embed_catch>>(ka, s_catch, s_cnt, s_net);
    else bsx_embed_returns_body<bsx_embed_drawn<bsx_embed_catch>>(ka, s_catch, s_cnt, s_net);
  }
}

int bsx_launch_embed(const bsx_embed_args& a, hipStream_t st) {
  const int64_t n_lanes = a.family == BSX_FAM_DEEP_SEA ? a.fam.deep_sea.ctl.n_lanes : a.fam.catch_.ctl.n_lanes;
  bsx_embed_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), 0, st>>>(a);
  return bsx_launch_status();
}
