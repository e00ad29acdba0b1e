// torso.hip — evaluate_mlp2 / rollout_mlp2 (bsx_<family>_mlp2_evaluate, bsx_<family>_mlp2_rollout) and evaluate_sampled_mlp2 /
// sample_mlp2 (bsx_<family>_mlp2_sample_evaluate, bsx_<family>_mlp2_sample): ONE kernel for cartpole, swing-up and
// mountain_car under a policy with two ReLU hidden layers.  The family, its variant, whether the triple of matrices is
// shared, whether the call records its trajectory and whether its actions are greedy or drawn (a.mode) are uniform switches,
// taken once per launch; each of the twenty-four branches is bsx_torso_body (bsx_torso.h) instantiated for its case — the
// twelve greedy ones with the mode's defaulted parameter left out, instruction for instruction what they were before the
// drawn mode joined (the drawn bodies come first: with that order no greedy call measured slower).  A shared
// triple is staged in dynamic LDS before the switch (its size depends on the call: the launch sizes the segment).  The
// entry points are in cartpole.hip and mountain_car.hip; their one body is bsx_torso_entry (bsx_torso.h).
#include "bsx_torso.h"

template <class Fam, int V>
__device__ __forceinline__ void bsx_torso_switch(bsx_torso_kernarg ka, bool shared, bool record, bool drawn, float* s_w,
                                                 unsigned int* s_cnt) {
  if (drawn) {
    if (record) {
      if (shared) bsx_torso_body<Fam, V, true, true, true>(ka, s_w, s_cnt);
      else bsx_torso_body<Fam, V, false, true, true>(ka, s_w, s_cnt);
    } else {
      if (shared) bsx_torso_body<Fam, V, true, false, true>(ka, s_w, s_cnt);
      else bsx_torso_body<Fam, V, false, false, true>(ka, s_w, s_cnt);
    }
  } else if (record) {
    if (shared) bsx_torso_body<Fam, V, true, true>(ka, s_w, s_cnt);
    else bsx_torso_body<Fam, V, false, true>(ka, s_w, s_cnt);
  } else {
    if (shared) bsx_torso_body<Fam, V, true, false>(ka, s_w, s_cnt);
    else bsx_torso_body<Fam, V, false, false>(ka, s_w, s_cnt);
  }
}

__global__ void __launch_bounds__(BSX_BLOCK) bsx_torso_kernel(const bsx_torso_args a) {
  extern __shared__ __attribute__((aligned(16))) float s_w[];             // a shared triple: bsx_torso_lds's layout
  __shared__ unsigned int s_cnt[2];
  const bsx_torso_kernarg ka = (bsx_torso_kernarg)__builtin_amdgcn_kernarg_segment_ptr();           // = &a, in constant memory
  const bool shared = a.p.n_policies == 1, record = a.record != 0;        // uniform
  const bool drawn = a.mode == BSX_TORSO_DRAWN;
  const bool car = a.family == BSX_FAM_MOUNTAIN_CAR, swingup = !car && a.fam.cartpole.cfg.swingup;
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  if (shared) bsx_torso_stage(bsx_torso_view(ka), car ? mountain_car_env::numel_of(0) : cartpole_env::numel_of(swingup ? 1 : 0), s_w);
  __syncthreads();
  if (car) bsx_torso_switch<bsx_torso_mountain_car, 0>(ka, shared, record, drawn, s_w, s_cnt);
  else if (swingup) bsx_torso_switch<bsx_torso_cartpole, 1>(ka, shared, record, drawn, s_w, s_cnt);
  else bsx_torso_switch<bsx_torso_cartpole, 0>(ka, shared, record, drawn, s_w, s_cnt);
}

int bsx_launch_torso(const bsx_torso_args& a, hipStream_t st) {
  const bool car = a.family == BSX_FAM_MOUNTAIN_CAR;
  const int64_t n_lanes = car ? a.fam.mountain_car.ctl.n_lanes : a.fam.cartpole.ctl.n_lanes;
  const int D = car ? mountain_car_env::numel_of(0) : cartpole_env::numel_of(a.fam.cartpole.cfg.swingup ? 1 : 0);
  const size_t lds = a.p.n_policies == 1 ? sizeof(float) * (size_t)BSX_TORSO_LDS_FLOATS(D, a.p.hidden1, a.p.hidden2, a.p.width) : 0;
  bsx_torso_kernel<<<dim3((unsigned)bsx_blocks_of(n_lanes)), dim3(BSX_BLOCK), lds, st>>>(a);
  return bsx_launch_status();
}
