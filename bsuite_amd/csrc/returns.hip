// returns.hip — lambda_returns / td_lambda (bsx_lambda_returns): the backward recursion over the time axis of a [T,B]
// trajectory, cut at episode ends, in ONE launch.  The definition (include/bsuite_amd.h has it with the reasons), per lane i,
// in float64, every multiply and add rounded on its own (-ffp-contract=off), one_minus = 1.0 - lambda computed on the host:
//   vals(t) = values ? (double)values[t][i] : +0.0
//   carry   = values ? (double)values[T][i] : (bootstrap ? (double)bootstrap[i] : +0.0)
//   for t = T-1 .. 0:
//     g = step_type && step_type[t][i] == BSX_FIRST
//           ? vals(t)
//           : (double)reward[t][i] + (gamma * (double)discount[t][i]) * (one_minus * vals(t+1) + lambda * carry)
//     carry = g;  returns[t][i] = (float)g;  td_errors[t][i] = (float)(g - vals(t))
// "Values absent" is that arithmetic with +0.0, additions included: skipping them would turn a -0.0 into +0.0 or back.
//
// One lane per thread: the recursion is serial in t, the addresses are not.  A wave reads one contiguous 256-byte range
// of each float row (64 bytes of the step types) and walks the rows from T-1 down.  The loads run BSX_RETURNS_AHEAD rows
// ahead of the dependent chain through a ring of registers (the loop is unrolled by the ring's length, so every slot is a
// fixed register): row t's arithmetic needs its own loads only, which were issued AHEAD rows earlier, so a turn of the ring
// has the loads of AHEAD rows in flight behind one latency (in the ISA: 25 / 33 loads in front of the first vmcnt wait;
// counted waits inside the loop without values, one full wait per turn with them).  Rows below 0 are clamped to row 0 for the loads (always inside the arrays) and skipped by the arithmetic,
// so every T — below the ring's length, not a multiple of it — takes the same loop.  No LDS, no atomics, no scratch.
// `values` present or absent is a template parameter (two kernels); step_type, bootstrap and the two outputs are
// launch-uniform run-time choices.
#include "bsx_host.h"

#define BSX_RETURNS_AHEAD 8
// cache policy: bit 0 = non-temporal input loads, bit 1 = non-temporal output stores.  Plain loads and non-temporal stores,
// 8 rows ahead: measured (profiles/returns/ab_returns.jsonl) against the other three policies and against rings
// of 4 and 16 rows — the tuning build compiles all of them and reads BSX_RETURNS_POLICY / BSX_RETURNS_AHEAD.
#define BSX_RETURNS_POLICY 2

struct bsx_returns_args {
  const float* reward;
  const float* discount;
  const int8_t* step_type;
  const float* values;
  const float* bootstrap;
  float* returns;
  float* td_errors;
  double gamma, lambda, one_minus;
  int64_t n_lanes;
  int32_t n_steps;
};

template <bool NT, class T>
__device__ __forceinline__ T bsx_returns_ld(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

struct bsx_returns_row { float r, d, v; int8_t s; };

template <bool VALS, bool STEPS, int POLICY, int D>
__device__ __forceinline__ void bsx_returns_body(const bsx_returns_args& a, int64_t i) {
  constexpr bool NT_LD = (POLICY & 1) != 0;
  constexpr int ST = (POLICY & 2) != 0 ? BSX_ST_NT : BSX_ST_PLAIN;
  const int64_t B = a.n_lanes;
  const int T = a.n_steps;
  auto load = [&](int t) {
    const int64_t at = (int64_t)(t > 0 ? t : 0) * B + i;
    bsx_returns_row x;
    x.r = bsx_returns_ld<NT_LD>(a.reward + at);
    x.d = bsx_returns_ld<NT_LD>(a.discount + at);
    x.v = VALS ? bsx_returns_ld<NT_LD>(a.values + at) : 0.0f;
    x.s = STEPS ? bsx_returns_ld<NT_LD>(a.step_type + at) : (int8_t)BSX_MID;
    return x;
  };
  bsx_returns_row ring[D];
#pragma unroll
  for (int j = 0; j < D; ++j) ring[j] = load(T - 1 - j);
  double carry = 0.0, vnext = 0.0;                            // vals(t+1) and g of row t+1
  if (VALS) vnext = carry = (double)a.values[(int64_t)T * B + i];
  else if (a.bootstrap != nullptr) carry = (double)a.bootstrap[i];
  const bool want_returns = a.returns != nullptr, want_td = VALS && a.td_errors != nullptr;      // uniform
  for (int top = T - 1; top >= 0; top -= D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int t = top - j;
      const bsx_returns_row x = ring[j];
      ring[j] = load(t - D);
      if (t >= 0) {                                           // uniform: false in the last, partial turn of the ring only
        const double v = VALS ? (double)x.v : 0.0;
        const double dg = a.gamma * (double)x.d;
        const double mix = a.one_minus * vnext + a.lambda * carry;
        const double step = (double)x.r + dg * mix;
        const double g = (STEPS && x.s == BSX_FIRST) ? v : step;
        carry = g;
        vnext = v;
        const int64_t at = (int64_t)t * B + i;
        if (want_returns) bsx_st<ST>(a.returns + at, (float)g);
        if (want_td) bsx_st<ST>(a.td_errors + at, (float)(g - v));
      }
    }
  }
}

template <bool VALS, int POLICY, int AHEAD>
__global__ void __launch_bounds__(BSX_BLOCK) bsx_lambda_scan_kernel(const bsx_returns_args a) {
  const int64_t i = (int64_t)blockIdx.x * BSX_BLOCK + threadIdx.x;
  if (i >= a.n_lanes) return;
  if (a.step_type != nullptr) bsx_returns_body<VALS, true, POLICY, AHEAD>(a, i);       // uniform
  else bsx_returns_body<VALS, false, POLICY, AHEAD>(a, i);
}

template <int POLICY, int AHEAD>
static void bsx_launch_returns(const bsx_returns_args& a, int64_t blocks, hipStream_t st) {
  const dim3 g((unsigned)blocks), b(BSX_BLOCK);
  if (a.values != nullptr) bsx_lambda_scan_kernel<true, POLICY, AHEAD><<<g, b, 0, st>>>(a);
  else bsx_lambda_scan_kernel<false, POLICY, AHEAD><<<g, b, 0, st>>>(a);
}

extern "C" int bsx_lambda_returns(const bsx_returns_t* r, void* hip_stream) {
  if (r == nullptr) return BSX_ENULL;
  if (r->n_steps < 1 || r->n_lanes < 0 || r->n_lanes > ((int64_t)1 << 40)) return BSX_EINVAL;
  if (!(r->gamma >= 0.0 && r->gamma <= 1.0) || !(r->lambda >= 0.0 && r->lambda <= 1.0)) return BSX_ERANGE;   // NaN included
  if ((r->bootstrap != nullptr && r->values != nullptr) || (r->td_errors != nullptr && r->values == nullptr)) return BSX_EMODE;
  if (r->n_lanes == 0) return 0;
  if (r->reward == nullptr || r->discount == nullptr || (r->returns == nullptr && r->td_errors == nullptr)) return BSX_ENULL;
  const int64_t blocks = bsx_blocks_of(r->n_lanes);
  // (and the byte offset of the last element of values [T+1,B] must fit the kernel's int64 index math)
  if (blocks > 0x7FFFFFFF || r->n_lanes > (INT64_MAX / 4) / ((int64_t)r->n_steps + 1)) return BSX_EINVAL;
  bsx_returns_args a;
  a.reward = r->reward; a.discount = r->discount; a.step_type = r->step_type; a.values = r->values; a.bootstrap = r->bootstrap;
  a.returns = r->returns; a.td_errors = r->td_errors;
  a.gamma = r->gamma; a.lambda = r->lambda; a.one_minus = 1.0 - r->lambda;
  a.n_lanes = r->n_lanes; a.n_steps = r->n_steps;
  hipStream_t st = (hipStream_t)hip_stream;
#ifdef BSX_TUNING
  static const int policy = bsx_env_int("BSX_RETURNS_POLICY", BSX_RETURNS_POLICY);
  static const int ahead = bsx_env_int("BSX_RETURNS_AHEAD", BSX_RETURNS_AHEAD);
#define RETURNS_LAUNCH(P)                                                    \
  {                                                                          \
    if (ahead == 16) bsx_launch_returns<P, 16>(a, blocks, st);               \
    else if (ahead == 4) bsx_launch_returns<P, 4>(a, blocks, st);            \
    else bsx_launch_returns<P, 8>(a, blocks, st);                            \
  }
  switch (policy & 3) {
    case 0: RETURNS_LAUNCH(0) break;
    case 1: RETURNS_LAUNCH(1) break;
    case 2: RETURNS_LAUNCH(2) break;
    default: RETURNS_LAUNCH(3) break;
  }
#undef RETURNS_LAUNCH
#else
  bsx_launch_returns<BSX_RETURNS_POLICY, BSX_RETURNS_AHEAD>(a, blocks, st);
#endif
  return bsx_launch_status();
}
