// mountain_car_env.h — device code of mountain_car (bsuite/environments/mountain_car.py:62-90): the family as small_obs.h's skeleton sees it
// (the interface is written down at the top of small_obs.h).
#ifndef BSX_MOUNTAIN_CAR_ENV_H_
#define BSX_MOUNTAIN_CAR_ENV_H_

#include "bsx_math.h"
#include "small_obs.h"

// Info column 0 = raw_return = -(steps taken): every step pays -1 (mountain_car.py:75-76), so the
// column is folded at episode ends (+= -t, exact) and the host subtracts the running episode's t;
// under the fused Logging wrapper (rows snapshot the column mid-episode) it is kept per step.
struct mountain_car_env : small_regs_defaults {
  struct args {
    bsx_ctl ctl; const int32_t* action; float* state; int32_t* steps; bsx_timestep_t out;
    double* info; int32_t obs_numel; int32_t max_steps;
  };
  // (resets are rare — 1000-step episodes — and one Philox block: not pooled; the 12-byte rows of a wave are one dense
  // 768-byte range already: staging them gained nothing, profiles/r03/ab_rows_via_lds.log)
  static constexpr bool HAS_REGS = true, PACKED = false;
  __host__ __device__ static constexpr int numel_of(int) { return 3; }
  static int variant_of(const args&) { return 0; }
  struct regs { float pos, vel; int32_t sk; double inf0; };             // inf0: raw_return in a fused rollout
  __device__ static __forceinline__ void clear(regs& r) { r.sk = 0; }
  __device__ static __forceinline__ bool reset_pending(const regs& r) { return (r.sk & CP_RESET_BIT) != 0; }
  // Fused rollouts read the time fraction t / max_steps (an f32 division: 11 of the step's ~95 vector instructions)
  // from a table in LDS that the workgroup fills once per launch with that same division.
  static constexpr int TABLE_MAX_BYTES = 16384;
  __host__ __device__ static bool table_fits(const args& a) { return ((int64_t)a.max_steps + 1) * 4 <= TABLE_MAX_BYTES; }
  static size_t table_bytes(const args& a) { return table_fits(a) ? ((size_t)a.max_steps + 1) * 4 : 0; }
  __device__ static __forceinline__ bsx_lds_table stage_tables(const args& a, float* s_dyn) {
    for (int k = threadIdx.x; k <= a.max_steps; k += BSX_BLOCK) s_dyn[k] = (float)k / (float)a.max_steps;
    return (bsx_lds_table)s_dyn;
  }
  template <int V = -1>
  __device__ static __forceinline__ void load_info(const args& a, int64_t i, regs& r) { r.inf0 = a.info[i]; }
  template <int V = -1>
  __device__ static __forceinline__ void store_info(const args& a, int64_t i, const regs& r) { a.info[i] = r.inf0; }
  __device__ static __forceinline__ void load(const args& a, int64_t i, regs& r) {
    r.sk = a.steps[i]; r.pos = a.state[i]; r.vel = a.state[a.ctl.n_lanes + i];
  }
  __device__ static __forceinline__ void store(const args& a, int64_t i, const regs& r) {
    a.state[i] = r.pos; a.state[a.ctl.n_lanes + i] = r.vel; a.steps[i] = r.sk;
  }
  template <int LOG, int MT>
  __device__ static int step(const args& a, int64_t i, int64_t oi, uint64_t lane, uint64_t step, float* o, double& reward) {
    regs r;
    load(a, i, r);
    const int act = a.ctl.force_reset ? 0 : bsx_action(a.ctl, a.action, oi, step);
    const int type = core<LOG, MT>(a, r, act, i, lane, step, o, reward);
    store(a, i, r);
    return type;
  }
  template <int LOG, int MT, bool IREGS = false, bool TAB = false, bool POOL = false, int V = -1, bool NOFORCE = false>
  __device__ static __forceinline__ int core(const args& a, regs& rg, const int act, int64_t i, uint64_t lane, uint64_t step,
                                             float* o, double& reward, bsx_lds_table s_tf = (bsx_lds_table)0,
                                             const bsx_reset_pool* = nullptr) {
    BSX_NO_CONTRACT
    const int32_t sk = rg.sk;
    int t = sk & 0x3FFFFFFF;
    auto info_add = [&](double v) { if constexpr (IREGS) rg.inf0 += v; else a.info[i] += v; };
    float pos, vel;
    int type;
    if ((!NOFORCE && a.ctl.force_reset) || (sk & CP_RESET_BIT)) {   // mountain_car.py:66-71
      bsx_draws d;
      bsx_draws_begin<MT>(&d, a.ctl, i, lane, step);
      // an explicit reset() in mid-episode abandons it: its t rewards of -1 stay in raw_return
      if (!(LOG == 1 || (LOG == -1 && a.ctl.log.steps != nullptr)) && !(sk & CP_RESET_BIT) && t > 0) info_add(-(double)t);
      t = 0;
      pos = (float)(-0.6 + (-0.4 - -0.6) * bsx_uniform(&d));
      bsx_draws_end<MT>(&d, a.ctl, i);
      vel = 0.0f;
      type = BSX_FIRST;
    } else {
      pos = rg.pos; vel = rg.vel;
      t += 1;                                                   // :74
      reward = -1.0;
      float sn, cs;
      bsx_sincosf(3.0f * pos, &sn, &cs);                        // position is clipped to [-1.2, 0.6]
      vel += (float)(act - 1) * 0.001f + cs * -0.0025f;            // :79-80
      vel = fminf(fmaxf(vel, -0.07f), 0.07f);                   // :81
      pos += vel;                                               // :82
      pos = fminf(fmaxf(pos, -1.2f), 0.6f);                     // :83
      if (pos == -1.2f) vel = fminf(fmaxf(vel, 0.0f), 0.07f);   // :84-85
      type = (pos >= 0.5f || t >= a.max_steps) ? BSX_LAST : BSX_MID;   // :88-90
      if (LOG == 1 || (LOG == -1 && a.ctl.log.steps != nullptr)) info_add(reward);   // :76, per step under Logging
      else if (type == BSX_LAST) info_add(-(double)t);          // the episode's t rewards of -1, exact
    }
    rg.pos = pos; rg.vel = vel;
    rg.sk = t | (type == BSX_LAST ? CP_RESET_BIT : 0);
    o[0] = pos;                                                 // :62-64
    o[1] = vel;
    if constexpr (TAB) o[2] = s_tf[t];                          // (t <= max_steps)
    else o[2] = (float)t / (float)a.max_steps;                  // both exact in f32; correctly rounded quotient
    return type;
  }
};
// (with its 12-byte rows non-temporal, mountain_car's rollout is faster with ORDINARY scalar stores: 4.45 against 4.7 us per step)
template <> struct small_rollout_nt_scalars<mountain_car_env> { static constexpr bool value = false; };

#endif  // BSX_MOUNTAIN_CAR_ENV_H_
