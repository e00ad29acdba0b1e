// cartpole_env.h — device code of cartpole / cartpole_swingup (bsuite/environments/cartpole.py:37-177,
// bsuite/experiments/cartpole_swingup/cartpole_swingup.py:81-150): the family as small_obs.h's skeleton sees it
// (the interface is written down at the top of small_obs.h).
#ifndef BSX_CARTPOLE_ENV_H_
#define BSX_CARTPOLE_ENV_H_

#include "bsx_math.h"
#include "small_obs.h"

// Info columns (f64 [4,B]): 0 raw_return, 1 best_episode, 2 episode_return, 3 total_upright.
// Classic cartpole pays r in {0, 1}: an episode of k steps returns (k-1) + [last step rewarded], so
// raw_return / best_episode / episode_return are EXACT integer-valued functions of the step counter and
// are folded into the f64 columns only when the episode ends (column 0 then holds finished episodes;
// the host adds the running episode's k, environments/cartpole.py).  That removes two f64
// read-modify-writes (32 B) per lane per step — a third of the step's HBM traffic.  Swing-up's
// rewards (-0.1*|a-1| + 1) do not sum exactly out of order and the fused Logging rows snapshot the
// columns mid-episode, so swing-up and logging runs keep the reference's per-step accumulation.
struct cartpole_env {
  struct args {
    bsx_ctl ctl; const int32_t* action; float* state; int32_t* steps; bsx_timestep_t out;
    double* info; int32_t obs_numel; bsx_cartpole_t cfg;
    // derived on the host in f64, rounded once (cartpole_make)
    float inv_m_total, pole_ml, pole_ml_over_mt, den_a, den_b, inv_x_threshold;
  };
  // The lane's state in registers: step() = load + core + store; the fused rollout loads once, runs core
  // T times and stores once (small_obs_body), instead of a round trip through L2 every step.
  static constexpr bool HAS_REGS = true, PACKED = false, POOLED_RESETS = true, ROWS_VIA_LDS = true;
  static constexpr int EAGER_LPT_MIN_BLOCKS = 0, EAGER_LPT = 2;      // (equal within noise at 2^20 lanes, 4 % slower at 2^19)
  // compile-time variants of the lean fused rollout (small_obs_regs_rollout, V): 0 = classic, 1 = swing-up
  static constexpr int N_VARIANTS = 2;
  __host__ __device__ static constexpr int numel_of(int v) { return v == 1 ? 8 : 6; }
  static int variant_of(const args& a) { return a.cfg.swingup ? 1 : 0; }
  struct regs { float x, xd, th, thd; int32_t sk; double inf[4]; };     // inf: the info columns in a fused rollout
  // NOFORCE: inside a rollout (n_steps > 1 excludes force_reset: bsx_check_call)
  template <bool NOFORCE = false>
  __device__ static __forceinline__ bool wants_reset(const args& a, const regs& r) { return (!NOFORCE && a.ctl.force_reset) || (r.sk & CP_RESET_BIT); }
  __device__ static __forceinline__ void clear(regs& r) { r.sk = 0; }
  __device__ static __forceinline__ bool reset_pending(const regs& r) { return (r.sk & CP_RESET_BIT) != 0; }
  // Half of a lane's reset (cartpole.py:118-128), counter-based stream only: part 0 = x, x_dot from words 0..3 of
  // the (lane, step) stream, part 1 = theta, theta_dot from words 4..7 and the new angle's sine / cosine — the same
  // words, the same arithmetic as core()'s in-line reset, one Philox block per part.
  // (Tried: these parameters in LDS, read where they are used, instead of ten scalar registers live through the
  // whole step loop — no spill reload left in any variant's loop, but either the Philox key schedule moves to the
  // vector unit (80 VGPRs) or, with the words read back into scalar registers, the allocator still ends at 68-71
  // VGPRs instead of 61-65: one reload per step is the cheaper price.)
  __device__ static __forceinline__ void reset_part(const args& a, uint64_t lane, uint64_t step, int part, unsigned owner,
                                                    bsx_reset_pool* pool) {
    BSX_NO_CONTRACT
    const bsx_cartpole_t& g = a.cfg;
    bsx_draws d;
    bsx_draws_init(&d, a.ctl.seed, lane, step, BSX_STREAM_ENV);
    d.next = 4u * (uint32_t)part;
    const double lo = -g.init_range, hi = g.init_range;
    const double w0 = lo + (hi - lo) * bsx_uniform(&d);
    const double w1 = lo + (hi - lo) * bsx_uniform(&d);
    const float v0 = (float)(part ? g.theta_offset + w0 : w0), v1 = (float)w1;
    float si, co;
    bsx_sincosf(v0, &si, &co);
    pool->vals[2 * part][owner] = v0;
    pool->vals[2 * part + 1][owner] = v1;
    if (part) { pool->vals[4][owner] = si; pool->vals[5][owner] = co; }
  }
  // Fused rollouts keep the time-fraction table in LDS when it is small (the default 1002 entries: 4 KiB)
  static constexpr int TABLE_MAX_BYTES = 16384;
  __host__ __device__ static bool table_fits(const args& a) { return ((int64_t)a.cfg.last_step + 1) * 4 <= TABLE_MAX_BYTES; }
  static size_t table_bytes(const args& a) { return table_fits(a) ? ((size_t)a.cfg.last_step + 1) * 4 : 0; }
  __device__ static __forceinline__ bsx_lds_table stage_tables(const args& a, float* s_dyn) {
    const int n = a.cfg.last_step + 1;
    for (int k = threadIdx.x; k < n; k += BSX_BLOCK) s_dyn[k] = a.cfg.time_frac[k];
    return (bsx_lds_table)s_dyn;
  }
  template <int V = -1>
  __device__ static __forceinline__ void load_info(const args& a, int64_t i, regs& r) {
    const int64_t B = a.ctl.n_lanes;
    r.inf[0] = a.info[i]; r.inf[1] = a.info[B + i];
    if (V >= 0 ? V == 1 : (bool)a.cfg.swingup) { r.inf[2] = a.info[2 * B + i]; r.inf[3] = a.info[3 * B + i]; }
    else { r.inf[2] = 0.0; r.inf[3] = 0.0; }
  }
  template <int V = -1>
  __device__ static __forceinline__ void store_info(const args& a, int64_t i, const regs& r) {
    const int64_t B = a.ctl.n_lanes;
    a.info[i] = r.inf[0]; a.info[B + i] = r.inf[1];
    if (V >= 0 ? V == 1 : (bool)a.cfg.swingup) { a.info[2 * B + i] = r.inf[2]; a.info[3 * B + i] = r.inf[3]; }
  }
  __device__ static __forceinline__ void load(const args& a, int64_t i, regs& r) {
    const int64_t B = a.ctl.n_lanes;
    r.sk = a.steps[i];
    r.x = a.state[i]; r.xd = a.state[B + i]; r.th = a.state[2 * B + i]; r.thd = a.state[3 * B + i];
  }
  __device__ static __forceinline__ void store(const args& a, int64_t i, const regs& r) {
    const int64_t B = a.ctl.n_lanes;
    a.state[i] = r.x; a.state[B + i] = r.xd; a.state[2 * B + i] = r.th; a.state[3 * B + i] = r.thd;
    a.steps[i] = r.sk;
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
  // IREGS: the info columns are rg.inf[] (fused rollout without Logging), else read-modify-written in HBM.
  // s_tf: the time-fraction table in LDS, or nullptr (-> g.time_frac in device memory).
  // POOL: the reset values were computed by the workgroup's pool (reset_part) and wait in s_pool.
  // V: -1 = swing-up or not is a.cfg.swingup, 0 / 1 = known at compile time.  NOFORCE: see wants_reset.
  template <int LOG, int MT, bool IREGS = false, bool TAB = false, bool POOL = false, int V = -1, bool NOFORCE = false>
  __device__ static __forceinline__ int core(const args& a, regs& rg, const int act, int64_t i, uint64_t lane, uint64_t step,
                                             float* o, double& reward, bsx_lds_table s_tf = (bsx_lds_table)0,
                                             const bsx_reset_pool* s_pool = nullptr) {
    BSX_NO_CONTRACT
    const int64_t B = a.ctl.n_lanes;
    const bsx_cartpole_t& g = a.cfg;
    const bool swingup = V >= 0 ? V == 1 : (bool)g.swingup;
    auto info_get = [&](int col) -> double { if constexpr (IREGS) return rg.inf[col]; else return a.info[(int64_t)col * B + i]; };
    auto info_set = [&](int col, double v) { if constexpr (IREGS) rg.inf[col] = v; else a.info[(int64_t)col * B + i] = v; };
    const int32_t sk = rg.sk;
    const bool per_step_info = swingup || LOG == 1 || (LOG == -1 && a.ctl.log.steps != nullptr);
    int k = sk & 0x3FFFFFFF;
    float x, xd, th, thd, si, co;
    int type;
    if ((!NOFORCE && a.ctl.force_reset) || (sk & CP_RESET_BIT)) {   // cartpole.py:118-128 / swingup:81-91
      // (Tried, not adopted — profiles/r03/ab_regs_rollout_scalar_reset_draws.log: walking the wave's few resetting
      // lanes one at a time with wave-uniform inputs puts the Philox rounds on the scalar unit and cuts the vector
      // instructions by 19 %, but the ~200-instruction dependent scalar chain per resetting lane stalls the wave
      // longer than the divergent branch did: fused rollout 12.5 -> 14.7 us per step.)
      if constexpr (POOL) {
        const unsigned me = threadIdx.x;
        x = s_pool->vals[0][me]; xd = s_pool->vals[1][me]; th = s_pool->vals[2][me]; thd = s_pool->vals[3][me];
        si = s_pool->vals[4][me]; co = s_pool->vals[5][me];
      } else {
        bsx_draws d;
        bsx_draws_begin<MT>(&d, a.ctl, i, lane, step);
        const double lo = -g.init_range, hi = g.init_range;
        x = (float)(lo + (hi - lo) * bsx_uniform(&d));
        xd = (float)(lo + (hi - lo) * bsx_uniform(&d));
        th = (float)(g.theta_offset + (lo + (hi - lo) * bsx_uniform(&d)));
        thd = (float)(lo + (hi - lo) * bsx_uniform(&d));
        bsx_draws_end<MT>(&d, a.ctl, i);
        bsx_sincosf(th, &si, &co);                             // |theta_offset| + init_range <= 32 (cartpole_make)
      }
      // an explicit reset() in mid-episode abandons it: the k rewards of 1 it has paid stay in raw_return
      if (!per_step_info && !(sk & CP_RESET_BIT) && k > 0) info_set(0, info_get(0) + (double)k);
      k = 0;
      if (per_step_info) info_set(2, 0.0);                      // _episode_return = 0
      type = BSX_FIRST;
    } else {
      x = rg.x; xd = rg.xd; th = rg.th; thd = rg.thd;
      // step_cartpole, cartpole.py:37-65, in f32.  One sine/cosine pair per step: that of the OLD
      // angle; the new angle's pair follows from it by the angle-addition formulas below.
      float s0, c0;
      bsx_sincosf(th, &s0, &c0);                                // th is in [0, 2*pi) or a reset value
      const float force = (float)(act - 1) * g.force_mag;
      const float temp = (force + a.pole_ml * (thd * thd) * s0) * a.inv_m_total;
      // theta_acc = (g sin - cos*temp) / (l (4/3 - m_p cos^2 / m_t)); v_rcp_f32 is 1 ulp and the
      // accelerations enter the state scaled by dt = 0.01
      const float theta_acc = (g.gravity * s0 - c0 * temp) * __builtin_amdgcn_rcpf(a.den_a - a.den_b * (c0 * c0));
      const float x_acc = temp - a.pole_ml_over_mt * theta_acc * c0;
      const float dth = g.timescale * thd;
      x = __builtin_fmaf(g.timescale, xd, x);
      xd = __builtin_fmaf(g.timescale, x_acc, xd);
      // np.remainder(theta + dt*theta_dot, 2*pi) in f64 (the period is not the f32 2*pi): one
      // conditional +-2*pi is exact (Sterbenz) whenever the sum is within one period of [0, 2*pi)
      const double raw_ang = (double)th + (double)g.timescale * (double)thd;
      double ang = raw_ang >= 6.283185307179586 ? raw_ang - 6.283185307179586       // selects, not branches
                   : (raw_ang < 0.0 ? raw_ang + 6.283185307179586 : raw_ang);
      if (!(ang >= 0.0 && ang < 6.283185307179586)) {           // |dt*theta_dot| > 2*pi (theta_dot > 600 rad/s:
        ang = (double)th + (double)g.timescale * (double)thd;   // only reachable from a loaded state)
        ang -= 6.283185307179586 * floor(ang / 6.283185307179586);
        if (!(ang >= 0.0 && ang < 6.283185307179586)) ang = 0.0;
      }
      th = (float)ang;
      thd = __builtin_fmaf(g.timescale, theta_acc, thd);
      if (fabsf(dth) <= 0.5f) bsx_sincos_advance(s0, c0, dth, &si, &co);
      else bsx_sincosf(th, &si, &co);                           // th is in [0, 2*pi) here
      k += 1;                                                   // time_elapsed += timescale (:63)
      const bool timeout = k >= g.last_step;                    // time_elapsed > max_time
      bool end;
      double r;
      if (!swingup) {                                           // cartpole.py:142-153
        const bool ok = (co > g.height_threshold) && (fabsf(x) < g.x_threshold);
        r = ok ? 1.0 : 0.0;
        end = timeout || !ok;
      } else {                                                  // swingup:104-123
        const bool up = (co > g.height_threshold) && (fabsf(thd) < g.theta_dot_threshold) &&
                        (fabsf(x) < g.x_reward_threshold);
        r = -1.0 * fabs((double)(act - 1)) * g.move_cost;
        if (up) { r += 1.0; info_set(3, info_get(3) + 1.0); }
        end = timeout || (fabsf(x) > g.x_threshold);
      }
      reward = r;
      type = end ? BSX_LAST : BSX_MID;
      if (per_step_info) {
        info_set(0, info_get(0) + r);                           // _raw_return
        const double ep = info_get(2) + r;                      // _episode_return
        info_set(2, ep);
        if (end) {
          const double best = info_get(1);
          info_set(1, ep > best ? ep : best);                   // max(episode_return, best_episode)
        }
      } else if (end) {
        const double ep = (double)(k - 1) + r;                  // sum of the episode's rewards, exact
        info_set(0, info_get(0) + ep);
        const double best = info_get(1);
        info_set(1, ep > best ? ep : best);
      }
    }
    rg.x = x; rg.xd = xd; rg.th = th; rg.thd = thd;
    rg.sk = k | (type == BSX_LAST ? CP_RESET_BIT : 0);
    o[0] = x * a.inv_x_threshold;                               // cartpole.py:171-176
    o[1] = xd * a.inv_x_threshold;
    o[2] = si;
    o[3] = co;
    o[4] = thd;
    const int kf = k < g.last_step ? k : g.last_step;
    if constexpr (TAB) o[5] = s_tf[kf];                         // the fused rollout's LDS copy
    else o[5] = g.time_frac[kf];
    if (swingup) {                                              // swingup:147-149
      o[6] = (fabsf(x) < g.x_reward_threshold) ? 1.0f : -1.0f;
      o[7] = (fabsf(thd) < g.theta_dot_threshold) ? 1.0f : -1.0f;
    }
    return type;
  }
};

#endif  // BSX_CARTPOLE_ENV_H_
