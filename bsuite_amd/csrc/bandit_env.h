// bandit_env.h — device code of bandit (bsuite/environments/bandit.py:54-64): the family as small_obs.h's skeleton sees it
// (the interface is written down at the top of small_obs.h).
#ifndef BSX_BANDIT_ENV_H_
#define BSX_BANDIT_ENV_H_

#include "small_obs.h"

struct bandit_env : small_regs_defaults {
  // (register-resident in a fused rollout: the generic loop re-read the reset flag from L2 behind a drain of the previous
  // step's stores and read-modify-wrote the f64 regret column on every second step — 16 of the step's 33 bytes)
  static constexpr bool HAS_REGS = true, PACKED = false;
  __host__ __device__ static constexpr int numel_of(int) { return 1; }
  struct regs { int32_t st; double inf0; };                    // inf0: total_regret in a fused rollout
  struct args {
    bsx_ctl ctl; const int32_t* action; int32_t* state; bsx_timestep_t out; double* info;
    int32_t obs_numel; int32_t num_actions; double rewards[BSX_BANDIT_MAX_ACTIONS];
  };
  static int variant_of(const args&) { return 0; }
  __device__ static __forceinline__ void clear(regs& r) { r.st = 0; }
  __device__ static __forceinline__ bool reset_pending(const regs& r) { return r.st != 0; }
  template <int V = -1>
  __device__ static __forceinline__ void load_info(const args& a, int64_t i, regs& r) { r.inf0 = a.info[i]; }
  template <int V = -1>
  __device__ static __forceinline__ void store_info(const args& a, int64_t i, const regs& r) { a.info[i] = r.inf0; }
  __device__ static __forceinline__ void load(const args& a, int64_t i, regs& r) { r.st = a.state[i]; }
  __device__ static __forceinline__ void store(const args& a, int64_t i, const regs& r) { a.state[i] = r.st; }
  // (the same transitions as step() below; tests/test_gpu_rollout.py holds rollout(T) to T step() calls bit for bit)
  template <int LOG, int MT, bool IREGS = false, bool TAB = false, bool POOL = false, int V = -1, bool NOFORCE = false>
  __device__ static __forceinline__ int core(const args& a, regs& rg, int act, int64_t i, uint64_t, uint64_t,
                                             float* o, double& reward, bsx_lds_table = (bsx_lds_table)0,
                                             const bsx_reset_pool* = nullptr) {
    BSX_NO_CONTRACT
    o[0] = 1.0f;                                                // bandit.py:54 (ones)
    if ((!NOFORCE && a.ctl.force_reset) || rg.st) { rg.st = 0; return BSX_FIRST; }
    if (act < 0 || act >= a.num_actions) {                      // reference: IndexError (bandit.py:61)
      bsx_note_invalid_action(a.ctl, i);
      act = act < 0 ? 0 : a.num_actions - 1;
    }
    reward = a.rewards[act];                                    // :61
    if constexpr (IREGS) rg.inf0 += 1.0 - reward; else a.info[i] += 1.0 - reward;   // :62
    rg.st = 1;
    return BSX_LAST;                                            // :64
  }
  template <int LOG, int MT>
  __device__ static int step(const args& a, int64_t i, int64_t oi, uint64_t, uint64_t step, float* o, double& reward) {
    BSX_NO_CONTRACT
    o[0] = 1.0f;                                                // bandit.py:54 (ones)
    if (a.ctl.force_reset || a.state[i]) { a.state[i] = 0; return BSX_FIRST; }
    int act = bsx_action(a.ctl, a.action, oi, step);
    if (act < 0 || act >= a.num_actions) {                      // reference: IndexError (bandit.py:61)
      bsx_note_invalid_action(a.ctl, i);
      act = act < 0 ? 0 : a.num_actions - 1;                    // never read OOB
    }
    reward = a.rewards[act];                                    // :61
    a.info[i] += 1.0 - reward;                                  // :62 (every second call of every lane: a plain
                                                                //      read-modify-write beats 2^20 atomics, 9.6 vs 11.2 us)
    a.state[i] = 1;
    return BSX_LAST;                                            // :64
  }
};

template <>
struct small_obs_duo_group<bandit_env> { static constexpr bool value = true; };   // (small_obs.h)

#endif  // BSX_BANDIT_ENV_H_
