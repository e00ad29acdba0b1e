// discounting_chain_env.h — device code of discounting_chain (bsuite/environments/discounting_chain.py:63-88): the family as small_obs.h's skeleton sees it
// (the interface is written down at the top of small_obs.h).
#ifndef BSX_DISCOUNTING_CHAIN_ENV_H_
#define BSX_DISCOUNTING_CHAIN_ENV_H_

#include "small_obs.h"

#define DC_RESET_BIT (1 << 12)
struct discounting_chain_env : small_regs_defaults {
  static constexpr bool HAS_REGS = true, PACKED = false;        // (register-resident in a fused rollout, like the bandit)
  static constexpr int EAGER_LPT_MIN_BLOCKS = 4096;              // (two lanes per thread: equal at 2^19 lanes)
  __host__ __device__ static constexpr int numel_of(int) { return 2; }
  struct regs { int32_t st; };
  struct args {
    bsx_ctl ctl; const int32_t* action; int32_t* state; bsx_timestep_t out;
    int32_t obs_numel; int32_t bonus;
  };
  static int variant_of(const args&) { return 0; }
  // state word: timestep (bits 0-7) | context + 6 (bits 8-11: the context is the episode's first action, -5..4, -1 after a
  // reset — the reference indexes Python lists with it, so -5..-1 are legal and wrap, discounting_chain.py:76-81) | reset_next
  __device__ static __forceinline__ int dc_context(int32_t st) { return ((st >> 8) & 0xF) - 6; }
  __device__ static __forceinline__ int32_t dc_pack(int t, int ctx, bool last) {
    return t | ((ctx + 6) << 8) | (last ? DC_RESET_BIT : 0);
  }
  __device__ static __forceinline__ void clear(regs& r) { r.st = dc_pack(0, -1, false); }
  __device__ static __forceinline__ bool reset_pending(const regs& r) { return (r.st & DC_RESET_BIT) != 0; }
  __device__ static __forceinline__ void load(const args& a, int64_t i, regs& r) { r.st = a.state[i]; }
  __device__ static __forceinline__ void store(const args& a, int64_t i, const regs& r) { a.state[i] = r.st; }
  template <int LOG, int MT, bool IREGS = false, bool TAB = false, bool POOL = false, int V = -1, bool NOFORCE = false>
  __device__ static __forceinline__ int core(const args& a, regs& rg, const int act, int64_t i, uint64_t, uint64_t,
                                             float* o, double& reward, bsx_lds_table = (bsx_lds_table)0,
                                             const bsx_reset_pool* = nullptr) {
    BSX_NO_CONTRACT
    const int32_t st = rg.st;
    int t = st & 0xFF, ctx = dc_context(st);
    if ((!NOFORCE && a.ctl.force_reset) || (st & DC_RESET_BIT)) {   // discounting_chain.py:69-73
      o[0] = -1.0f; o[1] = 0.0f;
      rg.st = dc_pack(0, -1, false);
      return BSX_FIRST;
    }
    if (t == 0) {                                               // :76-77
      ctx = act;
      if (ctx < -5 || ctx > 4) {                                // reference: IndexError at the lookup of :80
        bsx_note_invalid_action(a.ctl, i);
        ctx = ctx < 0 ? 0 : 4;
      }
    }
    t += 1;
    const int chain = ctx < 0 ? ctx + 5 : ctx;                  // :80-81 index Python lists: -5..-1 wrap, the context stays negative
    const int when = chain == 0 ? 1 : chain == 1 ? 3 : chain == 2 ? 10 : chain == 3 ? 30 : 100;   // :49
    if (t == when) reward = (chain == a.bonus) ? 1.0 + 0.1 : 1.0;                          // :57-58,80-83
    o[0] = (float)ctx;                                          // :65
    o[1] = (float)((double)t / 100.0);                          // :66
    const int type = (t == 100) ? BSX_LAST : BSX_MID;           // :86-88
    rg.st = dc_pack(t, ctx, type == BSX_LAST);
    return type;
  }
  template <int LOG, int MT>
  __device__ static int step(const args& a, int64_t i, int64_t oi, uint64_t, uint64_t step, float* o, double& reward) {
    BSX_NO_CONTRACT
    int32_t st = a.state[i];
    int t = st & 0xFF, ctx = dc_context(st);
    if (a.ctl.force_reset || (st & DC_RESET_BIT)) {             // discounting_chain.py:69-73
      t = 0; ctx = -1;
      o[0] = -1.0f; o[1] = 0.0f;
      a.state[i] = dc_pack(0, -1, false);
      return BSX_FIRST;
    }
    if (t == 0) {                                               // :76-77
      ctx = bsx_action(a.ctl, a.action, oi, step);
      if (ctx < -5 || ctx > 4) {                                // reference: IndexError at the lookup of :80
        bsx_note_invalid_action(a.ctl, i);
        ctx = ctx < 0 ? 0 : 4;                                  // action_spec: 5 values; never OOB
      }
    }
    t += 1;
    const int chain = ctx < 0 ? ctx + 5 : ctx;                  // :80-81 index Python lists: -5..-1 wrap, the context stays negative
    const int when = chain == 0 ? 1 : chain == 1 ? 3 : chain == 2 ? 10 : chain == 3 ? 30 : 100;   // :49
    if (t == when) reward = (chain == a.bonus) ? 1.0 + 0.1 : 1.0;                          // :57-58,80-83
    o[0] = (float)ctx;                                          // :65
    o[1] = (float)((double)t / 100.0);                          // :66
    const int type = (t == 100) ? BSX_LAST : BSX_MID;           // :86-88
    a.state[i] = dc_pack(t, ctx, type == BSX_LAST);
    return type;
  }
};

template <>
struct small_obs_duo_group<discounting_chain_env> { static constexpr bool value = true; };   // (small_obs.h)

#endif  // BSX_DISCOUNTING_CHAIN_ENV_H_
