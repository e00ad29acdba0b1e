// memory_chain_env.h — device code of memory_chain (bsuite/environments/memory_chain.py:60-97): the family as small_obs.h's skeleton sees it
// (the interface is written down at the top of small_obs.h).
#ifndef BSX_MEMORY_CHAIN_ENV_H_
#define BSX_MEMORY_CHAIN_ENV_H_

#include "small_obs.h"

#define MC_RESET_BIT (1 << 28)
struct memory_chain_env : small_regs_defaults {
  // Register-resident in a fused rollout of SHORT rows (num_bits <= 6: the row is stored by the lane's own thread) — every
  // memory_len id has one context bit.  The generic rollout re-read the lane's state word and context from L2 on every
  // step behind a drain of the previous step's stores (three dependent round trips per step): memory_len/10 took 13.6 us
  // per step inside rollout(16) against 12.3 us for an eager step() (profiles/r05/bench_default_call1.json).
  static constexpr bool HAS_REGS = true, PACKED = true;
  __host__ __device__ static constexpr int numel_of(int) { return 3; }     // variant 0: one context bit, rows of 3 floats
  struct regs { int32_t st; uint64_t ctx; double inf[2]; };                // inf: total_perfect, total_regret in a fused rollout
  struct args {
    bsx_ctl ctl; const int32_t* action; int32_t* state; uint64_t* context; bsx_timestep_t out;
    double* info; int32_t obs_numel; int32_t L; int32_t nb; uint32_t numel_magic;
    uint32_t* rows; int64_t row_plane_words;                   // bsx_call_t.row_scratch (bsx_rows.h) + words per plane, or nullptr
  };
  // Packed rows: HEAD = [time, query]; element 2+b is 0 unless t == 0, then +-1 by context bit b: plane 0 says
  // "non-zero", plane 1 carries the context bit (memory_rows, row_stream.h).
  // (PACKED path: the time fractions in LDS when the chain has at most 1024 steps)
  __host__ __device__ static bool tf_table_fits(const args& a) { return a.L <= 1023; }
  typedef memory_rows rows_t;
  static constexpr int HEAD = rows_t::HEAD, PLANES = rows_t::PLANES;
  __device__ static float decode(uint32_t nonzero, uint32_t bit) { return rows_t::decode(nonzero, bit); }
  template <bool PACK, class Sink>
  __device__ static void observe(const args& a, float* o, int t, int query, uint64_t ctx, const Sink* sink) {
    BSX_NO_CONTRACT
    // (PACK: o[0], the time fraction of :64, is step()'s — bsx_chain_time_fraction)
    if constexpr (!PACK) o[0] = (float)(1.0 - (double)t / (double)a.L);   // memory_chain.py:64
    o[1] = (t == a.L - 1) ? (float)query : 0.0f;                // :66-67
    if constexpr (PACK) {
      if (t == 0) {                                             // :69-70 (the tile is zero-filled before every step)
        const int n0 = a.nb < 32 ? a.nb : 32;
        sink->put(0, 0, 0xFFFFFFFFu, n0);
        sink->put(1, 0, (uint32_t)ctx, n0);
        if (a.nb > 32) {
          sink->put(0, 1, 0xFFFFFFFFu, a.nb - 32);
          sink->put(1, 1, (uint32_t)(ctx >> 32), a.nb - 32);
        }
      }
    } else {
      for (int b = 0; b < a.nb; ++b)                            // :69-70
        o[2 + b] = (t == 0) ? (float)(2 * (int)((ctx >> b) & 1ull) - 1) : 0.0f;
    }
  }
  // ---- the register-resident form (small_obs_regs_rollout): state word + context in registers for the T steps
  static int variant_of(const args& a) { return a.nb == 1 ? 0 : -1; }
  __device__ static __forceinline__ void clear(regs& r) { r.st = 0; r.ctx = 0ull; }
  __device__ static __forceinline__ bool reset_pending(const regs& r) { return (r.st & MC_RESET_BIT) != 0; }
  // the time fraction 1 - t / L (an f64 division per step) from a table in LDS that the workgroup fills once per launch with
  // that same division
  static constexpr int TABLE_MAX_BYTES = 16384;
  __host__ __device__ static bool table_fits(const args& a) { return ((int64_t)a.L + 1) * 4 <= TABLE_MAX_BYTES; }
  static size_t table_bytes(const args& a) { return table_fits(a) ? ((size_t)a.L + 1) * 4 : 0; }
  __device__ static __forceinline__ bsx_lds_table stage_tables(const args& a, float* s_dyn) {
    BSX_NO_CONTRACT
    for (int k = threadIdx.x; k <= a.L; k += BSX_BLOCK) s_dyn[k] = (float)(1.0 - (double)k / (double)a.L);
    return (bsx_lds_table)s_dyn;
  }
  template <int V = -1>
  __device__ static __forceinline__ void load_info(const args& a, int64_t i, regs& r) { r.inf[0] = a.info[i]; r.inf[1] = a.info[a.ctl.n_lanes + i]; }
  template <int V = -1>
  __device__ static __forceinline__ void store_info(const args& a, int64_t i, const regs& r) { a.info[i] = r.inf[0]; a.info[a.ctl.n_lanes + i] = r.inf[1]; }
  __device__ static __forceinline__ void load(const args& a, int64_t i, regs& r) { r.st = a.state[i]; r.ctx = a.context[i]; }
  __device__ static __forceinline__ void store(const args& a, int64_t i, const regs& r) { a.state[i] = r.st; a.context[i] = r.ctx; }
  // One reset()/step() of the lane in `rg` (memory_chain.py:60-97; the same transitions, draws and info updates as step()
  // below — tests/test_gpu_rollout.py holds rollout(T) to T step() calls bit for bit).  Short rows only: o[0 .. nb + 2).
  template <int LOG, int MT, bool IREGS = false, bool TAB = false, bool POOL = false, int V = -1, bool NOFORCE = false>
  __device__ static __forceinline__ int core(const args& a, regs& rg, const int act, int64_t i, uint64_t lane, uint64_t step,
                                             float* o, double& reward, bsx_lds_table s_tf = (bsx_lds_table)0,
                                             const bsx_reset_pool* = nullptr) {
    BSX_NO_CONTRACT
    const int nb = V == 0 ? 1 : a.nb;
    const int32_t st = rg.st;
    int t = st & 0xFFFFF, query = (st >> 20) & 0xFF;
    uint64_t ctx = rg.ctx;
    const bool reset = (!NOFORCE && a.ctl.force_reset) || (st & MC_RESET_BIT);
    if (reset) {                                                // :91-97
      bsx_draws d;
      bsx_draws_begin<MT>(&d, a.ctl, i, lane, step);
      ctx = 0;
      if (MT == 0 || d.mt == nullptr) {
        ctx = (uint64_t)bsx_word(&d) & ((1ull << nb) - 1ull);   // BernVec(nb), nb <= 6 here: the low bits of one word
      } else {
        uint32_t w = 0;
        for (int b = 0; b < nb; ++b) ctx |= (uint64_t)bsx_bern_vec_bit(&d, b, &w) << b;
      }
      query = (int)bsx_randint(&d, (uint32_t)nb);
      bsx_draws_end<MT>(&d, a.ctl, i);
      t = 0;
      rg.ctx = ctx;
    }
    // the observation of the state BEFORE the step's increment (:74; after a reset: of the fresh state)
    if constexpr (TAB) o[0] = s_tf[t];                          // (t <= L)
    else o[0] = (float)(1.0 - (double)t / (double)a.L);         // :64
    o[1] = (t == a.L - 1) ? (float)query : 0.0f;                // :66-67
#pragma unroll
    for (int b = 0; b < 6; ++b)
      if (b < nb) o[2 + b] = (t == 0) ? (float)(2 * (int)((ctx >> b) & 1ull) - 1) : 0.0f;   // :69-70
    if (reset) { rg.st = t | (query << 20); return BSX_FIRST; }
    t += 1;                                                     // :75
    if (t - 1 < a.L) { rg.st = t | (query << 20); return BSX_MID; }   // :77-79
    const bool hit = act == (int)((ctx >> query) & 1ull);
    reward = hit ? 1.0 : -1.0;                                  // :83-88
    if constexpr (IREGS) {
      if (hit) rg.inf[0] += 1.0; else rg.inf[1] += 2.0;
    } else {
      const bool quiet = a.L >= 8 && bsx_info_quiet<LOG>(a.ctl);
      if (hit) bsx_info_add(quiet, &a.info[i], 1.0); else bsx_info_add(quiet, &a.info[a.ctl.n_lanes + i], 2.0);
    }
    rg.st = t | (query << 20) | MC_RESET_BIT;
    return BSX_LAST;
  }
  template <int LOG, int MT, bool PACK = false, class Sink = bsx_bit_sink>
  __device__ static int step(const args& a, int64_t i, int64_t oi, uint64_t lane, uint64_t step, float* o, double& reward,
                             const Sink* sink = nullptr) {
    int32_t st = a.state[i];
    const int act = a.ctl.force_reset ? 0 : bsx_action(a.ctl, a.action, oi, step);   // (see umbrella_chain_env::step)
    int t = st & 0xFFFFF, query = (st >> 20) & 0xFF;
    uint64_t ctx = a.context[i];
    const bool resets = a.ctl.force_reset || (st & MC_RESET_BIT);
    // :64 — of the state BEFORE the increment (:74), or of the fresh one (short rows: observe() does it, where it always was)
    if constexpr (PACK) o[0] = bsx_chain_time_fraction<PACK>(resets ? 0 : t, a.L, sink);
    if (resets) {                                               // :91-97
      bsx_draws d;
      bsx_draws_begin<MT>(&d, a.ctl, i, lane, step);
      ctx = 0;
      if (MT == 0 || d.mt == nullptr) {                         // BernVec(nb) = the low nb bits of ceil(nb/32) words
        ctx = (uint64_t)bsx_word(&d);
        if (a.nb > 32) ctx |= (uint64_t)bsx_word(&d) << 32;
        ctx &= (1ull << a.nb) - 1ull;                           // nb <= 62
      } else {
        uint32_t w = 0;
        for (int b = 0; b < a.nb; ++b) ctx |= (uint64_t)bsx_bern_vec_bit(&d, b, &w) << b;   // one legacy double per bit
      }
      query = (int)bsx_randint(&d, (uint32_t)a.nb);
      bsx_draws_end<MT>(&d, a.ctl, i);
      t = 0;
      a.context[i] = ctx;
      a.state[i] = t | (query << 20);
      observe<PACK>(a, o, t, query, ctx, sink);
      return BSX_FIRST;
    }
    observe<PACK>(a, o, t, query, ctx, sink);                   // :74 — before the increment
    t += 1;                                                     // :75
    if (t - 1 < a.L) { a.state[i] = t | (query << 20); return BSX_MID; }   // :77-79
    // (the episode's one bsuite_info update: a no-return atomic when episodes are long, i.e. when only a few lanes of a
    // wave end on a given call — bsx_info_add)
    const bool quiet = a.L >= 8 && bsx_info_quiet<LOG>(a.ctl);
    if (act == (int)((ctx >> query) & 1ull)) { reward = 1.0; bsx_info_add(quiet, &a.info[i], 1.0); }   // :83-85
    else { reward = -1.0; bsx_info_add(quiet, &a.info[a.ctl.n_lanes + i], 2.0); }   // :86-88
    a.state[i] = t | (query << 20) | MC_RESET_BIT;
    return BSX_LAST;
  }
};

#endif  // BSX_MEMORY_CHAIN_ENV_H_
