// umbrella_chain_env.h — device code of umbrella_chain (bsuite/environments/umbrella_chain.py:60-92): the family as small_obs.h's skeleton sees it
// (the interface is written down at the top of small_obs.h).
#ifndef BSX_UMBRELLA_CHAIN_ENV_H_
#define BSX_UMBRELLA_CHAIN_ENV_H_

#include "small_obs.h"

#define UC_RESET_BIT (1 << 22)
struct umbrella_chain_env {
  static constexpr bool HAS_REGS = false, PACKED = true;
  struct regs { int unused; };
  struct args {
    bsx_ctl ctl; const int32_t* action; int32_t* state; bsx_timestep_t out; double* info;
    int32_t obs_numel; int32_t L; int32_t nd; uint32_t numel_magic;
    uint32_t* rows; int64_t row_plane_words;                   // bsx_call_t.row_scratch (bsx_rows.h) + words per plane, or nullptr
  };
  // Packed rows: HEAD = [need, has, time]; element 3+b is distractor bit b as 0.0 / 1.0 (one plane; umbrella_rows).
  __host__ __device__ static bool tf_table_fits(const args& a) { return a.L <= 1023; }
  typedef umbrella_rows rows_t;
  static constexpr int HEAD = rows_t::HEAD, PLANES = rows_t::PLANES;
  __device__ static float decode(uint32_t bit, uint32_t) { return rows_t::decode(bit, 0u); }
  template <bool PACK, int MT, class Sink>
  __device__ static void observe(const args& a, float* o, int t, int need, int has, bsx_draws* d, const Sink* sink) {
    BSX_NO_CONTRACT
    o[0] = (float)need;                                         // umbrella_chain.py:62
    o[1] = (float)has;                                          // :63
    // (o[2], the time fraction of :64, is step()'s: bsx_chain_time_fraction)
    uint32_t w = 0;
    if constexpr (PACK) {
      if (MT == 0 || d->mt == nullptr) {
        // :65 BernVec(nd) IS a run of stream words (bit i of the vector = bit i%32 of word i/32): hand the words to
        // the tile as they come — a bit-by-bit loop cost ~30 scalar + ~5 vector instructions per distractor
        // (3400 SALU per wave at nd = 100, profiles/r03/umbrella_distract_before_pmc_sq.json)
        for (int k = 0; 32 * k < a.nd; ++k) {
          const int n = a.nd - 32 * k;
          sink->put(0, k, bsx_word(d), n < 32 ? n : 32);
        }
      } else {
        uint32_t acc = 0;
        for (int b = 0; b < a.nd; ++b) {                        // MT19937-exact mode: one legacy double per bit
          acc |= bsx_bern_vec_bit(d, b, &w) << (b & 31);
          if ((b & 31) == 31 || b == a.nd - 1) { sink->put(0, b >> 5, acc, (b & 31) + 1); acc = 0; }
        }
      }
    } else {
      for (int b = 0; b < a.nd; ++b) o[3 + b] = (float)bsx_bern_vec_bit(d, b, &w);   // :65 BernVec(nd)
    }
  }
  template <int LOG, int MT, bool PACK = false, class Sink = bsx_bit_sink>
  __device__ static int step(const args& a, int64_t i, int64_t oi, uint64_t lane, uint64_t step, float* o, double& reward,
                             const Sink* sink = nullptr) {
    BSX_NO_CONTRACT
    int32_t st = a.state[i];
    // (the action matters on the episode's first step only, but which lanes are there is known when the state word has
    // arrived: loaded now, beside it, not in a second dependent round trip — in any real batch every wave holds such a
    // lane, and the line is fetched for it anyway)
    const int act = a.ctl.force_reset ? 0 : bsx_action(a.ctl, a.action, oi, step);
    int t = st & 0xFFFFF, need = (st >> 20) & 1, has = (st >> 21) & 1;
    bsx_draws d;
    bsx_draws_begin<MT>(&d, a.ctl, i, lane, step);
    // (every path below draws from block 0 of the lane's stream: computed once, before the lanes of a wave — at different
    // episode phases in any real batch — part ways; 659 -> see profiles/r05/ab_umbrella_shared_philox_block.log)
    bsx_draws_prime(&d);
    const bool resets = a.ctl.force_reset || (st & UC_RESET_BIT);
    o[2] = bsx_chain_time_fraction<PACK>(resets ? 0 : t + 1, a.L, sink);   // :64 — of the state AFTER the increment (:69)
    if (resets) {                                               // :87-92
      t = 0;
      need = (int)bsx_bern(&d);
      has = (int)bsx_bern(&d);
      observe<PACK, MT>(a, o, t, need, has, &d, sink);
      bsx_draws_end<MT>(&d, a.ctl, i);
      a.state[i] = t | (need << 20) | (has << 21);
      return BSX_FIRST;
    }
    t += 1;                                                     // :69
    if (t == 1) has = (act == 1);   // :71-72 (action_spec: {0,1})
    int type;
    if (t == a.L) {                                             // :74-81
      if (has == need) reward = 1.0;
      else { reward = -1.0; a.info[i] += 2.0; }
      observe<PACK, MT>(a, o, t, need, has, &d, sink);
      type = BSX_LAST;
    } else {                                                    // :83-85
      reward = 2.0 * (double)bsx_bern(&d) - 1.0;
      observe<PACK, MT>(a, o, t, need, has, &d, sink);
      type = BSX_MID;
    }
    bsx_draws_end<MT>(&d, a.ctl, i);
    a.state[i] = t | (need << 20) | (has << 21) | (type == BSX_LAST ? UC_RESET_BIT : 0);
    return type;
  }
};

#endif  // BSX_UMBRELLA_CHAIN_ENV_H_
