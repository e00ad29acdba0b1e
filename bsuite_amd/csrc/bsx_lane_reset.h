// bsx_lane_reset.h — the per-word arithmetic of a per-lane reset mark (bsx_lane_reset_mark, misc.hip).  Plain C99 +
// BSX_HD so that the CPU tests compile the very same code with gcc (tests/csrc/lane_reset_shim.c): a wrong bit here
// is a lane that silently keeps its episode, or regret that silently disappears.
//
// Every family's reset test is `force_reset || (word & <FAM>_RESET_BIT)`, so a lane whose bit is set takes exactly the
// path of an explicit reset() at its next call.  What the forced branch does BEYOND taking that path is done here:
// cartpole (classic) and mountain_car keep the running episode's return in the step counter of the word and fold it into
// the raw_return column only when an episode ends; a forced reset in mid-episode folds the k rewards the abandoned
// episode has paid (cartpole_env::core, mountain_car_env::core), and so does the mark.  A word whose bit
// is already set (after LAST, fresh, marked before) is returned as it is: nothing is folded twice.
#ifndef BSX_LANE_RESET_H_
#define BSX_LANE_RESET_H_

#include <stdint.h>

#include "../../include/bsuite_amd.h"   // BSX_FAM_*
#include "../../include/bsx_stream.h"   // BSX_HD

// The reset-next bit of the family's state word (the `steps` column of cartpole / mountain_car, the packed `state`
// column of every other family); 0 = bandit, whose whole word is the flag; -1 = no such family.  The same numbers as
// DS_RESET_BIT, CATCH_RESET_BIT, MC_RESET_BIT, UC_RESET_BIT, DC_RESET_BIT, CP_RESET_BIT, MN_RESET_BIT (misc.hip
// holds them together with static_asserts).
BSX_HD int32_t bsx_lane_reset_bit(int32_t family) {
  switch (family) {
    case BSX_FAM_DEEP_SEA: return 1 << 17;            // bit 18, the call-parity tag, stays as it is
    case BSX_FAM_CATCH: return 1 << 24;               // bits 25..31, the pending misses, stay as they are
    case BSX_FAM_BANDIT: return 0;
    case BSX_FAM_MEMORY_CHAIN: return 1 << 28;
    case BSX_FAM_UMBRELLA_CHAIN: return 1 << 22;
    case BSX_FAM_DISCOUNTING_CHAIN: return 1 << 12;
    case BSX_FAM_CARTPOLE: return 1 << 30;
    case BSX_FAM_MOUNTAIN_CAR: return 1 << 30;
    case BSX_FAM_MNIST: return 1 << 28;
    default: return -1;
  }
}

// Does a mark of this family fold something into info column 0?  `folded`: the columns are maintained per episode (no
// call->logging), the `folded` of bsx_bsuite_info.  Swing-up (variant 1) accumulates per step: nothing is pending.
BSX_HD int bsx_lane_reset_folds(int32_t family, int32_t variant, int32_t folded) {
  return folded != 0 && ((family == BSX_FAM_CARTPOLE && variant == 0) || family == BSX_FAM_MOUNTAIN_CAR);
}

// word -> the word of a lane marked for reset; *info_delta = what to add to info column 0 (0.0: leave the column alone).
BSX_HD int32_t bsx_lane_reset_word(int32_t word, int32_t family, int32_t variant, int32_t folded, double* info_delta) {
  *info_delta = 0.0;
  const int32_t bit = bsx_lane_reset_bit(family);
  if (bit == 0) return word != 0 ? word : 1;          // bandit: any non-zero word resets
  if (bit < 0 || (word & bit) != 0) return word;
  if (bsx_lane_reset_folds(family, variant, folded)) {
    const double k = (double)(word & 0x3FFFFFFF);     // rewards of +1 (cartpole) / -1 (mountain_car) paid so far
    *info_delta = family == BSX_FAM_CARTPOLE ? k : -k;
  }
  return word | bit;
}

#endif  // BSX_LANE_RESET_H_
