// deep_sea_hint.h — the hint word of the one-launch eager deep_sea step (bsx_deep_sea_step_hinted: the hint mode of deep_sea_step1_kernel, deep_sea.hip).
// Plain C99 + BSX_HD, like bsx_index.h: the CPU tests compile the very same code with gcc
// (tests/test_deep_sea_hint_math.py).
//
// Deterministic deep_sea has two outcomes per lane and call, and which one occurs is `action == mapping[row, col]`
// (deep_sea.py:118).  The lane advance of call t-1 therefore leaves, per lane, the hot cell of BOTH boards call t can
// show in one 32-bit word, and the observation stream of call t reads that word and the action and selects — it needs
// nothing the lane advance of call t produces.
//   bits  0..12  R = 1 + hot cell of the next board if the lane moves right (action == M)
//   bits 13..25  L = the same if it moves left
//   bit  26      M = the mapping bit of the lane's current cell
// A field is 0 for the all-zero board (the next row is N: the terminal observation, deep_sea.py:105-107); a lane that
// resets on its next call shows cell 0 whatever the action: R = L = 1.  13 bits hold BSX_DEEP_SEA_MAX_SIZE^2 + 1 values.
#ifndef BSX_DEEP_SEA_HINT_H_
#define BSX_DEEP_SEA_HINT_H_

#include <stdint.h>

#include "../../include/bsuite_amd.h"   // BSX_DEEP_SEA_MAX_SIZE
#include "../../include/bsx_stream.h"   // BSX_HD

#define DS_HINT_FIELD_BITS 13
#define DS_HINT_FIELD_MASK ((1u << DS_HINT_FIELD_BITS) - 1u)
#define DS_HINT_L_SHIFT DS_HINT_FIELD_BITS
#define DS_HINT_M_SHIFT (2 * DS_HINT_FIELD_BITS)

#if BSX_DEEP_SEA_MAX_SIZE * BSX_DEEP_SEA_MAX_SIZE + 1 > (1 << DS_HINT_FIELD_BITS)
#error "a hint field must hold every hot cell + 1"
#endif

// The hint of a lane at (row, col) — the fields of its packed state word — for its NEXT call.  `reset_pending`: the word's
// reset bit (the lane is fresh or its episode has ended).  mapping_bits: bit row * N + col of the action mapping.
BSX_HD uint32_t ds_hint_pack(int row, int col, int reset_pending, int N, const uint32_t* mapping_bits) {
  if (reset_pending) return 1u | (1u << DS_HINT_L_SHIFT);                // deep_sea.py:110-114: row = col = 0
  if ((unsigned)row >= (unsigned)N || (unsigned)col >= (unsigned)N) return 0u;   // (no word the library writes)
  const int cell = row * N + col;
  const uint32_t m = (mapping_bits[cell >> 5] >> (cell & 31)) & 1u;
  uint32_t r = 0u, l = 0u;
  if (row + 1 < N) {                                                      // :137-143: row N is the all-zero board
    const int base = (row + 1) * N + 1;
    r = (uint32_t)(base + (col + 1 > N - 1 ? N - 1 : col + 1));           // :129-132
    l = (uint32_t)(base + (col - 1 < 0 ? 0 : col - 1));                   // :133-136
  }
  return r | (l << DS_HINT_L_SHIFT) | (m << DS_HINT_M_SHIFT);
}

// The hot cell of the board the lane shows after acting `action` — any int32: only the mapping bit itself moves the
// lane right (deep_sea_fam::advance, `right = (act == mapped)`) — or -1 for the all-zero board.
BSX_HD int ds_hint_hot(uint32_t hint, int32_t action) {
  const int32_t m = (int32_t)((hint >> DS_HINT_M_SHIFT) & 1u);
  const uint32_t f = action == m ? hint : hint >> DS_HINT_L_SHIFT;
  return (int)(f & DS_HINT_FIELD_MASK) - 1;
}

#endif  // BSX_DEEP_SEA_HINT_H_
