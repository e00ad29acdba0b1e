// small_obs.h — the kernel skeleton of the families whose observation is a short row (1..256 floats per lane).  The
// families themselves are one header each:
//   bandit_env.h             bsuite/environments/bandit.py:54-64
//   memory_chain_env.h       bsuite/environments/memory_chain.py:60-97
//   umbrella_chain_env.h     bsuite/environments/umbrella_chain.py:60-92
//   discounting_chain_env.h  bsuite/environments/discounting_chain.py:63-88
//   cartpole_env.h           bsuite/environments/cartpole.py:37-177,
//                            bsuite/experiments/cartpole_swingup/cartpole_swingup.py:81-150
//   mountain_car_env.h       bsuite/environments/mountain_car.py:62-90
// each with the auto-reset of bsuite/environments/base.py:54-65.
//
// What a family `Env` provides to the skeleton (everything static):
//   ALWAYS
//     HAS_REGS, PACKED          which of the two groups below apply
//     struct args               the kernel argument: bsx_ctl ctl, const int32_t* action, bsx_timestep_t out, int32_t obs_numel,
//                               then the family's columns and parameters
//     step<LOG, MT>(a, i, oi, lane, step, o, reward) -> step type
//                               one reset() / step() of lane i against its columns in memory: reads action[oi], writes the
//                               row into o[] (<= 8 floats) and the f64 reward; PACKED: step<LOG, MT, true>(..., &sink) leaves
//                               HEAD floats in o[] and the rest of the row as bits in the sink
//   HAS_REGS — the lane's state fits in registers: fused rollouts (small_obs_regs_rollout) and the lean eager step with
//   several lanes per thread (small_obs_eager2_kernel) hold it there; small_regs_defaults has the no-op members
//     struct regs; clear(r); load(a, i, r); store(a, i, r)          the state, zeroed / from / to its columns
//     reset_pending(r)          does the lane begin an episode at its next step?
//     core<LOG, MT, IREGS, TAB, POOL, V, NOFORCE>(a, r, act, i, lane, step, o, reward, s_tab, s_pool) -> step type
//                               step() on the registers: the same transitions, draws and info updates
//     load_info<V> / store_info<V>(a, i, r)                          the bsuite_info columns that core<IREGS = true> keeps in r
//     N_VARIANTS, numel_of(v), variant_of(a)                         compile-time variants of the lean rollout (row length), -1 = none fits
//     TABLE_MAX_BYTES, table_fits(a), table_bytes(a), stage_tables(a, s_dyn)   a table the rollout stages in LDS (0 = none)
//     POOLED_RESETS, wants_reset<NOFORCE>(a, r), reset_part(a, lane, step, part, owner, pool)
//                               big launches: a lane's reset draws computed by the workgroup's pool, two parts per lane
//     ROWS_VIA_LDS              big launches: a wave's rows leave as 16-byte chunks through LDS (small_obs_store_rows_wave)
//     EAGER_LPT_MIN_BLOCKS, EAGER_LPT                                lean eager step: lanes per thread, and from how many workgroups up
//   PACKED — the row length is a parameter and the row is HEAD floats followed by values that one or two bits encode
//     rows_t                    the row format of row_stream.h (memory_rows, umbrella_rows); HEAD, PLANES from it
//     decode(bit0, bit1)        the float that a tile element's plane bits stand for
//     tf_table_fits(a)          do the time fractions 1 - t / L fit the tile's LDS table?
//     args: L, numel_magic (bsx_div_magic(obs_numel)), rows, row_plane_words (the call's row scratch: chain_rows.h)
//
// One kernel shape for all of them: thread t advances lane (block*256 + t) from coalesced SoA column
// loads and either stores its short observation row itself or — the wide rows of memory_chain /
// umbrella_chain — leaves it as bits in an LDS tile that the whole block streams to HBM as consecutive
// 16-byte chunks (small_obs_body, below).  Physics state is f32 on the device (the reference holds
// Python floats); rewards and the time-fraction observation are formed in f64 exactly as the reference
// forms them and cast once.
#ifndef BSX_SMALL_OBS_H_
#define BSX_SMALL_OBS_H_

#include "bsx_host.h"
#include "pair_mixed.h"
#include "row_stream.h"

// n_steps == 1 is env.step()/reset(); n_steps = T > 1 is the fused rollout: the same thread advances
// its lane T times inside one launch (actions [T,B], outputs [T,B,...]); per-lane state columns are
// re-read from L2 by the thread that wrote them, so HBM sees only the action/TimeStep streams —
// the tiny families are otherwise bound by one ~8 us launch per step.
// LOG / NOISE / MT: -1 = decide at run time, 0 = compiled out, 1 = always on.  The common call (no
// Logging wrapper, no RewardNoise, counter-based draws) runs the <0,0,0> instantiation: without the
// MT19937 twist, the f64 normal transform and the row snapshots the kernel is a fifth of the size.
//
// Two ways for a row to reach HBM:
//   DIRECT  rows of 1, 3 or an even number <= 8 floats: the thread that advances a lane stores its row
//           itself — no LDS, no barrier.  Every family with a fixed short row (bandit, discounting_chain,
//           cartpole, mountain_car) always takes it.
//   PACKED  the families whose row length is a parameter (memory_chain: nb+2, umbrella_chain: 3+nd, up to
//           256 floats) and whose row is a few floats (HEAD) followed by values that one or two BITS
//           encode.  The block keeps the tile [256 x numel] as flat bit planes in LDS — bit (l*numel + j) of
//           a plane belongs to element j of lane l — which each lane ORs its bits into; after a barrier
//           the block streams the tile to HBM as consecutive 16-byte chunks: chunk c is the nibble at bit
//           4c of each plane, four v_bfe/v_cvt away from a float4 (a lane-per-row store would be a
//           stride-(4*numel) scatter; an f32 tile costs 32x the LDS — up to 32 KiB per workgroup, which
//           capped the resident workgroups per CU — and per-element records cost ~80 VALU instructions
//           per chunk: profiles/r02/ab_packed_records_v*.log).  The HEAD floats stay in the lane's
//           registers and overwrite their (zero) places in the tile after a second barrier.
//           LDS per workgroup: 32*numel bytes per plane (<= 8 KiB).
//   ROWS    the same wide rows when the call brings a scratch (bsx_call_t.row_scratch, ABI v12) and is a single step:
//           every WAVE builds its 64 lanes' flat bit planes in wave-private LDS — no workgroup barrier — and stores
//           them into the scratch; a store stream decodes them into the observation array in a second launch
//           (row_stream.h).
// A lane's handle on the tile's bit planes.
struct bsx_bit_sink {
  uint32_t* planes;        // LDS: PLANES x `stride` words
  int stride;              // words per plane = 8 * numel
  uint32_t base;           // flat bit index of the lane's element HEAD
  const float* tf = nullptr;  // LDS: the family's time fractions 1 - t / L for t = 0..L (small_obs_body, PACKED), or null
  // ORs bits [32k, 32k+n) of the lane's bit string (n in 1..32, the low n bits of w) into plane p
  __device__ __forceinline__ void put(int p, int k, uint32_t w, int n) const {
    uint32_t word, lo, hi;
    int has_hi;
    bsx_plane_split(base + 32u * (uint32_t)k, w, n, &word, &lo, &hi, &has_hi);
    uint32_t* dst = planes + p * stride + word;
    atomicOr(dst, lo);
    if (has_hi) atomicOr(dst + 1, hi);
  }
};

// A table staged in LDS, typed as such: a generic pointer would make every read a FLAT load, which counts in vmcnt
// AND lgkmcnt and drags a full `s_waitcnt vmcnt(0)` (a drain of the wave's stores) in front of its first use.
typedef const float __attribute__((address_space(3)))* bsx_lds_table;

// Reset values of a workgroup's lanes, computed by a few threads on behalf of their owners (small_obs_regs_rollout).
struct bsx_reset_pool {
  float vals[6][BSX_BLOCK];          // [value][owner thread]
  unsigned short list[BSX_BLOCK];    // the threads whose lane begins an episode at this step, in arrival order
  unsigned int n[2];                 // how many; [step parity]
};

// The cache policy of the OUTPUT stores (bsx_st<POLICY>: bsx_device.h; round 6).  What a step or a rollout writes —
// TimeStep columns and observation rows — is never read again by the engine, while what it READS (actions a run ahead, state
// and info columns, tables) is what the stores evict: the fused rollouts were bound by exactly those reads (r04: 6.5 us with,
// 4.8 without the action loads).  A FUSED ROLLOUT's outputs are NON-TEMPORAL wherever a wave's store instruction covers one
// contiguous range: mountain_car r16 6.45 -> 4.45-4.7 us per step, memory_len r16 7.0 -> 5.2, discounting_chain r16 5.2 ->
// 3.8, bandit r16 5.0 -> 4.0, cartpole r16 9.8 -> 7.7 (its rows leave as 16-byte chunks through the wave's LDS), umbrella_length
// r16 23.8 -> 21.4 (profiles/r06/ab_small_families_nt*.log, ab_nt_wide_rows_and_small_batches.log).  An EAGER step's outputs are
// WRITE-THROUGH: non-temporal ones make the step itself faster still (umbrella_length 25.8 -> 21.7 us, mountain_car 8.2 -> 7.3)
// but cost the agent that reads the observation next more than that (ab_nt_outputs_closed_loop_policy.log); write-through:
// cartpole 17.7 -> 15.8 us, discounting_chain 7.05 -> 6.05, memory_len 10.0 -> 9.25, bandit 8.46 -> 7.96, the closed loop equal or
// faster everywhere (ab_eager_output_policy.log).  NEITHER for rows written as 8-byte pieces at the row stride (cartpole
// row-per-lane: 18 -> 25 us non-temporal — partial lines want the L2 to merge them).  deep_sea / catch / mnist / the sweep are
// not touched by this (ab_small_nt_other_paths.log).  The policy of each kind of output, in a fused rollout and in an eager step:
// (struct bsx_out_policy, bsx_policy, BSX_OUT_SCALARS — the reward / discount / step_type columns: bsx_device.h; BSX_OUT_INDEX: bsx_pair_device.h)
constexpr bsx_out_policy BSX_OUT_ROW12 = {BSX_ST_NT, BSX_ST_WT};          // rows of one or two floats stored by their own thread
constexpr bsx_out_policy BSX_OUT_STAGED = {BSX_ST_NT, BSX_ST_WT};         // rows staged through a wave's LDS, stored as 16-byte chunks
constexpr bsx_out_policy BSX_OUT_PARTIAL = {BSX_ST_PLAIN, BSX_ST_PLAIN};  // rows of 4 / 6 / 8 floats stored by their own thread as
                                                                          // 8-byte pieces at the row stride (partial lines)
constexpr bsx_out_policy BSX_OUT_ROW3 = {BSX_ST_NT, BSX_ST_WT};           // rows of three floats (one 12-byte store per lane)
constexpr bsx_out_policy BSX_OUT_TILE = {BSX_ST_NT, BSX_ST_WT};           // the 16-byte chunks of the wide rows' bit-plane tiles
// Per family: does the fused rollout store reward / discount / step_type non-temporal?
template <class Env> struct small_rollout_nt_scalars { static constexpr bool value = true; };

// A lane's own thread stores its short row (<= 8 floats).  A wave's 64 rows are one contiguous range, written by
// back-to-back instructions that the L2 merges line by line.
template <bool ROLLOUT_ST>
__device__ __forceinline__ void small_obs_store_row(float* __restrict__ dst, const float* o, int numel) {
  constexpr int P12 = bsx_policy(BSX_OUT_ROW12, ROLLOUT_ST), P3 = bsx_policy(BSX_OUT_ROW3, ROLLOUT_ST);
  constexpr int PP = bsx_policy(BSX_OUT_PARTIAL, ROLLOUT_ST);
  if ((numel & 1) == 0) {
    bsx_f2* __restrict__ d2 = reinterpret_cast<bsx_f2*>(dst);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (2 * k < numel) {
        bsx_f2 v; v.x = o[2 * k]; v.y = o[2 * k + 1];
        if (numel == 2) bsx_st<P12>(&d2[k], v);
        else bsx_st<PP>(&d2[k], v);
      }
  } else if (numel == 3) {
    // one 12-byte store per lane (global_store_dwordx3): a wave's 64 rows are 768 contiguous bytes.  (The non-temporal builtin
    // takes a 3-float vector, not a struct; bsx_st's write-through store is sized by sizeof, which is 16 for that vector.)
    if constexpr (P3 == BSX_ST_NT) {
      typedef float row3v __attribute__((ext_vector_type(3), aligned(4)));
      row3v v; v.x = o[0]; v.y = o[1]; v.z = o[2];
      __builtin_nontemporal_store(v, reinterpret_cast<row3v*>(dst));
    } else {
      struct __attribute__((packed, aligned(4))) row3 { float a, b, c; };
      row3 v; v.a = o[0]; v.b = o[1]; v.c = o[2];
      bsx_st<P3>(reinterpret_cast<row3*>(dst), v);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 7; ++k)                                   // numel == 1, 5, 7: 4-byte stores
      if (k < numel) {
        if (numel == 1) bsx_st<P12>(&dst[k], o[k]);
        else dst[k] = o[k];
      }
  }
}

// An element `off` BYTES (32 bits, per lane) behind a wave-uniform base: the address add is the memory instruction's
// (global_store ... v_off, v_data, s[base:base+1]), not three or four 64-bit VALU instructions per access.
// The pointer is typed as GLOBAL memory (address_space(1)): the slab pointers pass through an opaque asm statement
// every step (see the loop), after which the compiler no longer knows where a generic pointer leads and would emit
// FLAT accesses — which count in vmcnt AND lgkmcnt and have no scalar-base form.
#if defined(__HIP_DEVICE_COMPILE__)
#define BSX_GLOBAL __attribute__((address_space(1)))
#else
#define BSX_GLOBAL              /* (the host pass only parses the device functions) */
#endif
template <class T>
__device__ __forceinline__ BSX_GLOBAL T* bsx_at_off(T* base, uint32_t off) {
  return (BSX_GLOBAL T*)((BSX_GLOBAL char*)base + off);
}
template <class T>
__device__ __forceinline__ const BSX_GLOBAL T* bsx_at_off(const T* base, uint32_t off) {
  return (const BSX_GLOBAL T*)((const BSX_GLOBAL char*)base + off);
}

// The 64 rows of a full wave, through a wave-private LDS staging area, as 16-byte chunks: row-per-lane stores of a
// 24-byte row are 8-byte pieces at stride 24 — every store instruction touches all of the wave's 64-byte segments with
// a third of their bytes, three write requests per segment where one would do, and the fused rollouts of the physics
// families turned out to be bound by exactly that (profiles/r03/exp_store_ablation.log: without the row stores
// cartpole's step takes 8.1 us instead of 13.3).  No workgroup barrier: LDS serves a wave's accesses in order.
// chunk(c) = the address of the wave's 16-byte chunk c (its first row 16-byte aligned: the caller checks), s_wave = 64 * 8
// floats, wl = lane in the wave.
template <bool ROLLOUT_ST, class Chunk>
__device__ __forceinline__ void small_obs_store_rows_wave(Chunk chunk, const float* o, int numel, float* s_wave, int wl) {
  float* mine = s_wave + wl * numel;
  if ((numel & 1) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (2 * k < numel) *reinterpret_cast<float2*>(mine + 2 * k) = make_float2(o[2 * k], o[2 * k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (k < numel) mine[k] = o[k];
  }
  bsx_wave_sync();
  const int chunks = 16 * numel;                                 // 64 rows x numel floats / 4
  for (int c = wl; c < chunks; c += 64)
    bsx_st<bsx_policy(BSX_OUT_STAGED, ROLLOUT_ST)>(chunk(c), reinterpret_cast<const bsx_f4*>(s_wave)[c]);
  __builtin_amdgcn_wave_barrier();                               // (the next step's rows are written after these reads)
}

// The same value, opaque to the optimiser: what is computed from it stays where it is written (no hoisting out of loops).
__device__ __forceinline__ uint32_t bsx_fresh(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Fused T-step rollout of a family whose lane state fits in registers (cartpole, swing-up, mountain_car): ONE launch,
// and nothing inside the step loop ever waits for memory —
//  * the state AND the bsuite_info accumulators of the lane live in registers for the T steps (without the Logging
//    wrapper, whose rows snapshot the columns): the episode-end read-modify-writes were `s_waitcnt vmcnt(0)` in the
//    loop, i.e. a drain of every store the wave had in flight, on 6 steps in 10 (some lane of 64 ends an episode);
//  * actions are loaded RUN steps at a time, ahead of the run: on gfx9 stores count in vmcnt too, so waiting for a
//    one-step-ahead prefetch issued before a divergent number of stores also meant vmcnt(0) — once per step;
//  * cartpole's time-fraction table sits in LDS (lgkmcnt) when it fits.
// r02 (prefetch + in-loop RMW): 70 % of the wave cycles were waits, cartpole 15.1 us per step at 53 % VALU-busy
// (profiles/r03/cartpole_rollout16_before_pmc_sq.json).
// V: the family's variant as a compile-time constant (Env::numel_of(V) floats per row, cartpole: 0 classic / 1 swing-up),
// or -1 = read obs_numel / the flags from the arguments.  With the row length a run-time value every `2*k < numel` of
// the row store became a loop-invariant 64-bit condition mask of its own: 119 SGPR spills and ~90 v_readlane reloads
// in each copy of the step loop (r03 build; profiles/r04/cartpole_rollout_loop_isa_before.txt).
// V >= 0 also promises (launch_regs_rollout) that a [B, numel] slab is shorter than 4 GiB: every output of step t is
// then addressed as {uniform slab pointer, advanced once per step on the scalar unit} + {the lane's 32-bit byte offset,
// loop-invariant}, and no 64-bit index t*B + i is formed per step and array.
template <class Env, int LOG, int NOISE, int MT, bool TAB, bool BIG, int V = -1>
__device__ __forceinline__ void small_obs_regs_rollout(const typename Env::args& a, const int n_steps, const uint32_t block_id,
                                                       float* s_dyn, unsigned int* s_cnt, bsx_reset_pool* s_pool, float* s_rows) {
  constexpr bool IREGS = LOG == 0;
  // BIG: the launch fills the chip several times over (launch_small_obs) — the loop is then bound by throughput (vector
  // instructions, write requests) and pools the resets / stages the rows; a small launch is bound by the latency of a
  // wave's own step, to which the pool's two barriers and the LDS round trip only add (2^17 lanes: cartpole 2.1 -> 2.5 us
  // per step, profiles/r03/ab_rows_small_batches.log).
  constexpr bool POOL = BIG && Env::POOLED_RESETS && MT == 0;
  constexpr bool ROWS = BIG && Env::ROWS_VIA_LDS;
  constexpr bool OFF32 = V >= 0;
  constexpr int RUN = 8;                // (16: no drain inside a T=16 launch at all, and 3-7 % slower — profiles/r03/ab_rollout_run16.log)
  if (threadIdx.x < 2) {
    s_cnt[threadIdx.x] = 0;
    if constexpr (POOL) s_pool->n[threadIdx.x] = 0;
  }
  // TAB: the family's table is staged in LDS (a compile-time fact inside the loop: were the source of a value
  // decided at run time, the compiler would wait for the global load it MIGHT have been — vmcnt — at every use)
  bsx_lds_table s_tab = (bsx_lds_table)0;
  if constexpr (TAB) s_tab = Env::stage_tables(a, s_dyn);
  __syncthreads();
  const int numel = V >= 0 ? Env::numel_of(V) : a.obs_numel;
  constexpr bool F64 = !(LOG == 0 && NOISE == 0 && MT == 0);       // bsx_ctl_lean: no f64 reward copy
  const int64_t B = a.ctl.n_lanes;
  const int64_t i = (int64_t)block_id * BSX_BLOCK + threadIdx.x;
  const uint32_t iu0 = (uint32_t)i;
  // (Tried: BIG variants for whole workgroups only, i.e. no `mine` mask in the loop — fewer scalar registers, but the
  // scheduler then interleaves across the former block boundary: 65 -> 71 VGPRs for cartpole, 68 -> 85 for swing-up.)
  const bool mine = i < B;
  const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;
  const uint64_t step0 = bsx_step_of(a.ctl);
  // rows leave through the wave's LDS staging area when every row of the wave exists and every step's block of rows
  // starts on a 16-byte boundary (wave-uniform)
  const int wl = (int)(threadIdx.x & 63u);
  const bool rows_via_lds = ROWS && (((int64_t)B * numel) & 3) == 0 && (i - wl + 64) <= B;
  // LAST lanes are counted per thread and pooled once per launch (the per-step wave ballots + LDS atomics of
  // bsx_count_types were ~12 instructions and two LDS round trips of every wave-step); FIRST steps follow from them:
  // every LAST is followed by a FIRST except one at the launch's final step, and a lane that arrives with its reset
  // pending begins with one (no force_reset inside a rollout).
  uint32_t n_last = 0;
  typename Env::regs rg;
  Env::clear(rg);
  if (mine) {
    Env::load(a, i, rg);
    if constexpr (IREGS) Env::template load_info<V>(a, i, rg);
  }
  const uint32_t pending_in = Env::reset_pending(rg) ? 1u : 0u;
  // the slabs of the step under way (OFF32): [B] reward / discount / step_type, [B, numel] observation, [B] action
  float* rp = a.out.reward;
  float* dp = a.out.discount;
  int8_t* sp = a.out.step_type;
  float* op = a.out.observation;
  const int32_t* ap = a.action;
  // (Tried, profiles/r04/ab_rollout_action_prepack.log: a pre-pass that leaves action[t, i] as a BYTE in step_type[t, i] —
  // the slot this loop overwrites after reading it — so that the loop reads 1 byte per lane-step from an array one
  // read-dominated pass has just produced.  The loop does not get faster by what the pre-pass costs: cartpole 9.9-10.2 ->
  // 10.9-11.0 us per step, mountain_car 5.9-6.5 -> 5.8-6.1 at 2^20 lanes but 2.64 -> 2.93 at 2^19 and 5.5 -> 6.2 at
  // T = 64.  Not adopted.
  // Nor did removing the per-run drain: the next run's actions loaded by inline asm at the START of the current run
  // (invisible to the compiler's wait insertion) and awaited at its end with `s_waitcnt vmcnt(8 x stores per step)`,
  // which the loads alone satisfy — correct (rollout tests), mountain_car r16 6.5-6.65 -> 6.25-6.4 us, nothing at
  // T = 32 / 64, cartpole +-1 % at the price of its eighth wave (profiles/r04/ab_rollout_prefetched_runs.log).  The loop
  // is 26-36 % faster without its action loads (exp_action_load_ablation.log) — and so is the bare access pattern
  // (tools/micro/step_stores.hip, same box: 3.95 us without loads, 5.04 in runs of eight, 4.64 with all rows loaded
  // before the first store = the loads' own 0.69 us added; prefetched a run ahead 5.70): reads among a saturating
  // stream of per-lane stores cost at least their own time, in any arrangement.)
#pragma unroll 1
  for (int t0 = 0; t0 < n_steps; t0 += RUN) {
    const int run = n_steps - t0 < RUN ? n_steps - t0 : RUN;             // uniform
    // The run's actions: eight registers for eight 2-bit values were what stood between the pooled cartpole loop and
    // 64 VGPRs (8 waves per SIMD), and picking act[j] cost 7 selects per step.  OFF32 packs them, 4 bits each, into
    // ONE register (unpacked by one v_bfe_u32 with a scalar shift).  Any int32 is a legal action of these families
    // (the reference computes (action - 1) * force with whatever it gets, cartpole.py:48): a run in which some lane
    // of the wave holds an action outside 0..15 re-reads its actions from memory step by step instead (wave-uniform
    // branch; the wait it needs drains the wave's stores — slow, exact, and never taken by in-spec actions).
    int acts[OFF32 ? 1 : RUN];
    uint32_t packed = 0;
    bool wide = false;
    const int32_t* const ap_run = ap;
    if constexpr (OFF32) {
      if (mine) {
        // (rows beyond the run re-read its last row: no per-row condition, no table of row strides in scalar registers)
        const uint32_t off = bsx_fresh(iu0) * 4u;
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
          const uint32_t aj = (uint32_t)*bsx_at_off(ap, off);
          packed |= (aj & 15u) << (4 * j);
          wide |= aj > 15u;
          if (j + 1 < run) ap += B;                                      // uniform
        }
        ap += B;
      }
    } else {
#pragma unroll
      for (int j = 0; j < RUN; ++j) acts[j] = (mine && j < run) ? a.action[(int64_t)(t0 + j) * B + i] : 0;
    }
    // (one scalar pair says both whether and where: the start of the run's actions, or null)
    const int32_t* const ap_wide = (OFF32 && __ballot(wide) != 0ull) ? ap_run : nullptr;     // uniform
    // Everything loaded so far has landed before the run starts (vmcnt(0) lgkmcnt(0)): the compiler's wait insertion
    // then knows that no register is waiting for memory inside the run — otherwise every first use of a
    // conditionally loaded value (the swing-up info columns) gets its own vmcnt(0), and on gfx9 that is a drain of
    // the STORES in flight as well.  One drain per RUN steps instead of several per step.
    __builtin_amdgcn_s_waitcnt(0x0070);
    // (a ROLLED loop: unrolled, the scheduler interleaves the steps and the kernel needs 140 VGPRs instead of ~75 —
    // half the waves per SIMD, no gain, profiles/r03/ab_regs_rollout.log; the run's action is picked by selects)
#pragma unroll 1
    for (int j = 0; j < run; ++j) {
      const int t = t0 + j;
      int type = -1;
      int act;
      if constexpr (OFF32) {
        act = (int)((packed >> (4 * j)) & 15u);
        if (ap_wide != nullptr) {
          act = mine ? *bsx_at_off(ap_wide + (int64_t)j * B, bsx_fresh(iu0) * 4u) : 0;
          __builtin_amdgcn_s_waitcnt(0x0070);                            // landed: nothing pends beyond this block
        }
      } else {
        act = acts[0];
#pragma unroll
        for (int q = 1; q < RUN; ++q) act = j == q ? acts[q] : act;
      }
      if constexpr (POOL) {
        // The lanes that begin an episode at this step hand the draws of their reset to a pool: some lane of a
        // wave does on 4 steps in 10 (cartpole, random actions), and then the whole wave walks through two Philox
        // blocks and four f64 uniforms for its sake — ~230 vector instructions beside the step's ~150.  Pooled, ONE
        // wave of the workgroup computes all of them in one pass, two threads per lane (a Philox block each), and
        // the waves take turns at it step by step so that the work lands on every SIMD: 306 -> ~215 vector
        // instructions per wave and step, 77 -> 63 VGPRs (profiles/r03/ab_pooled_resets.log).
        const int par = t & 1;
        if (mine && Env::template wants_reset<true>(a, rg)) {
          const unsigned slot = atomicAdd(&s_pool->n[par], 1u);
          s_pool->list[slot] = (unsigned short)threadIdx.x;
        }
        __syncthreads();
        const unsigned n2 = 2u * s_pool->n[par];
        if (threadIdx.x == 0) s_pool->n[par ^ 1] = 0;
        for (unsigned h = (threadIdx.x + 64u * ((unsigned)t + block_id)) & (BSX_BLOCK - 1u); h < n2; h += BSX_BLOCK) {
          const unsigned e = s_pool->list[h >> 1];
          Env::reset_part(a, a.ctl.lane_offset + (uint64_t)block_id * BSX_BLOCK + e, step0 + (uint64_t)t, (int)(h & 1u), e, s_pool);
        }
        __syncthreads();
      }
      if (mine) {
        // (the lane's byte offsets are formed HERE, from a value the compiler cannot trace to the loop's outside: hoisted
        // out of the loop they are four more live registers, and — zero-extended in another basic block — they no longer
        // match the {scalar base + 32-bit vector offset} addressing mode, so every access paid a 64-bit add again)
        const uint32_t iu = bsx_fresh(iu0);
        const int64_t oi = (int64_t)t * B + i;                           // (dead in the lean instantiations)
        double reward = 0.0;
        float o[8];
        type = Env::template core<LOG, MT, IREGS, TAB, POOL, V, true>(a, rg, act, i, lane, step0 + (uint64_t)t, o, reward, s_tab, s_pool);
        if constexpr (OFF32) {
          float r, d;
          bsx_emit_values<LOG, NOISE, F64, MT>(a.ctl, i, oi, lane, step0 + (uint64_t)t, type, reward, r, d);
          constexpr int NTS = small_rollout_nt_scalars<Env>::value ? BSX_OUT_SCALARS.rollout : BSX_ST_PLAIN;
          bsx_st<NTS>(bsx_at_off(rp, iu * 4u), r);
          bsx_st<NTS>(bsx_at_off(dp, iu * 4u), d);
          bsx_st<NTS>(bsx_at_off(sp, iu), (int8_t)type);
          if (rows_via_lds) {
            const uint32_t wave_off = (iu - (uint32_t)wl) * (uint32_t)(numel * 4);   // byte offset of the wave's first row
            small_obs_store_rows_wave<true>([=](int c) { return bsx_at_off(reinterpret_cast<bsx_f4*>(op), wave_off + 16u * (uint32_t)c); },
                                            o, numel, s_rows + (threadIdx.x - wl) * 8, wl);
          } else {
            small_obs_store_row<true>(bsx_at_off(op, iu * (uint32_t)(numel * 4)), o, numel);
          }
        } else {
          bsx_emit_at<LOG, NOISE, F64, MT, BSX_OUT_SCALARS.rollout>(a.ctl, a.out, i, oi, lane, step0 + (uint64_t)t, type, reward);
          if (rows_via_lds) {
            bsx_f4* w4 = reinterpret_cast<bsx_f4*>(a.out.observation + (oi - wl) * (int64_t)numel);
            small_obs_store_rows_wave<true>([=](int c) { return w4 + c; }, o, numel, s_rows + (threadIdx.x - wl) * 8, wl);
          } else {
            small_obs_store_row<true>(a.out.observation + oi * (int64_t)numel, o, numel);
          }
        }
      }
      if constexpr (OFF32) {
        // (a slab is shorter than 4 GiB: 32-bit strides — three scalar registers instead of three pairs)
        const uint32_t b1 = (uint32_t)B;
        rp = (float*)((char*)rp + b1 * 4u); dp = (float*)((char*)dp + b1 * 4u); sp += b1;
        op = (float*)((char*)op + b1 * (uint32_t)(numel * 4));
      } else {
        rp += B; dp += B; sp += B; op += B * (int64_t)numel;              // uniform: the scalar unit's
      }
      if constexpr (OFF32) {
        // (opaque, or loop strength reduction folds the four pointers into ONE running offset t*B*4 and every address
        // becomes base + (offset + lane): not the {scalar base, vector offset} form any more)
        asm volatile("" : "+s"(rp), "+s"(dp), "+s"(sp), "+s"(op));
      }
      n_last += (type == BSX_LAST) ? 1u : 0u;
    }
  }
  const uint32_t n_first = n_last + pending_in - (Env::reset_pending(rg) ? 1u : 0u);
  if (mine) {
    Env::store(a, i, rg);
    if constexpr (IREGS) Env::template store_info<V>(a, i, rg);
  }
  // (bsx_pool_counts written out: through the helper, the assembly listings of cartpole, memory_chain and mountain_car
  // are no longer the same text — profiles/layout_split/README.md)
  if (a.ctl.counters != nullptr) {
    if (n_last) atomicAdd(&s_cnt[0], n_last);
    if (n_first) atomicAdd(&s_cnt[1], n_first);
  }
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, block_id);
}

// TABSEL: the register-resident families' table (cartpole's time fractions) is staged in LDS (1) or read from device
// memory (0) — the launcher knows; -1 = both loops in the kernel, chosen per launch by table_fits().
template <class Env, bool ROLLOUT, int LOG, int NOISE, int MT, bool DIRECT_ARG, bool BIG = false, int V = -1, int TABSEL = -1,
          bool ROWS_ARG = false>
__device__ __forceinline__ void small_obs_body(const typename Env::args& a, const int n_steps_arg,
                                               const uint32_t block_id, float* s_obs, unsigned int* s_cnt) {
  constexpr bool ROWS = ROWS_ARG && Env::PACKED && !ROLLOUT;         // wide rows, packed, into the call's row scratch
  constexpr bool DIRECT = DIRECT_ARG || !Env::PACKED;
  // (a family whose row length is a parameter — memory_chain — is register-resident in the rows its own thread stores)
  if constexpr (ROLLOUT && Env::HAS_REGS && (DIRECT_ARG || !Env::PACKED)) {
    bsx_reset_pool* pool = nullptr;
    float* rows = nullptr;
    if constexpr (BIG && Env::POOLED_RESETS && MT == 0) {
      __shared__ bsx_reset_pool s_pool;
      pool = &s_pool;
    }
    if constexpr (BIG && Env::ROWS_VIA_LDS) {
      __shared__ __attribute__((aligned(16))) float s_rows[BSX_BLOCK * 8];         // 64 rows of <= 8 floats per wave
      rows = s_rows;
    }
    if constexpr (TABSEL == 1) small_obs_regs_rollout<Env, LOG, NOISE, MT, true, BIG, V>(a, n_steps_arg, block_id, s_obs, s_cnt, pool, rows);
    else if constexpr (TABSEL == 0) small_obs_regs_rollout<Env, LOG, NOISE, MT, false, BIG, V>(a, n_steps_arg, block_id, s_obs, s_cnt, pool, rows);
    else if (Env::table_fits(a)) small_obs_regs_rollout<Env, LOG, NOISE, MT, true, BIG, V>(a, n_steps_arg, block_id, s_obs, s_cnt, pool, rows);   // uniform
    else small_obs_regs_rollout<Env, LOG, NOISE, MT, false, BIG, V>(a, n_steps_arg, block_id, s_obs, s_cnt, pool, rows);
    return;
  }
  constexpr bool F64 = !(LOG == 0 && NOISE == 0 && MT == 0);       // bsx_ctl_lean: no f64 reward copy
  const int n_steps = ROLLOUT ? n_steps_arg : 1;   // the single-step instantiation has no loop: keeping
                                                    // every kernarg live across iterations costs ~120 VGPRs
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int numel = a.obs_numel;
  const int64_t B = a.ctl.n_lanes;
  const int64_t lane0 = (int64_t)block_id * BSX_BLOCK;
  const int64_t remaining = B - lane0;
  const int lanes_here = remaining < BSX_BLOCK ? (int)remaining : BSX_BLOCK;
  const uint64_t step0 = bsx_step_of(a.ctl);
  const bool mine = (int)threadIdx.x < lanes_here;
  const int64_t i = lane0 + threadIdx.x;
  const uint64_t lane = a.ctl.lane_offset + (uint64_t)i;

#pragma unroll 1
  for (int t = 0; t < n_steps; ++t) {
    const int64_t oi = (int64_t)t * B + i;
    int type = -1;
    if constexpr (ROWS) {
      // Wide rows into the call's row scratch (bsx_rows.h) for the store stream of the next launch (row_stream.h): the
      // advance of the PACKED path below without its workgroup barriers.  Every WAVE keeps its own flat bit planes in
      // LDS — 64 lanes x numel bits = 2 * numel whole words per plane, LDS serves a wave's accesses in order — which
      // its lanes OR their bits into and which it then stores as consecutive words of the global planes; the row
      // elements that are genuine floats go to one f32 column each, the 0.0 / 1.0 HEAD elements of umbrella_chain (need,
      // has) are plane bits like the distractors.
      typedef typename Env::rows_t R;
      const int wl = (int)(threadIdx.x & 63u);
      const uint32_t wstride = 2u * (uint32_t)numel;                       // words per plane of one wave
      uint32_t* __restrict__ wplanes = reinterpret_cast<uint32_t*>(s_obs) + (threadIdx.x >> 6) * ((uint32_t)R::PLANES * wstride);
      for (uint32_t w = (uint32_t)wl; w < (uint32_t)R::PLANES * wstride; w += BSX_WAVE) wplanes[w] = 0u;
      bsx_wave_sync();
      if (mine) {
        double reward = 0.0;
        float o[Env::HEAD];
        const bsx_bit_sink sink{wplanes, (int)wstride, (uint32_t)(wl * numel + Env::HEAD)};
        type = Env::template step<LOG, MT, true>(a, i, oi, lane, step0 + (uint64_t)t, o, reward, &sink);
        bsx_emit_at<LOG, NOISE, F64, MT, bsx_policy(BSX_OUT_SCALARS, ROLLOUT)>(a.ctl, a.out, i, oi, lane, step0 + (uint64_t)t, type, reward);
        float* __restrict__ heads = reinterpret_cast<float*>(a.rows + (uint64_t)R::PLANES * (uint64_t)a.row_plane_words);
        uint32_t head_bits = 0u;
#pragma unroll
        for (int k = 0; k < Env::HEAD; ++k) {
          bool is_float = false;
#pragma unroll
          for (int q = 0; q < R::NF; ++q)
            if ((int)bsx_rows_fpos(R::KIND, q) == k) { heads[(int64_t)q * B + i] = o[k]; is_float = true; }
          if (!is_float) head_bits |= (o[k] != 0.0f ? 1u : 0u) << k;     // (0.0 / 1.0: decode(1) == 1.0f for such a family)
        }
        if (R::NF < Env::HEAD) {
          const bsx_bit_sink hs{wplanes, (int)wstride, (uint32_t)(wl * numel)};
          hs.put(0, 0, head_bits, Env::HEAD);
        }
      }
      bsx_count_types(a.ctl, type, s_cnt);
      bsx_wave_sync();
      const int64_t wave_lane0 = lane0 + (int64_t)(threadIdx.x & ~63u);
      if (wave_lane0 < B) {                                              // (uniform per wave)
        uint32_t* __restrict__ gp = a.rows + (uint64_t)(wave_lane0 >> 6) * wstride;
#pragma unroll
        for (int p = 0; p < R::PLANES; ++p)
          for (uint32_t w = (uint32_t)wl; w < wstride; w += BSX_WAVE) gp[(uint64_t)p * (uint64_t)a.row_plane_words + w] = wplanes[(uint32_t)p * wstride + w];
      }
    } else if constexpr (DIRECT) {
      // the waves of a block (and the steps of a fused rollout) never wait for each other
      if (mine) {
        double reward = 0.0;
        float o[8];
        type = Env::template step<LOG, MT>(a, i, oi, lane, step0 + (uint64_t)t, o, reward);
        bsx_emit_at<LOG, NOISE, F64, MT, bsx_policy(BSX_OUT_SCALARS, ROLLOUT)>(a.ctl, a.out, i, oi, lane, step0 + (uint64_t)t, type, reward);
        // (row-per-lane stores also in a big launch: staging the rows like the fused rollout does left the eager step
        // where it was — 17.5 / 17.5 vs 18.0 / 17.4 us at 2^20 lanes — and cost 4 % at 2^18,
        // profiles/r03/ab_eager_rows_via_lds.log: one memory round trip per launch bounds it, not the write requests;
        // pooled resets in the eager step: 17.6 -> 19.1-19.6 us, the barriers wait for the slowest wave's loads,
        // profiles/r03/ab_eager_pooled_resets.log)
        // Rows of 4-8 floats (cartpole, swing-up): a full wave stages its 64 rows in LDS and stores them as NON-TEMPORAL 16-byte
        // chunks (small_obs_store_rows_wave) — row-per-lane they are 8-byte pieces at the row stride, partial lines that must
        // not be non-temporal (18 -> 25 us), and ordinary stores evict the columns the next call reads.  Round 3 had measured the
        // staging alone as equal (ab_eager_rows_via_lds.log); with non-temporal chunks: cartpole/0 17.4-18.7 -> 15.4-16.0 us per
        // step at 2^20 lanes, 7.8 -> 7.2 at 2^18 (profiles/r06/ab_cartpole_eager_rows_lds_nt.log).
        bool staged = false;
        if constexpr (Env::HAS_REGS) {
          if constexpr (Env::ROWS_VIA_LDS && !ROLLOUT) {
            float* s_rows_e = s_obs;                                // dynamic LDS: small_obs_lds() reserves 256 rows x 8 floats
            const int wl_e = (int)(threadIdx.x & 63u);
            if (i - wl_e + 64 <= B) {                              // (uniform per wave: all 64 lanes are in range)
              bsx_f4* w4 = reinterpret_cast<bsx_f4*>(a.out.observation + (oi - wl_e) * (int64_t)numel);
              small_obs_store_rows_wave<false>([=](int c) { return w4 + c; }, o, numel, s_rows_e + (threadIdx.x - wl_e) * 8, wl_e);
              staged = true;
            }
          }
        }
        if (!staged) small_obs_store_row<ROLLOUT>(a.out.observation + oi * (int64_t)numel, o, numel);
      }
      bsx_count_types(a.ctl, type, s_cnt);
    } else {
      constexpr int HEAD = Env::HEAD, PLANES = Env::PLANES;          // numel >= 9 here (bsx_small_direct_shape)
      // LDS: PLANES data planes + 1 plane marking the HEAD elements (a fixed pattern: bits l*numel + k, k < HEAD —
      // built once per launch), `stride` words each; then the 256 lanes' HEAD floats (4 floats of padding either side).
      uint32_t* __restrict__ planes = reinterpret_cast<uint32_t*>(s_obs);
      const int stride = numel * (BSX_BLOCK / 32);                       // words per plane
      uint32_t* __restrict__ head_plane = planes + PLANES * stride;
      float* __restrict__ s_head = reinterpret_cast<float*>(head_plane + stride) + 4;
      // ... then the time fractions 1 - t / L, t = 0..L, when the chain is short enough (small_obs_lds): every lane's row
      // holds one, an f64 division per lane-step that the workgroup's first L + 1 threads now do once per launch
      // (umbrella_length: 13 threads of one wave instead of all four waves)
      // (single steps only: inside the fused rollout's step loop the table made umbrella_length r16 9 % SLOWER, 25.1 ->
      // 27.4 us per step, while the eager step gained 2.6 %: profiles/r05/ab_chain_time_fraction_table.log)
      const float* s_tf = nullptr;
      if (!ROLLOUT && Env::tf_table_fits(a)) {
        float* tab = s_head + BSX_BLOCK * HEAD + 4;
        s_tf = tab;
        if (t == 0) {
          BSX_NO_CONTRACT
          for (int k = threadIdx.x; k <= a.L; k += BSX_BLOCK) tab[k] = (float)(1.0 - (double)k / (double)a.L);
        }
      }
      if (t == 0) {
        for (int w = threadIdx.x; w < (PLANES + 1) * stride; w += BSX_BLOCK) planes[w] = 0u;
      } else {
        __syncthreads();                                                 // every chunk of step t-1 has been read
        for (int w = threadIdx.x; w < PLANES * stride; w += BSX_BLOCK) planes[w] = 0u;
      }
      __syncthreads();
      if (mine) {
        double reward = 0.0;
        float head[HEAD];
        const bsx_bit_sink sink{planes, stride, (uint32_t)((int)threadIdx.x * numel + HEAD), s_tf};
        type = Env::template step<LOG, MT, true>(a, i, oi, lane, step0 + (uint64_t)t, head, reward, &sink);
        bsx_emit_at<LOG, NOISE, F64, MT, bsx_policy(BSX_OUT_SCALARS, ROLLOUT)>(a.ctl, a.out, i, oi, lane, step0 + (uint64_t)t, type, reward);
#pragma unroll
        for (int k = 0; k < HEAD; ++k) s_head[threadIdx.x * HEAD + k] = head[k];
        if (t == 0) {
          const bsx_bit_sink hs{head_plane, stride, (uint32_t)((int)threadIdx.x * numel)};
          hs.put(0, 0, 0xFFFFFFFFu, HEAD);
        }
      }
      bsx_count_types(a.ctl, type, s_cnt);
      __syncthreads();

      // Stream the tile: [lanes_here x numel] floats, contiguous in HBM, 16-byte aligned start, every byte written
      // exactly once and only by full 16-byte chunks (1 KiB per wave instruction).  Chunk c is the nibble at bit 4c of
      // each plane, four bit-tests away from a float4; where the HEAD plane's nibble is non-zero the lane's HEAD
      // floats are spliced in from LDS: numel >= 9 means at most ONE lane's HEAD run lies in a chunk, so one magic
      // division finds it and element j of the chunk is s_head[base + j].  What this replaces, and why
      // (profiles/r03/ab_wide_rows*.log): r02 streamed zeros into the HEAD places and patched them with a 12-byte
      // store per lane after a third barrier and the store acknowledgements of the whole tile; storing the HEAD
      // chunks from their own lanes instead (no patch, no third barrier) was no faster — the L2 is bound by write
      // REQUESTS here, and a million scattered partial-line stores are a third of all requests: without any HEAD
      // stores the same kernel takes 86 us instead of 116 (umbrella_distract).
      float* __restrict__ tile = a.out.observation + ((int64_t)t * B + lane0) * (int64_t)numel;
      const int total = lanes_here * numel;
      const bool vec = ((((int64_t)t * B * numel) & 3) == 0);            // [t] slice 16-byte aligned?
      const int n_chunks = vec ? total >> 2 : 0;
      const uint32_t numel_magic = a.numel_magic;                        // f / numel = __umulhi(f, magic), f < 2^16
      bsx_f4* __restrict__ t4 = reinterpret_cast<bsx_f4*>(tile);
      for (int ch = threadIdx.x; ch < n_chunks; ch += BSX_BLOCK) {
        const int sh = (ch & 7) << 2;
        const uint32_t n0 = planes[ch >> 3] >> sh;
        const uint32_t n1 = PLANES > 1 ? planes[stride + (ch >> 3)] >> sh : 0u;
        const uint32_t hm = (head_plane[ch >> 3] >> sh) & 0xFu;
        bsx_f4 q;
        q.x = Env::decode(n0 & 1u, n1 & 1u);
        q.y = Env::decode((n0 >> 1) & 1u, (n1 >> 1) & 1u);
        q.z = Env::decode((n0 >> 2) & 1u, (n1 >> 2) & 1u);
        q.w = Env::decode((n0 >> 3) & 1u, (n1 >> 3) & 1u);
        if (hm != 0u) {
          const int j1 = __ffs((int)hm) - 1;                             // first HEAD element of the chunk
          const uint32_t f1 = ((uint32_t)ch << 2) + (uint32_t)j1;
          const uint32_t l = __umulhi(f1, numel_magic);                  // its lane
          const int base = (int)(l * (uint32_t)HEAD + (f1 - l * (uint32_t)numel)) - j1;   // >= -3: padded
          const float h0 = s_head[base], h1 = s_head[base + 1], h2 = s_head[base + 2], h3 = s_head[base + 3];
          q.x = (hm & 1u) ? h0 : q.x;
          q.y = (hm & 2u) ? h1 : q.y;
          q.z = (hm & 4u) ? h2 : q.z;
          q.w = (hm & 8u) ? h3 : q.w;
        }
        bsx_st<bsx_policy(BSX_OUT_TILE, ROLLOUT)>(&t4[ch], q);
      }
      // elements beyond the 16-byte chunks (an unaligned [t] slice, or the < 4 floats at the end of an odd tile)
      for (int f = (n_chunks << 2) + (int)threadIdx.x; f < total; f += BSX_BLOCK) {
        const uint32_t b0 = (planes[f >> 5] >> (f & 31)) & 1u;
        const uint32_t b1 = PLANES > 1 ? (planes[stride + (f >> 5)] >> (f & 31)) & 1u : 0u;
        float v = Env::decode(b0, b1);
        if ((head_plane[f >> 5] >> (f & 31)) & 1u) {
          const uint32_t l = __umulhi((uint32_t)f, numel_magic);
          v = s_head[l * (uint32_t)HEAD + ((uint32_t)f - l * (uint32_t)numel)];
        }
        tile[f] = v;
      }
    }
  }
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, block_id);
}

template <class Env, bool ROLLOUT, int LOG, int NOISE, int MT, bool DIRECT, bool ROWS = false>
__global__ void __launch_bounds__(BSX_BLOCK) small_obs_kernel(const typename Env::args a, const int n_steps) {
  extern __shared__ __attribute__((aligned(16))) float s_obs[];
  __shared__ unsigned int s_cnt[2];
  small_obs_body<Env, ROLLOUT, LOG, NOISE, MT, DIRECT, false, -1, -1, ROWS>(a, n_steps, blockIdx.x, s_obs, s_cnt);
}

// Eager step of a register-resident family, LPT = 2 or 4 lanes per thread (lean calls of 2^19+ lanes): thread t of
// workgroup b advances lanes b*LPT*256 + h*256 + t, the loads of ALL of them issued before the first use.  At 2^20 lanes
// the one-lane kernel is 4096 workgroups = two dispatch rounds of a launch whose every wave is one dependent chain
// {column loads -> step -> stores}; this one is a single round with LPT times the bytes in flight per wave.
// r04 measured cartpole / mountain_car only, called them equal and left it off.  Round 5, same call, two repetitions, with
// bandit, discounting_chain and memory_len now register-resident (profiles/r05/ab_eager_lanes_per_thread.log), 1 -> 2 lanes
// per thread at 2^20 lanes: bandit 9.55 -> 8.65 us, discounting_chain 8.7 -> 7.2, memory_len 12.0 -> 10.2, mountain_car
// 9.95 -> 9.0, cartpole 18.9 -> 18.5 (noise); at 2^19: bandit 6.3 -> 6.1, memory_len 7.75 -> 7.1, mountain_car 6.7 -> 6.4,
// discounting_chain equal, cartpole 10.8 -> 11.2 (SLOWER); at 2^18 all equal.  Four lanes per thread are never better than
// two (discounting_chain 8.1, memory_len 10.4 at 2^20; everything slower at 2^19).  Env::EAGER_LPT_MIN_BLOCKS per family.
template <class Env, int V, int LPT>
__global__ void __launch_bounds__(BSX_BLOCK) small_obs_eager2_kernel(const typename Env::args a) {
  __shared__ unsigned int s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int numel = Env::numel_of(V);
  const int64_t B = a.ctl.n_lanes;
  const uint64_t step = bsx_step_of(a.ctl);
  int64_t i[LPT];
  bool mine[LPT];
  typename Env::regs rg[LPT];
  int act[LPT], type[LPT];
#pragma unroll
  for (int h = 0; h < LPT; ++h) {
    i[h] = (int64_t)blockIdx.x * (LPT * BSX_BLOCK) + h * BSX_BLOCK + threadIdx.x;
    mine[h] = i[h] < B;
    Env::clear(rg[h]);
    act[h] = 0;
    type[h] = -1;
    if (mine[h]) {
      Env::load(a, i[h], rg[h]);
      if (!a.ctl.force_reset) act[h] = bsx_action(a.ctl, a.action, i[h], step);
    }
  }
#pragma unroll
  for (int h = 0; h < LPT; ++h) {
    if (mine[h]) {
      double reward = 0.0;
      float o[8];
      type[h] = Env::template core<0, 0, false, false, false, V>(a, rg[h], act[h], i[h], a.ctl.lane_offset + (uint64_t)i[h], step, o, reward);
      bsx_emit_at<0, 0, false, -1, BSX_OUT_SCALARS.eager>(a.ctl, a.out, i[h], i[h], a.ctl.lane_offset + (uint64_t)i[h], step, type[h], reward);
      small_obs_store_row<false>(a.out.observation + i[h] * (int64_t)numel, o, numel);
      Env::store(a, i[h], rg[h]);
    }
    bsx_count_types(a.ctl, type[h], s_cnt);
  }
  bsx_final_barrier();
  bsx_flush_counts(a.ctl, s_cnt, blockIdx.x);
}

// The lean fused rollout of a register-resident family (no Logging wrapper, no RewardNoise, counter-based draws):
// one instantiation per (big launch, variant, table in LDS) — everything the step loop would otherwise carry as
// run-time conditions in scalar registers.
// (Tried: holding the pooled cartpole loop, 65 VGPRs, to 64 = 8 waves per SIMD, so that the 16 workgroups a CU runs at
// 2^20 lanes are 8 + 8 instead of 7 + 7 + 2.  amdgpu_waves_per_eu(8, 8) also caps the SCALAR registers at 80 of the
// 102 — the attribute that made sweep_phase0_kernel spill 157 of them in r03 — and the ~35 reloads per step it costs
// here cancel the gain: 10.2-10.3 vs 10.0-10.1 us per step, profiles/r04/ab_rollout_8_waves.log; amdgpu_num_vgpr(64)
// is ignored by this compiler.)
template <class Env, bool BIG, int V, bool TAB>
__global__ void __launch_bounds__(BSX_BLOCK) small_obs_lean_rollout_kernel(const typename Env::args a, const int n_steps) {
  extern __shared__ __attribute__((aligned(16))) float s_obs[];
  __shared__ unsigned int s_cnt[2];
  small_obs_body<Env, true, 0, 0, 0, true, BIG, V, TAB ? 1 : 0>(a, n_steps, blockIdx.x, s_obs, s_cnt);
}

// Dynamic LDS of one workgroup stepping `a`.
template <class Env>
static size_t small_obs_lds(const typename Env::args& a) {
  if constexpr (Env::PACKED)     // PLANES data planes + the HEAD-position plane + the lanes' HEAD floats (padded) + the time fractions
    return bsx_small_direct_shape(a.obs_numel) ? 0 : (size_t)(Env::PLANES + 1) * a.obs_numel * (BSX_BLOCK / 32) * 4 + (size_t)(BSX_BLOCK * Env::HEAD + 8) * 4 +
                                                     (Env::tf_table_fits(a) ? ((size_t)a.L + 1) * 4 : 0);
  else if constexpr (Env::HAS_REGS) return Env::ROWS_VIA_LDS ? (size_t)BSX_BLOCK * 8 * 4 : 0;     // the eager step's row staging (small_obs_body, DIRECT)
  else return 0;
}
// does a single-step call of this segment take the row path (flat bit planes into a.rows + the wide-row store stream)?
template <class Env>
static bool small_obs_rows(const typename Env::args& a) {
  if constexpr (Env::PACKED) return a.rows != nullptr && !bsx_small_direct_shape(a.obs_numel);
  else return false;
}
// dynamic LDS of one workgroup on the row path: every wave's own PLANES x 2 * numel plane words
template <class Env>
static size_t small_obs_rows_lds(const typename Env::args& a) {
  if constexpr (Env::PACKED) return (size_t)(BSX_BLOCK / BSX_WAVE) * Env::PLANES * 2 * (size_t)a.obs_numel * 4;
  else return 0;
}
// the arguments of the wide-row store stream of a segment on the row path
template <class Env>
static bsx_row_seg small_obs_row_seg(const typename Env::args& a) {
  bsx_row_seg g{};
  if constexpr (Env::PACKED) {
    g.obs = a.out.observation; g.planes = a.rows; g.n_lanes = a.ctl.n_lanes; g.plane_words = (uint64_t)a.row_plane_words;
    g.numel = (uint32_t)a.obs_numel; g.numel_magic = bsx_div_magic(g.numel); g.dv = bsx_make_div64(g.numel);
  }
  return g;
}
// ... and of a fused rollout: the tables a register-resident family stages (cartpole: the time fractions)
template <class Env>
static size_t small_obs_rollout_lds(const typename Env::args& a) {
  if constexpr (Env::HAS_REGS && Env::PACKED) return bsx_small_direct_shape(a.obs_numel) ? Env::table_bytes(a) : small_obs_lds<Env>(a);
  else if constexpr (Env::HAS_REGS) return Env::table_bytes(a);
  else return small_obs_lds<Env>(a);
}

// One workgroup of a grouped launch: the single-step body.  A segment without Logging wrapper, RewardNoise and
// MT19937 draws (uniform per workgroup) runs the lean instantiation, like a stand-alone call does: a cartpole
// workgroup then issues a third fewer instructions, and the heavy workgroups are what a sweep's lane advance
// waits for (profiles/r02/sweep_phase0_trace.json).
// MT = 0: the group holds no segment in MT19937-exact mode (the whole-sweep group refuses them, bsx_mixed_put): the
// wrapped segments' bodies are compiled without the generator's twist and numpy's legacy samplers.
template <class Env, bool D, int MT = -1, bool ROWS = false>
__device__ __forceinline__ void small_obs_group_body_d(const typename Env::args& a, const uint32_t blk, float* s_obs,
                                                       unsigned int* s_cnt) {
  if (bsx_ctl_lean(a.ctl)) small_obs_body<Env, false, 0, 0, 0, D, false, -1, -1, ROWS>(a, 1, blk, s_obs, s_cnt);
  else small_obs_body<Env, false, -1, -1, MT, D, false, -1, -1, ROWS>(a, 1, blk, s_obs, s_cnt);
}
// ROWS_OK: the launch is followed by the wide-row store stream (the whole-sweep group's phase 1): a segment that
// brought a row scratch leaves its rows there, packed; everywhere else wide rows go through the LDS bit planes.
template <class Env, int MT = -1, bool ROWS_OK = false>
__device__ __forceinline__ void small_obs_group_body(const typename Env::args& a, const uint32_t blk, float* s_obs,
                                                     unsigned int* s_cnt) {
  if constexpr (Env::PACKED) {
    if (!bsx_small_direct_shape(a.obs_numel)) {                 // uniform per workgroup
      if constexpr (ROWS_OK) {
        if (a.rows != nullptr) {
          small_obs_group_body_d<Env, true, MT, true>(a, blk, s_obs, s_cnt);
          return;
        }
      }
      small_obs_group_body_d<Env, false, MT>(a, blk, s_obs, s_cnt);
      return;
    }
  }
  small_obs_group_body_d<Env, true, MT>(a, blk, s_obs, s_cnt);
}

// Grouped launch: every workgroup looks up its segment and runs the single-step body on that
// segment's argument struct (device memory).
template <class Env>
__global__ void __launch_bounds__(BSX_BLOCK) small_obs_group_kernel(const typename Env::args* __restrict__ table,
                                                                    const bsx_group_index gi) {
  extern __shared__ __attribute__((aligned(16))) float s_obs[];
  __shared__ unsigned int s_cnt[2];
  const bsx_group_slot w = bsx_group_find(gi, (int)blockIdx.x);
  small_obs_group_body<Env>(table[w.seg], w.block, s_obs, s_cnt);
}

// bandit and discounting_chain — the two families whose whole step is a register-resident row of one or two floats — share
// ONE kernel for their single-family groups, off every measured path: small_obs_duo_group_kernel (sweep_mixed.hip), the
// family a uniform switch and each branch small_obs_group_body<Env> unchanged.  Their env headers say so here.
template <class Env>
struct small_obs_duo_group { static constexpr bool value = false; };
// launch of a single-family group of bandit or discounting_chain (g->family says which; sweep_mixed.hip)
int bsx_small_duo_launch(bsx_group* g, int phase, hipStream_t st);

template <class Env>
static int small_obs_group_launch(bsx_group* g, int phase, hipStream_t st) {
  if constexpr (small_obs_duo_group<Env>::value) {
    return bsx_small_duo_launch(g, phase, st);
  } else {
    if (phase == 1) return 0;               // one kernel per step: everything happens in phase 0
    const dim3 grid((unsigned)g->total_blocks), block(BSX_BLOCK);
    const typename Env::args* table = (const typename Env::args*)g->d_args;
    small_obs_group_kernel<Env><<<grid, block, g->lds_bytes, st>>>(table, g->index1());
    return (int)hipGetLastError();
  }
}

// A BSX_FAM_SMALL_MIXED group holds segments of ANY of the families in this file: every segment's
// argument struct sits in a fixed-stride slot next to a family tag, and one launch
// advances them all (the kernel switches on the tag per workgroup).  Six ~8 us launches of a
// heterogeneous sweep become one.
#define SMALL_MIXED_STRIDE 1024
// launch of a BSX_FAM_SMALL_MIXED group (sweep_mixed.hip)
int bsx_small_mixed_launch(bsx_group* g, int phase, hipStream_t st);


// Records one segment of a small-observation family in a group (of its own family, or mixed).
template <class Env>
static int small_obs_group_put(bsx_group* g, int32_t family, int32_t index, const bsx_call_t* call,
                               const typename Env::args& a_in) {
  static_assert(sizeof(typename Env::args) <= SMALL_MIXED_STRIDE, "argument struct exceeds the mixed-group slot");
  typename Env::args a = a_in;
  const uint64_t nb = (uint64_t)bsx_blocks_of(a.ctl.n_lanes);
  if (g != nullptr && g->family == BSX_FAM_SWEEP_MIXED) {     // one segment of the whole-sweep group
    if (small_obs_rows<Env>(a)) {
      // wide rows with a row scratch: phase 0 leaves them packed, the phase-1 store stream writes the observations
      const bsx_row_seg sg = small_obs_row_seg<Env>(a);
      return bsx_mixed_put(g, family, index, call, &a, sizeof(a), &sg, sizeof(sg), nb,
                           bsx_flat_blocks((uint64_t)a.ctl.n_lanes * sg.numel, BSX_ROW_STREAM_K), small_obs_rows_lds<Env>(a));
    }
    return bsx_mixed_put(g, family, index, call, &a, sizeof(a), nullptr, 0, nb, 0, small_obs_lds<Env>(a));   // phase 0 only
  }
  if constexpr (Env::PACKED) a.rows = nullptr;                // single-launch groups: the LDS bit planes
  const size_t lds = small_obs_lds<Env>(a);
  const bool mixed = g != nullptr && g->family == BSX_FAM_SMALL_MIXED;
  int rc = bsx_group_check_set(g, mixed ? BSX_FAM_SMALL_MIXED : family, index, call,
                               mixed ? SMALL_MIXED_STRIDE : sizeof(typename Env::args), mixed ? sizeof(int32_t) : 0, BSX_BLOCK);
  if (rc != 0) return rc;
  memcpy(&g->args[(size_t)index * g->arg_size], &a, sizeof(a));
  if (mixed) memcpy(&g->args2[(size_t)index * sizeof(int32_t)], &family, sizeof(int32_t));
  if (nb > 0x3FFFFFFFull) return BSX_EINVAL;
  g->blocks[index] = (int32_t)nb;
  if (lds > g->lds_bytes) g->lds_bytes = lds;
  g->is_set[index] = 1;
  g->launch = mixed ? bsx_small_mixed_launch : small_obs_group_launch<Env>;
  return 0;
}

// variant 1 of a register-resident family that has one (else the instantiation is the same kernel as variant 0's)
template <class Env>
static constexpr int small_obs_v1() {
  if constexpr (Env::HAS_REGS) return Env::N_VARIANTS > 1 ? 1 : 0;
  else return -1;
}

// does the family's fused rollout have a variant for big launches (small_obs_regs_rollout, BIG)?
template <class Env>
static constexpr bool small_obs_has_big() {
  if constexpr (Env::HAS_REGS) return Env::POOLED_RESETS || Env::ROWS_VIA_LDS;
  else return false;
}

// Launches the lean fused rollout of a register-resident family (small_obs_lean_rollout_kernel).
template <class Env>
static void launch_regs_rollout(const typename Env::args& a, int n_steps, int v, bool big, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if constexpr (Env::HAS_REGS) {
    constexpr bool HB = small_obs_has_big<Env>();
    constexpr int V1 = small_obs_v1<Env>();
    // (a family without a table — TABLE_MAX_BYTES = 0: bandit, discounting_chain, whose table_fits() is the constant false —
    // has no TAB instantiation at all: a kernel that can never launch still counts against the library's kernel budget)
    constexpr bool HT = Env::TABLE_MAX_BYTES > 0;
    const bool tab = HT && Env::table_fits(a);
#define REGS_ROLLOUT(BIGV, VV)                                                                                     \
    {                                                                                                              \
      if constexpr (HT) {                                                                                          \
        if (tab) small_obs_lean_rollout_kernel<Env, BIGV, VV, true><<<g, b, lds, st>>>(a, n_steps);                \
      }                                                                                                            \
      if (!tab) small_obs_lean_rollout_kernel<Env, BIGV, VV, false><<<g, b, lds, st>>>(a, n_steps);                \
    }
    if (v == 1 && big) REGS_ROLLOUT(HB, V1)
    else if (v == 1) REGS_ROLLOUT(false, V1)
    else if (big) REGS_ROLLOUT(HB, 0)
    else REGS_ROLLOUT(false, 0)
#undef REGS_ROLLOUT
  }
}

// LPT lanes per thread for the lean eager step of a register-resident family (Env::EAGER_LPT_MIN_BLOCKS: from this many
// one-lane workgroups up, 0 = never; Env::EAGER_LPT)
// (a family whose gate is 0 — cartpole: never, measured equal or slower — has the kernel in the tuning build alone, where
// BSX_EAGER2_MIN_BLOCKS can open the gate: a kernel that can never launch still counts against the library's kernel budget)
template <class Env>
static constexpr bool small_obs_has_eager_lpt() {
#ifdef BSX_TUNING
  return Env::HAS_REGS;
#else
  if constexpr (Env::HAS_REGS) return Env::EAGER_LPT_MIN_BLOCKS > 0;
  else return false;
#endif
}
template <class Env, int LPT>
static void launch_eager_lpt(const typename Env::args& a, int v, hipStream_t st) {
  if constexpr (small_obs_has_eager_lpt<Env>()) {
    const dim3 g((unsigned)((a.ctl.n_lanes + LPT * BSX_BLOCK - 1) / (LPT * BSX_BLOCK))), b(BSX_BLOCK);
    if (v == 1) small_obs_eager2_kernel<Env, small_obs_v1<Env>(), LPT><<<g, b, 0, st>>>(a);
    else small_obs_eager2_kernel<Env, 0, LPT><<<g, b, 0, st>>>(a);
  }
}
template <class Env>
static void launch_eager2(const typename Env::args& a, int v, int lpt, hipStream_t st) {
#ifdef BSX_TUNING
  if (lpt == 4) { launch_eager_lpt<Env, 4>(a, v, st); return; }      // measured: never better than 2 (see below)
#endif
  (void)lpt;
  launch_eager_lpt<Env, 2>(a, v, st);
}

template <class Env>
static int launch_small_obs(const typename Env::args& a, int n_steps, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  if (n_steps < 1) return BSX_EINVAL;
  const bool logging = a.ctl.log.steps != nullptr, noise = a.ctl.wrap_kind >= BSX_WRAP_NOISE;
  // (the wrapped rollouts are compiled with and without the MT19937-exact draws: the common wrapped run draws from the
  // counter-based stream, and the generator's twist + numpy's legacy samplers cost the loop 50-70 VGPRs)
  const bool mt = a.ctl.mt_state != nullptr;
  const bool lean = bsx_ctl_lean(a.ctl);
  // the register-resident families' lean rollouts are compiled per variant (row length, swing-up): -1 = none
  // (and address every [B, numel] slab with 32-bit byte offsets: a slab of 4 GiB or more takes the generic loop)
  int regs_v = -1, Env_variant = 0;
  bool eager2 = false;
  int eager_lpt = 2;
  if constexpr (Env::HAS_REGS) {
    Env_variant = Env::variant_of(a);
    if (a.ctl.n_lanes * (int64_t)a.obs_numel * 4 < ((int64_t)1 << 32)) regs_v = Env_variant;
    if (Env::PACKED && !bsx_small_direct_shape(a.obs_numel)) regs_v = -1;      // wide rows: the LDS bit planes, step by step
    static const int eager2_min_blocks = bsx_env_int("BSX_EAGER2_MIN_BLOCKS", Env::EAGER_LPT_MIN_BLOCKS);
    static const int eager_lpt_knob = bsx_env_int("BSX_EAGER_LPT", Env::EAGER_LPT);
    eager2 = eager2_min_blocks > 0 && Env_variant >= 0 && bsx_blocks_of(a.ctl.n_lanes) >= eager2_min_blocks;
    eager_lpt = eager_lpt_knob;
  }
  const int64_t blocks = bsx_blocks_of(a.ctl.n_lanes);
  if (blocks > 0x7FFFFFFF) return BSX_EINVAL;
  const size_t lds = n_steps > 1 ? small_obs_rollout_lds<Env>(a) : small_obs_lds<Env>(a);
  const dim3 g((unsigned)blocks), b(BSX_BLOCK);
  // the register-resident families' fused rollout: pooled resets / staged rows from 2^19 lanes (8 workgroups per CU) up
  static const int big_min_blocks = bsx_env_int("BSX_REGS_ROLLOUT_BIG_MIN_BLOCKS", 2048);
  const bool big = small_obs_has_big<Env>() && blocks >= big_min_blocks;
  // Per-thread stores (4-byte / 12-byte / 8-byte stores, each wave writing one contiguous range) against
  // an f32 LDS tile, measured on bandit, discounting_chain, cartpole, mountain_car, memory_len: eager equal
  // or 2-4 % faster, fused rollout 3-15 % faster (profiles/r02/ab_small_direct_stores.log).  Three 4-byte
  // stores at stride 12 for the 3-float rows were 5-8 % SLOWER than the tile; one global_store_dwordx3 is
  // faster.
#define SMALL_OBS_LAUNCH(D)                                                                                \
  {                                                                                                        \
    if (n_steps == 1 && lean && eager2) launch_eager2<Env>(a, Env_variant, eager_lpt, st);                 \
    else if (n_steps == 1 && lean) small_obs_kernel<Env, false, 0, 0, 0, D><<<g, b, lds, st>>>(a, 1);      \
    else if (n_steps == 1) small_obs_kernel<Env, false, -1, -1, -1, D><<<g, b, lds, st>>>(a, 1);           \
    else if (logging && noise && !mt) small_obs_kernel<Env, true, 1, 1, 0, D><<<g, b, lds, st>>>(a, n_steps); \
    else if (logging && !mt) small_obs_kernel<Env, true, 1, 0, 0, D><<<g, b, lds, st>>>(a, n_steps);       \
    else if (noise && !mt) small_obs_kernel<Env, true, 0, 1, 0, D><<<g, b, lds, st>>>(a, n_steps);         \
    else if (logging && noise) small_obs_kernel<Env, true, 1, 1, -1, D><<<g, b, lds, st>>>(a, n_steps);    \
    else if (logging) small_obs_kernel<Env, true, 1, 0, -1, D><<<g, b, lds, st>>>(a, n_steps);             \
    else if (noise) small_obs_kernel<Env, true, 0, 1, -1, D><<<g, b, lds, st>>>(a, n_steps);               \
    else if (lean && regs_v >= 0) launch_regs_rollout<Env>(a, n_steps, regs_v, big, g, b, lds, st);        \
    else if (lean) small_obs_kernel<Env, true, 0, 0, 0, D><<<g, b, lds, st>>>(a, n_steps);                 \
    else small_obs_kernel<Env, true, 0, 0, -1, D><<<g, b, lds, st>>>(a, n_steps);                          \
  }
  if constexpr (Env::PACKED) {
    if (!bsx_small_direct_shape(a.obs_numel)) {
      if (n_steps == 1 && small_obs_rows<Env>(a)) {
        // wide rows, a single step, a row scratch: lane advance (rows packed into the scratch) + the store stream
        // that decodes them (row_stream.h) instead of the one launch with the LDS bit planes and its three barriers
        const size_t rlds = small_obs_rows_lds<Env>(a);
        if (lean) small_obs_kernel<Env, false, 0, 0, 0, true, true><<<g, b, rlds, st>>>(a, 1);
        else small_obs_kernel<Env, false, -1, -1, -1, true, true><<<g, b, rlds, st>>>(a, 1);
        const bsx_row_seg sg = small_obs_row_seg<Env>(a);
        static const int row_k = bsx_env_int("BSX_ROW_STREAM_K", BSX_ROW_STREAM_K);
        const int k = row_k == 1 || row_k == 4 ? row_k : 2;
        const uint64_t sblocks = bsx_flat_blocks((uint64_t)a.ctl.n_lanes * sg.numel, k);
        if (sblocks > 0x7FFFFFFFull) return BSX_EINVAL;
        const dim3 gs((unsigned)sblocks);
#ifdef BSX_TUNING     // (the knob is read in the tuning build only: the product library carries the K = 2 stream alone)
        if (k == 1) bsx_row_stream_kernel<typename Env::rows_t, 1><<<gs, b, 0, st>>>(sg);
        else if (k == 4) bsx_row_stream_kernel<typename Env::rows_t, 4><<<gs, b, 0, st>>>(sg);
        else
#endif
        bsx_row_stream_kernel<typename Env::rows_t, 2><<<gs, b, 0, st>>>(sg);
        return bsx_launch_status();
      }
      SMALL_OBS_LAUNCH(false)
      return bsx_launch_status();
    }
  }
  SMALL_OBS_LAUNCH(true)
#undef SMALL_OBS_LAUNCH
  return bsx_launch_status();
}

// ------------------------------------------------------------------------------ shared by more than one family
// What a register-resident family (HAS_REGS) inherits unless it has something to say: no pooled resets, rows stored by
// their own threads, one variant, no table, no info columns held in registers (A = the family's args, R = its regs).  A
// family that overrides a member declares its own; cartpole, which would override nearly all, declares every member itself.
struct small_regs_defaults {
  static constexpr bool POOLED_RESETS = false, ROWS_VIA_LDS = false;
  static constexpr int N_VARIANTS = 1, TABLE_MAX_BYTES = 0;
  static constexpr int EAGER_LPT_MIN_BLOCKS = 2048, EAGER_LPT = 2;   // lean eager step: lanes per thread (launch_small_obs)
  template <bool NOFORCE = false, class A, class R> __device__ static __forceinline__ bool wants_reset(const A&, const R&) { return false; }
  template <class A> __device__ static __forceinline__ void reset_part(const A&, uint64_t, uint64_t, int, unsigned, bsx_reset_pool*) {}
  template <class A> __host__ __device__ static bool table_fits(const A&) { return false; }
  template <class A> static size_t table_bytes(const A&) { return 0; }
  template <class A> __device__ static __forceinline__ bsx_lds_table stage_tables(const A&, float*) { return (bsx_lds_table)0; }
  template <int V = -1, class A, class R> __device__ static __forceinline__ void load_info(const A&, int64_t, R&) {}
  template <int V = -1, class A, class R> __device__ static __forceinline__ void store_info(const A&, int64_t, const R&) {}
};

// The time fraction 1 - t / L of the chains' rows (memory_chain.py:64, umbrella_chain.py:64): from the workgroup's LDS
// table where the PACKED path staged one (bsx_bit_sink::tf), else the f64 division itself.  Evaluated ONCE per step(),
// before the reset / step paths part ways.
template <bool PACK, class Sink>
__device__ __forceinline__ float bsx_chain_time_fraction(int t, int L, const Sink* sink) {
  BSX_NO_CONTRACT
  if constexpr (PACK) {
    if (sink->tf != nullptr) return sink->tf[t];               // (t <= L; uniform branch)
  }
  return (float)(1.0 - (double)t / (double)L);
}

// The reset flag of the physics families' `steps` word (cartpole, swing-up, mountain_car: step count | flag).
#define CP_RESET_BIT (1 << 30)

#endif  // BSX_SMALL_OBS_H_
