// gg_v5.h - the multi-ply kernel for batches that fill the machine: THIRTY-TWO BOARDS PER WAVEFRONT (one pair of lanes per
// board), the floods of a ply compacted into a job list.
#pragma once
#include "gg_v4.h"

namespace gg {

// ===================================================================== v5: 32 boards per wave, flood jobs
// k_rollout4 (gg_v4.h) gives every board a quad of lanes: lane t floods whatever q's neighbour in direction t holds, and
// 39 % of those flood lanes carry a flood (1.56 per board and ply) - the flood batch, the liberty count and the seed set-up,
// 54 % of a ply's instructions, cost the same whatever their lanes carry.  Here a board is a PAIR of lanes (lane t owns
// the RPL = ceil(R / 2) adjacent rows RPL t ..), a wave holds 32 boards, and a ply is
//   1.  sampling, as in k_rollout4 (the pair scan is one DPP swap, the row of the k-th point a search tree over the prefix
//       counts); the point leaves the pair as (row << 5) | column and stays that way through the ply - phases 2a and 3 and the job
//       lanes take it apart by shift and mask, the flat index is formed once for last_actions (round 20: three divisions by N per
//       wave-ply gone, 12 -> 9 v_mul_lo_u32 in the ply loop, +1.7 % on the headline launch, docs/history/r20.md);
//   2a. the board's own lanes look at q's four neighbours (two directions each) and post the floods the ply needs as JOBS:
//       one per opponent stone next to q, and ONE for the mover's group G when q has a friendly neighbour (k_rollout4 runs
//       that flood in every friendly lane); the slots come from two ballots (v_mbcnt prefix), the descriptors - board, seed as
//       (row, column), colour, direction - go to LDS;
//   2b. lane L runs job L - 32 boards x 1.56 = 50 jobs in 64 lanes (a second batch when a ply posts more than 64: 0.7 %) -
//       with the fill in registers from the seed to the liberty count.  The batch's loop ends as soon as every flood of a G
//       is closed as far as stones OUTSIDE M go (the rows of M come out of an LDS plane the board lanes keep, round 29): the
//       minimum of three sweeps on 98 % of the batches; an opponent group whose part found so far has two liberties is
//       settled, the few lanes left with fewer flood on.  What phase 3 needs leaves the lane at the end: G as a block of its
//       board, an opponent group that is captured or leaves M ORed into the board's collection block, a captured direction
//       and G's liberties ORed into the board's info word;
//   3.  class patch, captures, ko and the next mover's mask on the pair lanes, from ONE collection block per board: it
//       splits by M alone (captured = not in M: q was the only liberty).
// Instructions per board: the flood batch is shared by twice the boards, and so is everything in phases 1 and 3 that does not
// scale with the rows a lane holds (the draw, the k-th-bit search, the capture / ko logic, addresses): 47.6 VALU per env step
// (PMC) in the first version against k_rollout4's 73.2, fewer since.  65 536 games are 2 048 waves = TWO per SIMD (19.5 KB of
// LDS, up to 256 VGPRs per wave); a SIMD with two waves sustains one dependent VALU instruction per 1.77 ns against 1.60
// with four (tools/ubench/dep_chain.hip), which is why the kernel pays from 256 games per CU on and not below.
// Scope: drawn moves on full-size boards (N == R), byte planes or tracked boards - the fused rollout of big batches; every
// other form stays on k_rollout4.
constexpr int kNB5 = 32;
#ifndef GG_AB_MPLANE1
#define GG_AB_MPLANE1 1   // (round 29's switch, described with the other switches below; Lds5 sizes the plane by it)
#endif
constexpr int kJobCap = 128;   // jobs of one ply: <= 4 per board (four opponent neighbours leave no friendly one)

template <int R>
struct Lds5 {
  // words per row block.  (13x13: 20 instead of the 16 of the other kernels - the lanes of a wave address 32 or 64 blocks at once,
  // and a stride of 16 words puts every fourth of them on the same LDS banks: 1.42 -> ms per launch of 65 536 games x 256 plies)
  static constexpr int RS = R == 13 ? 20 : Cfg<R>::kRowStride;
  static constexpr int RPL = (R + 1) / 2;                        // rows per lane in phases 1 and 3
  static_assert(2 * RPL <= RS, "a pair's rows must fit the row stride");
  static constexpr int kPad = 4;                                 // zero words in front of the planes: "row -1" / "row -2" of the first board
  static constexpr int kState = kPad;                            // [2][kNB5][RS]: black, white
  static constexpr int kMeta = kState + 2 * kNB5 * RS;           // flags[32], last[32], played[32], rng[64]
  static constexpr int kFair = kMeta + 5 * kNB5;                 // [16]: FairShare
  static constexpr int kTmp = kFair + 16;                        // [2][2][RS]: layout change of one pair at load
  static constexpr int kUnion = kTmp + 4 * RS;
  // ply loop: per job its descriptor, per board an info word (what its jobs found); per board the block of the mover's group G and the block in which the
  // opponent groups that are captured or leave M are collected (one OR per job that has such a group); per LANE a seed block
  // that is all zero between two uses (a job's seed is staged through it)
  static constexpr int kZero = kJobCap, kDump = kJobCap + 1;     // slot of an absent job (its class word is zero, never written) / of a write nobody reads
  static constexpr int kCls = kUnion;                            // [kJobCap + 4]: the first kNB5 words are the boards' info words
  static constexpr int kJob = kCls + kJobCap + 4;                // [kJobCap + 4]
  static constexpr int kG = kJob + kJobCap + 4;                  // [kNB5][2][RS]: G, the collected opponent groups
  static constexpr int kSc = kG + 2 * kNB5 * RS;                 // [kWave][RS]
  // (-DGG_AB_MPLANE1=1, 19x19) the rows of M of every board, [kNB5][RS] as one stone plane: live from the end of the load to the last
  // ply, behind everything the ply loop uses - the load's scratch and landing area and the emitter's bits may lie over it, the plane
  // is written when the load is done with them and dead when the write-back begins
  static constexpr bool kHasMpl = GG_AB_MPLANE1 != 0 && R == 19;
  static constexpr int kMpl = kSc + kWave * RS;
  static constexpr int kLoopEnd = kMpl + (kHasMpl ? kNB5 * RS : 0);
  // (-DGG_AB_FLAT1=1) the meta words - flags, last action, played - of a board that does not move are stored into the words of kCls
  // behind the boards' info words, which nothing else uses: laid out as kMeta's first three rows, never read
  static constexpr int kDumpMeta = kCls + kNB5;
  static_assert(kNB5 + 3 * kNB5 <= kJobCap, "the dump words end in front of the slot of an absent job");
  // load: the v2 analysis in its compact form (region 0 only); tracked boards: the DMA landing area, the parked rows
  static constexpr int kV2 = kUnion;
  static constexpr int kIoEnd = kV2 + (Lds2<R>::kRegion0 > 768 ? Lds2<R>::kRegion0 : 768);
  static constexpr int kDmaWords = (((kNB5 * (5 * R + 1) * 4 + 12 + 15) / 16 + kWave - 1) / kWave) * 256;
  static constexpr int kDmaEnd = kUnion + kDmaWords;
  // byte-plane write-back of a whole group (emit_group)
  static constexpr int kGrpBits = kUnion;
  static constexpr int kGrpWords = ((15 + kNB5 * 6 * R * R + 31) / 32 + 4) & ~3;
  static constexpr int kGrpLut = kGrpBits + kGrpWords;           // uint2[256]
  static constexpr int kGrpEnd = kGrpLut + 512;
  static constexpr int kMax2(int a, int b) { return a > b ? a : b; }
  static constexpr int kTotal = kMax2(kMax2(kLoopEnd, kIoEnd), kMax2(kDmaEnd, kGrpEnd));
  static_assert(kTotal * 4 <= 20480, "two waves per SIMD: 20 KB of LDS per wave");
  static_assert(kUnion % 4 == 0 && kG % 4 == 0 && kSc % 4 == 0 && kMpl % 4 == 0, "16-byte alignment of the flood blocks");
  static_assert(3 * kNB5 * RS <= kLoopEnd - kUnion, "parked tracked rows fit the loop area");
};

// set bits of a ballot in the lanes below this one
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
constexpr int QP_L0 = 0xA0;   // quad_perm [0,0,2,2]: the even lane of each pair

// kth_set_bit (gg_v4.h) for TEN rows per lane: the row is found by a search tree over the prefix counts (5 | 2 + 3 | 1 + 1 (+ 1):
// 31 instructions) instead of nine select steps in a row (45); the bit search inside the row is the same.
__device__ __forceinline__ void kth_set_bit10(const uint32_t (&v)[10], const uint32_t (&p)[10], uint32_t tt, int &rr, uint32_t &pos) {
  uint32_t ntt = ~tt;
  // c + ~tt = c - tt - 1 is negative iff tt >= c: the target lies beyond the rows counted by c
  const uint32_t g5 = (uint32_t)((int32_t)(p[4] + ntt) >> 31);
  uint32_t a[5], t[4];
#pragma unroll
  for (int i = 0; i < 5; ++i) a[i] = B3(g5, v[5 + i], v[i], T_SEL);
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = B3(g5, p[5 + i], p[i], T_SEL);
  uint32_t base = g5 & p[4], row = g5 & 5u;
  const uint32_t g2 = (uint32_t)((int32_t)(t[1] + ntt) >> 31);            // rows 2 .. 4 of the half
  const uint32_t b0 = B3(g2, a[2], a[0], T_SEL), b1 = B3(g2, a[3], a[1], T_SEL), u0 = B3(g2, t[2], t[0], T_SEL);
  base = B3(g2, t[1], base, T_SEL);
  row = B3(g2, 2u, row, T_ANDOR);                                          // (0 or 5) + 2: no carry
  const uint32_t g1 = (uint32_t)((int32_t)(u0 + ntt) >> 31);
  uint32_t vr = B3(g1, b1, b0, T_SEL);
  base = B3(g1, u0, base, T_SEL);
  row -= g1;
  const uint32_t g1b = B3(g2, g1, (uint32_t)((int32_t)(t[3] + ntt) >> 31), TA & TB & TC);   // the last row of the three-row group
  vr = B3(g1b, a[4], vr, T_SEL);
  base = B3(g1b, t[3], base, T_SEL);
  row -= g1b;
  ntt += base;                                                          // ~(tt - base)
  uint32_t ps = 0;
#pragma unroll
  for (int sh = 16; sh >= 1; sh >>= 1) {
    const uint32_t e = (uint32_t)__popc((vr >> ps) & ((1u << sh) - 1u)) + ntt;
    const uint32_t ge = (uint32_t)((int32_t)e >> 31);
    ntt = B3(ge, e, ntt, T_SEL);
    ps = B3((uint32_t)sh, ge, ps, T_ANDOR);
  }
  rr = (int)row;
  pos = ps;
}

// the first closure test of a flood batch comes after this many sweeps (from then on every sweep is followed by its test).
// 19x19: after down + up - 2.03 sweeps up to the weak closure instead of 3.00; 26 % of the batches then have an unsettled
// lane, open in the ONE direction the last sweep did not close, and run on for 1.07 sweeps (flood_jobs resumes in place): 2.31
// sweeps per batch in all against 3.02, 1.204 -> 1.154 ms per launch of 65 536 games x 256 plies (tools/exp/r5_sweeps.py,
// profiles/r12_sweeps.txt).  9x9 and 13x13 keep the test after down + up + down (the early test measured -1.5 % / -3 % there
// in round 6) and their restart form, flood_jobs_restart.  (A/B builds: -DGG_AB_FLOODK=3 for the three-sweep schedule at 19x19.)
template <int R>
constexpr int flood_first_test() {
#ifdef GG_AB_FLOODK
  return R == 19 ? GG_AB_FLOODK : 3;
#else
  return R == 19 ? 2 : 3;
#endif
}

#ifdef GG_AB_SWEEPS
// A/B builds only (make ab EXTRA=-DGG_AB_SWEEPS, tools/exp/r5_sweeps.py), per flood batch of k_rollout5: [0] sweeps up to the
// weak closure of the G lanes, [1] batches, [2] batches with an unsettled lane at that point, [3 .. 6] those batches by the
// sweeps they run on until no lane is unsettled (1, 2, 3, 4 or more), [7] / [8] unsettled lanes at that point that flood a
// G / an opponent group, [9] sweeps run on in all
static __device__ unsigned long long gg_sweeps5[10];
#endif

// A/B switches of round 17 (make ab EXTRA=-DGG_AB_LIBSUM=0 ...; the defaults are what measured best together, docs/history/r17.md:
// +3.0 % on the headline launch; the third alone +1.2 %, the first alone nothing):
// GG_AB_LIBSUM 1: job_liberties keeps the OR and the SUM of the liberty rows, 0: the OR and the doubly-set columns (round 8's form);
// GG_AB_PEEL 1: the first trip of flood_jobs<19> is straight-line code in front of its loop, 0: the loop alone;
// GG_AB_PRIO 1: the wave's priority is lowered directly in front of the flood, 0: in front of the job set-up (gg_v5_kernel.h).
#ifndef GG_AB_LIBSUM
#define GG_AB_LIBSUM 1
#endif
#ifndef GG_AB_PEEL
#define GG_AB_PEEL 1
#endif
#ifndef GG_AB_PRIO
#define GG_AB_PRIO 1
#endif
// A/B switches of round 19, the hand-over behind the flood (gg_v5_kernel.h; docs/history/r19.md; 0 = round 17's code):
// GG_AB_HAND1 1 (shipped: +1.8 % to +2.0 % on the headline launch): G leaves its lane by the same ds_or_b64 row pairs as a collected
//   opponent group, one region under one exec mask, 0: G by ds_write_b128 in a region of its own;
// GG_AB_PRIO_HAND 1: the wave's priority is raised again directly behind the flood and its liberties, inside the job loop, 0 (shipped):
//   behind the loop.  On top of GG_AB_HAND1 its medians were +0.1 %, +0.6 % and +1.0 % in three alternations, never every run above
//   every run without it: not shipped.
#ifndef GG_AB_PRIO_HAND
#define GG_AB_PRIO_HAND 0
#endif
#ifndef GG_AB_HAND1
#define GG_AB_HAND1 1
#endif

// A/B switch of round 20, the move inside the ply (gg_v5_kernel.h, phases 1 / 2a / 2b / 3; docs/history/r20.md; 0 = round 19's code):
// GG_AB_MOVE_RC 1 (shipped: +1.7 % on the headline launch): the move travels through the ply as (row << 5) | column and a job
//   descriptor carries its seed that way in bits 5-14; the flat index is formed once by one v_mad_u32_u24, for last_actions and the
//   pass / idle tests, 0: the flat index travels, and phases 2a and 3 and every job lane divide it by N again (split_action).
// (The round's other part, phase 2a's neighbour rows read in phase 1 ahead of its stores, did not pay - +0.7 % alone, +0.2 % on top
// of this one, neither told apart from the run-to-run spread - and is not in the source.)
#ifndef GG_AB_MOVE_RC
#define GG_AB_MOVE_RC 1
#endif

// A/B switches of round 27, the per-ply bookkeeping of the main path (gg_v5_kernel.h, flood_jobs below; docs/history/r27.md; 0 = round
// 20's code, line for line).  Shipped: all four together, +3.2 % and +3.7 % on the headline launch in two alternations, every run above
// every run of the parent; singly each is inside the parent's spread, and leaving one out of the four costs 0.8 % to 2.0 % on the medians.
// GG_AB_LANE1 1: the lane number and everything that depends on it alone - board, lane of the pair, first row, the lane-dependent row
//   of full[], the LDS addresses of the board's planes, blocks, info and meta words and of the job lane's seed block - are formed once
//   in front of the ply loop; the plane of the mover is a select between two kept addresses, not a multiply.  19x19 only (187 -> 202 of
//   the 256 VGPRs two waves per SIMD allow; 13x13 and 9x9 have no register to spare for it), 0: a fresh v_mbcnt every ply and every
//   address re-derived from it;
// GG_AB_BALLOT1 1: the hot wave-wide tests are ONE compare of masked words, whose lane mask is the test's result, 0: a bool put
//   together from several tests, which the compiler materialises as v_cndmask 0 / 1 and compares with zero again (two VALU and one more
//   VALU -> SALU dependency per test; __builtin_amdgcn_ballot_w64 of such a bool compiles to the same pair);
// GG_AB_FLAT1 1: the small stores of the main path run under the full exec mask - both lanes of a pair clear the board's info word,
//   phase 1 ORs the new stone (or zero) into the mover's plane and into the cleared G block, phase 3 stores the board's meta words
//   through an address that is the board's or, for a board that does not move, a dump word's (Lds5::kDumpMeta); the hand-over forms
//   its block offset and info word by selects in front of its one region.  19x19 only (at 13x13 and 9x9 it costs the byte-plane kernels
//   the two VGPRs they stand below three and four waves per SIMD), 0: one exec region per store;
// GG_AB_TURN1 1: the first visit of a sweep of flood_jobs directly behind the opposite sweep - the row that sweep has just run-filled
//   in both directions, no vertical input - is the bit-order flip alone (one v_bfrev instead of the visit's six), 0: the full visit.
// GG_AB_PRIO_HAND (round 19's switch) on top of the four: -0.6 % on the median, stays 0.
#ifndef GG_AB_LANE1
#define GG_AB_LANE1 1
#endif
#ifndef GG_AB_BALLOT1
#define GG_AB_BALLOT1 1
#endif
#ifndef GG_AB_FLAT1
#define GG_AB_FLAT1 1
#endif
#ifndef GG_AB_TURN1
#define GG_AB_TURN1 1
#endif
// A/B switches of round 29, the job loop's bookkeeping and phase 3's padding (gg_v5_kernel.h; docs/history/r29.md; both at 0 = round 27's
// code, line for line).  Both are in force at 19x19 only: 13x13 and 9x9 keep round 20's machine code and their LDS size.
// GG_AB_MPLANE1 1 (shipped: +1.4 % and +1.6 % on the headline launch in two alternations, every run above every run of the parent): the
//   rows of M of every board stand in an LDS plane [kNB5][RS] (Lds5::kMpl) behind the ply loop's blocks - written once behind the load,
//   zeroed by the reset path, rewritten by the board lanes at the end of phase 3 (flat, five row pairs a lane) - and a job lane reads
//   the rows of its board's M beside its stone rows, in their wait group (four ds_read_b128 and one ds_read_b96), 0: nineteen
//   ds_bpermute_b32 out of the board lanes' registers.  19 472 -> 20 016 B of LDS, of the 20 480 two waves per SIMD leave a wave;
// GG_AB_SHL1 1: the atari-join of phase 3 forms the shl1 of all its rows in front of the rows' chains (seeds: of cap[], a trip: of the
//   f[] it starts from), so that no consumer directly follows its inline-asm add and the compiler pads none of them with s_nop 0
//   (18 s_nop and no other instruction fewer in the listing), 0 (shipped): each add directly in front of the v_bitop3 that takes it.
//   Alone it measured 0.6 % and 0.7 % BELOW the parent on the medians, on top of GG_AB_MPLANE1 0.6 % and 0.8 % below it: stays 0.
// (The round's third part, res[] of flood_jobs in two-element vectors so that the hand-over's ds_or_b64 take register pairs as they
// are, took eight of the hand-over's ten v_mov_b32 out and put twenty-five into the flood's tests, at 221 VGPRs: not in the source.)
#ifndef GG_AB_SHL1
#define GG_AB_SHL1 0
#endif
// A/B switches of round 32, the mask rows and the draw counter of phases 1 and 3 (gg_v5_kernel.h; docs/history/r32.md; all at 0 = round
// 29's code, line for line).  All are in force at 19x19 only: 13x13 and 9x9 keep round 20's machine code.  Shipped: VALID1 and DRAWADD1
// together, +2.0 % and +2.4 % on the headline launch in two alternations, every run above every run of the parent; VALID1 alone +2.0 % on
// both medians with one run of twelve inside the parent's spread, DRAWADD1 alone +0.1 % and +0.6 %, not told apart from the spread;
// ALLMOVE1 alone is inside the spread and on top of the other two it LOWERS the median both times (-0.3 %, -0.4 %): it stays 0.
// GG_AB_VALID1 1 (shipped): a lane carries the VALID points of its rows (full & ~invalid) from the load to the write-back - the load converts once,
//   the write-back forms full & ~valid once, so the stored words are what they were - and phase 1 draws from the carried rows as they
//   are; the register part of the reset path (wave-uniform, known from the flag word) stands in front of the draw and sets the rows
//   of a board being reset to full[] and its M to zero, its LDS clears with it (ahead of the policies' stone reads and of phase 1's
//   stone store; the policy sets keep their & ~rm); phase 3 forms valid = (h3 | dn) & e in two v_bitop3 a row (e lies inside full) and
//   ko clears its bit, 0: the invalid rows travel, phase 1 turns every row round (ten v_bitop3) and phase 3 takes three a row;
// GG_AB_ALLMOVE1 1: when every lane's board moves (GG_BALLOT5(!moves_now) == 0: every full wave of live games) phase 3 assigns the new
//   mask rows; otherwise - absent slots of a short wave, frozen boards - it selects as before, 0 (shipped): the select on every
//   wave-ply (1: the compiler keeps two copies of the rows' last loop behind a scalar test and a branch);
// GG_AB_DRAWADD1 1 (shipped): the pre-mix counter of the draw is a running 64-bit value that starts at x0 + t5 c and is advanced by 2 c behind each
//   mix (one add-with-carry pair), 0: x0 + (t + t5) c by a 32 x 64 multiply every second ply.
// (The round's fourth part, no row copy of M between the atari-join's branch and the mask rule, was built in round 35: GG_AB_MINPLACE1.)
#ifndef GG_AB_VALID1
#define GG_AB_VALID1 1
#endif
#ifndef GG_AB_ALLMOVE1
#define GG_AB_ALLMOVE1 0
#endif
#ifndef GG_AB_DRAWADD1
#define GG_AB_DRAWADD1 1
#endif
// A/B switches of round 35, leftover copies and recomputed rows of the 19x19 ply (gg_v5_kernel.h, job_liberties / flood_jobs below;
// docs/history/r35.md; all at 0 = round 32's code, line for line).  All are in force at 19x19 only: 13x13 and 9x9 keep round 20's machine
// code.  Shipped: EMPTY1 and MINPLACE1 together, +1.2 % and +1.5 % on the headline launch in two alternations, every run above every run of
// the parent; each alone +0.6 % on the medians, inside the parent's spread; DESC1 and DRAWC1 on top of the pair LOWER its median both
// times (-0.3 % to -0.7 %) and stay 0.
// GG_AB_EMPTY1 1 (shipped): the job set-up of phase 2b overwrites ot[r] - the other colour's rows, which nothing inside flood_jobs uses but
//   the liberties - with the EMPTY row FULLROW & ~(ot[r] | m[r]), and job_liberties takes that array as it is: nineteen v_bitop3 fewer in
//   every liberties pass of a batch after its first, none more on the straight path (the set-up pays what the first pass loses), the same
//   registers, 0: every pass forms the empty rows again;
// GG_AB_MINPLACE1 1 (shipped): the atari-join of phase 3 leaves M alone - its fill (the seeds when no trip is run, zero on a wave-ply
//   without a capture) is a row set of its own that the mask rule ORs in, in the same two v_bitop3 a row: u = (M | fill) & ~all4, then
//   G | u or u & ~G by gsel (the fill lies inside the mover's stones outside M and G) - so M is the same registers on every path to the
//   rule: the ten v_mov_b32 that copied it in front of the join's wave-uniform branch and the ten v_or_b32 behind its loop are gone,
//   0: the fill is ORed into M behind the loop;
// GG_AB_DESC1 1: a job descriptor carries its board's row offset, board * RS (<= 620), in bits 21-30 - the board lane holds the word
//   as a kept constant - and the job lane reaches the stone planes, the plane of M and the G blocks by a shift (a lane without a job
//   reads the zero descriptor of the absent job, not the dump slot's), 0 (shipped): by board * RS again (three v_mul_u32_u24 in the
//   set-up and a v_mad_u32_u24 in the hand-over);
// GG_AB_DRAWC1 1 (needs GG_AB_DRAWADD1): the running draw counter starts one c further on, at x0 + (t5 + 1) c, and the mix takes it as
//   it is, 0 (shipped): the mix adds c to a copy (one add-with-carry pair every second ply).
#ifndef GG_AB_EMPTY1
#define GG_AB_EMPTY1 1
#endif
#ifndef GG_AB_MINPLACE1
#define GG_AB_MINPLACE1 1
#endif
#ifndef GG_AB_DESC1
#define GG_AB_DESC1 0
#endif
#ifndef GG_AB_DRAWC1
#define GG_AB_DRAWC1 0
#endif
#if GG_AB_BALLOT1
// (used where a board size R is in scope; 13x13 and 9x9 keep __ballot and with it round 20's machine code)
#define GG_BALLOT5(p) (R == 19 ? (unsigned long long)__builtin_amdgcn_ballot_w64(p) : __ballot(p))
#else
#define GG_BALLOT5(p) __ballot(p)
#endif

// the mix of splitmix_next (gg_common.h) alone, for a counter that is advanced already (-DGG_AB_DRAWC1=1)
__device__ __forceinline__ uint64_t splitmix_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// liberties (dilate & empty) of the group gt[], SATURATED: min(count, 2) - all any caller uses; m[] = the rows of its colour,
// ot[] = the other colour's rows (read from LDS together with m[], BEFORE the flood: read behind it they cost the lane a round
// trip).  Nothing is counted: o = the OR of the liberty rows, S = their integer SUM (R rows below 2^R: no carry leaves the
// word).  S - o = the sum over the columns c of (n_c - [n_c > 0]) 2^c, n_c = the rows that hold a liberty in column c: zero iff
// no column is set in two rows, and S >= o >= the lowest bit of o.  So there are two or more liberties iff a column is set twice
// (S != o) or o has two bits - in one test, iff S != o & -o.  Five instructions a row: four form the liberty row, and one
// v_or3_b32 and one v_add3_u32 take in two rows each.  Three chains over the row pairs p % 3 (for an odd R row 0 starts chain 0
// for nothing), joined by one v_or3 / v_add3.  (Round 8 kept o and the doubly-set columns, one v_bitop3 a row each: six a row
// and a majority to join the chains; counting took nineteen v_bcnt.)
// (EMPTY, -DGG_AB_EMPTY1=1 at 19x19: ot[] holds the EMPTY rows of the board already, formed once by the job set-up, and m[] is not read)
template <int R, bool EMPTY = false>
__device__ __forceinline__ uint32_t job_liberties(const uint32_t (&gt)[R], const uint32_t (&ot)[R], const uint32_t (&m)[R]) {
  constexpr uint32_t FULLROW = (1u << R) - 1u;
  static_assert(R < 27, "the sum of R rows below 2^R stays inside 32 bits");
  auto row = [&](int r) -> uint32_t {
    const uint32_t e = EMPTY ? ot[r] : B3(ot[r], m[r], FULLROW, ~(TA | TB) & TC & 0xFF);   // empty points
    const uint32_t up = r > 0 ? gt[r - 1] : 0u, dn = r + 1 < R ? gt[r + 1] : 0u;
    const uint32_t dd = B3(shl1(gt[r]), gt[r] >> 1, up, T_OR3);
    return B3(dd, dn, e, (TA | TB) & TC);
  };
#if GG_AB_LIBSUM
  uint32_t o3[3] = {0u, 0u, 0u}, s3[3] = {0u, 0u, 0u};
  if (R & 1) o3[0] = s3[0] = row(0);
#pragma unroll
  for (int r = R & 1; r < R; r += 2) {
    const int c = (r / 2) % 3;
    const uint32_t la = row(r), lb = row(r + 1);
    o3[c] = la | lb | o3[c];   // v_or3_b32
    s3[c] = la + lb + s3[c];   // v_add3_u32
  }
  const uint32_t o = o3[0] | o3[1] | o3[2], s = s3[0] + s3[1] + s3[2];
  const uint32_t two = B3(o, 0u - o, s, (TA & TB) ^ TC);   // (o & -o) ^ S
#else
  uint32_t o3[3] = {0u, 0u, 0u}, d3[3] = {0u, 0u, 0u};
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t l = row(r);
    d3[r % 3] = B3(l, o3[r % 3], d3[r % 3], T_ANDOR);
    o3[r % 3] = B3(l, o3[r % 3], 0u, T_OR3);
  }
  const uint32_t o = B3(o3[0], o3[1], o3[2], T_OR3);
  const uint32_t d = B3(d3[0], d3[1], d3[2], T_OR3) | B3(o3[0], o3[1], o3[2], T_MAJ);
  const uint32_t two = B3(o - 1u, o, d, T_ANDOR);   // o & (o - 1) | d
#endif
  return (o != 0u ? 1u : 0u) + (two != 0u ? 1u : 0u);
}

// The 9x9 and 13x13 form of the batch (flood_jobs below is the 19x19 one; with the SAME schedule the one-loop form measured
// 2.3 % slower than this one at 19x19, and these sizes keep the three-sweep schedule: docs/history/r12.md): a first call with WEAK and need = the G lanes, the
// liberties, and for the lanes left unsettled a second call from the re-encoded fill.
// flood2_serial (gg_common.h; seeds with their odd rows bit-reversed) for a batch of JOBS of which only some need a fixed
// point: the sweeps go on while a lane with `need` is open.  WEAK: such a lane counts as open only where the fill could still
// grow into a stone that is NOT in `mm` (the rows of M, the stones whose group had >= 2 liberties before the move).  res[] =
// the fill as the last closure test saw it, normal bit order; `open` = what that test found for this lane (0: its fill is
// closed).  A lane whose flood is cut short holds a PART of its group - every liberty of the part is a liberty of the group.
template <int R, bool WEAK>
__device__ __forceinline__ void flood_jobs_restart(const uint32_t (&m)[R], const uint32_t (&mrev)[R], uint32_t (&f)[R], uint32_t (&res)[R],
                                           bool need, const uint32_t (&mm)[R], uint32_t &open) {
  int sweeps = 0;
#pragma unroll 1
  for (int it = 0; it < R * R; ++it) {
#pragma unroll
    for (int r = 0; r < R; ++r) FLOOD_VISIT(r, r - 1, (r & 1) != 0);       // down: domain (r&1) -> ((r+1)&1)
    if (it > 0) {
      uint32_t op = 0, opw = 0, pend = 0, above = 0;
#pragma unroll
      for (int r = R - 1; r >= 0; --r) {
        const uint32_t g = ((r + 1) & 1) ? __brev(f[r]) : f[r];
        res[r] = g;
        if (r < R - 1) {
          const uint32_t t = B3(above, m[r], g, T_AND_ANDN);   // a filled stone below a fillable, unfilled one
          if (WEAK) { op |= t; opw = B3(t, mm[r], opw, (TA & ~TB & 0xFF) | TC); }
          else or_pairs(op, pend, (R - 2 - r) & 1, t);
        }
        above = g;
      }
      if (!WEAK && ((R - 1) & 1)) op |= pend;
      open = op;
      if (GG_BALLOT5((WEAK ? opw : op) != 0 && need) == 0) { sweeps = 2 * it + 1; break; }
    }
#pragma unroll
    for (int r = R - 1; r >= 0; --r) FLOOD_VISIT(r, r + 1, ((r + 1) & 1) != 0);  // up: domain ((r+1)&1) -> (r&1)
    if (it > 0) {   // (a first test already after the second sweep: 2.23 sweeps per batch, but 27 % of the batches then have a lane to flood on: 1.351 -> 1.385 ms)
      uint32_t op = 0, opw = 0, pend = 0, below = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t g = (r & 1) ? __brev(f[r]) : f[r];
        res[r] = g;
        if (r > 0) {
          const uint32_t t = B3(below, m[r], g, T_AND_ANDN);
          if (WEAK) { op |= t; opw = B3(t, mm[r], opw, (TA & ~TB & 0xFF) | TC); }
          else or_pairs(op, pend, (r - 1) & 1, t);
        }
        below = g;
      }
      if (!WEAK && ((R - 1) & 1)) op |= pend;
      open = op;
      if (GG_BALLOT5((WEAK ? opw : op) != 0 && need) == 0) { sweeps = 2 * it + 2; break; }
    }
  }
  (void)sweeps;
}

// flood2_serial (gg_common.h; seeds with their odd rows bit-reversed) for a batch of JOBS of which only some need a fixed
// point, from the seeds to the liberty counts: returns min(liberties, 2) of res[] = the fill as the last closure test saw
// it, normal bit order.  A lane whose flood is cut short holds a PART of its group - every liberty of the part is a liberty
// of the group.  One loop, sweeps alternately down and up, the fill in f[] in the alternating bit order from the first
// sweep to the last (a test reads f[], it never writes it); from sweep flood_first_test<R>() on every sweep is followed by
// its closure test (after a down sweep only upwards, after an up sweep only downwards):
//  * until the lanes with isG are WEAKLY closed - open only where the fill could still grow into a stone that is NOT in mm
//    (the rows of M, the stones whose group had >= 2 liberties before the move) - a test ends there;
//  * then the liberties of every lane's part are taken, and a lane that is open (in the strong sense, G or not) with fewer
//    than two of them is UNSETTLED: its group may be captured or leave M, its full extent matters.  While there is one, the
//    loop goes on in place - the next sweep of the alternation, its test, the liberties again.  Such a lane is open in the one
//    direction the last sweep did not close: one more sweep settles nearly all of them.
// What becomes of the lanes that were settled while others sweep on: nothing is masked and nothing latched - every lane
// sweeps, and res[] / the count are those of the LAST test for all of them (as the restart this replaces recomputed them
// for every lane).  That is exact because being settled is monotone in the fill and what a settled lane hands on does not
// depend on how far its fill got: a closed fill is a fixed point of a sweep; a part with two liberties keeps them as it
// grows (the count is saturated), and then an opponent lane hands on nothing at all while a G lane hands on a part of G
// that holds all of G's stones outside M - the weak closure, which further growth through stones of M cannot undo (a group
// outside M hangs on q stone by stone, never behind a group of M) - and phase 3 only ORs it into M.  The same holds for
// the lanes of a batch that merely wait for its slowest flood, with this schedule as with any other.
template <int R>
__device__ __forceinline__ uint32_t flood_jobs(const uint32_t (&m)[R], const uint32_t (&mrev)[R], uint32_t (&f)[R], uint32_t (&res)[R],
                                               const uint32_t (&ot)[R], const uint32_t (&mm)[R], bool isG, bool have) {
  constexpr int K = flood_first_test<R>();
  static_assert(K >= 1 && K <= 3, "the first closure test comes after one, two or three sweeps");
  constexpr bool EMPTY = GG_AB_EMPTY1 != 0 && R == 19;   // (ot[] = the empty rows of the board: the set-up of phase 2b, gg_v5_kernel.h)
  uint32_t cnt = 0;
  bool resumed = false;   // (wave-uniform) the G lanes are weakly closed: every test from here on is followed by the liberties
#ifdef GG_AB_SWEEPS
  int sw_ = 0, sw0_ = 0;
  uint32_t ng_ = 0, no_ = 0;
#define GG_SW5_SWEEP() (++sw_)
#else
#define GG_SW5_SWEEP() ((void)0)
#endif
  // after a test (op / opw = where this lane is open / weakly open): is the batch done?
#if GG_AB_BALLOT1
  // (once per batch: the tests AND words and their one compare is the mask; through an empty asm, or the compiler turns the AND of a
  // mask word back into the AND of two tests)
  uint32_t gm = isG ? ~0u : 0u, hm = have ? ~0u : 0u;
  asm volatile("" : "+v"(gm), "+v"(hm));
#endif
  auto done = [&](uint32_t op, uint32_t opw) -> bool {
#if GG_AB_BALLOT1
    if (!resumed && GG_BALLOT5((opw & gm) != 0u) != 0) return false;
    cnt = job_liberties<R, EMPTY>(res, ot, m);
    // (cnt <= 2: cnt - 2 is negative iff cnt < 2)
    const bool unsettled = B3(op, hm, (uint32_t)((int32_t)(cnt - 2u) >> 31), TA & TB & TC) != 0u;
#else
    if (!resumed && GG_BALLOT5(opw != 0u && isG) != 0) return false;
    cnt = job_liberties<R, EMPTY>(res, ot, m);
    const bool unsettled = have && op != 0u && cnt < 2u;
#endif
    const uint64_t u = GG_BALLOT5(unsettled);
#ifdef GG_AB_SWEEPS
    if (!resumed) { sw0_ = sw_; ng_ = (uint32_t)__popcll(GG_BALLOT5(unsettled && isG)); no_ = (uint32_t)__popcll(u) - ng_; }
#endif
    resumed = true;
    return u == 0;
  };
  // turn (-DGG_AB_TURN1=1): the sweep comes directly behind the opposite one, whose last visit left this sweep's first row run-filled
  // in both directions - the fill of a row is whole runs of m[] there - and in the bit order that visit ends in.  The first visit has
  // no vertical input (NB is off the board), its two carry fills add nothing to whole runs, and what is left of it is the flip.
  auto sweep_down = [&](bool turn) {   // domain (r&1) -> ((r+1)&1)
    if (turn) f[0] = __brev(f[0]);
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (!(turn && r == 0)) FLOOD_VISIT(r, r - 1, (r & 1) != 0);
    GG_SW5_SWEEP();
  };
  auto sweep_up = [&](bool turn) {     // domain ((r+1)&1) -> (r&1)
    if (turn) f[R - 1] = __brev(f[R - 1]);
#pragma unroll
    for (int r = R - 1; r >= 0; --r)
      if (!(turn && r == R - 1)) FLOOD_VISIT(r, r + 1, ((r + 1) & 1) != 0);
    GG_SW5_SWEEP();
  };
  // the test after a down sweep (is the fill closed UPWARDS?) and after an up sweep (downwards), with what follows it
  auto done_after_down = [&]() -> bool {
    uint32_t op = 0, opw = 0, above = 0;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
      const uint32_t g = ((r + 1) & 1) ? __brev(f[r]) : f[r];
      res[r] = g;
      if (r < R - 1) {
        const uint32_t t = B3(above, m[r], g, T_AND_ANDN);   // a filled stone below a fillable, unfilled one
        op |= t;
        opw = B3(t, mm[r], opw, (TA & ~TB & 0xFF) | TC);
      }
      above = g;
    }
    return done(op, opw);
  };
  auto done_after_up = [&]() -> bool {
    uint32_t op = 0, opw = 0, below = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t g = (r & 1) ? __brev(f[r]) : f[r];
      res[r] = g;
      if (r > 0) {
        const uint32_t t = B3(below, m[r], g, T_AND_ANDN);
        op |= t;
        opw = B3(t, mm[r], opw, (TA & ~TB & 0xFF) | TC);
      }
      below = g;
    }
    return done(op, opw);
  };
  // The first trip with the test after down + up (K == 2), peeled out of the loop as straight-line code: 74 % of the batches end
  // here (profiles/r12_sweeps.txt).  The others enter the loop at its next down sweep with the fill, res[], cnt and `resumed` as
  // the loop itself would have them there; from then on every sweep has its test.
  constexpr bool PEEL = GG_AB_PEEL != 0 && K == 2;
  bool fin = false;
  constexpr bool TURN = GG_AB_TURN1 != 0;   // (the very first down sweep starts from the seed: it keeps its row-0 visit)
  if constexpr (PEEL) {
    sweep_down(false);
    sweep_up(TURN);
    fin = done_after_up();
  }
  if (!fin) {
#pragma unroll 1
    for (int it = PEEL ? 1 : 0; it < R * R; ++it) {
      sweep_down(TURN && PEEL);   // (without the peeled trip the loop's first down sweep is the first of all)
      if ((PEEL || K <= 1 || it > 0) && done_after_down()) break;
      sweep_up(TURN);
      if ((PEEL || K <= 2 || it > 0) && done_after_up()) break;
    }
  }
#undef GG_SW5_SWEEP
#ifdef GG_AB_SWEEPS
  { int l_; asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l_));
    if (l_ == 0) {
      const int ex_ = sw_ - sw0_;
      atomicAdd(&gg_sweeps5[0], (unsigned long long)sw0_); atomicAdd(&gg_sweeps5[1], 1ull);
      if (ng_ + no_) { atomicAdd(&gg_sweeps5[2], 1ull); atomicAdd(&gg_sweeps5[2 + (ex_ < 4 ? ex_ : 4)], 1ull); }
      atomicAdd(&gg_sweeps5[7], (unsigned long long)ng_); atomicAdd(&gg_sweeps5[8], (unsigned long long)no_);
      atomicAdd(&gg_sweeps5[9], (unsigned long long)ex_);
    } }
#endif
  return cnt;
}

#ifdef GG_AB_P3
// A/B builds only (make ab EXTRA=-DGG_AB_P3, tools/exp/r5_p3_counts.py): the wave-plies that take each wave-wide branch of
// phase 3 and the trip count of the atari-join, counted in registers (the branches are wave-uniform) and added up once per group
// of boards.  [0] wave-plies, [1] capt_m, [2] ncapn == 1 && libsG == 0, [3] ko1, [4] anya && capt_m (the branch in front of the
// atari-join's seeds up to round 7; gone since, always 0), [5] anyf, [6] atari-join trips, [7] the most trips of one wave-ply
// (max), [8] boards that capture, [9] boards that move
static __device__ unsigned long long gg_p3[10];
#define GG_P3(k, n) (p3c_[k] += (n))
#else
#define GG_P3(k, n) ((void)0)
#endif
#ifdef GG_AB_MARK
#define GG_MARK(k) asm volatile("; GGMARK " #k ::: "memory")   // phase-3 branch bodies in the listing (tools/exp/r5_p3_mix.py)
#else
#define GG_MARK(k) do {} while (0)
#endif
#if defined(GG_AB_P3) || defined(GG_AB_LIVE)
// A/B builds with -DGG_AB_LIVE (or the -DGG_AB_P3 counter build) only: boards whose live plies were not a prefix of the launch or
// whose played count is not their number of draws.  Its own switch, not every GG_AB build: the per-ply bookkeeping sits in phase 1
// and would skew the phase clocks (-DGG_AB_PROF) of one side of an A/B comparison.
#define GG_LIVE_CHECK 1
static __device__ unsigned long long gg_live_bad;
#endif

#ifdef GG_AB_MCHECK
// A/B builds only (make ab EXTRA=-DGG_AB_MCHECK, tools/exp/r5_mplane_check.py): [0] rows of M a job lane of k_rollout5<19, ..> read out of
// the plane of M (-DGG_AB_MPLANE1=1) that differ from the row the board's lanes hold in their registers, fetched by the ds_bpermute of
// the other setting as well; [1] rows compared.  No result depends on the plane unless a flood batch ends early, which the parity tests
// see only in rare positions: this counter is the direct check that plane and registers are the same.
static __device__ unsigned long long gg_mcheck[2];
#endif
#ifdef GG_AB_WS
// A/B builds only (make ab EXTRA=-DGG_AB_WS, tools/exp/r5_ws_counts.py): the pairs of boards of workspace launches whose analysis
// the load skipped ([0]: both boards stand in the workspace stone for stone) and the pairs it analysed ([1]), counted in registers
// (the branch is wave-uniform) and added up once per group of boards
static __device__ unsigned long long gg_wsc[2];
#define GG_WSC_DECL uint32_t wsc_[2] = {0u, 0u}
#define GG_WSC(hit) (wsc_[(hit) ? 0 : 1] += 1u)
#define GG_WSC_FLUSH do { if (ws && ln0 == 0) { atomicAdd(&gg_wsc[0], (unsigned long long)wsc_[0]); \
    atomicAdd(&gg_wsc[1], (unsigned long long)wsc_[1]); } } while (0)
#else
#define GG_WSC_DECL do {} while (0)
#define GG_WSC(hit) ((void)0)
#define GG_WSC_FLUSH do {} while (0)
#endif
#ifdef GG_AB_LOADSPLIT
// A/B builds only (make ab EXTRA=-DGG_AB_LOADSPLIT, tools/exp/r5_load_split.py): shader-clock time of the parts of the byte-plane
// load of k_rollout5, summed over the pairs of a wave: [0] staging + bytes -> rows, [1] the analysis (or the workspace compare),
// [2] the hand-over of the mask and M rows to the lanes that own the boards, [3] groups of boards.  LDS waits only: the next
// pair's global loads stay in flight across the marks, as in the shipped kernel.
static __device__ unsigned long long gg_lsplit[4];
#define GG_LS_DECL unsigned long long tls_[3] = {0, 0, 0}, tlc_ = clock64()
#define GG_LS(k) do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); \
    const unsigned long long n_ = clock64(); __builtin_amdgcn_sched_barrier(0); tls_[k] += n_ - tlc_; tlc_ = n_; } while (0)
#define GG_LS_START do { __builtin_amdgcn_sched_barrier(0); tlc_ = clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define GG_LS_FLUSH do { if (ln0 == 0) { for (int k_ = 0; k_ < 3; ++k_) atomicAdd(&gg_lsplit[k_], tls_[k_]); \
    atomicAdd(&gg_lsplit[3], 1ull); } } while (0)
#else
#define GG_LS_DECL do {} while (0)
#define GG_LS(k) do {} while (0)
#define GG_LS_START do {} while (0)
#define GG_LS_FLUSH do {} while (0)
#endif

// job descriptor: bits 0-4 board, 5-14 the seed ((row << 5) | column; -DGG_AB_MOVE_RC=0: 5-13, the flat point index), 15 the colour flooded, 16 the job floods G, 18 the job exists,
// 19-20 the direction of q's neighbour it starts from (0 up, 1 down, 2 left, 3 right); (-DGG_AB_DESC1=1, 19x19) 21-30 board * RS
// info word of a board (cleared in phase 1, ORed by its jobs): bits 0-3 the directions whose opponent group was captured, 4-5 the
// liberties of G (saturated at 2)
// the kernel, once per playout policy of its draw (gg_v5_kernel.h)
#define GG_R5_NAME k_rollout5
#define GG_R5_POL kPolUniform
#include "gg_v5_kernel.h"
#undef GG_R5_NAME
#undef GG_R5_POL
#define GG_R5_NAME k_rollout5_pol
#define GG_R5_POL kPolNoEyeFill
#include "gg_v5_kernel.h"
#undef GG_R5_NAME
#undef GG_R5_POL
#define GG_R5_NAME k_rollout5_tac
#define GG_R5_POL kPolTactical
#include "gg_v5_kernel.h"
#undef GG_R5_NAME
#undef GG_R5_POL
#define GG_R5_NAME k_rollout5_pat
#define GG_R5_POL kPolPattern
#include "gg_v5_kernel.h"
#undef GG_R5_NAME
#undef GG_R5_POL

}  // namespace gg
