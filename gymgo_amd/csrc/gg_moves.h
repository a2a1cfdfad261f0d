// gg_moves.h - MOVE-OUTCOME PLANES (gg_batch_move_planes, gg_batch_move_planes_tracked, gg_batch_move_counts of
// include/gymgo_amd.h): for every candidate point of the mover what playing there would do - the liberties of
// the played stone's chain afterwards, the stones the move captures, the size of that chain - as counts or as twelve 0 / 1
// planes.
//
// Layout: gg_feat.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards.
//
// Two paths fill the same accumulators (MoveAcc: per quantity the bit planes of min(value, 255), or its four class rows):
//   1. THE GROUP ROUNDS (moves_groups), feat_groups' seed-and-flood rounds, black and white side by side.  While a group's
//      stones F and liberties L are in registers: an opponent group with one liberty is filed (its stones would be captured
//      by a move on that liberty); for an own group its liberty count - 1, its size + 1 and, per point of L, the number of
//      empty neighbours of the point outside L are ORed into bit-sliced per-point numbers AT the points of L, and a
//      two-step counter (c1, c2) notes the points that are liberties of one / of two and more own groups.  After the rounds,
//      for a candidate p that captures nothing:
//        no own group next to p:   libs = the empty neighbours of p, size = 1;
//        exactly one, g:           libs = |L_g| - 1 + the empty neighbours of p outside L_g, size = |g| + 1
//      (the new chain is g and p; its liberties are L_g without p and what p brings, two disjoint sets) - bit-sliced adds over
//      the whole board at once.  The numbers filed at a point with two own groups are the OR of two numbers and are not used.
//   2. THE EXACT PATH (moves_exact), one candidate per board and round, the boards of a wave in lock-step: the captured
//      stones = the flood of (neighbours of p that are opponent stones of one-liberty groups) within those stones - such a
//      group next to the empty p has p as its liberty, and groups of one colour never touch, so one flood gives them all;
//      the chain = the flood of p within own | p; both floods run as one pair (plane_move_flood of gg_planes.h, which the
//      move hashes share).  libs = the points of
//      dilate(chain) & (empty | captured) without p; the three numbers are three 10-bit fields of one board sum.
//      Candidates that capture, or that join two and more own groups, come here - with -DGG_AB_MOVES_EXACT=1 (make ab) every
//      candidate does, and feat_groups files the one-liberty groups.
// Every loop is bounded: a group round takes a stone off some board, an exact round a candidate.
// EMISSION: planes - k_life's (plane_emit of gg_planes.h); counts - k_group_liberties' (LDS bytes, stage_out).
#pragma once
#include "gg_feat.h"

#ifndef GG_AB_MOVES_EXACT
#define GG_AB_MOVES_EXACT 0
#endif

namespace gg {

constexpr int kMovePlanes = 12;   // libs 1 / 2 / 3 / >= 4, captured 1 / 2 / 3 / >= 4, self-atari by size 1 / 2 / 3 / >= 4
constexpr int kMoveCounts = 3;    // libs, captured, size

template <int R>
struct Moves {
  using Pl = Planes<R>;
  static constexpr int LPB = Pl::LPB, NBW = Pl::NBW, K = Pl::K;
  static constexpr int kBsWords = plane_bs_words<R>(kMovePlanes, 15);
  static constexpr int kCntWords = (NBW * kMoveCounts * R * R + 15 + 15) / 4 + 1;   // the count bytes on their way out
  static constexpr int kLdsWords = kBsWords > Pl::kIoWords ? kBsWords : Pl::kIoWords;   // (the staged input is dead by then)
  static_assert(kCntWords <= kLdsWords, "the count bytes reuse the same buffer");
  static constexpr int kNum = 9;   // bits of a per-point number: sizes and liberty counts are below 512 on 19x19
};

// What the two paths fill, per quantity (0 libs, 1 captured, 2 size): COUNTS - bit k of min(value, 255) at every point;
// else the points where the value is exactly 1 / 2 / 3 / >= 4.  A point that is never filed has value 0.
template <bool COUNTS>
struct MoveAcc {
  static constexpr int W = COUNTS ? 8 : 4;
  uint32_t v[kMoveCounts][W];
};

// file `val` - the same number in every lane of the board - at the point q (one bit in the lane of its row, or none)
template <bool COUNTS>
__device__ __forceinline__ void moves_file_value(uint32_t (&a)[MoveAcc<COUNTS>::W], uint32_t q, uint32_t val) {
  if constexpr (COUNTS) {
    const uint32_t c = val < 255u ? val : 255u;
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] |= q & (0u - ((c >> k) & 1u));
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] |= val == (uint32_t)(k + 1) ? q : 0u;
    a[3] |= val >= 4u ? q : 0u;
  }
}
// file the bit-sliced numbers b (bit k of the number of point c is bit c of b[k]) at the points m
template <bool COUNTS, int NB>
__device__ __forceinline__ void moves_file_bits(uint32_t (&a)[MoveAcc<COUNTS>::W], uint32_t m, const uint32_t (&b)[NB]) {
  if constexpr (COUNTS) {
    constexpr int LOW = NB < 8 ? NB : 8;   // (a number of fewer than eight bits does not saturate)
    uint32_t sat = 0;
#pragma unroll
    for (int k = 8; k < NB; ++k) sat |= b[k];
#pragma unroll
    for (int k = 0; k < LOW; ++k) a[k] |= m & (b[k] | sat);
  } else {
    uint32_t hi = 0;
#pragma unroll
    for (int k = 2; k < NB; ++k) hi |= b[k];
    const uint32_t lo = m & ~hi;
    a[0] |= lo & b[0] & ~b[1];
    a[1] |= lo & ~b[0] & b[1];
    a[2] |= lo & b[0] & b[1];
    a[3] |= m & hi;
  }
}

// per point the number (0 .. 4) of its four neighbours that lie in X, bit-sliced
template <int LPB>
__device__ __forceinline__ void moves_neighbours(uint32_t X, uint32_t (&s)[3]) {
  const uint32_t a = shl1(X), b = X >> 1, c = lat_above<LPB>(X), d = lat_below<LPB>(X);
  const uint32_t p0 = a ^ b, q0 = a & b, p1 = c ^ d, q1 = c & d, cy = p0 & p1;
  s[0] = p0 ^ p1;
  s[1] = q0 ^ q1 ^ cy;   // (q0 + q1 + cy <= 2: a carry needs both pairs odd)
  s[2] = q0 & q1;
}

// THE EXACT PATH: every point of `todo` (empty points of the board), one per board and round.  own: the mover's stones,
// opp1: the opponent's stones of groups with exactly one liberty, E: the empty points.
template <int R, bool COUNTS>
__device__ __forceinline__ void moves_exact(uint32_t own, uint32_t opp1, uint32_t E, uint32_t todo, MoveAcc<COUNTS> &acc) {
  constexpr int LPB = Moves<R>::LPB;
#pragma unroll 1
  for (int it = 0; it < R * R + 1; ++it) {   // (a round takes a point off every board that still has one)
    if (__ballot(todo != 0u) == 0ull) break;
    const uint32_t Q = plane_first<LPB>(todo);
    todo &= ~Q;
    uint32_t G, C;
    plane_move_flood<R, true>(own, opp1, Q, G, C);
    const uint32_t L = lat_dilate<LPB>(G) & ((E & ~Q) | C);
    const uint32_t S = lat_board_sum<LPB>((uint32_t)__popc(L) | ((uint32_t)__popc(C) << 10) | ((uint32_t)__popc(G) << 20));   // (<= 361 each)
    const uint32_t nl = S & 1023u;
    const bool suicide = nl == 0u;
    moves_file_value<COUNTS>(acc.v[0], Q, nl);
    moves_file_value<COUNTS>(acc.v[1], Q, suicide ? 0u : (S >> 10) & 1023u);
    moves_file_value<COUNTS>(acc.v[2], Q, suicide ? 0u : S >> 20);
  }
}

// THE GROUP ROUNDS and what follows from them without a flood per candidate.  bl / wh: this lane's rows (zero in rows >= N
// and on boards that are not there), white: the mover, cand: the candidate points.  Files every candidate that captures
// nothing and has at most one own group next to it; -> the candidates left for the exact path, opp1 for it.
template <int R, bool COUNTS>
__device__ __forceinline__ uint32_t moves_groups(uint32_t bl, uint32_t wh, bool white, uint32_t full, uint32_t cand,
                                                 MoveAcc<COUNTS> &acc, uint32_t &opp1) {
  using M_ = Moves<R>;
  constexpr int LPB = M_::LPB, K = M_::K, NB = M_::kNum;
  const uint32_t E = full & ~(bl | wh);
  uint32_t Mk[K], Mkr[K], Ee[K];
  plane_pair<R>(bl, wh, Mk);
  plane_pair<R>(E, E, Ee);
#pragma unroll
  for (int k = 0; k < K; ++k) Mkr[k] = __brev(Mk[k]);
  uint32_t X[K];
  plane_pair<R>(bl, wh, X);                 // the stones not yet counted
  uint32_t gl[NB], gs[NB], ex[NB], c1 = 0, c2 = 0;   // (ex: two bits in use)
#pragma unroll
  for (int k = 0; k < NB; ++k) gl[k] = gs[k] = ex[k] = 0;
  opp1 = 0;
#pragma unroll 1
  for (int it = 0; it < 2 * R * R; ++it) {   // (a round takes at least one stone off some board: the bound is never reached)
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) any |= X[k];
    if (__ballot(any != 0u) == 0ull) break;
    uint32_t F[K], Lb[K];
    plane_seeds<R>(X, F);
    lat_flood<LPB, K>(F, Mk, Mkr);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      Lb[k] = lat_dilate<LPB>(F[k]) & Ee[k];
      X[k] &= ~F[k];
    }
    const uint32_t fb = plane_field<R>(F, 0), fw = plane_field<R>(F, 1), lb = plane_field<R>(Lb, 0), lw = plane_field<R>(Lb, 1);
    const uint32_t fo = white ? fw : fb, fp = white ? fb : fw, lo = white ? lw : lb, lp = white ? lb : lw;
    // the mover's group: liberties and stones; the opponent's: liberties (a lane's share saturated at 2: the sum says 0, 1, more)
    const uint32_t plp = (uint32_t)__popc(lp);
    const uint32_t S = lat_board_sum<LPB>((uint32_t)__popc(lo) | ((uint32_t)__popc(fo) << 10) | ((plp < 2u ? plp : 2u) << 20));
    const uint32_t no = S & 1023u, so = (S >> 10) & 1023u, np = S >> 20;
    opp1 |= np == 1u ? fp : 0u;
    c2 |= c1 & lo;
    c1 |= lo;
    const uint32_t nm = no - 1u, sz = so + 1u;   // (no >= 1 wherever lo has a point)
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      gl[k] |= lo & (0u - ((nm >> k) & 1u));
      gs[k] |= lo & (0u - ((sz >> k) & 1u));
    }
    uint32_t s[3];
    moves_neighbours<LPB>(E & ~lo, s);        // (a liberty has a stone next to it: at most three, s[2] is clear there)
    ex[0] |= lo & s[0];
    ex[1] |= lo & s[1];
  }
  const uint32_t own = white ? wh : bl;
  const uint32_t caps = lat_dilate<LPB>(opp1);
  const uint32_t quiet = cand & ~caps;
  // no own group next to the point: its empty neighbours, a chain of one
  {
    uint32_t s[3];
    moves_neighbours<LPB>(E, s);
    const uint32_t m = quiet & ~c1;
    moves_file_bits<COUNTS, 3>(acc.v[0], m, s);
    acc.v[2][0] |= m & (s[0] | s[1] | s[2]);   // size 1 (bit 0 of the count, class "1") unless the move is a suicide
  }
  // exactly one: (|L| - 1) + the empty neighbours outside L, bit-sliced; |g| + 1
  {
    uint32_t sum[NB], cy = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      sum[k] = gl[k] ^ ex[k] ^ cy;
      cy = (gl[k] & ex[k]) | (cy & (gl[k] ^ ex[k]));
      nz |= sum[k];
    }
    const uint32_t m = quiet & c1 & ~c2;
    moves_file_bits<COUNTS, NB>(acc.v[0], m, sum);
    moves_file_bits<COUNTS, NB>(acc.v[2], m & nz, gs);
  }
  return cand & (caps | c2);
}

// gg_batch_move_planes / gg_batch_move_planes_tracked (COUNTS = false): out [B][12][N][N] of elements of 1 << esh bytes
// (`one`: the bit pattern of 1), aligned to its element; orient int32 [B] or null (feat_orient on the loaded rows).
// gg_batch_move_counts (COUNTS = true, byte planes): out uint8 [B][3][N][N].  One single-wave workgroup per NBW boards
// (grid-stride).
template <int R, bool TRACKED, bool COUNTS>
__global__ __launch_bounds__(kWave) void k_moves(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                 uint8_t *__restrict__ out, int esh, uint32_t one, int64_t B, int N) {
  using M_ = Moves<R>;
  constexpr int LPB = M_::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[M_::kLdsWords];
  PlaneFrame<R> f(N);
  const int P = N * N;
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, orient, f, B, N, lds, bl, wh, inv, fl);
    const bool white = (fl & 1u) != 0, over = (fl & 4u) != 0;
    const uint32_t own = white ? wh : bl, opp = white ? bl : wh;
    const uint32_t E = f.full & ~(bl | wh);
    const uint32_t cand = over ? 0u : (E & ~inv);   // plane 10 of the feature planes
    MoveAcc<COUNTS> acc;
#pragma unroll
    for (int q = 0; q < kMoveCounts; ++q)
#pragma unroll
      for (int k = 0; k < MoveAcc<COUNTS>::W; ++k) acc.v[q][k] = 0;
    uint32_t opp1, todo;
#if GG_AB_MOVES_EXACT
    {
      uint32_t cls[4];
      feat_groups<R, false>(bl, wh, f.full, cls);
      opp1 = opp & cls[0];
      todo = cand;
    }
#else
    todo = moves_groups<R, COUNTS>(bl, wh, white, f.full, cand, acc, opp1);
#endif
    moves_exact<R, COUNTS>(own, opp1, E, todo, acc);
    if constexpr (COUNTS) {
      uint8_t *g0 = out + f.b_first * (int64_t)(kMoveCounts * P);
      uint8_t *lb = reinterpret_cast<uint8_t *>(lds) + ((uintptr_t)g0 & 15u);   // (stage_out: byte i of the slice at lds[mis + i])
      WAVE_SYNC();
      if (f.on && f.r < N) {
#pragma unroll
        for (int q = 0; q < kMoveCounts; ++q) {
#pragma unroll
          for (int c = 0; c < R; ++c) {
            if (c < N) {
              uint32_t v = 0;
#pragma unroll
              for (int k = 0; k < 8; ++k) v |= ((acc.v[q][k] >> c) & 1u) << k;
              lb[(f.j * kMoveCounts + q) * P + f.r * N + c] = (uint8_t)v;
            }
          }
        }
      }
      WAVE_SYNC();
      stage_out(g0, f.nb * kMoveCounts * P, reinterpret_cast<const uint8_t *>(lds), f.lane);
      WAVE_SYNC();
    } else {
      const uint32_t *l = acc.v[0], *c = acc.v[1], *s = acc.v[2];
      const uint32_t rows[kMovePlanes] = {l[0], l[1], l[2], l[3], c[0], c[1], c[2], c[3],
                                          l[0] & s[0], l[0] & s[1], l[0] & s[2], l[0] & s[3]};
      plane_emit<R, kMovePlanes>(out, esh, one, rows, lds, f, N);
    }
  }
}

}  // namespace gg
