// gg_prior.h - THE MOVE PRIORS (gg_batch_move_priors, gg_batch_move_priors_tracked, gg_uct_prior_begin, gg_uct_prior_expand of
// include/gymgo_amd_prior.h, gg_uct_prior_expand_leaves of include/gymgo_amd_uct_leaves.h): per legal point of a
// board the pair (visits, 2 wins) of virtual simulations that the sets
// of the tactical and the pattern playout policy give it - C capture points, E escape points, P pattern points, L pattern points
// next to the previous move, X the mover's own eyes -, stored per board or ADDED to the (n~, s~) pairs of a node of the RAVE tree.
//
// Layout: gg_planes.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards (grid-stride).
// The rows are k_tactics' and k_patterns': M from feat_groups, C / E from tactical_rows, the eyes from eye_row, P from pattern_row
// on padded rows - the statements of gg_common.h the rollout kernels draw from; nothing of the rule is restated here.
//
// EMISSION: a lane's row is N pairs of 8 bytes, the rows of a board are contiguous, so the pairs are staged in LDS as int32 words
// at the word offset the destination has inside its 16-byte vector, and the wave writes (TREE: reads, adds and writes) every
// aligned 16-byte vector that lies inside the destination and the up to three words at either ragged end one by one: nothing
// outside the destination is written, no atomics - a board belongs to one group of lanes of one wave.  The destination needs the
// alignment of an int32 only.
//   TREE = false: the boards of a wave are one contiguous slice of out [B][N^2][2]: ONE segment per wave, stored.
//   TREE = true:  board b goes to node y of its tree t, node_amaf + ((t (I + 1) + y) N^2) 2: one segment per board, added.
//                 t = b, or with VL (the L slots of a root and round) t = b / L.
#pragma once
#include "gg_feat.h"

namespace gg {

constexpr int kPriorTerms = 6;   // even, capture, escape, pattern, local, eye_fill: weights int32 [6][2] = (visits, wins)

template <int R>
struct Prior {
  static constexpr int LPB = Planes<R>::LPB, NBW = Planes<R>::NBW;
  static constexpr int kSegWords = (2 * R * R + 3 + 3) / 4 * 4;   // a board's pairs behind a word offset <= 3, whole vectors
  static constexpr int kOutWords = NBW * kSegWords;               // (>= the wave's contiguous slice behind its offset)
  static constexpr int kLdsWords = kOutWords > Planes<R>::kIoWords ? kOutWords : Planes<R>::kIoWords;   // (the staged input is dead by then)
};

// LDS -> HBM of one segment of nw int32 words: seg[mo + e] = word e, mo = ((uintptr_t)dst & 15) / 4.  Aligned 16-byte vectors
// for what they cover, lanes 0-3 the ragged head, lanes 4-7 the ragged tail; ADD: the words are added to what is there.
template <bool ADD>
__device__ __forceinline__ void prior_store(uint32_t *dst, const uint32_t *seg, int mo, int nw, int lane) {
  const int end = mo + nw;
  uint32_t *ga = dst - mo;
  const int v0 = mo ? 1 : 0, v1 = end >> 2;
  for (int v = v0 + lane; v < v1; v += kWave) {
    V16a x = *reinterpret_cast<const V16a *>(seg + 4 * v);
    V16a *gp = reinterpret_cast<V16a *>(ga + 4 * (int64_t)v);
    if (ADD) {
      const V16a o = *gp;
#pragma unroll
      for (int i = 0; i < 4; ++i) x.w[i] += o.w[i];
    }
    *gp = x;
  }
  int e0 = -1, estep = nw;
  if (v1 >= v0) {
    const int head = mo ? 4 - mo : 0, tail = end & 3;
    if (lane < 4) { if (lane < head) e0 = lane; }
    else if (lane < 8 && lane - 4 < tail) e0 = nw - tail + (lane - 4);
  } else {   // a segment inside one vector
    e0 = lane;
    estep = kWave;
  }
  for (int e = e0; e >= 0 && e < nw; e += estep) dst[e] = ADD ? dst[e] + seg[mo + e] : seg[mo + e];
}

// in: byte planes or tracked boards of B boards; last int32 [B] or null: the previous action of every board; weights int32 [6][2].
// TREE = false: out int32 [B][N^2][2].  TREE = true: out = node_amaf int32 [B][I + 1][N^2][2], node int32 [B] or null (node 0):
// the node of every board's tree; a board whose node is outside [0, I] is skipped, and with need_move one whose last[b] < 0.
// VL (TREE only): out = node_amaf int32 [B / L][I + 1][N^2][2], board b seeds a node of tree b / L.  The boards of a tree that
// are not skipped name different nodes - each is a node of its own, made in this round -, so no two boards add to the same words.
// L is a template switch and not a plain divisor: b / L at run time costs the one-leaf tree form a 64-bit division.
template <int R, bool TRACKED, bool TREE, bool VL = false>
__global__ __launch_bounds__(kWave) void k_move_priors(const void *__restrict__ in, const int32_t *__restrict__ last,
                                                       const int32_t *__restrict__ weights, uint32_t *__restrict__ out,
                                                       const int32_t *__restrict__ node, int need_move, int I, int64_t B, int N, int L) {
  static_assert(TREE || !VL, "the slots of a round belong to trees");
  using Q = Prior<R>;
  constexpr int LPB = Q::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Q::kLdsWords];
  PlaneFrame<R> f(N);
  const uint32_t full = f.full;
  const bool top = f.r == 0, bot = f.r == N - 1;
  const uint32_t tf = top ? full : 0u, bf = bot ? full : 0u;
  const uint32_t edge = (top || bot) ? full : (1u | (1u << (N - 1)));
  const int P = N * N;
  uint32_t wv[kPriorTerms], ws[kPriorTerms];   // visits, 2 wins: the units of (n~, s~)
#pragma unroll
  for (int k = 0; k < kPriorTerms; ++k) {
    wv[k] = (uint32_t)weights[2 * k];
    ws[k] = 2u * (uint32_t)weights[2 * k + 1];
  }
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, nullptr, f, B, N, lds, bl, wh, inv, fl);
    uint32_t cls[4];
    feat_groups<R, false>(bl, wh, full, cls);
    const bool white = (fl & 1u) != 0, done = (fl & 4u) != 0;
    const uint32_t me = white ? wh : bl, op = white ? bl : wh;
    const uint32_t M = B3(cls[1], cls[2], cls[3], T_OR3);   // the stones of groups with >= 2 liberties
    // (the DPP moves run in every lane, outside any select: a lane masked off while its neighbour reads it would hand over zero)
    const uint32_t aboveM = lat_above<LPB>(me), belowM = lat_below<LPB>(me);
    const uint32_t aboveO = lat_above<LPB>(op), belowO = lat_below<LPB>(op);
    const uint32_t aboveC = lat_above<LPB>(M), belowC = lat_below<LPB>(M);
    const uint32_t meU = aboveM | tf, meD = belowM | bf;
    uint32_t Cr, Er;
    tactical_rows(me, op, M, meU, meD, aboveO, belowO, aboveC | tf, belowC | bf, full, Cr, Er);
    const uint32_t valid = done ? 0u : (full & ~inv);
    const uint32_t Xr = valid & eye_row(me, op, meU, meD, aboveO, belowO, full, edge, N);   // valid & ~F: the mover's own eyes
    uint32_t Pr = 0u;
    if (f.on && f.r < N && !done) {
      const uint32_t uM = top ? ~0u : pattern_pad(aboveM, N), uO = top ? ~0u : pattern_pad(aboveO, N);
      const uint32_t dM = bot ? ~0u : pattern_pad(belowM, N), dO = bot ? ~0u : pattern_pad(belowO, N);
      Pr = pattern_row(uM, uO, pattern_pad(me, N), pattern_pad(op, N), dM, dO, N) & full & ~(me | op);
    }
    // the previous point: a point of the board or nothing (k_patterns', without an orientation)
    const int64_t b = f.on ? f.b_first + f.j : 0;
    const int la = (last && f.on) ? last[b] : -1;
    uint32_t near = 0u;
    if ((uint32_t)la < (uint32_t)P) {
      const int pr = la / N, pc = la - pr * N;
      if (f.r >= pr - 1 && f.r <= pr + 1) near = ((7u << pc) >> 1) & ~(f.r == pr ? 1u << pc : 0u);
    }
    const uint32_t rows[kPriorTerms] = {valid, Cr & valid, Er & valid, Pr & valid, valid & ~Xr & Pr & near, Xr};
    // this lane's destination: the wave's slice, or its board's node
    uint32_t *dst = out + f.b_first * (int64_t)(2 * P);
    bool go = f.on;
    int so = f.j * 2 * P;   // this board's words inside the segment, and the segment inside LDS
    if (TREE) {
      const int y = (node && f.on) ? node[b] : 0;
      go = f.on && y >= 0 && y <= I && !(need_move && la < 0);
      dst = out + (((VL ? b / L : b) * (int64_t)(I + 1) + (go ? y : 0)) * P) * 2;
      so = f.j * Q::kSegWords;
    }
    const int mo = (int)(((uintptr_t)dst & 15u) >> 2);
    WAVE_SYNC();
    if (go && f.r < N) {
      uint32_t *w = lds + so + mo + f.r * 2 * N;
      for (int c = 0; c < N; ++c) {
        uint32_t v = 0u, s = 0u;
#pragma unroll
        for (int k = 0; k < kPriorTerms; ++k) {
          const uint32_t m = 0u - ((rows[k] >> c) & 1u);
          v += m & wv[k];
          s += m & ws[k];
        }
        w[2 * c] = v;
        w[2 * c + 1] = s;
      }
    }
    WAVE_SYNC();
    if (TREE) {
      // board by board, the whole wave: every lane works the destination out again from the board's own words
      for (int j = 0; j < f.nb; ++j) {
        const int64_t bj = f.b_first + j;
        const int y = node ? node[bj] : 0;
        if (y < 0 || y > I || (need_move && last[bj] < 0)) continue;
        uint32_t *dj = out + (((VL ? bj / L : bj) * (int64_t)(I + 1) + y) * P) * 2;
        prior_store<true>(dj, lds + j * Q::kSegWords, (int)(((uintptr_t)dj & 15u) >> 2), 2 * P, f.lane);
      }
    } else {
      prior_store<false>(dst, lds, mo, f.nb * 2 * P, f.lane);
    }
    WAVE_SYNC();
  }
}

}  // namespace gg
