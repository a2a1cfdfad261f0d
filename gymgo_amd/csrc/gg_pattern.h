// gg_pattern.h - THE PATTERN PLANES (gg_batch_patterns, gg_batch_patterns_tracked of include/gymgo_amd_pattern.h): the
// two sets the pattern playout policy adds to the tactical ones - P, the empty points whose 3x3 neighbourhood matches one of the
// thirteen patterns, and L, the candidates of no_eye_fill among the eight neighbours of the previous move that are in P - of every
// board, from byte planes or tracked boards, in one launch.  The rule on its own, as gg_batch_tactics is for DESIGN 34: for
// users, and for the tests that hold the draw of k_rollout_lat_pol / k_rollout5_pat to it.
//
// Layout: gg_planes.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards (grid-stride).
// No flood: the patterns look at stones, and the eyes of F at stones too.  The decision is pattern_match of gg_common.h, the
// statement the rollout kernels draw from, with the rows above / below one DPP move away.
//
// `last` refers to the UNTURNED board: with an orientation the previous point is turned with the board (feat_orient's geometry).
//
// EMISSION (plane_emit of gg_planes.h): 2 N^2 elements per board, so `out` needs the alignment of its element only.
#pragma once
#include "gg_planes.h"

namespace gg {

constexpr int kPatternPlanes = 2;

template <int R>
struct Patterns {
  static constexpr int LPB = Planes<R>::LPB;
  static constexpr int kBsWords = plane_bs_words<R>(kPatternPlanes, 15);
  static constexpr int kLdsWords = kBsWords > Planes<R>::kIoWords ? kBsWords : Planes<R>::kIoWords;   // (the staged input is dead by then)
};

// gg_batch_patterns / gg_batch_patterns_tracked: out [B][2][N][N] of elements of 1 << esh bytes (`one`: the bit pattern of 1),
// aligned to its element; last int32 [B] or null; orient int32 [B] or null.  One single-wave workgroup per NBW boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_patterns(const void *__restrict__ in, const int32_t *__restrict__ last,
                                                    const int32_t *__restrict__ orient, uint8_t *__restrict__ out, int esh, uint32_t one,
                                                    int64_t B, int N) {
  constexpr int LPB = Patterns<R>::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Patterns<R>::kLdsWords];
  PlaneFrame<R> f(N);
  const uint32_t full = f.full;
  const bool top = f.r == 0, bot = f.r == N - 1;
  const uint32_t tf = top ? full : 0u, bf = bot ? full : 0u;
  const uint32_t edge = (top || bot) ? full : (1u | (1u << (N - 1)));
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, orient, f, B, N, lds, bl, wh, inv, fl);
    const bool white = (fl & 1u) != 0, done = (fl & 4u) != 0;
    const uint32_t me = white ? wh : bl, op = white ? bl : wh;
    // (the DPP moves run in every lane, outside any select: a lane masked off while its neighbour reads it would hand over zero)
    const uint32_t aboveM = lat_above<LPB>(me), belowM = lat_below<LPB>(me);
    const uint32_t aboveO = lat_above<LPB>(op), belowO = lat_below<LPB>(op);
    const uint32_t meU = aboveM | tf, meD = belowM | bf;
    const uint32_t valid = done ? 0u : (full & ~inv);
    const uint32_t Fr = valid & ~eye_row(me, op, meU, meD, aboveO, belowO, full, edge, N);
    uint32_t Pr = 0u;
    if (f.on && f.r < N && !done) {
      const uint32_t uM = top ? ~0u : pattern_pad(aboveM, N), uO = top ? ~0u : pattern_pad(aboveO, N);
      const uint32_t dM = bot ? ~0u : pattern_pad(belowM, N), dO = bot ? ~0u : pattern_pad(belowO, N);
      Pr = pattern_row(uM, uO, pattern_pad(me, N), pattern_pad(op, N), dM, dO, N) & full & ~(me | op);
    }
    // the previous point, a point of the unturned board or nothing, in the view the board was turned into
    uint32_t near = 0u;
    if (last && f.on) {
      const int la = last[f.b_first + f.j];
      if ((uint32_t)la < (uint32_t)(N * N)) {
        int pr = la / N, pc = la - pr * N;
        const int o = orient ? (orient[f.b_first + f.j] & 7) : 0;
        if (o & 4) {
          const int r0 = pr, c0 = pc;
          pr = (o & 1) ? c0 : N - 1 - c0;
          pc = (o & 2) ? N - 1 - r0 : r0;
        } else {
          if (o & 2) pr = N - 1 - pr;
          if (o & 1) pc = N - 1 - pc;
        }
        if (f.r >= pr - 1 && f.r <= pr + 1) near = ((7u << pc) >> 1) & ~(f.r == pr ? 1u << pc : 0u);
      }
    }
    const uint32_t rows[kPatternPlanes] = {Pr, Fr & Pr & near};
    plane_emit<R, kPatternPlanes>(out, esh, one, rows, lds, f, N);
  }
}

}  // namespace gg
