// gg_tactics.h - THE TACTICAL PLANES (gg_batch_tactics, gg_batch_tactics_tracked of include/gymgo_amd_tactics.h): the
// three sets the tactical playout policy draws from - C capture points, E escape points, F the candidates of no_eye_fill - of
// every board, from byte planes or tracked boards, in one launch.  The rule on its own, as gg_batch_eye_mask is for DESIGN 15:
// for users, and for the tests that hold the draw of k_rollout_lat_pol / k_rollout5_tac to it.
//
// Layout: gg_planes.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards (grid-stride).
//
// `low` comes from feat_groups (gg_feat.h): every group is flooded and its liberties counted from the stones alone, whatever
// the input form - the class rows a tracked board carries are not read (they would have to be turned with the board), which
// is why the tracked and the byte-plane result cannot differ.  The rows themselves are tactical_rows and eye_row of
// gg_common.h, the statements the rollout kernels draw from, with the rows above / below one DPP move away.
//
// EMISSION (plane_emit of gg_planes.h): 3 N^2 elements per board, so `out` needs the alignment of its element only.
#pragma once
#include "gg_feat.h"

namespace gg {

constexpr int kTacticsPlanes = 3;

template <int R>
struct Tactics {
  static constexpr int LPB = Planes<R>::LPB;
  static constexpr int kBsWords = plane_bs_words<R>(kTacticsPlanes, 15);
  static constexpr int kLdsWords = kBsWords > Planes<R>::kIoWords ? kBsWords : Planes<R>::kIoWords;   // (the staged input is dead by then)
};

// gg_batch_tactics / gg_batch_tactics_tracked: out [B][3][N][N] of elements of 1 << esh bytes (`one`: the bit pattern of 1),
// aligned to its element; orient int32 [B] or null.  One single-wave workgroup per NBW boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_tactics(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                   uint8_t *__restrict__ out, int esh, uint32_t one, int64_t B, int N) {
  constexpr int LPB = Tactics<R>::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Tactics<R>::kLdsWords];
  PlaneFrame<R> f(N);
  const uint32_t full = f.full;
  const bool top = f.r == 0, bot = f.r == N - 1;
  const uint32_t tf = top ? full : 0u, bf = bot ? full : 0u;
  const uint32_t edge = (top || bot) ? full : (1u | (1u << (N - 1)));
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, orient, f, B, N, lds, bl, wh, inv, fl);
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
    const uint32_t rows[kTacticsPlanes] = {Cr & valid, Er & valid, valid & ~eye_row(me, op, meU, meD, aboveO, belowO, full, edge, N)};
    plane_emit<R, kTacticsPlanes>(out, esh, one, rows, lds, f, N);
  }
}

}  // namespace gg
