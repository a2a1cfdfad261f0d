// gg_area.h - AREA OWNERSHIP PLANES (gg_batch_area, gg_batch_area_tracked of include/gymgo_amd_area.h): which points of
// a board Tromp-Taylor scoring counts for which colour, and which for neither, from byte planes or tracked boards, in one
// launch - the per-point form of gg_batch_areas, as network input (the current position) and as training target (the final
// position of a game, seen by the mover of a sampled one).
//
// Layout: gg_planes.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards (grid-stride).
//
// THE RULE (gym_go/gogame.py:275-300, point by point): E = the empty points; Rb = the empty points connected through E to an
// empty point next to a black stone, Rw alike for white.  Black owns bl | (Rb & ~Rw), white wh | (Rw & ~Rb); what is left -
// empty points whose region touches both colours, or none - is neutral.  Rb and Rw are the two floods of E seeded with
// dilate(stones) & E, run as ONE pair through lat_flood (two fields of one register for R <= 13, two registers for R = 19):
// lat_area_floods of gg_lat.h, the one statement of the rule that lat_areas (the env-step and search kernels), lat_areas_owned
// (the playout harvest, gg_po.h) and this file share.
//
// The view: side[b] (uint8, 0 black / non-zero white) when given, else the board's turn flag - the mover's view of every
// other plane family.  The targets need the first form: the final position of a game is seen by the mover of the SAMPLED
// position, not by its own.  Only the stones and that flag are read; invalid points, pass and done do not matter.
//
// EMISSION (plane_emit of gg_planes.h): 3 N^2 elements per board, so `out` needs the alignment of its element only.
// counts int32 [B][2] = the popcounts of planes 0 and 1 (lat_board_sum, one lane per board stores both words).
#pragma once
#include "gg_planes.h"

namespace gg {

constexpr int kAreaPlanes = 3;

template <int R>
struct Area {
  static constexpr int LPB = Planes<R>::LPB;
  static constexpr int kBsWords = plane_bs_words<R>(kAreaPlanes, 15);
  static constexpr int kLdsWords = kBsWords > Planes<R>::kIoWords ? kBsWords : Planes<R>::kIoWords;   // (the staged input is dead by then)
};

// bl / wh: this lane's row of black / white stones (zero in rows >= N and on boards that are not there) -> the rows black
// and white own
template <int R>
__device__ __forceinline__ void area_owned(uint32_t bl, uint32_t wh, uint32_t full, uint32_t &own_b, uint32_t &own_w) {
  uint32_t fb, fw;
  lat_area_floods<R>(bl, wh, full, fb, fw);
  own_b = bl | (fb & ~fw);
  own_w = wh | (fw & ~fb);
}

// gg_batch_area / gg_batch_area_tracked: out [B][3][N][N] of elements of 1 << esh bytes (`one`: the bit pattern of 1), aligned to
// its element; orient int32 [B] or null (feat_orient on the loaded rows: the planes are geometric, the counts do not turn);
// side uint8 [B] or null; counts int32 [B][2] or null.  One single-wave workgroup per NBW boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_area(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                const uint8_t *__restrict__ side, uint8_t *__restrict__ out,
                                                int32_t *__restrict__ counts, int esh, uint32_t one, int64_t B, int N) {
  constexpr int LPB = Area<R>::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Area<R>::kLdsWords];
  PlaneFrame<R> f(N);
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, orient, f, B, N, lds, bl, wh, inv, fl);
    uint32_t ob, ow;
    area_owned<R>(bl, wh, f.full, ob, ow);
    const bool white = side ? (f.on && side[f.b_first + f.j] != 0) : (fl & 1u) != 0;
    if (counts) {
      const uint32_t sum = lat_board_sum<LPB>((uint32_t)__popc(ob) | ((uint32_t)__popc(ow) << 16));   // (<= 361 each)
      if (f.on && f.r == 0) {
        const int32_t cb = (int32_t)(sum & 0xFFFFu), cw = (int32_t)(sum >> 16);
        int32_t *c = counts + 2 * (f.b_first + f.j);
        c[0] = white ? cw : cb;
        c[1] = white ? cb : cw;
      }
    }
    const uint32_t rows[kAreaPlanes] = {white ? ow : ob, white ? ob : ow, f.full & ~(ob | ow)};
    plane_emit<R, kAreaPlanes>(out, esh, one, rows, lds, f, N);
  }
}

}  // namespace gg
