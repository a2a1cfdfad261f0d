// gg_status.h - STONE STATUS AND THE FINAL SCORE FROM PLAYOUT OWNERSHIP (gg_batch_status, gg_batch_status_tracked of
// include/gymgo_amd_status.h): which chains of a board are alive, dead or unsettled by the vote of K playouts over
// the ownership of their stones, and the Tromp-Taylor areas of the board once the dead chains are taken off - from byte planes
// or tracked boards and the ownership counts batch_playouts(ownership=True) returns, in one launch.
//
// Layout: gg_planes.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards (grid-stride).
//
// THE RULE.  own int32 [B][2][N][N]: own[b][0][p] / own[b][1][p] = in how many of K playouts point p ended in black's / white's
// area (0 <= own <= K, own[0] + own[1] <= K per point: the caller's contract), in the board's stored frame.  num / den: the
// threshold, 1 <= num <= den <= 1024 and 2 num > den; 1 <= K <= 2^20.  For every chain C (4-connected stones of one colour c)
// with |C| stones:
//   D(C) = the sum over the stones p of C of own[1 - c][p],   A(C) = the sum over the stones p of C of own[c][p];
//   C is DEAD iff D den >= num K |C|;  else ALIVE iff A den >= num K |C|;  else UNSETTLED.
// D + A <= K |C| and 2 num > den make dead and alive exclusive.  Every product is a 64-bit integer (num K |C| < 2^39,
// D den < 2^39 inside the contract) and no floating point appears, so the result is bit-defined.  Values outside the contract
// give an unspecified status for their chain: the sums wrap in 32 bits, and no address and no loop bound depends on a value.
// own on empty points is never read.  After the vote the dead chains of both colours are taken off and area_owned (gg_area.h)
// runs on what remains; unsettled chains stay on the board, so the shared liberties of a seki come out neutral, as
// Tromp-Taylor has them.
//
// THE KERNEL, per grid-stride step: plane_load (unturned); the wave's slice of own - contiguous in HBM - copied into LDS word
// by word (LDS-staged: the staged byte planes are dead by then, the bit-string of the emission is built after the last read);
// chain rounds as in feat_groups (gg_feat.h): black and white chains flooded in lock-step through lat_flood, one round per
// chain of the slower colour, at most 2 R^2 rounds.  In a round every lane walks the set bits of its row of the two chains
// (at most N LDS reads of two words) and sums the own-colour and the other colour's count of each stone; lat_board_sum reduces
// |C| of both colours in one word and D and A of either colour in a word of their own (a sum reaches 360 * 2^20: it needs
// the whole word, not one of the 16-bit fields used elsewhere).  Then the dead set is cleared from the stones, area_owned,
// the nine rows are turned into view orient[b] (feat_orient, three at a time: the analysis runs unturned, so own is read in
// its stored frame), plane_emit.
#pragma once
#include "gg_area.h"

namespace gg {

constexpr int kStatusPlanes = 9;

template <int R>
struct Status {
  using Pl = Planes<R>;
  static constexpr int LPB = Pl::LPB, NBW = Pl::NBW, K = Pl::K;
  static constexpr int kBsWords = plane_bs_words<R>(kStatusPlanes, 15);
  static constexpr int kOwnWords = NBW * 2 * R * R;                             // the wave's slice of own
  static constexpr int kLdsWords = kOwnWords > Pl::kIoWords ? (kOwnWords > kBsWords ? kOwnWords : kBsWords)
                                                            : (Pl::kIoWords > kBsWords ? Pl::kIoWords : kBsWords);
};

// THE VOTE.  bl / wh: this lane's row of black / white stones (zero in rows >= N and on boards that are not there); vals: the
// wave's slice of own in LDS, [NBW][2][N][N]; numK = num K.  -> dead[c] / alive[c]: this lane's row of the dead / alive stones
// of colour c (0 black, 1 white); a stone in neither is unsettled.
template <int R>
__device__ __forceinline__ void status_vote(uint32_t bl, uint32_t wh, const uint32_t *vals, const PlaneFrame<R> &f, int N,
                                            uint32_t numK, uint32_t den, uint32_t (&dead)[2], uint32_t (&alive)[2]) {
  constexpr int LPB = Status<R>::LPB, K = Status<R>::K;
  const int P = N * N, base = f.j * 2 * P + f.r * N;
  uint32_t Mk[K], Mkr[K];
  plane_pair<R>(bl, wh, Mk);
#pragma unroll
  for (int k = 0; k < K; ++k) Mkr[k] = __brev(Mk[k]);
  dead[0] = dead[1] = alive[0] = alive[1] = 0;
  uint32_t remb = bl, remw = wh;
#pragma unroll 1
  for (int it = 0; it < 2 * R * R; ++it) {   // (a round takes at least one stone off some board: the bound is never reached)
    if (__ballot((remb | remw) != 0u) == 0ull) break;
    uint32_t X[K], F[K];
    plane_pair<R>(remb, remw, X);
    plane_seeds<R>(X, F);
    lat_flood<LPB, K>(F, Mk, Mkr);
    const uint32_t fb = plane_field<R>(F, 0), fw = plane_field<R>(F, 1);
    // this lane's stones of the two chains: their own colour's count (a) and the other colour's (d), from LDS
    uint32_t ab = 0, db = 0, aw = 0, dw = 0;
    for (uint32_t m = fb | fw; m != 0u; m &= m - 1u) {   // (fb, fw != 0 only in rows < N of boards that are there)
      const int c = __ffs((int)m) - 1;
      const uint32_t v0 = vals[base + c], v1 = vals[base + P + c];
      const bool black = ((fb >> c) & 1u) != 0u;
      ab += black ? v0 : 0u; db += black ? v1 : 0u;
      aw += black ? 0u : v1; dw += black ? 0u : v0;
    }
    const uint32_t n = lat_board_sum<LPB>((uint32_t)__popc(fb) | ((uint32_t)__popc(fw) << 16));   // (<= 361 each)
    const uint32_t Ab = lat_board_sum<LPB>(ab), Db = lat_board_sum<LPB>(db);
    const uint32_t Aw = lat_board_sum<LPB>(aw), Dw = lat_board_sum<LPB>(dw);
    const uint64_t needb = (uint64_t)numK * (n & 0xFFFFu), needw = (uint64_t)numK * (n >> 16);
    const bool deadb = (uint64_t)Db * den >= needb, deadw = (uint64_t)Dw * den >= needw;
    const bool liveb = !deadb && (uint64_t)Ab * den >= needb, livew = !deadw && (uint64_t)Aw * den >= needw;
    dead[0] |= deadb ? fb : 0u; alive[0] |= liveb ? fb : 0u;
    dead[1] |= deadw ? fw : 0u; alive[1] |= livew ? fw : 0u;
    remb &= ~fb;
    remw &= ~fw;
  }
}

// gg_batch_status / gg_batch_status_tracked: out [B][9][N][N] of elements of 1 << esh bytes (`one`: the bit pattern of 1),
// aligned to its element; orient int32 [B] or null; side uint8 [B] or null; own int32 [B][2][N][N]; counts int32 [B][4] or
// null (own area, opponent area, own dead stones, opponent dead stones; they do not turn).  One single-wave workgroup per NBW
// boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_status(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                  const uint8_t *__restrict__ side, const uint32_t *__restrict__ own, uint32_t numK,
                                                  uint32_t den, uint8_t *__restrict__ out, int32_t *__restrict__ counts, int esh,
                                                  uint32_t one, int64_t B, int N) {
  constexpr int LPB = Status<R>::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Status<R>::kLdsWords];
  PlaneFrame<R> f(N);
  const int P = N * N;
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, nullptr, f, B, N, lds, bl, wh, inv, fl);
    WAVE_SYNC();
    const uint32_t *src = own + f.b_first * (int64_t)(2 * P);
    for (int i = f.lane; i < f.nb * 2 * P; i += kWave) lds[i] = src[i];   // (nb 2 N^2 <= kOwnWords)
    WAVE_SYNC();
    uint32_t dead[2], alive[2];
    status_vote<R>(bl, wh, lds, f, N, numK, den, dead, alive);
    uint32_t ob, ow;
    area_owned<R>(bl & ~dead[0], wh & ~dead[1], f.full, ob, ow);
    const bool white = side ? (f.on && side[f.b_first + f.j] != 0) : (fl & 1u) != 0;
    if (counts) {
      const uint32_t area = lat_board_sum<LPB>((uint32_t)__popc(ob) | ((uint32_t)__popc(ow) << 16));            // (<= 361 each)
      const uint32_t gone = lat_board_sum<LPB>((uint32_t)__popc(dead[0]) | ((uint32_t)__popc(dead[1]) << 16));
      if (f.on && f.r == 0) {
        int32_t *c = counts + 4 * (f.b_first + f.j);
        c[0] = (int32_t)(white ? area >> 16 : area & 0xFFFFu);
        c[1] = (int32_t)(white ? area & 0xFFFFu : area >> 16);
        c[2] = (int32_t)(white ? gone >> 16 : gone & 0xFFFFu);
        c[3] = (int32_t)(white ? gone & 0xFFFFu : gone >> 16);
      }
    }
    const uint32_t sm = white ? wh : bl, so = white ? bl : wh;
    const uint32_t dm = white ? dead[1] : dead[0], d_o = white ? dead[0] : dead[1];
    const uint32_t am = white ? alive[1] : alive[0], ao = white ? alive[0] : alive[1];
    uint32_t rows[kStatusPlanes] = {am, dm, sm & ~(am | dm), ao, d_o, so & ~(ao | d_o),
                                    white ? ow : ob, white ? ob : ow, f.full & ~(ob | ow)};
    if (orient) {
      const int o = f.on ? (orient[f.b_first + f.j] & 7) : 0;
#pragma unroll
      for (int p = 0; p < kStatusPlanes; p += 3) feat_orient<R>(rows[p], rows[p + 1], rows[p + 2], o, N, f.r, f.lane, f.full);
    }
    WAVE_SYNC();   // (the last reads of own are behind: the string takes the buffer)
    plane_emit<R, kStatusPlanes>(out, esh, one, rows, lds, f, N);
  }
}

}  // namespace gg
