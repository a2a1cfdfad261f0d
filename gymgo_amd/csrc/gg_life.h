// gg_life.h - PASS-ALIVE (Benson) LIFE PLANES (gg_batch_life, gg_batch_life_tracked of include/gymgo_amd.h): the
// stones that can never be captured and the points they decide, from byte planes or tracked boards, in one launch.
//
// Layout: gg_feat.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards.  Black and
// white are analysed in lock-step: every row set below is a PAIR, two bit fields of one register (R <= 13) or two registers
// (R = 19), exactly the pairs lat_flood floods together in feat_groups.
//
// For a colour X with stones S: CHAINS are the components of S, REGIONS the components of full & ~S (empty points and the
// other colour's stones together).  A region is VITAL to a chain when it has an empty point and every empty point of it is
// next to the chain.  Benson: start with all chains alive; a chain stays alive while two regions are vital to it that border
// no chain that is already dead.  Here as PASSES until the alive set stops changing; a pass, with A = the stones alive so far:
//   the regions are enumerated by seed-and-flood (the lowest unvisited point of the board's first lane that has one, one board
//   scan for both colours - feat_groups' round); a region r is dismissed when
//     1. dilate(r) & S & ~A is not empty anywhere on the board (it borders a dead chain), or
//     2. r has no empty point, or some empty point of r is not in dilate(A) (it touches no alive chain: vital to none);
//   what survives - small eyes, mostly - can only be vital to a chain next to its LOWEST empty point: the at most four chains
//   there are flooded one after the other (again seed-and-flood, over the up to four neighbouring stones), each tested with
//   r & E & ~dilate(chain) == 0 over the board and counted in a saturating two-step counter kept as stone masks
//   (twice |= chain & once; once |= chain), the region remembered in `safe`;
//   at the end of the pass A' = twice.
// The pass that leaves A unchanged has counted exactly the regions that border alive chains only, so its `safe` is the result.
// Every loop is bounded by construction: a region round takes a point off some board's unvisited set, a candidate round a
// stone off some board's (at most four) candidates, a pass that is not the last a chain off some board's alive set.
//
// EMISSION (plane_emit of gg_planes.h): 4 N^2 elements per board - not a multiple of 16 bytes for odd N in uint8, so `out` needs element alignment only.
// The boards of a wave are contiguous in `out`: the lanes OR their four row masks into one bit-string per wave in LDS whose
// bit (mo + e) is element e of the wave's slice, mo = the slice's misalignment in elements; every aligned 16-byte vector
// inside the slice is then a run of 16 / element size bits that never crosses a word (k_features' walk), and the two ragged
// ends of the slice leave as single elements (stage_out's lanes 0 - 15 / 16 - 31).  Nothing outside the slice is written.
#pragma once
#include "gg_feat.h"

namespace gg {

constexpr int kLifePlanes = 4;

template <int R>
struct Life {
  using F_ = Feat<R>;
  static constexpr int LPB = F_::LPB, NBW = F_::NBW, FW = F_::FW, K = F_::K;
  static constexpr uint32_t FM = Planes<R>::FM;
  static constexpr int kBsWords = plane_bs_words<R>(kLifePlanes, 15);
  static constexpr int kLdsWords = kBsWords > F_::kIoWords ? kBsWords : F_::kIoWords;   // (the staged input is dead by then)
};

// bl / wh: this lane's row of black / white stones (zero in rows >= N and on boards that are not there) -> the rows of
// alive(black), alive(white), safe(black), safe(white)
template <int R>
__device__ __forceinline__ void life_benson(uint32_t bl, uint32_t wh, uint32_t full, uint32_t &ab, uint32_t &aw, uint32_t &sb,
                                            uint32_t &sw) {
  using L_ = Life<R>;
  constexpr int LPB = L_::LPB, K = L_::K;
  constexpr uint32_t FM = L_::FM;
  const uint32_t E = full & ~(bl | wh);
  uint32_t S[K], Sr[K], C[K], Cr[K], Ee[K], A[K], safe[K];
  plane_pair<R>(bl, wh, S);
  plane_pair<R>(full & ~bl, full & ~wh, C);
  plane_pair<R>(E, E, Ee);
#pragma unroll
  for (int k = 0; k < K; ++k) { Sr[k] = __brev(S[k]); Cr[k] = __brev(C[k]); A[k] = S[k]; safe[k] = 0; }
#pragma unroll 1
  for (int pass = 0; pass < R * R + 1; ++pass) {   // (a pass that is not the last takes a chain off some board's alive set)
    uint32_t rem[K], once[K], twice[K], dA[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { rem[k] = C[k]; once[k] = twice[k] = safe[k] = 0; dA[k] = lat_dilate<LPB>(A[k]); }
#pragma unroll 1
    for (int it = 0; it < 2 * R * R; ++it) {       // (a round takes at least one point off some board: the bound is never reached)
      uint32_t any = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) any |= rem[k];
      if (__ballot(any != 0u) == 0ull) break;
      uint32_t F[K];
      plane_seeds<R>(rem, F);
      lat_flood<LPB, K>(F, C, Cr);                 // the next region of either colour
      uint32_t bord[K], RE[K], nt[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        rem[k] &= ~F[k];
        bord[k] = lat_dilate<LPB>(F[k]) & S[k] & ~A[k];   // 1. next to a dead chain
        RE[k] = F[k] & Ee[k];
        nt[k] = RE[k] & ~dA[k];                            // 2. an empty point that touches no alive chain
      }
      // six flags per lane, summed over the board in one word of 5-bit fields (at most 19 rows are set)
      uint32_t w = 0;
#pragma unroll
      for (int c = 0; c < 2; ++c)
        w |= ((plane_field<R>(bord, c) ? 1u : 0u) | (plane_field<R>(RE, c) ? 32u : 0u) | (plane_field<R>(nt, c) ? 1024u : 0u)) << (15 * c);
      const uint32_t sum = lat_board_sum<LPB>(w);
      bool ok[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const uint32_t f = sum >> (15 * c);
        ok[c] = (f & 31u) == 0u && ((f >> 5) & 31u) != 0u && ((f >> 10) & 31u) == 0u;
      }
      if (__ballot(ok[0] || ok[1]) == 0ull) continue;
      // 3. the chains next to the region's lowest empty point (all of them alive, by 1.)
      uint32_t okm[K], REk[K], P0[K], cand[K];
      plane_pair<R>(ok[0] ? FM : 0u, ok[1] ? FM : 0u, okm);
#pragma unroll
      for (int k = 0; k < K; ++k) REk[k] = RE[k] & okm[k];
      plane_seeds<R>(REk, P0);
#pragma unroll
      for (int k = 0; k < K; ++k) cand[k] = lat_dilate<LPB>(P0[k]) & S[k];
#pragma unroll 1
      for (int ci = 0; ci < 4; ++ci) {             // (a round takes a chain's stones off the at most four candidates of a board)
        uint32_t anyc = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) anyc |= cand[k];
        if (__ballot(anyc != 0u) == 0ull) break;
        uint32_t G[K];
        plane_seeds<R>(cand, G);
        lat_flood<LPB, K>(G, S, Sr);
        uint32_t miss[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          cand[k] &= ~G[k];
          miss[k] = REk[k] & ~lat_dilate<LPB>(G[k]);
        }
        uint32_t w2 = 0;
#pragma unroll
        for (int c = 0; c < 2; ++c) w2 |= ((plane_field<R>(G, c) ? 1u : 0u) | (plane_field<R>(miss, c) ? 256u : 0u)) << (16 * c);
        const uint32_t s2 = lat_board_sum<LPB>(w2);
        uint32_t vm[K];   // the region is vital to the chain
        plane_pair<R>((s2 & 0xFFu) != 0u && (s2 & 0xFF00u) == 0u ? FM : 0u,
                     ((s2 >> 16) & 0xFFu) != 0u && (s2 >> 24) == 0u ? FM : 0u, vm);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const uint32_t g = G[k] & vm[k];
          twice[k] |= g & once[k];
          once[k] |= g;
          safe[k] |= F[k] & vm[k];
        }
      }
    }
    // 4. the chains counted twice stay alive
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) { diff |= A[k] ^ twice[k]; A[k] = twice[k]; }
    if (__ballot(diff != 0u) == 0ull) break;
  }
  ab = plane_field<R>(A, 0); aw = plane_field<R>(A, 1);
  sb = plane_field<R>(safe, 0); sw = plane_field<R>(safe, 1);
}

// gg_batch_life / gg_batch_life_tracked: out [B][4][N][N] of elements of 1 << esh bytes (`one`: the bit pattern of 1), aligned to
// its element; settled uint8 [B] or null; orient int32 [B] or null (feat_orient on the loaded rows: all four planes are
// geometric).  One single-wave workgroup per NBW boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_life(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                uint8_t *__restrict__ out, uint8_t *__restrict__ settled, int esh, uint32_t one,
                                                int64_t B, int N) {
  constexpr int LPB = Life<R>::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Life<R>::kLdsWords];
  PlaneFrame<R> f(N);
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, orient, f, B, N, lds, bl, wh, inv, fl);
    uint32_t ab, aw, sb, sw;
    life_benson<R>(bl, wh, f.full, ab, aw, sb, sw);
    if (settled) {   // every point of the board lies in some plane
      const uint32_t open = lat_board_sum<LPB>((ab | aw | sb | sw) != f.full ? 1u : 0u);
      if (f.on && f.r == 0) settled[f.b_first + f.j] = open == 0u ? 1 : 0;
    }
    const bool white = (fl & 1u) != 0;
    const uint32_t rows[kLifePlanes] = {white ? aw : ab, white ? ab : aw, white ? sw : sb, white ? sb : sw};
    plane_emit<R, kLifePlanes>(out, esh, one, rows, lds, f, N);
  }
}

}  // namespace gg
