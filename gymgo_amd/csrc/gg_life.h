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
// EMISSION: 4 N^2 elements per board - not a multiple of 16 bytes for odd N in uint8, so `out` needs element alignment only.
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
  static constexpr uint32_t FM = Lat<R>::FM;
  static constexpr int kBsWords = (15 + NBW * kLifePlanes * R * R + 31) / 32 + 2;   // the bit-string (+ the spill word of the last OR)
  static constexpr int kLdsWords = kBsWords > F_::kIoWords ? kBsWords : F_::kIoWords;   // (the staged input is dead by then)
};

// colour k's row of a pair
template <int R>
__device__ __forceinline__ uint32_t life_field(const uint32_t (&X)[Life<R>::K], int k) {
  constexpr int K = Life<R>::K;
  if (K == 1) return (k ? X[0] >> (Life<R>::FW & 31) : X[0]) & Life<R>::FM;
  return X[k ? K - 1 : 0];
}
// the pair (b, w)
template <int R>
__device__ __forceinline__ void life_pair(uint32_t b, uint32_t w, uint32_t (&X)[Life<R>::K]) {
  constexpr int K = Life<R>::K;
  if (K == 1) X[0] = b | (w << (Life<R>::FW & 31));
  else { X[0] = b; X[K - 1] = w; }
}
// per colour, the lowest point of the first lane of the board that holds one (feat_groups' seeds): X -> F
template <int R>
__device__ __forceinline__ void life_seeds(const uint32_t (&X)[Life<R>::K], uint32_t (&F)[Life<R>::K]) {
  const uint32_t xb = life_field<R>(X, 0), xw = life_field<R>(X, 1);
  const uint32_t has = (xb ? 1u : 0u) | (xw ? 0x10000u : 0u);
  const uint32_t incl = lat_board_scan<Life<R>::LPB>(has);
  const uint32_t sb = (xb != 0u && (incl & 0xFFFFu) == 1u) ? (xb & (0u - xb)) : 0u;
  const uint32_t sw = (xw != 0u && (incl >> 16) == 1u) ? (xw & (0u - xw)) : 0u;
  life_pair<R>(sb, sw, F);
}

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
  life_pair<R>(bl, wh, S);
  life_pair<R>(full & ~bl, full & ~wh, C);
  life_pair<R>(E, E, Ee);
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
      life_seeds<R>(rem, F);
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
        w |= ((life_field<R>(bord, c) ? 1u : 0u) | (life_field<R>(RE, c) ? 32u : 0u) | (life_field<R>(nt, c) ? 1024u : 0u)) << (15 * c);
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
      life_pair<R>(ok[0] ? FM : 0u, ok[1] ? FM : 0u, okm);
#pragma unroll
      for (int k = 0; k < K; ++k) REk[k] = RE[k] & okm[k];
      life_seeds<R>(REk, P0);
#pragma unroll
      for (int k = 0; k < K; ++k) cand[k] = lat_dilate<LPB>(P0[k]) & S[k];
#pragma unroll 1
      for (int ci = 0; ci < 4; ++ci) {             // (a round takes a chain's stones off the at most four candidates of a board)
        uint32_t anyc = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) anyc |= cand[k];
        if (__ballot(anyc != 0u) == 0ull) break;
        uint32_t G[K];
        life_seeds<R>(cand, G);
        lat_flood<LPB, K>(G, S, Sr);
        uint32_t miss[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          cand[k] &= ~G[k];
          miss[k] = REk[k] & ~lat_dilate<LPB>(G[k]);
        }
        uint32_t w2 = 0;
#pragma unroll
        for (int c = 0; c < 2; ++c) w2 |= ((life_field<R>(G, c) ? 1u : 0u) | (life_field<R>(miss, c) ? 256u : 0u)) << (16 * c);
        const uint32_t s2 = lat_board_sum<LPB>(w2);
        uint32_t vm[K];   // the region is vital to the chain
        life_pair<R>((s2 & 0xFFu) != 0u && (s2 & 0xFF00u) == 0u ? FM : 0u,
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
  ab = life_field<R>(A, 0); aw = life_field<R>(A, 1);
  sb = life_field<R>(safe, 0); sw = life_field<R>(safe, 1);
}

// gg_batch_life / gg_batch_life_tracked: out [B][4][N][N] of elements of 1 << esh bytes (`one`: the bit pattern of 1), aligned to
// its element; settled uint8 [B] or null; orient int32 [B] or null (feat_orient on the loaded rows: all four planes are
// geometric).  One single-wave workgroup per NBW boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_life(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                uint8_t *__restrict__ out, uint8_t *__restrict__ settled, int esh, uint32_t one,
                                                int64_t B, int N) {
  using L_ = Life<R>;
  constexpr int LPB = L_::LPB, NBW = L_::NBW;
  __shared__ __attribute__((aligned(16))) uint32_t lds[L_::kLdsWords];
  const int lane = threadIdx.x & (kWave - 1);
  const int r = lane & (LPB - 1), j = lane / LPB;
  const int P = N * N;
  const uint32_t full = r < N ? (1u << N) - 1u : 0u;
  const int epv = 16 >> esh;   // elements per 16-byte vector: 16, 8, 4
  const int64_t ngroups = (B + NBW - 1) / NBW;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t b_first = g * NBW;
    const int nb = (int)(B - b_first < NBW ? B - b_first : NBW);
    const bool on = j < nb;
    uint32_t bl, wh, inv, fl;
    if (TRACKED) feat_load_tracked(static_cast<const uint32_t *>(in), on ? b_first + j : B - 1, N, r, on, full, bl, wh, inv, fl);
    else feat_load_bytes<R>(static_cast<const uint8_t *>(in), b_first, nb, N, r, j, on, full, lds, lane, bl, wh, inv, fl);
    if (orient) feat_orient<R>(bl, wh, inv, on ? (orient[b_first + j] & 7) : 0, N, r, lane, full);
    uint32_t ab, aw, sb, sw;
    life_benson<R>(bl, wh, full, ab, aw, sb, sw);
    if (settled) {   // every point of the board lies in some plane
      const uint32_t open = lat_board_sum<LPB>((ab | aw | sb | sw) != full ? 1u : 0u);
      if (on && r == 0) settled[b_first + j] = open == 0u ? 1 : 0;
    }
    const bool white = (fl & 1u) != 0;
    const uint32_t rows[kLifePlanes] = {white ? aw : ab, white ? ab : aw, white ? sw : sb, white ? sb : sw};
    // the wave's bit-string: bit mo + e = element e of the wave's slice of `out`
    uint8_t *dst = out + ((b_first * (int64_t)(kLifePlanes * P)) << esh);
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
    const int mo = (int)(mis >> esh);
    const int nel = nb * kLifePlanes * P, end = mo + nel;
    for (int w = lane; w < ((end + 31) >> 5) + 1; w += kWave) lds[w] = 0;
    WAVE_SYNC();
    if (on && r < N) {
      const uint32_t q0 = (uint32_t)(mo + j * kLifePlanes * P + r * N);
#pragma unroll
      for (int p = 0; p < kLifePlanes; ++p) {
        if (rows[p]) {
          const uint32_t q = q0 + (uint32_t)(p * P);
          const uint64_t x = (uint64_t)rows[p] << (q & 31u);
          atomicOr(lds + (q >> 5), (uint32_t)x);
          if ((uint32_t)(x >> 32)) atomicOr(lds + (q >> 5) + 1, (uint32_t)(x >> 32));
        }
      }
    }
    WAVE_SYNC();
    uint8_t *ga = dst - mis;
    const int v0 = mo ? 1 : 0, v1 = end >> (4 - esh);
    for (int v = v0 + lane; v < v1; v += kWave) {
      const uint32_t q = (uint32_t)(v << (4 - esh));
      const uint32_t x = lds[q >> 5] >> (q & 31u);
      *reinterpret_cast<V16a *>(ga + 16 * (int64_t)v) = esh == 0 ? feat_expand<1>(x, one) : esh == 1 ? feat_expand<2>(x, one)
                                                                                                       : feat_expand<4>(x, one);
    }
    // the ragged ends as single elements: lanes 0 - 15 the head, 16 - 31 the tail; a slice inside one vector: all of it
    int e0 = -1, estep = nel;
    if (v1 >= v0) {
      const int head = mo ? epv - mo : 0, tail = end & (epv - 1);
      if (lane < 16) { if (lane < head) e0 = lane; }
      else if (lane < 32 && lane - 16 < tail) e0 = nel - tail + (lane - 16);
    } else {
      e0 = lane;
      estep = kWave;
    }
    for (int e = e0; e >= 0 && e < nel; e += estep) {
      const uint32_t q = (uint32_t)(mo + e);
      const uint32_t v = ((lds[q >> 5] >> (q & 31u)) & 1u) ? one : 0u;
      if (esh == 0) dst[e] = (uint8_t)v;
      else if (esh == 1) reinterpret_cast<uint16_t *>(dst)[e] = (uint16_t)v;
      else reinterpret_cast<uint32_t *>(dst)[e] = v;
    }
    WAVE_SYNC();
  }
}

}  // namespace gg
