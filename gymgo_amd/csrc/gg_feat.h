// gg_feat.h - NETWORK INPUT PLANES with per-group liberty counts (gg_batch_features, gg_batch_features_tracked,
// gg_batch_group_liberties of include/gymgo_amd.h): what an evaluator of the PUCT search is fed, straight from the
// byte planes or the tracked leaf boards, in one launch.
//
// Layout: ONE ROW PER LANE as in gg_lat.h - a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), the rows are bit masks in registers, left / right are shifts, up / down one DPP move.
// Two phases with different limits:
//   1. ANALYSIS, a latency chain.  The liberty count of a group needs the group on its own, so the groups are flooded one
//      after the other - but black and white at the same time (two groups of different colours are different groups): the
//      two floods share a register as two bit fields (R <= 13) or run in two registers in lock-step (R = 19), lat_flood of
//      gg_lat.h.  A round: the first lane of the board that still holds an uncounted stone of a colour seeds that colour's
//      flood with its lowest such stone (one board scan for both colours), flood to closure, liberties = dilate & empty,
//      counted per lane, summed over the board's lanes (both counts in one word), the group's stones filed under their
//      count.  A wave runs max(black groups, white groups) rounds of its slowest board.  The liberty classes that tracked
//      boards carry are NOT used: every group is counted, whatever the input form, which is why the tracked and the byte-plane
//      result cannot differ.
//   2. EMISSION, pure HBM writes: 16 N^2 elements per board.  The lanes OR their sixteen row masks into ONE bit-string per
//      wave in LDS (bit e = element e of the wave's boards, which are contiguous in the output), then the 64 lanes walk the
//      output in 16-byte vectors - consecutive lanes, consecutive addresses: vector v is bits [v E, (v + 1) E) of the string
//      (E = 16 / element size divides 32: never across a word) expanded to 0 / 1 of the element type.  A board's output is a
//      multiple of 16 bytes long, so with a 16-byte aligned `out` every store is an aligned 16-byte store and no wave
//      touches another wave's bytes.
// The count plane (gg_batch_group_liberties) keeps min(count, 255) as eight bit planes, one row each, and leaves through LDS
// bytes and stage_out (gg_common.h: aligned 16-byte stores, ragged edges as single bytes).
#pragma once
#include "gg_planes.h"

namespace gg {

constexpr int kFeatPlanes = 16;

template <int R>
struct Feat {
  using Pl = Planes<R>;
  static constexpr int LPB = Pl::LPB, NBW = Pl::NBW, FW = Pl::FW, K = Pl::K, kIoWords = Pl::kIoWords;
  static constexpr int kBsWords = plane_bs_words<R>(kFeatPlanes, 0);              // (out is 16-byte aligned: the string starts at bit 0)
  static constexpr int kLibWords = (NBW * R * R + 15 + 15) / 4 + 1;               // the count bytes on their way out
  static constexpr int kLdsWords = kBsWords > kIoWords ? kBsWords : kIoWords;     // (the staged input is dead when the bit-string is built)
  static_assert(kLibWords <= kLdsWords, "the count bytes reuse the same buffer");
};

// The groups of the wave's boards, counted.  bl / wh: this lane's row of black / white stones (zero in rows >= N and on
// boards that are not there).  COUNTS = false: cls[0 .. 3] = the stones (of either colour) whose group has exactly 1 / 2 / 3 /
// >= 4 liberties; a group without liberties (not reachable by play) is in none.  COUNTS = true: cls[k] = bit k of
// min(liberties, 255) of the stone's group.
template <int R, bool COUNTS>
__device__ __forceinline__ void feat_groups(uint32_t bl, uint32_t wh, uint32_t full, uint32_t (&cls)[COUNTS ? 8 : 4]) {
  using F_ = Feat<R>;
  constexpr int LPB = F_::LPB, FW = F_::FW, K = F_::K;
  constexpr uint32_t FM = Lat<R>::FM;
  const uint32_t E = full & ~(bl | wh);
  uint32_t Mk[K], Mkr[K], Ee[K];
  if (K == 1) {
    Mk[0] = bl | (wh << (FW & 31));
    Ee[0] = E | (E << (FW & 31));
  } else {
    Mk[0] = bl; Mk[K - 1] = wh;
    Ee[0] = E; Ee[K - 1] = E;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) Mkr[k] = __brev(Mk[k]);
#pragma unroll
  for (int k = 0; k < (COUNTS ? 8 : 4); ++k) cls[k] = 0;
  uint32_t remb = bl, remw = wh;
#pragma unroll 1
  for (int it = 0; it < 2 * R * R; ++it) {   // (a round takes at least one stone off some board: the bound is never reached)
    if (__ballot((remb | remw) != 0u) == 0ull) break;
    // the seeds: the lowest uncounted stone of the board's first lane that has one, per colour
    const uint32_t has = (remb ? 1u : 0u) | (remw ? 0x10000u : 0u);
    const uint32_t incl = lat_board_scan<LPB>(has);
    const uint32_t sb = (remb != 0u && (incl & 0xFFFFu) == 1u) ? (remb & (0u - remb)) : 0u;
    const uint32_t sw = (remw != 0u && (incl >> 16) == 1u) ? (remw & (0u - remw)) : 0u;
    uint32_t F[K];
    if (K == 1) F[0] = sb | (sw << (FW & 31));
    else { F[0] = sb; F[K - 1] = sw; }
    lat_flood<LPB, K>(F, Mk, Mkr);
    uint32_t Lb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) Lb[k] = lat_dilate<LPB>(F[k]) & Ee[k];
    const uint32_t fb = K == 1 ? (F[0] & FM) : F[0], fw = K == 1 ? ((F[0] >> (FW & 31)) & FM) : F[K - 1];
    const uint32_t lb = K == 1 ? (Lb[0] & FM) : Lb[0], lw = K == 1 ? ((Lb[0] >> (FW & 31)) & FM) : Lb[K - 1];
    const uint32_t S = lat_board_sum<LPB>((uint32_t)__popc(lb) | ((uint32_t)__popc(lw) << 16));   // (<= 361 each)
    const uint32_t nb = S & 0xFFFFu, nw = S >> 16;
    if (COUNTS) {
      const uint32_t cb = nb < 255u ? nb : 255u, cw = nw < 255u ? nw : 255u;
#pragma unroll
      for (int k = 0; k < 8; ++k) cls[k] |= (fb & (0u - ((cb >> k) & 1u))) | (fw & (0u - ((cw >> k) & 1u)));
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) cls[k] |= (nb == (uint32_t)(k + 1) ? fb : 0u) | (nw == (uint32_t)(k + 1) ? fw : 0u);
      cls[3] |= (nb >= 4u ? fb : 0u) | (nw >= 4u ? fw : 0u);
    }
    remb &= ~fb;
    remw &= ~fw;
  }
}

// gg_batch_features / gg_batch_features_tracked: out [B][16][N][N] of ESIZE-byte elements (`one`: the bit pattern of 1),
// 16-byte aligned.  One single-wave workgroup per NBW boards (grid-stride).  The body is spelled ONCE, as a macro, for the
// plain and the oriented kernel (ORIENT: null, or the orientations): as a function template shared by both, the plain kernels
// did not keep the machine code they had before the oriented ones existed (the inlined copy commuted operands and swapped
// instructions).  The emission bounds this kernel and `out` is 16-byte aligned, so it keeps its own walk with a compile-time
// element size: every store is an aligned 16-byte store (plane_store is the general form).  Two more pieces stay spelled out
// for this kernel, because as calls of the shared functions k_features<19, 1 | 2, true> went from 63 to 66 / 67 VGPRs and
// from 8 waves per SIMD to 7 (either one alone is enough for that): the zero-and-OR of the string below (plane_bits with
// mo = 0 is the same text) and the pairs and seeds inside feat_groups (plane_pair / plane_field / plane_seeds).
#define GG_FEATURES_BODY(ORIENT)                                                                                                      \
  using F_ = Feat<R>;                                                                                                                 \
  constexpr int LPB = F_::LPB, EPV = 16 / ESIZE;                                                                                      \
  __shared__ __attribute__((aligned(16))) uint32_t lds[F_::kLdsWords];                                                                \
  PlaneFrame<R> f(N);                                                                                                                 \
  const int P = N * N;                                                                                                                \
  const uint32_t full = f.full;                                                                                                       \
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {                                                                     \
    f.at(g, B);                                                                                                                       \
    uint32_t bl, wh, inv, fl;                                                                                                         \
    plane_load<R, TRACKED>(in, ORIENT, f, B, N, lds, bl, wh, inv, fl);                                                                \
    uint32_t cls[4];                                                                                                                  \
    feat_groups<R, false>(bl, wh, full, cls);                                                                                         \
    /* the sixteen rows of this lane (include/gymgo_amd.h: the table of planes) */                                                       \
    const bool white = (fl & 1u) != 0, done = (fl & 4u) != 0;                                                                         \
    const uint32_t own = white ? wh : bl, opp = white ? bl : wh;                                                                      \
    const uint32_t E = full & ~(bl | wh);                                                                                             \
    const uint32_t legal = done ? 0u : (E & ~inv);                                                                                    \
    const uint32_t cap = E & lat_dilate<LPB>(opp & cls[0]);   /* next to an opponent group whose one liberty is this point */            \
    const uint32_t rows[kFeatPlanes] = {own, opp, own & cls[0], own & cls[1], own & cls[2], own & cls[3],                             \
                                        opp & cls[0], opp & cls[1], opp & cls[2], opp & cls[3],                                       \
                                        legal, done ? 0u : (E & inv & cap), legal & cap,                                              \
                                        white ? 0u : full, (fl & 2u) ? full : 0u, full};                                              \
    /* the wave's bit-string (plane_bits, mo = 0) */                                                                                     \
    const int nbits = f.nb * kFeatPlanes * P;                                                                                         \
    for (int w = f.lane; w < ((nbits + 31) >> 5) + 1; w += kWave) lds[w] = 0;                                                         \
    WAVE_SYNC();                                                                                                                      \
    if (f.on && f.r < N) {                                                                                                            \
      const uint32_t q0 = (uint32_t)(f.j * kFeatPlanes * P + f.r * N);                                                                \
      _Pragma("unroll")                                                                                                                \
      for (int p = 0; p < kFeatPlanes; ++p) {                                                                                         \
        if (rows[p]) {                                                                                                                \
          const uint32_t q = q0 + (uint32_t)(p * P);                                                                                  \
          const uint64_t x = (uint64_t)rows[p] << (q & 31u);                                                                          \
          atomicOr(lds + (q >> 5), (uint32_t)x);                                                                                      \
          if ((uint32_t)(x >> 32)) atomicOr(lds + (q >> 5) + 1, (uint32_t)(x >> 32));                                                 \
        }                                                                                                                             \
      }                                                                                                                               \
    }                                                                                                                                 \
    WAVE_SYNC();                                                                                                                      \
    uint8_t *dst = out + f.b_first * (int64_t)(kFeatPlanes * ESIZE) * P;                                                              \
    const int nvec = f.nb * P * ESIZE;   /* = the string's bits / EPV */                                                                 \
    for (int v = f.lane; v < nvec; v += kWave) {                                                                                      \
      const uint32_t q = (uint32_t)(v * EPV);                                                                                         \
      *reinterpret_cast<V16a *>(dst + 16 * (int64_t)v) = feat_expand<ESIZE>(lds[q >> 5] >> (q & 31u), one);                           \
    }                                                                                                                                 \
    WAVE_SYNC();                                                                                                                      \
  }
template <int R, int ESIZE, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_features(const void *__restrict__ in, uint8_t *__restrict__ out, uint32_t one,
                                                    int64_t B, int N) {
  GG_FEATURES_BODY(nullptr)
}
// ... in view orient[b] (int32 [B]) of every board: gg_batch_features_oriented / gg_batch_features_tracked_oriented
template <int R, int ESIZE, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_features_oriented(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                             uint8_t *__restrict__ out, uint32_t one, int64_t B, int N) {
  GG_FEATURES_BODY(orient)
}
#undef GG_FEATURES_BODY

// gg_batch_group_liberties: libs uint8 [B][N][N] = min(liberties of the group of the stone at the point, 255), 0 at empty points
template <int R>
__global__ __launch_bounds__(kWave) void k_group_liberties(const uint8_t *__restrict__ states, uint8_t *__restrict__ libs, int64_t B,
                                                           int N) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[Feat<R>::kLdsWords];
  PlaneFrame<R> f(N);
  const int P = N * N;
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    feat_load_bytes<R>(states, f, N, lds, bl, wh, inv, fl);
    uint32_t cls[8];
    feat_groups<R, true>(bl, wh, f.full, cls);
    uint8_t *g0 = libs + f.b_first * (int64_t)P;
    uint8_t *lb = reinterpret_cast<uint8_t *>(lds) + ((uintptr_t)g0 & 15u);   // (stage_out: byte i of the slice at lds[mis + i])
    if (f.on && f.r < N) {
#pragma unroll
      for (int c = 0; c < R; ++c) {
        if (c < N) {
          uint32_t v = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) v |= ((cls[k] >> c) & 1u) << k;
          lb[f.j * P + f.r * N + c] = (uint8_t)v;
        }
      }
    }
    WAVE_SYNC();
    stage_out(g0, f.nb * P, reinterpret_cast<const uint8_t *>(lds), f.lane);
    WAVE_SYNC();
  }
}

}  // namespace gg
