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
#include "gg_lat.h"

namespace gg {

constexpr int kFeatPlanes = 16;

template <int R>
struct Feat {
  using L = Lat<R>;
  static constexpr int LPB = L::LPB, NBW = L::NBW, FW = L::FW;
  static constexpr int K = L::NF >= 2 ? 1 : 2;                                    // flood registers: two fields of one, or one per colour
  static constexpr int kBsWords = (NBW * kFeatPlanes * R * R + 31) / 32 + 2;      // the wave's bit-string (+ the spill word of the last OR)
  static constexpr int kIoWords = (NBW * 6 * R * R + 15 + 15 + 64) / 4 + 1;       // staged byte planes: both misalignments + plane_to_row's over-read
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

// The rows of the wave's boards from byte planes (uint8 [B][6][N][N]): the boards of a wave are ONE contiguous slice of HBM,
// staged with aligned 16-byte loads (stage_in), one row per lane.  on = this lane's board exists.
template <int R>
__device__ __forceinline__ void feat_load_bytes(const uint8_t *states, int64_t b_first, int nb, int N, int r, int j, bool on,
                                                uint32_t full, uint32_t *lds, int lane, uint32_t &bl, uint32_t &wh, uint32_t &inv,
                                                uint32_t &fl) {
  const int P = N * N, S = 6 * P;
  uint8_t *iob = reinterpret_cast<uint8_t *>(lds);
  WAVE_SYNC();
  const uint32_t mis = stage_in(states + b_first * (int64_t)S, nb * S, iob, lane);
  WAVE_SYNC();
  bl = wh = inv = fl = 0;
  if (on) {
    const uint8_t *io = iob + mis + j * S;
    bl = plane_to_row<R>(io, N, r) & full;
    wh = plane_to_row<R>(io + P, N, r) & full;
    inv = plane_to_row<R>(io + 3 * P, N, r) & full;
    fl = (io[2 * P] ? 1u : 0u) | (io[4 * P] ? 2u : 0u) | (io[5 * P] ? 4u : 0u);   // turn, passed, done
  }
  WAVE_SYNC();
}

// ... and from tracked boards (uint32 [B][5 N + 1]): a lane reads its own row words; the class rows are not read
__device__ __forceinline__ void feat_load_tracked(const uint32_t *tracked, int64_t b, int N, int r, bool on, uint32_t full,
                                                  uint32_t &bl, uint32_t &wh, uint32_t &inv, uint32_t &fl) {
  const uint32_t *gp = tracked + b * (int64_t)(5 * N + 1);
  const int rc = r < N ? r : 0;
  bl = gp[rc] & full; wh = gp[N + rc] & full; inv = gp[2 * N + rc] & full;
  fl = gp[5 * N] & 7u;
  if (!on) { bl = wh = inv = 0; fl = 0; }
}

// One 16-byte vector of the output: the low 16 / ESIZE bits of x as elements of ESIZE bytes, `one` = the element's 1
template <int ESIZE>
__device__ __forceinline__ V16a feat_expand(uint32_t x, uint32_t one) {
  V16a o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (ESIZE == 1) o.w[i] = (((x >> (4 * i)) & 0xFu) * 0x00204081u) & 0x01010101u;   // four bits -> four bytes
    else if (ESIZE == 2) o.w[i] = (((x >> (2 * i)) & 1u) ? one : 0u) | (((x >> (2 * i + 1)) & 1u) ? (one << 16) : 0u);
    else o.w[i] = ((x >> i) & 1u) ? one : 0u;
  }
  return o;
}

// ORIENTED planes (gg_batch_features_oriented / gg_batch_features_tracked_oriented): the three loaded row sets of a board
// (black, white, invalid) are turned into view o of the board in registers, right after the load - everything after it works
// on the turned position, so the sixteen planes come out turned alike (all of them are geometric; the flags do not move).
// The geometry is k_symmetry_rows' (gg_sym.h), in this layout:
//   no rotation:  out[r] bit c = x[R(r)] bit C(c)          R = the row flip: a lane permutation inside the board's lanes,
//   rotation:     out[r] bit c = xt[C(N-1-r)] bit R(c)     C = the column flip: a bit reversal of the row; xt = the transpose
// The transpose is the block-swap network over the board's lanes: four stages for a board of 16 lanes, five for 32.  Every
// stage is one lane exchange at a fixed distance: DPP quad permutes (1, 2), a DPP row rotation (8), ds_swizzle in bit mode
// (4, 16: no DPP control swaps at those distances inside a row of 16 / across two) - none touches memory.  The stage masks
// are periodic in 16 bits, so a board of 16 lanes transposes TWO row sets at once, one per half of a register.  The row
// selection is one ds_bpermute per register: its source depends on the board's own orientation, which differs from board to
// board of a wave.  A wave none of whose boards rotates skips the stages.
template <int J> __device__ __forceinline__ uint32_t feat_xchg(uint32_t x) {   // lane i reads lane i ^ J
  if (J == 1) return dpp0<0xB1>(x);         // quad_perm [1, 0, 3, 2]
  else if (J == 2) return dpp0<0x4E>(x);    // quad_perm [2, 3, 0, 1]
  else if (J == 8) return dpp0<0x128>(x);   // row_ror:8
  else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, (J << 10) | 0x1F);   // and 0x1F, or 0, xor J
}
template <int J> __device__ __forceinline__ uint32_t feat_tstage(uint32_t xt, int r) {
  constexpr uint32_t LOWM = J == 16 ? 0x0000FFFFu : J == 8 ? 0x00FF00FFu : J == 4 ? 0x0F0F0F0Fu : J == 2 ? 0x33333333u : 0x55555555u;
  const uint32_t y = feat_xchg<J>(xt);
  const uint32_t up = (xt & LOWM) | ((y & LOWM) << J);      // (r & J) == 0: the partner's low column blocks into the high ones
  const uint32_t dn = (xt & ~LOWM) | ((y & ~LOWM) >> J);    // (r & J) != 0: the partner's high blocks into the low ones
  return (r & J) ? dn : up;
}
// bit c of row r <- bit r of row c over the board's LPB lanes (LPB = 16: in both halves of the register)
template <int LPB> __device__ __forceinline__ uint32_t feat_transpose(uint32_t x, int r) {
  if (LPB == 32) x = feat_tstage<16>(x, r);
  x = feat_tstage<8>(x, r);
  x = feat_tstage<4>(x, r);
  x = feat_tstage<2>(x, r);
  return feat_tstage<1>(x, r);
}
// bl / wh / inv of every board of the wave -> view o of the board (o: this lane's board's orientation, 0 .. 7)
template <int R>
__device__ __forceinline__ void feat_orient(uint32_t &bl, uint32_t &wh, uint32_t &inv, int o, int N, int r, int lane, uint32_t full) {
  constexpr int LPB = Feat<R>::LPB, NX = LPB == 16 ? 2 : 3;
  uint32_t x[NX];
  if (LPB == 16) { x[0] = bl | (wh << 16); x[NX - 1] = inv; }
  else { x[0] = bl; x[1] = wh; x[NX - 1] = inv; }
  const bool rot = (o & 4) != 0;
  if (__ballot(rot) != 0ull) {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const uint32_t xt = feat_transpose<LPB>(x[k], r);
      x[k] = rot ? xt : x[k];
    }
  }
  // the source row: C(N-1-r) of the transposed set, R(r) of the plain one; then the reversal of the row's bits
  const bool down = rot ? (o & 1) == 0 : (o & 2) != 0;
  const int srow = r < N ? (down ? N - 1 - r : r) : 0;
  const int src = ((lane & ~(LPB - 1)) + srow) << 2;
  const bool rev = rot ? (o & 2) != 0 : (o & 1) != 0;
  const uint32_t sh = (uint32_t)(32 - N);
#pragma unroll
  for (int k = 0; k < NX; ++k) x[k] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)x[k]);
  uint32_t y[3];
  if (LPB == 16) { y[0] = x[0] & 0xFFFFu; y[1] = x[0] >> 16; y[2] = x[NX - 1]; }
  else { y[0] = x[0]; y[1] = x[1]; y[2] = x[NX - 1]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = (rev ? __brev(y[k]) >> sh : y[k]) & full;
  bl = y[0]; wh = y[1]; inv = y[2];
}

// gg_batch_features / gg_batch_features_tracked: out [B][16][N][N] of ESIZE-byte elements (`one`: the bit pattern of 1),
// 16-byte aligned.  One single-wave workgroup per NBW boards (grid-stride).  The body is spelled ONCE, as a macro, for the
// plain and the oriented kernel (TURN: the statement between the load and the analysis): the plain kernels then compile from
// the token sequence they had before the oriented ones existed and keep their machine code instruction for instruction - as
// a function template shared by both they did not (the inlined copy commuted operands and swapped instructions).
#define GG_FEATURES_BODY(TURN)                                                                                                        \
  using F_ = Feat<R>;                                                                                                                 \
  constexpr int LPB = F_::LPB, NBW = F_::NBW, EPV = 16 / ESIZE;                                                                       \
  __shared__ __attribute__((aligned(16))) uint32_t lds[F_::kLdsWords];                                                                \
  const int lane = threadIdx.x & (kWave - 1);                                                                                         \
  const int r = lane & (LPB - 1), j = lane / LPB;                                                                                     \
  const int P = N * N;                                                                                                                \
  const uint32_t full = r < N ? (1u << N) - 1u : 0u;                                                                                  \
  const int64_t ngroups = (B + NBW - 1) / NBW;                                                                                        \
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {                                                                         \
    const int64_t b_first = g * NBW;                                                                                                  \
    const int nb = (int)(B - b_first < NBW ? B - b_first : NBW);                                                                      \
    const bool on = j < nb;                                                                                                           \
    uint32_t bl, wh, inv, fl;                                                                                                         \
    if (TRACKED) feat_load_tracked(static_cast<const uint32_t *>(in), on ? b_first + j : B - 1, N, r, on, full, bl, wh, inv, fl);     \
    else feat_load_bytes<R>(static_cast<const uint8_t *>(in), b_first, nb, N, r, j, on, full, lds, lane, bl, wh, inv, fl);            \
    TURN;                                                                                                                             \
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
    /* the wave's bit-string */                                                                                                          \
    const int nbits = nb * kFeatPlanes * P;                                                                                           \
    for (int w = lane; w < ((nbits + 31) >> 5) + 1; w += kWave) lds[w] = 0;                                                           \
    WAVE_SYNC();                                                                                                                      \
    if (on && r < N) {                                                                                                                \
      const uint32_t q0 = (uint32_t)(j * kFeatPlanes * P + r * N);                                                                    \
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
    uint8_t *dst = out + b_first * (int64_t)(kFeatPlanes * ESIZE) * P;                                                                \
    const int nvec = nb * P * ESIZE;   /* = nbits / EPV */                                                                               \
    for (int v = lane; v < nvec; v += kWave) {                                                                                        \
      const uint32_t q = (uint32_t)(v * EPV);                                                                                         \
      *reinterpret_cast<V16a *>(dst + 16 * (int64_t)v) = feat_expand<ESIZE>(lds[q >> 5] >> (q & 31u), one);                           \
    }                                                                                                                                 \
    WAVE_SYNC();                                                                                                                      \
  }
template <int R, int ESIZE, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_features(const void *__restrict__ in, uint8_t *__restrict__ out, uint32_t one,
                                                    int64_t B, int N) {
  GG_FEATURES_BODY((void)0)
}
// ... in view orient[b] (int32 [B]) of every board: gg_batch_features_oriented / gg_batch_features_tracked_oriented
template <int R, int ESIZE, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_features_oriented(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                             uint8_t *__restrict__ out, uint32_t one, int64_t B, int N) {
  GG_FEATURES_BODY(feat_orient<R>(bl, wh, inv, on ? (orient[b_first + j] & 7) : 0, N, r, lane, full))
}
#undef GG_FEATURES_BODY

// gg_batch_group_liberties: libs uint8 [B][N][N] = min(liberties of the group of the stone at the point, 255), 0 at empty points
template <int R>
__global__ __launch_bounds__(kWave) void k_group_liberties(const uint8_t *__restrict__ states, uint8_t *__restrict__ libs, int64_t B,
                                                           int N) {
  using F_ = Feat<R>;
  constexpr int LPB = F_::LPB, NBW = F_::NBW;
  __shared__ __attribute__((aligned(16))) uint32_t lds[F_::kLdsWords];
  const int lane = threadIdx.x & (kWave - 1);
  const int r = lane & (LPB - 1), j = lane / LPB;
  const int P = N * N;
  const uint32_t full = r < N ? (1u << N) - 1u : 0u;
  const int64_t ngroups = (B + NBW - 1) / NBW;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t b_first = g * NBW;
    const int nb = (int)(B - b_first < NBW ? B - b_first : NBW);
    const bool on = j < nb;
    uint32_t bl, wh, inv, fl;
    feat_load_bytes<R>(states, b_first, nb, N, r, j, on, full, lds, lane, bl, wh, inv, fl);
    uint32_t cls[8];
    feat_groups<R, true>(bl, wh, full, cls);
    uint8_t *g0 = libs + b_first * (int64_t)P;
    uint8_t *lb = reinterpret_cast<uint8_t *>(lds) + ((uintptr_t)g0 & 15u);   // (stage_out: byte i of the slice at lds[mis + i])
    if (on && r < N) {
#pragma unroll
      for (int c = 0; c < R; ++c) {
        if (c < N) {
          uint32_t v = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) v |= ((cls[k] >> c) & 1u) << k;
          lb[j * P + r * N + c] = (uint8_t)v;
        }
      }
    }
    WAVE_SYNC();
    stage_out(g0, nb * P, reinterpret_cast<const uint8_t *>(lds), lane);
    WAVE_SYNC();
  }
}

}  // namespace gg
