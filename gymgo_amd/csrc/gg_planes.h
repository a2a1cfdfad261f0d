// gg_planes.h - what the PLANE KERNELS share (gg_feat.h: network features and group liberties, gg_life.h: pass-alive life,
// gg_ladder.h: ladders, gg_moves.h: move outcomes, gg_hash.h: position and move hashes, gg_area.h: area ownership, gg_past.h: history planes,
// gg_tactics.h: the sets of the tactical playout policy, gg_pattern.h: those of the pattern playout policy, gg_prior.h: the move priors
// of the RAVE search, gg_status.h: stone status from playout ownership).  Only those eleven units compile from this header.
//
// Layout: ONE ROW PER LANE as in gg_lat.h - a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), the rows are bit masks in registers, one single-wave workgroup per wave of boards
// (grid-stride).  A plane family writes its analysis and the rows[] of its planes; from here it takes
//   the frame      PlaneFrame: the lane's place on its board and the wave's boards of a grid-stride step;
//   the load       plane_load: byte planes (staged through LDS) or tracked rows, turned into view orient[b] in registers;
//   the pairs      plane_pair / plane_field / plane_seeds: black and white row sets side by side, as lat_flood floods them;
//   the candidate  plane_first: the next point of a per-board work list; plane_move_flood: the stones a move there captures
//                  (and the chain it makes) - one round of gg_moves.h's exact path and of gg_hash.h's capturing candidates;
//   the emission   plane_bits: the wave's planes as ONE bit-string in LDS (its boards are contiguous in the output);
//                  plane_store: the string expanded to 0 / 1 of the element type, aligned 16-byte vectors inside the wave's
//                  slice, single elements at its ragged ends, nothing outside it (plane_emit: both, for an element-aligned
//                  output);
//   the launch     plane_launch (host): argument checks, the dtype table, the owning device, the grid, the dispatch on the
//                  board-size template and the input form.
#pragma once
#include "gg_lat.h"
#include "gg_host.h"

namespace gg {

template <int R>
struct Planes {
  using L = Lat<R>;
  static constexpr int LPB = L::LPB, NBW = L::NBW, FW = L::FW;
  static constexpr int K = L::NF >= 2 ? 1 : 2;                                    // registers of a pair: two fields of one, or one per colour
  static constexpr uint32_t FM = L::FM;
  static constexpr int kIoWords = (NBW * 6 * R * R + 15 + 15 + 64) / 4 + 1;       // staged byte planes: both misalignments + plane_to_row's over-read
};
// words of the wave's bit-string of `planes` planes per board whose first bit is at most bit `mis` (+ the spill word of the last OR)
template <int R>
constexpr int plane_bs_words(int planes, int mis) { return (mis + Planes<R>::NBW * planes * R * R + 31) / 32 + 2; }

// The lane's place (fixed) and the wave's boards of the grid-stride step g (at): boards [b_first, b_first + nb) of B
template <int R>
struct PlaneFrame {
  static constexpr int LPB = Planes<R>::LPB, NBW = Planes<R>::NBW;
  int lane, r, j;     // the lane, its row of its board, its board of the wave
  uint32_t full;      // the points of the row (zero in rows >= N)
  int64_t b_first;
  int nb;
  bool on;            // this lane's board exists
  __device__ __forceinline__ explicit PlaneFrame(int N)
      : lane(threadIdx.x & (kWave - 1)), r(lane & (LPB - 1)), j(lane / LPB), full(r < N ? (1u << N) - 1u : 0u), b_first(0), nb(0),
        on(false) {}
  static __device__ __forceinline__ int64_t groups(int64_t B) { return (B + NBW - 1) / NBW; }
  __device__ __forceinline__ void at(int64_t g, int64_t B) {
    b_first = g * NBW;
    nb = (int)(B - b_first < NBW ? B - b_first : NBW);
    on = j < nb;
  }
};

// colour k's row of a pair
template <int R>
__device__ __forceinline__ uint32_t plane_field(const uint32_t (&X)[Planes<R>::K], int k) {
  constexpr int K = Planes<R>::K;
  if (K == 1) return (k ? X[0] >> (Planes<R>::FW & 31) : X[0]) & Planes<R>::FM;
  return X[k ? K - 1 : 0];
}
// the pair (b, w)
template <int R>
__device__ __forceinline__ void plane_pair(uint32_t b, uint32_t w, uint32_t (&X)[Planes<R>::K]) {
  constexpr int K = Planes<R>::K;
  if (K == 1) X[0] = b | (w << (Planes<R>::FW & 31));
  else { X[0] = b; X[K - 1] = w; }
}
// per colour, the lowest point of the first lane of the board that holds one: the seeds of a seed-and-flood round, X -> F
template <int R>
__device__ __forceinline__ void plane_seeds(const uint32_t (&X)[Planes<R>::K], uint32_t (&F)[Planes<R>::K]) {
  const uint32_t xb = plane_field<R>(X, 0), xw = plane_field<R>(X, 1);
  const uint32_t has = (xb ? 1u : 0u) | (xw ? 0x10000u : 0u);
  const uint32_t incl = lat_board_scan<Planes<R>::LPB>(has);
  const uint32_t sb = (xb != 0u && (incl & 0xFFFFu) == 1u) ? (xb & (0u - xb)) : 0u;
  const uint32_t sw = (xw != 0u && (incl >> 16) == 1u) ? (xw & (0u - xw)) : 0u;
  plane_pair<R>(sb, sw, F);
}

// the lowest point (row-major) of a row set of the board: the lowest bit of the first lane that holds one, zero elsewhere
template <int LPB> __device__ __forceinline__ uint32_t plane_first(uint32_t x) {
  const uint32_t incl = lat_board_scan<LPB>(x ? 1u : 0u);
  return (x != 0u && incl == 1u) ? (x & (0u - x)) : 0u;
}

// THE FLOODS OF ONE CANDIDATE per board, the boards of a wave in lock-step.  Q: the candidate (an empty point; one bit in the
// lane of its row, or none), own: the mover's stones, opp1: the opponent's stones of groups with exactly one liberty.
//   C = the stones a move at Q captures: the flood of (neighbours of Q in opp1) within opp1 - such a group next to the empty Q
//       has Q as its liberty, and groups of one colour never touch, so one flood gives them all;
//   G = (CHAIN) the chain of the played stone: the flood of Q within own | Q, run with the other as one pair; else 0, and
//       the capture flood runs alone in one register.
template <int R, bool CHAIN>
__device__ __forceinline__ void plane_move_flood(uint32_t own, uint32_t opp1, uint32_t Q, uint32_t &G, uint32_t &C) {
  constexpr int LPB = Planes<R>::LPB, K = Planes<R>::K;
  const uint32_t seeds = lat_dilate<LPB>(Q) & opp1;
  if constexpr (CHAIN) {
    uint32_t Mk[K], Mkr[K], F[K];
    plane_pair<R>(own | Q, opp1, Mk);
    plane_pair<R>(Q, seeds, F);
#pragma unroll
    for (int k = 0; k < K; ++k) Mkr[k] = __brev(Mk[k]);
    lat_flood<LPB, K>(F, Mk, Mkr);
    G = plane_field<R>(F, 0);
    C = plane_field<R>(F, 1);
  } else {
    uint32_t Mk[1] = {opp1}, Mkr[1] = {__brev(opp1)}, F[1] = {seeds};
    lat_flood<LPB, 1>(F, Mk, Mkr);
    G = 0;
    C = F[0];
  }
}

// The rows of the wave's boards from byte planes (uint8 [B][6][N][N]): the boards of a wave are ONE contiguous slice of HBM,
// staged with aligned 16-byte loads (stage_in), one row per lane.
template <int R>
__device__ __forceinline__ void feat_load_bytes(const uint8_t *states, const PlaneFrame<R> &f, int N, uint32_t *lds, uint32_t &bl,
                                                uint32_t &wh, uint32_t &inv, uint32_t &fl) {
  const int P = N * N, S = 6 * P;
  uint8_t *iob = reinterpret_cast<uint8_t *>(lds);
  WAVE_SYNC();
  const uint32_t mis = stage_in(states + f.b_first * (int64_t)S, f.nb * S, iob, f.lane);
  WAVE_SYNC();
  bl = wh = inv = fl = 0;
  if (f.on) {
    const uint8_t *io = iob + mis + f.j * S;
    bl = plane_to_row<R>(io, N, f.r) & f.full;
    wh = plane_to_row<R>(io + P, N, f.r) & f.full;
    inv = plane_to_row<R>(io + 3 * P, N, f.r) & f.full;
    fl = (io[2 * P] ? 1u : 0u) | (io[4 * P] ? 2u : 0u) | (io[5 * P] ? 4u : 0u);   // turn, passed, done
  }
  WAVE_SYNC();
}

// ... and from tracked boards (uint32 [B][5 N + 1]): a lane reads its own row words; the class rows are not read
template <int R>
__device__ __forceinline__ void feat_load_tracked(const uint32_t *tracked, const PlaneFrame<R> &f, int64_t B, int N, uint32_t &bl,
                                                  uint32_t &wh, uint32_t &inv, uint32_t &fl) {
  const uint32_t *gp = tracked + (f.on ? f.b_first + f.j : B - 1) * (int64_t)(5 * N + 1);
  const int rc = f.r < N ? f.r : 0;
  bl = gp[rc] & f.full; wh = gp[N + rc] & f.full; inv = gp[2 * N + rc] & f.full;
  fl = gp[5 * N] & 7u;
  if (!f.on) { bl = wh = inv = 0; fl = 0; }
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

// ORIENTED planes: the three loaded row sets of a board (black, white, invalid) are turned into view o of the board in
// registers, right after the load - everything after it works on the turned position, so the planes come out turned alike
// (all of them are geometric; the flags do not move).
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
  constexpr int LPB = Planes<R>::LPB, NX = LPB == 16 ? 2 : 3;
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

// THE LOAD: this lane's rows of black, white and invalid points (zero in rows >= N and on boards that are not there) and the
// board's flags (turn, passed, done) from byte planes or tracked boards, in view orient[b] of the board when orient is given
template <int R, bool TRACKED>
__device__ __forceinline__ void plane_load(const void *in, const int32_t *orient, const PlaneFrame<R> &f, int64_t B, int N,
                                           uint32_t *lds, uint32_t &bl, uint32_t &wh, uint32_t &inv, uint32_t &fl) {
  if (TRACKED) feat_load_tracked<R>(static_cast<const uint32_t *>(in), f, B, N, bl, wh, inv, fl);
  else feat_load_bytes<R>(static_cast<const uint8_t *>(in), f, N, lds, bl, wh, inv, fl);
  if (orient) feat_orient<R>(bl, wh, inv, f.on ? (orient[f.b_first + f.j] & 7) : 0, N, f.r, f.lane, f.full);
}

// THE WAVE'S BIT-STRING: lds[0 .. plane_bs_words) zeroed, then rows[p] of every lane ORed in at bit
// mo + j PLANES N^2 + p N^2 + r N - bit mo + e is element e of the wave's slice of an output [B][PLANES][N][N].
template <int R, int PLANES>
__device__ __forceinline__ void plane_bits(uint32_t *lds, const uint32_t (&rows)[PLANES], int mo, const PlaneFrame<R> &f, int N) {
  const int P = N * N, end = mo + f.nb * PLANES * P;
  for (int w = f.lane; w < ((end + 31) >> 5) + 1; w += kWave) lds[w] = 0;
  WAVE_SYNC();
  if (f.on && f.r < N) {
    const uint32_t q0 = (uint32_t)(mo + f.j * PLANES * P + f.r * N);
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
      if (rows[p]) {
        const uint32_t q = q0 + (uint32_t)(p * P);
        const uint64_t x = (uint64_t)rows[p] << (q & 31u);
        atomicOr(lds + (q >> 5), (uint32_t)x);
        if ((uint32_t)(x >> 32)) atomicOr(lds + (q >> 5) + 1, (uint32_t)(x >> 32));
      }
    }
  }
  WAVE_SYNC();
}

// THE STORE of a slice with element alignment only: dst = element 0 of the slice (elements of 1 << esh bytes), mo = its
// misalignment in elements = the bit of the string it sits at, nel elements.  Every aligned 16-byte vector inside the slice is
// a run of 16 >> esh bits that never crosses a word (k_features' walk); the ragged ends leave as single elements.
__device__ __forceinline__ void plane_store(uint8_t *dst, const uint32_t *lds, int mo, int nel, int esh, uint32_t one, int lane) {
  const int epv = 16 >> esh, end = mo + nel;   // elements per 16-byte vector: 16, 8, 4
  uint8_t *ga = dst - ((size_t)mo << esh);
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

// THE EMISSION of rows[] into out [B][PLANES][N][N], aligned to its element: the string, then the store
template <int R, int PLANES>
__device__ __forceinline__ void plane_emit(uint8_t *out, int esh, uint32_t one, const uint32_t (&rows)[PLANES], uint32_t *lds,
                                           const PlaneFrame<R> &f, int N) {
  uint8_t *dst = out + ((f.b_first * (int64_t)(PLANES * N * N)) << esh);
  const int mo = (int)(((uintptr_t)dst & 15u) >> esh);
  plane_bits<R, PLANES>(lds, rows, mo, f, N);
  plane_store(dst, lds, mo, f.nb * PLANES * N * N, esh, one, f.lane);
}

// THE LAUNCH (host) of a plane kernel behind its entry point.  K holds the kernel's arguments and launches it:
//   template <int R, bool TRACKED> void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const;
// in: byte planes or tracked boards (`tracked`); out: elements of dtype GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8 (esh: log2
// of their size, one: the bit pattern of 1), aligned to align_mask + 1 bytes and to its element; also: one more pointer that
// must not be null (or out again).  The checks in the order of include/gymgo_amd.h; the launch goes to the device that owns
// `in`: one single-wave workgroup per four (N <= 13) / two boards, at most 64 per compute unit (the rest: grid-stride).
template <int R, class K>
void plane_launch_r(const K &k, bool tracked, int cus, int64_t B, hipStream_t s, int esh, uint32_t one) {
  const int64_t groups = (B + Planes<R>::NBW - 1) / Planes<R>::NBW, cap = (int64_t)cus * 64;
  const unsigned grid = (unsigned)(groups < cap ? groups : cap);
  if (tracked) k.template launch<R, true>(grid, s, esh, one);
  else k.template launch<R, false>(grid, s, esh, one);
}
template <class K>
int32_t plane_launch(const K &k, bool tracked, const void *in, const void *out, const void *also, uintptr_t align_mask, int32_t dtype,
                     int64_t B, int32_t N, void *hip_stream) {
  if (N < 2 || N > GG_MAX_BOARD || B < 0 || dtype < GG_W_F32 || dtype > GG_FEAT_U8) return GG_E_BADSIZE;
  if (B == 0) return 0;
  if (!in || !out || !also) return GG_E_NULLPTR;
  static const struct { int esh; uint32_t one; } kTypes[4] = {{2, 0x3F800000u}, {1, 0x3F80u}, {1, 0x3C00u}, {0, 1u}};
  static_assert(GG_W_F32 == 0 && GG_W_BF16 == 1 && GG_W_F16 == 2 && GG_FEAT_U8 == 3, "the order of kTypes");
  const int esh = kTypes[dtype].esh;
  if ((uintptr_t)out & (align_mask | (uintptr_t)((1 << esh) - 1))) return GG_E_BADARG;
  OnDeviceOf on_dev(in);
  const int cus = on_dev.cus();
  hipStream_t s = (hipStream_t)hip_stream;
  by_rows(N, [&](auto t) { plane_launch_r<decltype(t)::R>(k, tracked, cus, B, s, esh, kTypes[dtype].one); });
  return (int32_t)hipGetLastError();
}

}  // namespace gg
