// gg_hash.h - POSITION HASHES AND POSITIONAL SUPERKO (gg_batch_hash, gg_batch_hash_tracked, gg_batch_move_hashes,
// gg_batch_move_hashes_tracked of include/gymgo_amd.h): the 64-bit Zobrist hash of every board, the hash of the
// position after every move of the mover WITHOUT building the child, and the moves that would recreate a position of the
// board's history.
//
// Layout: gg_feat.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards.
//
// THE KEYS (kHashKeys): key(c, y, x) = output number c 361 + y 19 + x + 1 of splitmix_next started at GG_HASH_SEED, for
// 19 x 19 whatever N is.  They are a constexpr table of 722 words (5 776 B) in the code object: no host-side initialisation, so
// the library keeps no state for them, and a key is ONE cached 8-byte load where computing it costs two 64-bit multiplies -
// some thirty VALU instructions, which a lone wave pays in full (a lane needs the N keys of its row per colour).
//
// THE BASE HASH: a lane XORs the keys of its row's stones, lat_board_xor folds the board's lanes (DPP, no LDS).
// THE MOVE HASHES, two paths:
//   1. a candidate that is not next to a one-liberty opponent group captures nothing: base ^ key(mover, p), every column of
//      the lane's row in one loop;
//   2. the others one per board and round, the boards of a wave in lock-step (moves_exact's rounds): the captured stones C by
//      plane_move_flood (the capture flood alone), X(C) = the XOR of their keys over the lanes, base ^ key(mover, p) ^ X(C).
// opp1, the opponent's stones in atari: feat_groups for byte planes; a tracked board carries it - its class rows hold the
// stones with >= 2 liberties, so opp1 = the opponent's stones outside them, and no group round runs at all.
// The wave's hashes are staged in LDS (the staged input is dead by then) as they lie in the output: [nb][N^2 + 1] words of
// 64 bits.  From there: the hashes themselves, the repeat bytes (lanes stride over the actions and compare against the
// board's valid history entries) and the repeat points as row masks.  Every store is a vector store inside the wave's slice.
// Every loop is bounded: a capture round takes a candidate off every board that has one, the history loop runs over at most H
// entries, the key loops over the set bits of a row.
#pragma once
#include "gg_feat.h"

namespace gg {

constexpr uint64_t kHashSeed = 0x676F2D6861736821ull;
constexpr int kHashKeys = 2 * 19 * 19;

struct HashKeyTable {
  uint64_t k[kHashKeys];
};
constexpr HashKeyTable hash_make_keys() {
  HashKeyTable t{};
  uint64_t x = kHashSeed;
  for (int i = 0; i < kHashKeys; ++i) {   // splitmix_next of gg_common.h, spelled again: that one is a device function
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    t.k[i] = z ^ (z >> 31);
  }
  return t;
}
static __device__ const HashKeyTable kHashTable = hash_make_keys();

template <int R>
struct Hash {
  using Pl = Planes<R>;
  static constexpr int LPB = Pl::LPB, NBW = Pl::NBW;
  static constexpr int kOutWords = 2 * NBW * (R * R + 1);   // the wave's hashes on their way out (64 bits each)
  static constexpr int kMain = kOutWords > Pl::kIoWords ? kOutWords : Pl::kIoWords;   // (the staged input is dead by then)
  static constexpr int kLdsWords = kMain + 2 * kWave;       // + per lane: its candidates, its repeat points
};

// the XOR of the keys of colour c (0 black, 1 white) at the points `row` of row r.  At most popc(row) <= 19 trips.
__device__ __forceinline__ uint64_t hash_row(uint32_t row, int c, int r) {
  const uint64_t *k = kHashTable.k + c * 361 + r * 19;
  uint64_t h = 0;
#pragma unroll 1
  while (row) {
    h ^= k[__ffs((int)row) - 1];
    row &= row - 1u;
  }
  return h;
}

// the hash of this lane's board (zero on boards that are not there), in every lane of the board
template <int LPB> __device__ __forceinline__ uint64_t hash_base(uint32_t bl, uint32_t wh, int r) {
  const int rc = r < 19 ? r : 0;   // (rows >= N hold no stones; the key row stays inside the table)
  return lat_board_xor<LPB>(hash_row(bl, 0, rc) ^ hash_row(wh, 1, rc));
}

// this lane's rows of a tracked board's stones with >= 2 liberties (black | white), as feat_load_tracked reads the others
template <int R>
__device__ __forceinline__ uint32_t hash_load_classes(const uint32_t *tracked, const PlaneFrame<R> &f, int64_t B, int N) {
  const uint32_t *gp = tracked + (f.on ? f.b_first + f.j : B - 1) * (int64_t)(5 * N + 1);
  const int rc = f.r < N ? f.r : 0;
  const uint32_t m = gp[3 * N + rc] | gp[4 * N + rc];
  return f.on ? m & f.full : 0u;
}

// gg_batch_hash / gg_batch_hash_tracked: out int64 [B].  One single-wave workgroup per NBW boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_hash(const void *__restrict__ in, int64_t *__restrict__ out, int64_t B, int N) {
  constexpr int LPB = Hash<R>::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Planes<R>::kIoWords];
  PlaneFrame<R> f(N);
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, nullptr, f, B, N, lds, bl, wh, inv, fl);
    const uint64_t base = hash_base<LPB>(bl, wh, f.r);
    if (f.on && f.r == 0) out[f.b_first + f.j] = (int64_t)base;
  }
}

// gg_batch_move_hashes / gg_batch_move_hashes_tracked: hashes int64 [B][N^2 + 1], repeat uint8 [B][N^2 + 1], rows uint32
// [B][N] - each may be null; history int64 [B][H] and count int32 [B] (read only when repeat or rows is asked for).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_move_hashes(const void *__restrict__ in, const int64_t *__restrict__ history,
                                                       const int32_t *__restrict__ count, int H, int64_t *__restrict__ hashes,
                                                       uint8_t *__restrict__ repeat, uint32_t *__restrict__ rows, int64_t B, int N) {
  using H_ = Hash<R>;
  constexpr int LPB = H_::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[H_::kLdsWords];
  uint64_t *hs = reinterpret_cast<uint64_t *>(lds);   // [nb][A]
  uint32_t *lcand = lds + H_::kMain, *lrep = lcand + kWave;
  PlaneFrame<R> f(N);
  const int P = N * N, A = P + 1;
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, nullptr, f, B, N, lds, bl, wh, inv, fl);
    const bool white = (fl & 1u) != 0, over = (fl & 4u) != 0;
    const uint32_t own = white ? wh : bl, opp = white ? bl : wh;
    const uint32_t E = f.full & ~(bl | wh);
    const uint32_t cand = over ? 0u : (E & ~inv);   // k_moves' candidates
    uint32_t opp1;
    if constexpr (TRACKED) {
      opp1 = opp & ~hash_load_classes<R>(static_cast<const uint32_t *>(in), f, B, N);
    } else {
      uint32_t cls[4];
      feat_groups<R, false>(bl, wh, f.full, cls);
      opp1 = opp & cls[0];
    }
    const uint64_t base = hash_base<LPB>(bl, wh, f.r);
    uint32_t todo = cand & lat_dilate<LPB>(opp1);
    const uint32_t quiet = cand & ~todo;
    const int rc = f.r < N ? f.r : 0;
    const uint64_t *kown = kHashTable.k + (white ? 361 : 0) + rc * 19;
    // path 1 and every point that is no candidate; the pass.  (plane_load has closed its use of the buffer.)
    uint64_t *hb = hs + f.j * A;
    if (f.on && f.r < N) {
#pragma unroll 1
      for (int c = 0; c < N; ++c)   // (N <= 19 trips)
        hb[f.r * N + c] = base ^ (((quiet >> c) & 1u) ? kown[c] : 0ull);
      if (f.r == 0) hb[P] = base;
    }
    lcand[f.lane] = cand;
    lrep[f.lane] = 0;
    // path 2: one capturing candidate per board and round
#pragma unroll 1
    for (int it = 0; it < R * R + 1; ++it) {   // (a round takes a point off every board that still has one)
      if (__ballot(todo != 0u) == 0ull) break;
      const uint32_t Q = plane_first<LPB>(todo);
      todo &= ~Q;
      uint32_t G, C;
      plane_move_flood<R, false>(own, opp1, Q, G, C);
      const uint64_t X = lat_board_xor<LPB>(hash_row(C, white ? 0 : 1, rc));
      if (Q) {   // (only on a board that is there, in a row < N)
        const int c = __ffs((int)Q) - 1;
        hb[f.r * N + c] = base ^ kown[c] ^ X;
      }
    }
    WAVE_SYNC();
    const int64_t a0 = f.b_first * (int64_t)A;
    if (hashes)
      for (int i = f.lane; i < f.nb * A; i += kWave) hashes[a0 + i] = (int64_t)hs[i];   // (8-byte stores, consecutive lanes)
    if (repeat || rows) {
      for (int j = 0; j < f.nb; ++j) {
        const int64_t b = f.b_first + j;
        const int32_t cn = count[b];
        const int n = cn < 0 ? 0 : (cn < H ? cn : H);   // the board's valid entries
        const int64_t *hist = history + b * (int64_t)H;
        for (int a = f.lane; a < A; a += kWave) {
          const int y = a / N, x = a - y * N;
          bool hit = false;
          if (a < P && ((lcand[j * LPB + y] >> x) & 1u)) {   // (the pass and a point that is no candidate: never)
            const int64_t v = (int64_t)hs[j * A + a];
#pragma unroll 1
            for (int e = 0; e < n; ++e) hit |= hist[e] == v;   // (n <= H trips)
          }
          if (repeat) repeat[a0 + j * A + a] = hit ? 1 : 0;
          if (hit) atomicOr(lrep + j * LPB + y, 1u << x);
        }
      }
      WAVE_SYNC();
      if (rows && f.on && f.r < N) rows[(f.b_first + f.j) * (int64_t)N + f.r] = lrep[f.lane];
    }
    WAVE_SYNC();
  }
}

}  // namespace gg
