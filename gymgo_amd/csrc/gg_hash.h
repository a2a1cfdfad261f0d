// gg_hash.h - POSITION HASHES AND POSITIONAL SUPERKO (gg_batch_hash, gg_batch_hash_tracked, gg_batch_move_hashes,
// gg_batch_move_hashes_tracked, gg_puct_superko of include/gymgo_amd.h): the 64-bit Zobrist hash of every
// board, the hash of the position after every move of the mover WITHOUT building the child, the moves that would recreate a
// position of the board's history, and - for the leaves of a PUCT round - those that would recreate a position of the leaf's
// own ancestors in its tree.
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
//
// THE TREE'S RULE (k_puct_superko): the boards are the played leaves of a select launch, row i = slot i % L of root
// i / L with y = leaf_id[i], m = move[i].  A row with y < 1, y > C or m < 0 is SKIPPED: it is given no candidates, so it takes
// part in nothing below and no byte of it is written.  The other rows get their move hashes staged exactly as k_move_hashes
// stages them (hash_stage_moves: the one body of both kernels), node_hash[r][y] = the leaf's own hash, and then THE CHAIN:
// the ancestors of y are a pointer chase through links, which is read ONCE PER BOARD and never per candidate.  The wave takes
// its boards one after the other; every lane follows the chase with the same wave-uniform node (the loads are uniform), lane k
// keeps the k-th ancestor of the chunk, and after at most kChainChunk = 64 steps the lanes fetch their ancestors' hashes side by
// side and stage them in LDS.  Every staged candidate of the board is then compared against the chunk (a lane holds the hashes
// of its points a = lane + 64 p in registers for the whole board; a chunk entry is read once per lane, one LDS address for the
// wave, a broadcast), and the next chunk is fetched.  The history's valid
// entries go through the same chunk and the same compare, kChainChunk at a time.  Hits are ORed into the lane-of-the-row words
// in LDS and leave as ONE vector store per row that has a hit, into words [2N, 3N) of the leaf.  A board without candidates - a
// game that is over, a skipped row - does no walk and no history read.
// Bounds: the chase goes on only while the parent p of x satisfies 0 <= p < x, so the node falls strictly, it stays inside
// the root's C + 1 nodes, and it ends at node 0 at the latest; a step counter stops it after C steps whatever links holds.
// The chunk loop therefore runs at most C / kChainChunk + 1 times, the history loop H / kChainChunk + 1 times, the compare
// over at most kChainChunk entries for each of at most ceil(N^2 / 64) points of a lane.
// No race between the slots of a root: the launch reads node_hash only at ancestors, which are evaluated nodes of earlier
// rounds, and writes it only at nodes made in this round; such a node is never on another slot's path (collision rule a of
// gg_puct_select_leaves), and an ended node taken by several slots has m = -1 and is skipped.
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
constexpr int kChainChunk = kWave;   // ancestors (or history entries) staged per compare of k_puct_superko: one per lane

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

// THE MOVE HASHES OF THE WAVE'S BOARDS, staged: hs [nb][N^2 + 1] in LDS as they lie in the output, lcand[lane] = this lane's
// candidates, lrep[lane] = 0 (the repeat points to come).  bl / wh: the lane's rows, white: the mover, cand: the candidate
// points of the lane's row (none on a board that is not there).  -> the board's own hash.  The body of k_move_hashes and of
// k_puct_superko; it ends without a WAVE_SYNC: the caller's comes before the first read of hs.
template <int R, bool TRACKED>
__device__ __forceinline__ uint64_t hash_stage_moves(const void *in, const PlaneFrame<R> &f, int64_t B, int N, uint32_t bl, uint32_t wh,
                                                     bool white, uint32_t cand, uint64_t *hs, uint32_t *lcand, uint32_t *lrep) {
  constexpr int LPB = Hash<R>::LPB;
  const int P = N * N, A = P + 1;
  const uint32_t own = white ? wh : bl, opp = white ? bl : wh;
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
  return base;
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
    const uint32_t E = f.full & ~(bl | wh);
    const uint32_t cand = over ? 0u : (E & ~inv);   // k_moves' candidates
    hash_stage_moves<R, TRACKED>(in, f, B, N, bl, wh, white, cand, hs, lcand, lrep);
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

// gg_puct_superko: the played leaves of a select launch (leaf uint32 [B][5 N + 1], B = roots x L; move, leaf_id int32 [B]) get the
// points that would recreate a position of their game's history or of their own ancestors ORed into their invalid rows, and
// node_hash [roots][C + 1] gets the leaves' own hashes.  The scheme and its bounds: the head of this file.
template <int R>
__global__ __launch_bounds__(kWave) void k_puct_superko(uint32_t *leaf, const int32_t *__restrict__ move,
                                                        const int32_t *__restrict__ leaf_id, const int32_t *__restrict__ links,
                                                        int64_t *node_hash, const int64_t *__restrict__ history,
                                                        const int32_t *__restrict__ count, int H, int C, int L, int64_t B, int N) {
  using H_ = Hash<R>;
  constexpr int LPB = H_::LPB, kChunkAt = (H_::kLdsWords + 1) & ~1;
  __shared__ __attribute__((aligned(16))) uint32_t lds[kChunkAt + 2 * kChainChunk];
  uint64_t *hs = reinterpret_cast<uint64_t *>(lds);   // [nb][A]
  uint32_t *lcand = lds + H_::kMain, *lrep = lcand + kWave;
  uint64_t *chunk = reinterpret_cast<uint64_t *>(lds + kChunkAt);   // [kChainChunk]
  PlaneFrame<R> f(N);
  const int P = N * N, A = P + 1, W = 5 * N + 1;
  const int64_t NN = (int64_t)C + 1;
  // A lane's points of a board: a = lane + 64 p.  Their staged hashes stay in registers for all the chunks of the board, so a
  // chunk entry is read ONCE per lane (one LDS address for the wave: a broadcast) and compared with every one of them.
  constexpr int kPts = (R * R + kWave - 1) / kWave;
  uint64_t v[kPts];
  uint32_t hit = 0;   // bit p: point p's hash is in the forbidden set (bits of points that are no candidates are dropped)
  auto compare = [&](int k) {
#pragma unroll 1
    for (int e = 0; e < k; ++e) {   // (k <= kChainChunk trips)
      const uint64_t c = chunk[e];
#pragma unroll
      for (int p = 0; p < kPts; ++p) hit |= (v[p] == c ? 1u : 0u) << p;
    }
  };
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, true>(leaf, nullptr, f, B, N, lds, bl, wh, inv, fl);
    const int64_t i = f.on ? f.b_first + f.j : B - 1;
    const int y = leaf_id[i], m = move[i];
    const bool marked = f.on && y >= 1 && y <= C && m >= 0;   // (else: an empty slot, a node evaluated again, the root)
    const bool white = (fl & 1u) != 0, over = (fl & 4u) != 0;
    const uint32_t cand = (over || !marked) ? 0u : (f.full & ~(bl | wh) & ~inv);
    const uint64_t base = hash_stage_moves<R, true>(leaf, f, B, N, bl, wh, white, cand, hs, lcand, lrep);
    if (marked && f.r == 0) node_hash[(i / L) * NN + y] = (int64_t)base;
    WAVE_SYNC();
    for (int j = 0; j < f.nb; ++j) {   // the wave's boards one after the other: everything below is wave-uniform
      if (__ballot(f.j == j && cand != 0u) == 0ull) continue;   // no candidates: no walk
      const int64_t ij = f.b_first + j, root = ij / L, n0 = root * NN;
      uint32_t valid = 0;
      hit = 0;
#pragma unroll
      for (int p = 0; p < kPts; ++p) {
        const int a = f.lane + p * kWave, y = a / N, x = a - y * N;
        const bool is = a < P && ((lcand[j * LPB + y] >> x) & 1u);
        v[p] = is ? hs[j * A + a] : 0ull;
        valid |= (is ? 1u : 0u) << p;
      }
      if (history) {
        const int cn = __builtin_amdgcn_readfirstlane(count[root]);
        const int n = cn < 0 ? 0 : (cn < H ? cn : H);   // the game's valid entries
#pragma unroll 1
        for (int e0 = 0; e0 < n; e0 += kChainChunk) {   // (n <= H)
          const int k = n - e0 < kChainChunk ? n - e0 : kChainChunk;
          WAVE_SYNC();
          if (f.lane < k) chunk[f.lane] = (uint64_t)history[root * (int64_t)H + e0 + f.lane];
          WAVE_SYNC();
          compare(k);
        }
      }
      // the chain: x falls from the leaf through its parents; lane k keeps the k-th ancestor of the chunk
      int x = __builtin_amdgcn_readfirstlane(leaf_id[ij]), steps = 0;
      bool more = true;
#pragma unroll 1
      while (more) {   // (at most C / kChainChunk + 1 trips: a trip that stages nothing is the last)
        int k = 0, mine = 0;
#pragma unroll 1
        for (; k < kChainChunk; ++k) {
          if (steps >= C) { more = false; break; }
          const int p = __builtin_amdgcn_readfirstlane(links[(n0 + x) * 2]);
          if (p < 0 || p >= x) { more = false; break; }   // (node 0's parent is -1; corrupt links end the walk here)
          if (f.lane == k) mine = p;
          x = p;
          ++steps;
        }
        if (k == 0) break;
        WAVE_SYNC();
        if (f.lane < k) chunk[f.lane] = (uint64_t)node_hash[n0 + mine];
        WAVE_SYNC();
        compare(k);
      }
      hit &= valid;
#pragma unroll
      for (int p = 0; p < kPts; ++p) {
        if ((hit >> p) & 1u) {
          const int a = f.lane + p * kWave, y = a / N;
          atomicOr(lrep + j * LPB + y, 1u << (a - y * N));
        }
      }
    }
    WAVE_SYNC();
    if (marked && f.r < N) {
      const uint32_t rep = lrep[f.lane];
      if (rep) {
        uint32_t *w = leaf + i * (int64_t)W + 2 * N + f.r;
        *w = *w | rep;
      }
    }
    WAVE_SYNC();
  }
}

}  // namespace gg
