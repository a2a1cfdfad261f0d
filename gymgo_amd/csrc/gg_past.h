// gg_past.h - HISTORY INPUT PLANES (gg_past_push, gg_batch_past, gg_puct_past and their tracked forms of
// include/gymgo_amd_past.h): the stones of the last T positions of a game and the points of its last T - 1 moves,
// from the mover's view, in one launch - AlphaGo Zero's history planes and KataGo's recent-move planes from one family.
//
// Layout: gg_planes.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards (grid-stride).
//
// THE RING (rows uint32 [B][H][2][N], count int32 [B]): the positions strictly BEFORE the current one, black rows then white
// rows per entry, bit c = column c as in tracked boards.  A push writes entry count % H and then count + 1, so the position
// t >= 1 plies ago is entry (count - t) mod H and exists iff t <= min(max(count, 0), H).  Black rows at p, white rows at p + N:
// the first 2 N words of a tracked board have the same shape, so one pointer per position serves the ring and the tree alike.
//
// THE PLANES, for a board whose turn flag at position 0 is s (T positions, `moves` 0 / 1):
//   2 t      (t = 0 .. T-1)   the stones at position t of the colour to move NOW (position 0's mover, whoever moved then)
//   2 t + 1                   the other colour's stones at position t
//   2 T + t  (t = 0 .. T-2)   with moves: occ_t & ~occ_{t+1} where position t + 1 exists, else empty - moves only add one
//                             stone and remove captured ones, and suicide is illegal, so that is exactly the point played t
//                             plies ago, and nothing for a pass
// A position that does not exist gives empty planes.  Every row read from a ring or a tree is ANDed with PlaneFrame::full, so
// garbage there cannot reach a point outside the board.  Only stones and the turn flag are read.
//
// THE LOADS of the T - 1 earlier positions are independent of each other: a lane computes their 2 (T - 1) addresses - always
// inside the ring or the tree, whether the position exists or not - issues them together, and masks afterwards.
// ORIENTATION: position 0 is turned by plane_load, the earlier positions by feat_orient three row sets at a time, all into
// the same view orient[b] of their board.
//
// EMISSION (past_emit): plane_emit of gg_planes.h takes its plane count as a template parameter; here it is a run-time
// number.  The lane's rows sit in ONE fixed array of kPastSlots = 23 - slots 0 .. 15 the stones of positions 0 .. 7, slots
// 16 .. 22 the moves -, statically indexed by a loop unrolled to 23; slot k goes to plane k (k < 2 T) or 2 T + k - 16
// (moves, k - 16 < T - 1) of the wave's bit-string and is skipped otherwise.  plane_store then writes the string as it does
// for every family.
#pragma once
#include "gg_planes.h"

namespace gg {

constexpr int kPastMaxT = 8;
constexpr int kPastSlots = 2 * kPastMaxT + (kPastMaxT - 1);   // 23: the most planes a board can have

__host__ __device__ constexpr int past_planes(int T, int moves) { return 2 * T + (moves ? T - 1 : 0); }

template <int R>
struct Past {
  static constexpr int LPB = Planes<R>::LPB;
  static constexpr int kBsWords = plane_bs_words<R>(kPastSlots, 15);
  static constexpr int kLdsWords = kBsWords > Planes<R>::kIoWords ? kBsWords : Planes<R>::kIoWords;   // (the staged input is dead by then)
};

// THE EMISSION of the slots into out [B][planes][N][N], aligned to its element: plane_bits with a run-time plane count over
// the fixed slot array, then plane_store
template <int R>
__device__ __forceinline__ void past_emit(uint8_t *out, int esh, uint32_t one, const uint32_t (&slots)[kPastSlots], int T, int moves,
                                          uint32_t *lds, const PlaneFrame<R> &f, int N) {
  const int planes = past_planes(T, moves), P = N * N;
  uint8_t *dst = out + ((f.b_first * (int64_t)(planes * P)) << esh);
  const int mo = (int)(((uintptr_t)dst & 15u) >> esh), end = mo + f.nb * planes * P;
  for (int w = f.lane; w < ((end + 31) >> 5) + 1; w += kWave) lds[w] = 0;
  WAVE_SYNC();
  if (f.on && f.r < N) {
    const uint32_t q0 = (uint32_t)(mo + f.j * planes * P + f.r * N);
#pragma unroll
    for (int k = 0; k < kPastSlots; ++k) {
      const bool stone = k < 2 * kPastMaxT;
      const int p = stone ? k : 2 * T + (k - 2 * kPastMaxT);
      const bool wanted = stone ? k < 2 * T : (moves && k - 2 * kPastMaxT < T - 1);
      if (wanted && slots[k]) {
        const uint32_t q = q0 + (uint32_t)(p * P);
        const uint64_t x = (uint64_t)slots[k] << (q & 31u);
        atomicOr(lds + (q >> 5), (uint32_t)x);
        if ((uint32_t)(x >> 32)) atomicOr(lds + (q >> 5) + 1, (uint32_t)(x >> 32));
      }
    }
  }
  WAVE_SYNC();
  plane_store(dst, lds, mo, f.nb * planes * P, esh, one, f.lane);
}

// The ring's word of board b, position k >= 1 plies before the ring's newest side (cn = count[b]): -> whether it exists;
// p = the lane's black row word of that entry (of entry 0 when it does not exist: an address inside the ring either way)
__device__ __forceinline__ bool past_ring_at(const uint32_t *rows, int64_t b, int cn, int H, int k, int N, int rc, const uint32_t *&p) {
  const int have = cn < 0 ? 0 : (cn < H ? cn : H);
  const bool ex = k <= have;
  const int e = ex ? (cn - k) % H : 0;   // (cn >= k >= 1 there)
  p = rows + ((b * H + e) * 2) * (int64_t)N + rc;
  return ex;
}

// THE BODY both plane kernels share.  bl / wh / fl: position 0 as plane_load gives it (turned already when o is given);
// p[t] / ex bit t (t = 1 .. T-1): the lane's black row word of position t - white at p[t] + N - and whether the position
// exists; load: whether p[] may be read at all (no ring and no tree: every earlier position is absent).  o: this lane's
// board's orientation, turn: whether to apply it.
template <int R>
__device__ __forceinline__ void past_body(uint32_t bl, uint32_t wh, uint32_t fl, const uint32_t *const (&p)[kPastMaxT], uint32_t ex,
                                          bool load, bool turn, int o, int T, int moves, uint8_t *out, int esh, uint32_t one,
                                          uint32_t *lds, const PlaneFrame<R> &f, int N) {
  uint32_t pb[kPastMaxT], pw[kPastMaxT];
  pb[0] = bl; pw[0] = wh;
#pragma unroll
  for (int t = 1; t < kPastMaxT; ++t) pb[t] = pw[t] = 0;
  if (load) {   // (wave-uniform, like every t < T below)
#pragma unroll
    for (int t = 1; t < kPastMaxT; ++t) {
      if (t < T) { pb[t] = p[t][0]; pw[t] = p[t][N]; }
    }
#pragma unroll
    for (int t = 1; t < kPastMaxT; ++t) {
      const uint32_t m = ((ex >> t) & 1u) ? f.full : 0u;
      pb[t] &= m; pw[t] &= m;
    }
    if (turn) {   // three row sets a turn: (b1, w1, b2), (w2, b3, w3), ...
      uint32_t s[3 * 5];
#pragma unroll
      for (int t = 1; t < kPastMaxT; ++t) { s[2 * (t - 1)] = pb[t]; s[2 * (t - 1) + 1] = pw[t]; }
      s[14] = 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        if (3 * k < 2 * (T - 1)) feat_orient<R>(s[3 * k], s[3 * k + 1], s[3 * k + 2], o, N, f.r, f.lane, f.full);
      }
#pragma unroll
      for (int t = 1; t < kPastMaxT; ++t) { pb[t] = s[2 * (t - 1)]; pw[t] = s[2 * (t - 1) + 1]; }
    }
  }
  const bool white = (fl & 1u) != 0;
  uint32_t slots[kPastSlots];
#pragma unroll
  for (int t = 0; t < kPastMaxT; ++t) {
    slots[2 * t] = white ? pw[t] : pb[t];
    slots[2 * t + 1] = white ? pb[t] : pw[t];
  }
#pragma unroll
  for (int t = 0; t < kPastMaxT - 1; ++t)
    slots[2 * kPastMaxT + t] = ((ex >> (t + 1)) & 1u) ? (pb[t] | pw[t]) & ~(pb[t + 1] | pw[t + 1]) : 0u;
  past_emit<R>(out, esh, one, slots, T, moves, lds, f, N);
}

// gg_past_push / gg_past_push_tracked: the current position of every board whose mask byte is set (mask null: all) enters
// its ring at count % H, and its count goes up by one.  Every lane of a board reads count before the board's one lane stores
// it: the row stores' addresses depend on the value read, so the wave has waited for that load before any store issues.
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_past_push(const void *__restrict__ in, const uint8_t *__restrict__ mask, uint32_t *rows,
                                                     int32_t *count, int H, int64_t B, int N) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[Planes<R>::kIoWords];
  PlaneFrame<R> f(N);
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, nullptr, f, B, N, lds, bl, wh, inv, fl);
    const int64_t b = f.on ? f.b_first + f.j : B - 1;
    const int cn = count[b];
    const bool go = f.on && (!mask || mask[b] != 0);
    int e = cn % H;
    if (e < 0) e += H;
    WAVE_SYNC();
    if (go && f.r < N) {
      uint32_t *w = rows + ((b * H + e) * 2) * (int64_t)N + f.r;
      w[0] = bl;
      w[N] = wh;
    }
    if (go && f.r == 0) count[b] = cn + 1;
  }
}

// gg_batch_past / gg_batch_past_tracked: out [B][planes][N][N]; rows / count (both or neither) the boards' rings; orient int32
// [B] or null
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_past(const void *__restrict__ in, const uint32_t *__restrict__ rows,
                                                const int32_t *__restrict__ count, int H, int T, int moves,
                                                const int32_t *__restrict__ orient, uint8_t *__restrict__ out, int esh, uint32_t one,
                                                int64_t B, int N) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[Past<R>::kLdsWords];
  PlaneFrame<R> f(N);
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, TRACKED>(in, orient, f, B, N, lds, bl, wh, inv, fl);
    const int64_t b = f.on ? f.b_first + f.j : B - 1;
    const int rc = f.r < N ? f.r : 0;
    const uint32_t *p[kPastMaxT];
    uint32_t ex = 0;
    p[0] = nullptr;
    if (rows) {
      const int cn = count[b];
#pragma unroll
      for (int t = 1; t < kPastMaxT; ++t) ex |= (past_ring_at(rows, b, cn, H, t, N, rc, p[t]) && t < T && f.on ? 1u : 0u) << t;
    } else {
#pragma unroll
      for (int t = 1; t < kPastMaxT; ++t) p[t] = nullptr;
    }
    const int o = (orient && f.on) ? (orient[b] & 7) : 0;
    past_body<R>(bl, wh, fl, p, ex, rows != nullptr, orient != nullptr, o, T, moves, out, esh, one, lds, f, N);
  }
}

// gg_puct_past: the history planes of the played leaves of a select launch (leaf uint32 [B][5 N + 1], leaf_id int32 [B],
// B = roots x L, row i = slot i % L of root r = i / L).  Position 0 is the leaf itself.  From x = leaf_id[i] the walk takes the
// parent p = links[r][x][0] while 0 <= p < x (gg_puct_superko's bound: the node falls strictly, stays inside root r's C + 1
// nodes and ends at node 0 at the latest, whatever links holds) and at most T - 1 times; d = the ancestors found.  Position
// t <= d is boards[r][the t-th ancestor], position t > d the ring's position t - d of root r (the ring holds the positions
// before node 0).  A row whose leaf_id lies outside [0, C] - an empty slot - has d = 0.
// WHY THE TREE CAN BE READ HERE: a slot's ancestors are nodes evaluated in earlier rounds, so their boards are in the tree -
// a node made in this round is never on another slot's path (collision rule a of gg_puct_select_leaves) -, and the new node's
// own links entry is written by the select launch, which this one follows on the stream.  Nothing in the tree is written.
template <int R>
__global__ __launch_bounds__(kWave) void k_puct_past(const uint32_t *__restrict__ leaf, const int32_t *__restrict__ leaf_id,
                                                     const uint32_t *__restrict__ boards, const int32_t *__restrict__ links,
                                                     const uint32_t *__restrict__ rows, const int32_t *__restrict__ count, int H, int T,
                                                     int moves, const int32_t *__restrict__ orient, uint8_t *__restrict__ out, int esh,
                                                     uint32_t one, int C, int L, int64_t B, int N) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[Past<R>::kLdsWords];
  PlaneFrame<R> f(N);
  const int W = 5 * N + 1;
  const int64_t NN = (int64_t)C + 1;
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, true>(leaf, orient, f, B, N, lds, bl, wh, inv, fl);
    const int64_t i = f.on ? f.b_first + f.j : B - 1, root = i / L, n0 = root * NN;
    const int rc = f.r < N ? f.r : 0;
    const int cn = rows ? count[root] : 0;
    int x = leaf_id[i], d = 0;
    bool alive = x >= 0 && x <= C;
    const uint32_t *p[kPastMaxT];
    uint32_t ex = 0;
    p[0] = nullptr;
#pragma unroll
    for (int t = 1; t < kPastMaxT; ++t) {
      p[t] = boards + n0 * W + rc;   // (node 0 of the root: an address inside the tree, read only where nothing better is known)
      if (t < T) {
        if (alive) {
          const int q = links[(n0 + x) * 2];
          if (q >= 0 && q < x) { x = q; d = t; }
          else alive = false;
        }
        if (alive) {
          p[t] = boards + (n0 + x) * W + rc;
          ex |= (f.on ? 1u : 0u) << t;
        } else if (rows) {
          ex |= (past_ring_at(rows, root, cn, H, t - d, N, rc, p[t]) && f.on ? 1u : 0u) << t;
        }
      }
    }
    const int o = (orient && f.on) ? (orient[i] & 7) : 0;
    past_body<R>(bl, wh, fl, p, ex, true, orient != nullptr, o, T, moves, out, esh, one, lds, f, N);
  }
}

}  // namespace gg
