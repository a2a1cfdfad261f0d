// gg_uct.h - batched UCT tree search (gg_uct_begin / gg_uct_select / gg_uct_backup): the tree of every root lives on the
// device, the select and backup kernels walk it, the playouts of gg_po.h evaluate the leaves.
//
// R independent searches of I iterations, one tree per root with room for I + 1 nodes (node 0 = the root).  Per node:
// its tracked board, parent / action (-1 at the root), integer stats n / black wins / white wins / draws, and a child
// table of A = N^2 + 1 entries (-1: not expanded).  One iteration on the host side is
//   k_uct_select -> gg_batch_play_moves_tracked(leaf, move, T = 1) -> gg_playouts_begin / _advance on leaf -> k_uct_backup
// so the leaf's move and its playouts reuse the existing kernels unchanged.
//
// SELECT (one wave per root): from x = 0, while x's game has not ended: the lanes stride over the A actions (legality from
// the invalid rows and the flag word, the child table row, a gather of the child's stats); a ballot finds the lowest legal
// action without a child - it is expanded (node y = nodes[r]++) and is the leaf - otherwise the wave's argmax of U (ties to
// the lowest action) names the child to descend to.  leaf[r] gets the board of the node the walk stopped at (the new node's
// parent, or the ended node itself), move[r] the expanded action (-1: evaluate the node as it is), leaf_id[r] the leaf.
// BACKUP (one wave per root): stores the played leaf board as node y's board and adds K and the iteration's counts along
// the parent chain.  No atomics: a root's tree belongs to one wave.
#pragma once
#include "gg_common.h"

namespace gg {

struct UctArgs {
  uint32_t *boards;          // [R][I+1][5N+1] tracked boards of the nodes
  int32_t *child;            // [R][I+1][A] child table, -1 = not expanded
  int32_t *links;            // [R][I+1][2] parent, action (-1 / -1 at the root and at unused nodes)
  int32_t *stats;            // [R][I+1][4] n, black wins, white wins, draws
  int32_t *nodes;            // [R] nodes in use
  uint32_t *leaf;            // [R][5N+1] the board to evaluate
  int32_t *move;             // [R] action to play on leaf first, -1 = none
  int32_t *leaf_id;          // [R] the leaf node
  const double *log_table;   // [I+1] log(t K) (select)
  const int32_t *counts;     // [R][4] the iteration's playout counts (backup)
  const int64_t *sums;       // [R][2] the iteration's playout sums (backup)
  int64_t *totals;           // [R][2] += unfinished, plies (backup; nullable)
  double c;
  int64_t R;
  int32_t N, I, K;
};

// U(x, a) = (2 w + d) / (2 n) + c sqrt(L[n_x / K] / n) in float64, each operation rounded to nearest in this order: no
// contraction into fused multiply-adds (the host restatement computes the same expression in IEEE doubles).
__device__ __noinline__ double uct_score(int32_t w, int32_t d, int32_t n, double log_nx, double c) {
#pragma clang fp contract(off)
  const double q = (2.0 * (double)w + (double)d) / (2.0 * (double)n);
  return q + c * __dsqrt_rn(log_nx / (double)n);
}

// node 0 of every tree = its root (the other buffers are set by the host side's memsets), nodes = 1
static __global__ void k_uct_begin(const uint32_t *__restrict__ roots, UctArgs a) {
  const int64_t W = 5 * a.N + 1;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.R * W) return;
  const int64_t r = i / W, k = i - r * W;
  a.boards[r * (a.I + 1) * W + k] = roots[i];
  if (k == 0) a.nodes[r] = 1;
}

static __global__ __launch_bounds__(4 * kWave) void k_uct_select(UctArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *bd = a.boards + r * NN * W;
    int32_t *ch = a.child + r * NN * A;
    int32_t *st = a.stats + r * NN * 4;
    const int nodes = min(a.nodes[r], NN);   // (nodes <= I + 1 by construction: every index below stays inside the tree)
    int x = 0, mv = -1, y = 0;
    // every step goes to a child with a larger id: at most I steps (the bound also stops a walk over corrupt links)
    for (int depth = 0; depth <= a.I; ++depth) {
      const uint32_t *g = bd + (int64_t)x * W;
      const uint32_t flag = g[5 * N];
      if (flag & 4u) {   // the game has ended at x: x is the leaf, nothing is added
        y = x;
        break;
      }
      const int t = st[4 * x] / a.K;   // n_x is a multiple of K, at most I K
      const double lx = a.log_table[t < 0 ? 0 : (t > a.I ? a.I : t)];
      const bool white = (flag & 1u) != 0;
      double best = -__builtin_inf();
      int besta = A;
      int freea = -1;
      for (int a0 = 0; a0 < A; a0 += kWave) {
        const int act = a0 + lane;
        bool legal = false;
        int c = -1;
        if (act < A) {
          const int row = act / N;
          legal = act == P || !((g[2 * N + (act < P ? row : 0)] >> (act - row * N)) & 1u);
          if (legal) c = ch[(int64_t)x * A + act];
        }
        const uint64_t free = __ballot(legal && c < 0);
        if (free) {   // the lowest legal action without a child: expand it
          freea = a0 + __builtin_ctzll(free);
          break;
        }
        if (legal && c > x && c < nodes) {   // (children always have larger ids than their parent)
          const int4 s = reinterpret_cast<const int4 *>(st)[c];
          const double u = uct_score(white ? s.z : s.y, s.w, s.x, lx, a.c);
          if (u > best) {   // (this lane's actions ascend: the first of equal scores stays)
            best = u;
            besta = act;
          }
        }
      }
      if (freea >= 0) {
        if (nodes <= a.I) {   // (a select beyond I iterations finds no room: x is evaluated as it is)
          y = nodes;
          mv = freea;
          if (lane == 0) {
            ch[(int64_t)x * A + freea] = y;
            a.links[(r * NN + y) * 2] = x;
            a.links[(r * NN + y) * 2 + 1] = freea;
            reinterpret_cast<int4 *>(st)[y] = make_int4(0, 0, 0, 0);
            a.nodes[r] = nodes + 1;
          }
        } else {
          y = x;
        }
        break;
      }
      // the wave's argmax, ties to the lowest action
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(besta, o);
        if (ob > best || (ob == best && oa < besta)) {
          best = ob;
          besta = oa;
        }
      }
      const int nx = besta < A ? ch[(int64_t)x * A + besta] : -1;
      if (nx <= x || nx >= nodes) {   // (only with corrupt buffers: stop here)
        y = x;
        break;
      }
      x = nx;
      y = x;
    }
    // the leaf board: the new node's parent (its move is played by the next launch) or the node itself
    const uint32_t *g = bd + (int64_t)x * W;
    uint32_t *out = a.leaf + r * W;
    for (int k = lane; k < W; k += kWave) out[k] = g[k];
    if (lane == 0) {
      a.move[r] = mv;
      a.leaf_id[r] = y;
    }
  }
}

static __global__ __launch_bounds__(4 * kWave) void k_uct_backup(UctArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int W = 5 * a.N + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const int y = a.leaf_id[r];
    if (y < 0 || y >= NN) continue;
    if (a.move[r] >= 0) {   // a new node: the played board is its board
      const uint32_t *src = a.leaf + r * W;
      uint32_t *dst = a.boards + (r * NN + y) * W;
      for (int k = lane; k < W; k += kWave) dst[k] = src[k];
    }
    if (lane == 0) {
      const int32_t *cn = a.counts + 4 * r;
      const int32_t bw = cn[0], ww = cn[1], d = cn[2];
      int32_t *st = a.stats + r * NN * 4;
      const int32_t *ln = a.links + r * NN * 2;
      int x = y;
      for (int depth = 0; depth <= a.I && x >= 0 && x < NN; ++depth) {   // (parents have smaller ids: at most I + 1 nodes)
        st[4 * x] += a.K;
        st[4 * x + 1] += bw;
        st[4 * x + 2] += ww;
        st[4 * x + 3] += d;
        x = ln[2 * x];
      }
      if (a.totals) {
        a.totals[2 * r] += cn[3];
        a.totals[2 * r + 1] += a.sums[2 * r + 1];
      }
    }
  }
}

}  // namespace gg
