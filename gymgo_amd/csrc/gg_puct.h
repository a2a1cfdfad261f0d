// gg_puct.h - batched PUCT tree search with priors and a caller-supplied evaluator (gg_puct_begin / gg_puct_select /
// gg_puct_backup): the tree of every root lives on the device, the select and backup kernels walk it, the leaves are handed
// out and their evaluations (priors, value) come back from outside the library.
//
// R independent searches of I iterations, one tree per root with room for I + 1 nodes (node 0 = the root).  Per node: its
// tracked board, parent / action (-1 at the root), the stat record {w: float64 sum of the backed-up values from black's point
// of view, n: int32 visits}, float32 priors [A] (zero until the node is evaluated) and a child table [A] (-1: no child),
// A = N^2 + 1.  One iteration on the host side is
//   k_puct_select -> gg_batch_play_moves_tracked(leaf, move, T = 1) -> gg_batch_untrack_states(leaf) -> the caller's
//   evaluator -> k_puct_backup
// so the leaf's move and its byte planes reuse the existing kernels unchanged.
//
// SELECT (one wave per root): from x = 0, while x's game has not ended and x has been evaluated (n_x > 0): the lanes stride
// over the A actions (legality from the invalid rows and the flag word, the prior, the child table row, one 16-byte gather
// of the child's record), each computes U (puct_score) and the wave's argmax (ties to the lowest action) names a*; without a
// child under a* a new node y = nodes[r]++ is linked in and is the leaf, otherwise the walk goes on at the child.  leaf[r]
// gets the board of the node the walk stopped at (the new node's parent, or the node to evaluate itself), move[r] the
// expanded action (-1: evaluate the node as it is), leaf_id[r] the leaf.
// BACKUP (one wave per root): the lanes store the played leaf board as node y's board and, at a node evaluated for the first
// time, the evaluator's priors masked by the leaf's legal actions; the value is the evaluator's (clamped, from the mover's to
// black's point of view) or, at a leaf whose game has ended, the Tromp-Taylor outcome (lat_areas: the floods of the harvest
// kernel, the leaf as the wave's first board); lane 0 adds n += 1, w += v along the parent chain.  No atomics: a root's tree
// belongs to one wave.  Every index is bounded by the tree: nodes clamped, child ids larger than their parent's, walks
// stopped after I + 1 steps.
#pragma once
#include "gg_common.h"
#include "gg_lat.h"

namespace gg {

struct __attribute__((aligned(16))) PuctStat {   // gg_puct_stat of include/gymgo_amd.h
  double w;       // sum of the backed-up values, black's point of view
  int32_t n;      // visits (the node's own evaluation included)
  int32_t v;      // virtual visits of the several-leaves path (the reserved word: 0 outside a round, never read by the one-leaf path)
};

struct PuctArgs {
  uint32_t *boards;          // [R][I+1][5N+1] tracked boards of the nodes
  int32_t *child;            // [R][I+1][A] child table, -1 = no child
  float *prior;              // [R][I+1][A] priors, 0 until the node is evaluated
  int32_t *links;            // [R][I+1][2] parent, action (-1 / -1 at the root and at unused nodes)
  PuctStat *stats;           // [R][I+1]
  int32_t *nodes;            // [R] nodes in use
  uint32_t *leaf;            // [R][5N+1] the board to evaluate
  int32_t *move;             // [R] action to play on leaf first, -1 = none
  int32_t *leaf_id;          // [R] the leaf node
  const float *priors;       // [R][A] the evaluator's priors (backup)
  const float *values;       // [R] the evaluator's values, mover's point of view (backup)
  double c;
  int64_t R;
  int32_t N, I;
  float komi;
};

// U(x, a) = q + c prior sqrt(n_x) / (1 + n_c), q = s w_c / n_c (0 without visits), in float64, each operation rounded to
// nearest in this order: no contraction into fused multiply-adds (the host restatement computes the same expression in IEEE
// doubles).  A NaN (c = 0 with an infinite prior) counts as -inf: it never beats a number.
__device__ __noinline__ double puct_score(double s, double wc, int32_t nc, float prior, int32_t nx, double c) {
#pragma clang fp contract(off)
  const double q = nc == 0 ? 0.0 : s * wc / (double)nc;
  const double t1 = c * (double)prior;
  const double t2 = __dsqrt_rn((double)nx);
  const double t3 = t1 * t2;
  const double t4 = t3 / (double)(1 + nc);
  const double u = q + t4;
  return u == u ? u : -__builtin_inf();
}

// node 0 of every tree = its root (the other buffers are set by the host side's memsets), nodes = 1
static __global__ void k_puct_begin(const uint32_t *__restrict__ roots, PuctArgs a) {
  const int64_t W = 5 * a.N + 1;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= a.R * W) return;
  const int64_t r = i / W, k = i - r * W;
  a.boards[r * (a.I + 1) * W + k] = roots[i];
  if (k == 0) a.nodes[r] = 1;
}

static __global__ __launch_bounds__(4 * kWave) void k_puct_select(PuctArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *bd = a.boards + r * NN * W;
    int32_t *ch = a.child + r * NN * A;
    const float *pr = a.prior + r * NN * A;
    const PuctStat *st = a.stats + r * NN;
    const int nodes = max(1, min(a.nodes[r], NN));   // (1 <= nodes <= I + 1 by construction: every index below stays inside the tree)
    int x = 0, mv = -1, y = 0;
    // every step goes to a child with a larger id: at most I steps (the bound also stops a walk over corrupt links)
    for (int depth = 0; depth <= a.I; ++depth) {
      const uint32_t *g = bd + (int64_t)x * W;
      const uint32_t flag = g[5 * N];
      const int32_t nx = st[x].n;
      y = x;
      if ((flag & 4u) || nx <= 0) break;   // the game has ended at x, or x has not been evaluated yet: x is the leaf
      const double s = (flag & 1u) ? -1.0 : 1.0;
      double best = -__builtin_inf();
      int besta = A;
      for (int a0 = 0; a0 < A; a0 += kWave) {
        const int act = a0 + lane;
        if (act >= A) continue;
        const int row = act / N;
        const bool legal = act == P || !((g[2 * N + (act < P ? row : 0)] >> (act - row * N)) & 1u);
        if (!legal) continue;
        const int c = ch[(int64_t)x * A + act];
        const float p = pr[(int64_t)x * A + act];
        double wc = 0.0;
        int32_t nc = 0;
        if (c > x && c < nodes) {   // (children always have larger ids than their parent)
          const PuctStat k = st[c];
          wc = k.w;
          nc = k.n < 0 ? 0 : k.n;
        }
        const double u = puct_score(s, wc, nc, p, nx, a.c);
        if (u > best || besta == A) {   // (this lane's actions ascend: the first of equal scores stays)
          best = u;
          besta = act;
        }
      }
      // the wave's argmax, ties to the lowest action (a lane without a legal action holds -inf / A and loses every tie)
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(besta, o);
        if (ob > best || (ob == best && oa < besta)) {
          best = ob;
          besta = oa;
        }
      }
      if (besta >= A) break;   // (the pass is always legal: only with corrupt buffers)
      const int nxt = ch[(int64_t)x * A + besta];
      if (nxt < 0) {
        if (nodes <= a.I) {   // (a select beyond I iterations finds no room: x is evaluated as it is)
          y = nodes;
          mv = besta;
          if (lane == 0) {
            ch[(int64_t)x * A + besta] = y;
            a.links[(r * NN + y) * 2] = x;
            a.links[(r * NN + y) * 2 + 1] = besta;
            a.nodes[r] = nodes + 1;
          }
        }
        break;
      }
      if (nxt <= x || nxt >= nodes) break;   // (only with corrupt buffers: stop here)
      x = nxt;
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

// RR: the row capacity of the lat_areas instantiation (9 / 13 / 19, N <= RR)
template <int RR>
static __global__ __launch_bounds__(4 * kWave) void k_puct_backup(PuctArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const int y = a.leaf_id[r];
    if (y < 0 || y >= NN) continue;
    const uint32_t *src = a.leaf + r * W;
    const uint32_t flag = __builtin_amdgcn_readfirstlane(src[5 * N]);   // (wave-uniform: the floods below are wave-collective)
    PuctStat *st = a.stats + r * NN;
    if (a.move[r] >= 0) {   // a new node: the played board is its board
      uint32_t *dst = a.boards + (r * NN + y) * W;
      for (int k = lane; k < W; k += kWave) dst[k] = src[k];
    }
    if (st[y].n == 0) {   // the node's first evaluation: its priors, zero on illegal actions, NaN and negatives -> 0
      const float *p = a.priors + r * A;
      float *dst = a.prior + (r * NN + y) * A;
      for (int act = lane; act < A; act += kWave) {
        const int row = act / N;
        const bool legal = !(flag & 4u) && (act == P || !((src[2 * N + (act < P ? row : 0)] >> (act - row * N)) & 1u));
        const float v = p[act];
        dst[act] = legal && v > 0.f ? v : 0.f;
      }
    }
    double vb;
    if (flag & 4u) {   // the game has ended: sign(black - white - komi) of the Tromp-Taylor areas, the evaluator's row ignored
      const bool mine = lane < N;   // the leaf is the wave's first board, one row per lane; the other boards are empty
      const uint32_t bl = mine ? src[lane] : 0u, wh = mine ? src[N + lane] : 0u;
      const uint32_t full = mine ? (1u << N) - 1u : 0u;
      uint32_t ab, aw;
      lat_areas<RR>(bl, wh, full, ab, aw);
      const float xk = (float)((int)ab - (int)aw) - a.komi;
      vb = xk > 0.f ? 1.0 : (xk < 0.f ? -1.0 : 0.0);
    } else {           // the evaluator's value, from the mover's point of view: clamped to [-1, 1], NaN -> 0
      float v = a.values[r];
      v = v != v ? 0.f : (v < -1.f ? -1.f : (v > 1.f ? 1.f : v));
      vb = ((flag & 1u) ? -1.0 : 1.0) * (double)v;
    }
    if (lane == 0) {
      const int32_t *ln = a.links + r * NN * 2;
      int x = y;
      for (int depth = 0; depth <= a.I && x >= 0 && x < NN; ++depth) {   // (parents have smaller ids: at most I + 1 nodes)
        st[x].n += 1;
        st[x].w += vb;
        x = ln[2 * x];
      }
    }
  }
}

// ---------------------------------------------------------------- several leaves per root per round, with virtual loss
// k_puct_select_leaves / k_puct_backup_leaves / k_puct_legal (gg_puct_select_leaves / gg_puct_backup_leaves / gg_puct_legal of
// include/gymgo_amd.h, which holds the normative text).  The tree is the one above with C + 1 nodes, C = rounds * L; the
// reserved word of the stat record is v, the node's virtual visits: a slot that has found its leaf adds 1 to v from the leaf
// up to the root, the backup of that slot takes it off again, so every v is 0 outside a round.  Slot j of root r is row
// r L + j of leaf / move / leaf_id / priors / values.  The slots of a root run strictly in order inside one wave: later
// slots read child entries, links and stat words that lane 0 stored for earlier ones, so each such hand-over is a
// release / acquire fence pair (puct_handover) - the stores are waited for and the loads after it are issued anew.

struct PuctLeavesArgs {
  PuctArgs t;                // the tree and the per-slot rows; t.I = C, the capacity
  int32_t L;                 // slots per root and round
};

// lane 0's stores above become visible to every lane's loads below (one wave; the scope is the workgroup's, which contains it)
__device__ __forceinline__ void puct_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// U'(x, a) = q + c prior sqrt(n_x + v_x) / (1 + n_c + v_c), q = (s w_c - v_c) / (n_c + v_c): one virtual visit is one loss for
// the side that chose the child.  puct_score's discipline: float64, this order, no contraction, NaN -> -inf.  With every
// v = 0 it is puct_score bit for bit (x - 0.0 = x for every x, -0.0 included).
__device__ __noinline__ double puct_score_vl(double s, double wc, int32_t nc, int32_t vc, float prior, int32_t nx, int32_t vx,
                                             double c) {
#pragma clang fp contract(off)
  const int32_t ne = nc + vc;
  const double q = ne == 0 ? 0.0 : (s * wc - (double)vc) / (double)ne;
  const double t1 = c * (double)prior;
  const double t2 = __dsqrt_rn((double)(nx + vx));
  const double t3 = t1 * t2;
  const double t4 = t3 / (double)(1 + ne);
  const double u = q + t4;
  return u == u ? u : -__builtin_inf();
}

static __global__ __launch_bounds__(4 * kWave) void k_puct_select_leaves(PuctLeavesArgs b) {
  const PuctArgs &a = b.t;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1, L = b.L;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *bd = a.boards + r * NN * W;
    int32_t *ch = a.child + r * NN * A;
    const float *pr = a.prior + r * NN * A;
    PuctStat *st = a.stats + r * NN;
    int32_t *ln = a.links + r * NN * 2;
    int nodes = max(1, min(a.nodes[r], NN));   // (1 <= nodes <= C + 1: every index below stays inside the tree)
    bool open = true;                          // false from the slot that met a collision on
    for (int j = 0; j < L; ++j) {
      int x = 0, mv = -1, y = -1;
      if (open) {
        puct_handover();   // the links, child entries and v of the slots before this one
        // every step goes to a child with a larger id: at most C steps (the bound also stops a walk over corrupt links)
        for (int depth = 0; depth <= a.I; ++depth) {
          const int32_t nx = st[x].n, vx = st[x].v;
          if (nx <= 0 && vx > 0) {   // handed out earlier in this round, no board yet: a collision, before any read of x's board
            open = false;
            y = -1;
            break;
          }
          const uint32_t *g = bd + (int64_t)x * W;
          const uint32_t flag = g[5 * N];
          y = x;
          if ((flag & 4u) || nx <= 0) break;   // the game has ended at x, or x has not been evaluated yet: x is the leaf
          const double s = (flag & 1u) ? -1.0 : 1.0;
          double best = -__builtin_inf();
          int besta = A;
          for (int a0 = 0; a0 < A; a0 += kWave) {
            const int act = a0 + lane;
            if (act >= A) continue;
            const int row = act / N;
            const bool legal = act == P || !((g[2 * N + (act < P ? row : 0)] >> (act - row * N)) & 1u);
            if (!legal) continue;
            const int c = ch[(int64_t)x * A + act];
            const float p = pr[(int64_t)x * A + act];
            double wc = 0.0;
            int32_t nc = 0, vc = 0;
            if (c > x && c < nodes) {   // (children always have larger ids than their parent)
              const PuctStat k = st[c];
              wc = k.w;
              nc = k.n < 0 ? 0 : k.n;
              vc = k.v < 0 ? 0 : k.v;
            }
            const double u = puct_score_vl(s, wc, nc, vc, p, nx, vx < 0 ? 0 : vx, a.c);
            if (u > best || besta == A) {   // (this lane's actions ascend: the first of equal scores stays)
              best = u;
              besta = act;
            }
          }
          // the wave's argmax, ties to the lowest action (a lane without a legal action holds -inf / A and loses every tie)
#pragma unroll
          for (int o = kWave / 2; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int oa = __shfl_xor(besta, o);
            if (ob > best || (ob == best && oa < besta)) {
              best = ob;
              besta = oa;
            }
          }
          if (besta >= A) break;   // (the pass is always legal: only with corrupt buffers)
          const int nxt = ch[(int64_t)x * A + besta];
          if (nxt < 0) {
            if (nodes <= a.I) {   // (a select beyond C leaves finds no room: x is evaluated as it is)
              y = nodes;
              mv = besta;
              if (lane == 0) {
                ch[(int64_t)x * A + besta] = y;
                ln[2 * y] = x;
                ln[2 * y + 1] = besta;
              }
              nodes += 1;
            }
            break;
          }
          if (nxt <= x || nxt >= nodes) break;   // (only with corrupt buffers: stop here)
          x = nxt;
          y = x;
        }
      }
      const int64_t row = r * L + j;
      if (y < 0) {   // an empty slot: the root's board, nothing to back up
        x = 0;
        mv = -1;
      } else if (lane == 0) {   // one virtual visit on every node from the leaf up to the root (parents have smaller ids)
        int z = y;
        for (int depth = 0; depth <= a.I && z >= 0 && z < NN; ++depth) {
          st[z].v += 1;
          z = ln[2 * z];
        }
      }
      // the leaf board: the new node's parent (its move is played by the next launch) or the node itself
      const uint32_t *g = bd + (int64_t)x * W;
      uint32_t *out = a.leaf + row * W;
      for (int k = lane; k < W; k += kWave) out[k] = g[k];
      if (lane == 0) {
        a.move[row] = mv;
        a.leaf_id[row] = y;
      }
    }
    if (lane == 0) a.nodes[r] = nodes;
  }
}

// RR: the row capacity of the lat_areas instantiation (9 / 13 / 19, N <= RR)
template <int RR>
static __global__ __launch_bounds__(4 * kWave) void k_puct_backup_leaves(PuctLeavesArgs b) {
  const PuctArgs &a = b.t;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1, L = b.L;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    PuctStat *st = a.stats + r * NN;
    const int32_t *ln = a.links + r * NN * 2;
    for (int j = 0; j < L; ++j) {
      const int64_t row = r * L + j;
      const int y = __builtin_amdgcn_readfirstlane(a.leaf_id[row]);
      if (y < 0 || y >= NN) continue;   // an empty slot (-1), or a leaf id outside the tree
      const uint32_t *src = a.leaf + row * W;
      const uint32_t flag = __builtin_amdgcn_readfirstlane(src[5 * N]);   // (wave-uniform: the floods below are wave-collective)
      if (a.move[row] >= 0) {   // a new node: the played board is its board
        uint32_t *dst = a.boards + (r * NN + y) * W;
        for (int k = lane; k < W; k += kWave) dst[k] = src[k];
      }
      puct_handover();   // n of the slots before this one (an ended node may be taken twice in one round)
      if (st[y].n == 0) {   // the node's first evaluation: its priors, zero on illegal actions, NaN and negatives -> 0
        const float *p = a.priors + row * A;
        float *dst = a.prior + (r * NN + y) * A;
        for (int act = lane; act < A; act += kWave) {
          const int rw = act / N;
          const bool legal = !(flag & 4u) && (act == P || !((src[2 * N + (act < P ? rw : 0)] >> (act - rw * N)) & 1u));
          const float v = p[act];
          dst[act] = legal && v > 0.f ? v : 0.f;
        }
      }
      double vb;
      if (flag & 4u) {   // the game has ended: sign(black - white - komi) of the Tromp-Taylor areas, the evaluator's row ignored
        const bool mine = lane < N;   // the leaf is the wave's first board, one row per lane; the other boards are empty
        const uint32_t bl = mine ? src[lane] : 0u, wh = mine ? src[N + lane] : 0u;
        const uint32_t full = mine ? (1u << N) - 1u : 0u;
        uint32_t ab, aw;
        lat_areas<RR>(bl, wh, full, ab, aw);
        const float xk = (float)((int)ab - (int)aw) - a.komi;
        vb = xk > 0.f ? 1.0 : (xk < 0.f ? -1.0 : 0.0);
      } else {           // the evaluator's value, from the mover's point of view: clamped to [-1, 1], NaN -> 0
        float v = a.values[row];
        v = v != v ? 0.f : (v < -1.f ? -1.f : (v > 1.f ? 1.f : v));
        vb = ((flag & 1u) ? -1.0 : 1.0) * (double)v;
      }
      if (lane == 0) {
        int x = y;
        for (int depth = 0; depth <= a.I && x >= 0 && x < NN; ++depth) {   // (parents have smaller ids: at most C + 1 nodes)
          PuctStat k = st[x];
          k.n += 1;
          k.w += vb;
          k.v = k.v > 0 ? k.v - 1 : 0;   // the slot's virtual visit comes off, never below 0
          st[x] = k;
          x = ln[2 * x];
        }
      }
    }
  }
}

// legal [B][A] (one byte 0 / 1 per action: the pass and every point whose invalid bit is clear, nothing once the game has
// ended) and live [B] (1 where leaf_id >= 0) of B played tracked boards: what the caller's evaluator gets next to the planes
static __global__ __launch_bounds__(256) void k_puct_legal(const uint32_t *__restrict__ leaf, const int32_t *__restrict__ leaf_id,
                                                           uint8_t *__restrict__ legal, uint8_t *__restrict__ live, int64_t B,
                                                           int32_t N) {
  const int W = 5 * N + 1, P = N * N, A = P + 1;
  const int64_t total = B * A;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += gridDim.x * (int64_t)blockDim.x) {
    const int64_t row = i / A;
    const int act = (int)(i - row * A);
    const uint32_t *g = leaf + row * W;
    const int rw = act / N;
    const bool ok = !(g[5 * N] & 4u) && (act == P || !((g[2 * N + (act < P ? rw : 0)] >> (act - rw * N)) & 1u));
    legal[i] = ok ? 1 : 0;
    if (act == 0) live[row] = leaf_id[row] >= 0 ? 1 : 0;
  }
}

}  // namespace gg
