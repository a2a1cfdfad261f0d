// gg_uct.h - batched UCT tree search (gg_uct_begin / gg_uct_select[_rave] / gg_uct_backup[_rave] and their _leaves forms of
// include/gymgo_amd_uct_leaves.h): the tree of every root lives on the device, the select and backup kernels walk it, the
// playouts of gg_po.h evaluate the leaves.
//
// R independent searches of I iterations, one tree per root with room for I + 1 nodes (node 0 = the root).  Per node:
// its tracked board, parent / action (-1 at the root), integer stats n / black wins / white wins / draws, and a child
// table of A = N^2 + 1 entries (-1: not expanded).  One iteration on the host side is
//   k_uct_select -> gg_batch_play_moves_tracked(leaf, move, T = 1) -> gg_playouts_begin / _advance on leaf -> k_uct_backup
// so the leaf's move and its playouts reuse the existing kernels unchanged.
//
// One select and one backup kernel, each instantiated four times: RAVE = false: plain UCT, true: RAVE (include/gymgo_amd_amaf.h,
// DESIGN 35); VL = false: one leaf per root and round, true: L leaves per root and round, chosen under virtual loss.
// RAVE differs in two places only, both under `if constexpr (RAVE)`: how a node scores its actions, and the AMAF fold that
// follows the backup.  Every difference of the several-leaves mode stands under `if (VL)`.
//
// SELECT (one wave per root): from x = 0, while x's game has not ended: the lanes stride over the A actions (legality from
// the invalid rows and the flag word, the child table row, a gather of the child's stats) and the node names one action.
// Plain: a ballot finds the lowest legal action without a child, otherwise the wave's argmax of uct_score over the children
// (ties to the lowest action).  RAVE: the argmax of rave_score over every legal action, expanded or not.  An action without a
// child is expanded (node y = nodes[r]++) and is the leaf; else the walk descends to the child.  leaf[r] gets the board of
// the node the walk stopped at (the new node's parent, or the ended node itself), move[r] the expanded action (-1: evaluate
// the node as it is), leaf_id[r] the leaf.
// BACKUP (one wave per root): stores the played leaf board as node y's board and adds K and the iteration's counts along
// the parent chain; RAVE then folds the iteration's first-play counts into the (n~, s~) of every node on the path.  No
// atomics: a root's tree belongs to one wave.
// VL: the tree has C + 1 nodes, C = rounds * L, plus virt = int32 [R][C+1]: v_x = the leaves handed out in the current round
// whose path goes through x.  Slot j of root r is row r L + j of leaf / move / leaf_id / counts / sums / amaf; the L slots of a
// root run strictly in order inside the root's wave.  Later slots read the child entries, links, stat words and v that lane 0
// stored for earlier ones, so every slot starts with a release / acquire fence pair (uct_handover).  With every v = 0 a slot
// chooses what the one-leaf walk chooses, bit for bit: uct_score and rave_score are the only float expressions.  No LDS and no
// scratch in the select and the backup.
#pragma once
#include "gg_common.h"

namespace gg {

struct UctArgs {
  uint32_t *boards;          // [R][I+1][5N+1] tracked boards of the nodes
  int32_t *child;            // [R][I+1][A] child table, -1 = not expanded
  int32_t *links;            // [R][I+1][2] parent, action (-1 / -1 at the root and at unused nodes)
  int32_t *stats;            // [R][I+1][4] n, black wins, white wins, draws
  int32_t *nodes;            // [R] nodes in use
  uint32_t *leaf;            // [R L][5N+1] the board to evaluate
  int32_t *move;             // [R L] action to play on leaf first, -1 = none
  int32_t *leaf_id;          // [R L] the leaf node (VL: -1 = an empty slot)
  const double *log_table;   // [I+1] log(t K) (select)
  const int32_t *counts;     // [R L][4] the iteration's playout counts (backup)
  const int64_t *sums;       // [R L][2] the iteration's playout sums (backup)
  int64_t *totals;           // [R][2] += unfinished, plies (backup; nullable)
  double c;
  int64_t R;
  int32_t N, I, K;
  // RAVE only (no plain instantiation reads these): per node x and point p the pair (n~, s~) - the simulations through x in
  // which x's mover played p first after x, twice its wins plus the draws among them
  int32_t *node_amaf;        // [R][I+1][N^2][2] n~, s~
  const int32_t *amaf;       // [R L][2][3][N][N] the iteration's first-play counts (backup)
  double k, fpu;             // rave_equiv, the value of an action without any count
  // VL only (no VL = false instantiation reads these or writes virt, which is null there).  They stand last, as the kernel
  // arguments behind UctArgs that they were: in front of the RAVE members the several-leaves kernels take a register more
  int32_t *virt;             // [R][I+1] v: the round's leaves through every node
  int32_t L;                 // the slots of a root (1 from the one-leaf entry points)
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

// U(x, a) of the RAVE select: (n~, s~) mixed into the value of every legal action, expanded or not, so that a node descends as soon
// as one action stands out.  In float64, each operation rounded to nearest in the order written, no contraction (the host
// restatement computes the same expression in IEEE doubles): s = 2 w + d and s~ arrive as integers
__device__ __noinline__ double rave_score(int32_t n, int32_t s, int32_t nt, int32_t st, double log_nx, double c, double k, double fpu) {
#pragma clang fp contract(off)
  const double dn = (double)n, dnt = (double)nt;
  double v;
  if (n > 0 && nt > 0) {
    const double q = (double)s / (2.0 * dn), qt = (double)st / (2.0 * dnt);
    const double beta = dnt / (dn + dnt + (dn * dnt) / k);
    v = (1.0 - beta) * q + beta * qt;
  } else if (n > 0) {
    v = (double)s / (2.0 * dn);
  } else if (nt > 0) {
    v = (double)st / (2.0 * dnt);
  } else {
    v = fpu;
  }
  return n > 0 ? v + c * __dsqrt_rn(log_nx / dn) : v;
}

// action act < A of the node with board g: the pass, or a point whose bit in the invalid rows is clear
__device__ __forceinline__ bool uct_legal(const uint32_t *g, int act, int N, int P) {
  const int row = act / N;
  return act == P || !((g[2 * N + (act < P ? row : 0)] >> (act - row * N)) & 1u);
}

// VL: lane 0's stores above become visible to every lane's loads below (one wave; the scope is the workgroup's, which contains it)
__device__ __forceinline__ void uct_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool RAVE, bool VL>
static __global__ __launch_bounds__(4 * kWave) void k_uct_select(UctArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1;
  const int L = VL ? a.L : 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *bd = a.boards + r * NN * W;
    int32_t *ch = a.child + r * NN * A;
    int32_t *st = a.stats + r * NN * 4;
    int32_t *ln = a.links + r * NN * 2;
    int32_t *vt = VL ? a.virt + r * NN : nullptr;
    // nodes <= I + 1 (by construction without VL): every index below stays inside the tree.  VL: nodes lives in a register over
    // the slots, 1 <= nodes, and is stored once per root; else it is stored at the expansion
    int nodes = min(a.nodes[r], NN);
    if (VL) nodes = max(1, nodes);
    bool open = true;   // VL: false from the slot that met a collision on
    for (int j = 0; j < L; ++j) {
      int x = 0, mv = -1, y = VL ? -1 : 0;
      if (open) {
        if (VL) uct_handover();   // the links, child entries, stats and v of the slots before this one
        // every step goes to a child with a larger id: at most I steps (the bound also stops a walk over corrupt links)
        for (int depth = 0; depth <= a.I; ++depth) {
          const int32_t nx0 = st[4 * x];
          if (VL && x > 0 && nx0 <= 0) {   // created earlier in this round, no board yet: a collision, before any read of x's board
            open = false;
            y = -1;
            break;
          }
          const uint32_t *g = bd + (int64_t)x * W;
          const uint32_t flag = g[5 * N];
          y = x;
          if (flag & 4u) break;   // the game has ended at x: x is the leaf, nothing is added
          int t = nx0 / a.K;         // n_x is a multiple of K, at most I K
          if (VL) t += vt[x];        // + v_x <= L
          const double lx = a.log_table[t < 0 ? 0 : (t > a.I ? a.I : t)];
          const bool white = (flag & 1u) != 0;
          double best = -__builtin_inf();
          int besta = A;
          int pick = -1;   // the action x chooses without an argmax
          for (int a0 = 0; a0 < A; a0 += kWave) {
            const int act = a0 + lane;
            const bool legal = act < A && uct_legal(g, act, N, P);
            const int c = legal ? ch[(int64_t)x * A + act] : -1;
            double u;
            if constexpr (RAVE) {   // every legal action has a score, expanded or not
              if (!legal) continue;
              int32_t n = 0, s = 0, nt = 0, sw = 0;
              if (c > x && c < nodes) {   // (children always have larger ids than their parent)
                const int4 q = reinterpret_cast<const int4 *>(st)[c];
                n = q.x;
                if (VL) n += a.K * vt[c];   // a virtual visit is K playouts, none of them won (n_c + K v_c <= I K)
                s = 2 * (white ? q.z : q.y) + q.w;
              }
              if (act < P) {
                const int2 e = reinterpret_cast<const int2 *>(a.node_amaf)[(r * NN + x) * P + act];
                nt = e.x;
                sw = e.y;
              }
              u = rave_score(n, s, nt, sw, lx, a.c, a.k, a.fpu);
            } else {   // the lowest legal action without a child goes first; only children have a score
              const uint64_t free = __ballot(legal && c < 0);
              if (free) {
                pick = a0 + __builtin_ctzll(free);
                break;
              }
              if (!(legal && c > x && c < nodes)) continue;
              const int4 s = reinterpret_cast<const int4 *>(st)[c];
              u = uct_score(white ? s.z : s.y, s.w, VL ? s.x + a.K * vt[c] : s.x, lx, a.c);
            }
            if (u > best) {   // (this lane's actions ascend: the first of equal scores stays)
              best = u;
              besta = act;
            }
          }
          if (pick < 0) {   // the wave's argmax, ties to the lowest action
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) {
              const double ob = __shfl_xor(best, o);
              const int oa = __shfl_xor(besta, o);
              if (ob > best || (ob == best && oa < besta)) {
                best = ob;
                besta = oa;
              }
            }
            pick = besta;
          }
          if (pick >= A) break;   // (no action scored: only with corrupt buffers - the pass is always legal)
          const int nx = ch[(int64_t)x * A + pick];
          if (nx < 0) {   // the chosen action has no child: expand it
            if (nodes <= a.I) {   // (a select beyond the capacity finds no room: x is evaluated as it is)
              y = nodes;
              mv = pick;
              if (lane == 0) {
                ch[(int64_t)x * A + pick] = y;
                ln[2 * y] = x;
                ln[2 * y + 1] = pick;
                reinterpret_cast<int4 *>(st)[y] = make_int4(0, 0, 0, 0);
                if (!VL) a.nodes[r] = nodes + 1;
              }
              if (VL) ++nodes;
            }
            break;
          }
          if (nx <= x || nx >= nodes) break;   // (only with corrupt buffers: stop here)
          x = nx;
          y = x;
        }
      }
      if (VL) {
        if (y < 0) {
          x = 0;   // an empty slot hands the root's board out
        } else if (lane == 0) {   // the hand-over - one more leaf through every node from y up to the root
          for (int z = y, depth = 0; depth <= a.I; ++depth) {   // (parents have smaller ids: at most I + 1 nodes)
            vt[z] += 1;
            const int p = ln[2 * z];
            if (p < 0 || p >= z) break;
            z = p;
          }
        }
      }
      // the leaf board: the new node's parent (its move is played by the next launch) or the node itself
      const uint32_t *g = bd + (int64_t)x * W;
      uint32_t *out = a.leaf + (r * L + j) * W;
      for (int k = lane; k < W; k += kWave) out[k] = g[k];
      if (lane == 0) {
        a.move[r * L + j] = mv;
        a.leaf_id[r * L + j] = y;
      }
    }
    if (VL && lane == 0) a.nodes[r] = nodes;
  }
}

// The AMAF fold of the RAVE backup: the lanes stride over the points: lane l owns the points l, l + 64, ... (at most kRavePts = 6
// on 19x19) and keeps, per point, the path index of its first occurrence among the tree moves below the node the walk stands at.
constexpr int kRavePts = (19 * 19 + kWave - 1) / kWave;

template <bool RAVE, bool VL>
static __global__ __launch_bounds__(4 * kWave) void k_uct_backup(UctArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, NN = a.I + 1, P = N * N;
  const int L = VL ? a.L : 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    int32_t *st = a.stats + r * NN * 4;
    const int32_t *ln = a.links + r * NN * 2;
    int32_t *vt = VL ? a.virt + r * NN : nullptr;
    for (int j = 0; j < L; ++j) {   // the slots in ascending order
      const int64_t row = r * L + j;
      const int y = a.leaf_id[row];
      if (y < 0 || y >= NN) continue;   // a leaf id outside the tree; VL: an empty slot (-1)
      // VL: the fence pair every slot starts with.  Nothing below depends on it across lanes - stats, v and totals are lane 0's
      // alone, a point's pair is read and rewritten by the lane that owns the point in every slot, and no board stored here is
      // read again in this launch - so it only keeps the slots' memory operations apart, as the rule's text asks
      if (VL) uct_handover();
      const uint32_t *src = a.leaf + row * W;
      if (a.move[row] >= 0) {   // a new node: the played board is its board
        uint32_t *dst = a.boards + (r * NN + y) * W;
        for (int k = lane; k < W; k += kWave) dst[k] = src[k];
      }
      const int32_t *cn = a.counts + 4 * row;
      const int32_t bw = cn[0], ww = cn[1], d = cn[2];
      if (lane == 0) {
        int x = y;
        for (int depth = 0; depth <= a.I && x >= 0 && x < NN; ++depth) {   // (parents have smaller ids: at most I + 1 nodes)
          st[4 * x] += a.K;
          st[4 * x + 1] += bw;
          st[4 * x + 2] += ww;
          st[4 * x + 3] += d;
          if (VL) vt[x] = max(vt[x] - 1, 0);   // the leaf is no longer out
          x = ln[2 * x];
        }
        if (a.totals) {
          a.totals[2 * r] += cn[3];
          a.totals[2 * r + 1] += a.sums[2 * row + 1];
        }
      }
      if constexpr (RAVE) {
        // the playout's part per owned point and colour: (first plays, twice the colour's wins plus the draws among them)
        int32_t pn[2][kRavePts], ps[2][kRavePts];
        int firstj[kRavePts];   // path index j of the first tree move below the current node at this point, 0 = none
        const int32_t *am = a.amaf + row * 6 * (int64_t)P;
#pragma unroll
        for (int k = 0; k < kRavePts; ++k) {
          const int p = lane + k * kWave;
          firstj[k] = 0;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            pn[c][k] = ps[c][k] = 0;
            if (p < P) {
              const int32_t e0 = am[(3 * c) * P + p], e1 = am[(3 * c + 1) * P + p], e2 = am[(3 * c + 2) * P + p];
              pn[c][k] = e0;
              ps[c][k] = 2 * (c ? e2 : e1) + e0 - e1 - e2;
            }
          }
        }
        // the depth of the leaf: the links up to the root (parents have smaller ids: at most I of them, whatever the buffers hold)
        int dpt = 0;
        for (int x = y; dpt < a.I; ++dpt) {
          const int p = ln[2 * x];
          if (p < 0 || p >= x) break;
          x = p;
        }
        // from the leaf up: node x = x_i gets its update, then the move that led to it joins the front of the sequence
        int x = y;
        for (int i = dpt; i >= 0; --i) {
          // (the leaf's board is in `leaf`, whether it is a new node or not; every other node's board was stored by an earlier
          // launch: no walk of the select passes through a node of this round)
          const uint32_t c = (i == dpt ? src[5 * N] : a.boards[(r * NN + x) * W + 5 * N]) & 1u;
          const int32_t S = 2 * (c ? ww : bw) + d;
          int2 *na = reinterpret_cast<int2 *>(a.node_amaf) + (r * NN + x) * (int64_t)P;
#pragma unroll
          for (int k = 0; k < kRavePts; ++k) {
            const int p = lane + k * kWave;
            if (p >= P) continue;
            int32_t dn, ds;
            if (firstj[k] == 0) {
              dn = c ? pn[1][k] : pn[0][k];
              ds = c ? ps[1][k] : ps[0][k];
            } else {
              const bool mine = ((firstj[k] - i) & 1) != 0;
              dn = mine ? a.K : 0;
              ds = mine ? S : 0;
            }
            if (dn | ds) {
              int2 e = na[p];
              e.x += dn;
              e.y += ds;
              na[p] = e;
            }
          }
          if (i == 0) break;
          const int m = ln[2 * x + 1];
#pragma unroll
          for (int k = 0; k < kRavePts; ++k)
            if (m >= 0 && m == lane + k * kWave && m < P) firstj[k] = i;
          x = ln[2 * x];
        }
      }
    }
  }
}

}  // namespace gg
