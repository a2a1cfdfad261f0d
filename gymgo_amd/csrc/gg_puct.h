// gg_puct.h - batched PUCT tree search with priors and a caller-supplied evaluator (gg_puct_begin / gg_puct_select /
// gg_puct_backup, and gg_puct_select_leaves / gg_puct_backup_leaves with several leaves per root and round): the tree of
// every root lives on the device, the select and backup kernels walk it, the leaves are handed out and their evaluations
// (priors, value) come back from outside the library.  There is ONE walk and ONE backup, k_puct_select<VL> and
// k_puct_backup<RR, VL>: VL = false is the one-leaf search, VL = true the search with virtual loss (further down).  The walk
// has a second parameter, Root: what chooses the action at node 0 (PuctNoRoot, the default: step d, as at every node).
//
// R independent searches of I iterations, one tree per root with room for I + 1 nodes (node 0 = the root).  Per node: its
// tracked board, parent / action (-1 at the root), the stat record {w: float64 sum of the backed-up values from black's point
// of view, n: int32 visits}, float32 priors [A] (zero until the node is evaluated) and a child table [A] (-1: no child),
// A = N^2 + 1.  One iteration on the host side is
//   k_puct_select -> gg_batch_play_moves_tracked(leaf, move, T = 1) -> gg_batch_untrack_states(leaf) or the feature planes
//   of the leaf -> k_puct_legal -> the caller's evaluator -> k_puct_backup
// so the leaf's move and its planes reuse the existing kernels unchanged.
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
//
// SEVERAL LEAVES PER ROOT AND ROUND, WITH VIRTUAL LOSS (VL = true; gg_puct_select_leaves / gg_puct_backup_leaves / gg_puct_legal
// of include/gymgo_amd.h, which holds the normative text).  The tree is the one above with C + 1 nodes, C = rounds * L; the
// reserved word of the stat record is v, the node's virtual visits: a slot that has found its leaf adds 1 to v from the leaf
// up to the root, the backup of that slot takes it off again, so every v is 0 outside a round.  Slot j of root r is row
// r L + j of leaf / move / leaf_id / priors / values.  The slots of a root run strictly in order inside one wave: later
// slots read child entries, links and stat words that lane 0 stored for earlier ones, so each such hand-over is a
// release / acquire fence pair (puct_handover) - the stores are waited for and the loads after it are issued anew.
// VL = false is the same code with one slot per root, every v taken as 0 and never loaded or stored, no fence and no
// collision test: every `if (VL)` below is one of these differences, and there are no others.
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
  uint32_t *leaf;            // [R L][5N+1] the board to evaluate
  int32_t *move;             // [R L] action to play on leaf first, -1 = none
  int32_t *leaf_id;          // [R L] the leaf node, -1 = an empty slot
  const float *priors;       // [R L][A] the evaluator's priors (backup)
  const float *values;       // [R L] the evaluator's values, mover's point of view (backup)
  double c;
  int64_t R;
  int32_t N, I;              // I: the capacity (C with several leaves)
  float komi;
  int32_t L;                 // slots per root and round (VL = true only; the one-leaf kernels have one)
};

// action act in [0, A) is legal on the tracked board g whose game has not ended: the pass, or a point whose bit in the
// invalid rows is clear (the ended-game test is the caller's)
__device__ __forceinline__ bool puct_legal(const uint32_t *g, int act, int N) {
  const int P = N * N, row = act / N;
  return act == P || !((g[2 * N + (act < P ? row : 0)] >> (act - row * N)) & 1u);
}

// lane 0's stores above become visible to every lane's loads below (one wave; the scope is the workgroup's, which contains it)
__device__ __forceinline__ void puct_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// U(x, a) = q + c prior sqrt(n_x + v_x) / (1 + n_c + v_c), q = (s w_c - v_c) / (n_c + v_c) (0 without visits): one virtual
// visit is one loss for the side that chose the child.  In float64, each operation rounded to nearest in this order: no
// contraction into fused multiply-adds (the host restatement computes the same expression in IEEE doubles).  A NaN (c = 0
// with an infinite prior) counts as -inf: it never beats a number.  VL = false takes every v as 0, which gives
// q = s w_c / n_c bit for bit (x - 0.0 = x for every x, -0.0 included) without the subtraction at run time.
template <bool VL>
__device__ __noinline__ double puct_score(double s, double wc, int32_t nc, int32_t vc, float prior, int32_t nx, int32_t vx,
                                          double c) {
#pragma clang fp contract(off)
  if (!VL) vc = vx = 0;
  const int32_t ne = nc + vc;
  const double q = ne == 0 ? 0.0 : (s * wc - (double)vc) / (double)ne;
  const double t1 = c * (double)prior;
  const double t2 = __dsqrt_rn((double)(nx + vx));
  const double t3 = t1 * t2;
  const double t4 = t3 / (double)(1 + ne);
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

// The root rule of the walk: what chooses a* at node 0 in place of step d.  PuctNoRoot is "nothing does", and with it every
// `if constexpr (Root::kOn)` below is discarded before any code is made: k_puct_select<VL> is the walk alone.  These blocks
// are the differences of a search with a root rule of its own (gg_gumbel.h has the one there is), and there are no others.
// A root rule names the kernel's argument struct, Args (PuctArgs, or a struct derived from it), and gives
//   begin(a, r)                                       -> the simulations of this move handed out so far (wave-uniform)
//   choose(a, r, t, g, ch, st, nodes, s, N, A, lane)  -> a* at node 0 for simulation t (wave-uniform, A = none)
//   end(a, r, t, lane)                                   the count after this launch's slots
struct PuctNoRoot {
  static constexpr bool kOn = false;
  using Args = PuctArgs;
};

template <bool VL, class Root = PuctNoRoot>
static __global__ __launch_bounds__(4 * kWave) void k_puct_select(typename Root::Args a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, A = N * N + 1, NN = a.I + 1, L = VL ? a.L : 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *bd = a.boards + r * NN * W;
    int32_t *ch = a.child + r * NN * A;
    const float *pr = a.prior + r * NN * A;
    PuctStat *st = a.stats + r * NN;
    int32_t *ln = a.links + r * NN * 2;
    int nodes = max(1, min(a.nodes[r], NN));   // (1 <= nodes <= I + 1 by construction: every index below stays inside the tree)
    bool open = true;                          // false from the slot that met a collision on (VL)
    [[maybe_unused]] int done = 0;             // (a root rule's count of this move's simulations)
    if constexpr (Root::kOn) done = Root::begin(a, r);
    for (int j = 0; j < L; ++j) {
      int x = 0, mv = -1, y = -1;
      [[maybe_unused]] bool ruled = false;     // the root rule chose this slot's action at node 0
      if (open) {
        if (VL) puct_handover();   // the links, child entries and v of the slots before this one
        // every step goes to a child with a larger id: at most I steps (the bound also stops a walk over corrupt links)
        for (int depth = 0; depth <= a.I; ++depth) {
          const int32_t nx = st[x].n, vx = VL ? st[x].v : 0;
          if (VL && nx <= 0 && vx > 0) {   // handed out earlier in this round, no board yet: a collision, before any read of x's board
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
          if constexpr (Root::kOn) {
            if (x == 0) {   // the root rule in place of step d
              besta = Root::choose(a, r, done, g, ch, st, nodes, s, N, A, lane);
              ruled = true;
            }
          }
          if (!Root::kOn || x != 0) {   // step d (a constant condition without a root rule)
            for (int a0 = 0; a0 < A; a0 += kWave) {
              const int act = a0 + lane;
              if (act >= A || !puct_legal(g, act, N)) continue;
              const int c = ch[(int64_t)x * A + act];
              const float p = pr[(int64_t)x * A + act];
              double wc = 0.0;
              int32_t nc = 0, vc = 0;
              if (c > x && c < nodes) {   // (children always have larger ids than their parent)
                const PuctStat k = st[c];
                wc = k.w;
                nc = k.n < 0 ? 0 : k.n;
                if (VL) vc = k.v < 0 ? 0 : k.v;
              }
              const double u = puct_score<VL>(s, wc, nc, vc, p, nx, vx < 0 ? 0 : vx, a.c);
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
          }
          if (besta >= A) break;   // (the pass is always legal: only with corrupt buffers)
          const int nxt = ch[(int64_t)x * A + besta];
          if (nxt < 0) {
            if (nodes <= a.I) {   // (a select beyond I leaves finds no room: x is evaluated as it is)
              y = nodes;
              mv = besta;
              nodes += 1;
              if (lane == 0) {
                ch[(int64_t)x * A + besta] = y;
                ln[2 * y] = x;
                ln[2 * y + 1] = besta;
                if (!VL) a.nodes[r] = nodes;
              }
            }
            break;
          }
          if (nxt <= x || nxt >= nodes) break;   // (only with corrupt buffers: stop here)
          x = nxt;
          y = x;
        }
      }
      const int64_t row = r * L + j;
      if (y < 0) {   // an empty slot (VL): the root's board, nothing to back up
        x = 0;
        mv = -1;
      } else if (VL && lane == 0) {   // one virtual visit on every node from the leaf up to the root (parents have smaller ids)
        int z = y;
        for (int depth = 0; depth <= a.I && z >= 0 && z < NN; ++depth) {
          st[z].v += 1;
          z = ln[2 * z];
        }
      }
      if constexpr (Root::kOn) {
        if (y >= 0 && ruled) done += 1;   // (a collision leaves the count as it leaves everything else)
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
    if (VL && lane == 0) a.nodes[r] = nodes;   // (the clamped count, whether or not a slot expanded)
    if constexpr (Root::kOn) Root::end(a, r, done, lane);
  }
}

// RR: the row capacity of the lat_areas instantiation (9 / 13 / 19, N <= RR)
template <int RR, bool VL>
static __global__ __launch_bounds__(4 * kWave) void k_puct_backup(PuctArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, A = N * N + 1, NN = a.I + 1, L = VL ? a.L : 1;
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
      if (VL) puct_handover();   // n of the slots before this one (an ended node may be taken twice in one round)
      if (st[y].n == 0) {   // the node's first evaluation: its priors, zero on illegal actions, NaN and negatives -> 0
        const float *p = a.priors + row * A;
        float *dst = a.prior + (r * NN + y) * A;
        for (int act = lane; act < A; act += kWave) {
          const bool legal = !(flag & 4u) && puct_legal(src, act, N);
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
        for (int depth = 0; depth <= a.I && x >= 0 && x < NN; ++depth) {   // (parents have smaller ids: at most I + 1 nodes)
          PuctStat &k = st[x];
          k.n += 1;
          k.w += vb;
          if (VL) k.v = k.v > 0 ? k.v - 1 : 0;   // the slot's virtual visit comes off, never below 0
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
  const int W = 5 * N + 1, A = N * N + 1;
  const int64_t total = B * A;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += gridDim.x * (int64_t)blockDim.x) {
    const int64_t row = i / A;
    const int act = (int)(i - row * A);
    const uint32_t *g = leaf + row * W;
    const bool ok = !(g[5 * N] & 4u) && puct_legal(g, act, N);
    legal[i] = ok ? 1 : 0;
    if (act == 0) live[row] = leaf_id[row] >= 0 ? 1 : 0;
  }
}

// ---------------------------------------------------------------- tree reuse across moves: keep the subtree of the move played
// k_puct_advance (gg_puct_advance of include/gymgo_amd.h, which holds the normative text).  Between two rounds (every v = 0)
// root r plays actions[r]: the subtree under that root child becomes the tree, in place, by an order-preserving renumbering;
// without such a child the tree is gg_puct_begin's for the board next[r]; -1 leaves the tree alone.  One wave per root, as
// everywhere in this file, in three steps:
//   MARK    ascending over 64 nodes at a time: node x is kept when it is k or its parent (smaller id) is kept.  Parents inside
//           the chunk are resolved by pointer jumping over shuffles, parents of earlier chunks from remap (a hand-over fence
//           per chunk); the new id of a kept node is the running count plus the ballot's prefix count.  remap[x] = new id, -1.
//   MOVE    ascending again, kPuctGroup kept nodes per turn: all their rows are loaded (dwordx4 per lane, the rows are only
//           4-byte aligned), then the child entries and the parent go through remap, then everything is stored at the new ids.
//           new(x) <= x and the sweep ascends, so a store never lands on a row that is still to be read: the rows of new id
//           j were those of a source <= every later source, and inside a turn every load precedes every store in program
//           order (the stores wait for their own operands, loads of one wave return in order).
//           HARDWARE ASSUMPTION, not the language's memory model: inside a turn one lane's store may land on words another
//           lane loaded in the same turn (new id n3 = source x1), with no fence between them.  That is safe because (a) a
//           wave's vector memory instructions issue in program order and its loads return in order (one vmcnt counter), so a
//           store, which waits for its own data, is issued after every earlier load of the wave has returned, and (b) the
//           compiler keeps the loads in front of the stores, which it must for a single lane already: both go through the
//           same base pointers at run-time indices.  Across lanes C++ calls this a data race; gfx9 wave execution orders it.
//           A puct_handover() in front of the store phase would say the same thing to the compiler; it is not there because
//           it is not needed on this target and its cost was not measured.
//   RESET   after a fence (every load above has returned): the nodes [kept, m) go back to gg_puct_begin's state as five flat
//           fills, dwordx4 from the first 16-byte boundary on.
// Every index is bounded by the tree: m clamped, parents in [k, x), children in (x, m), new ids clamped to [0, x].

typedef uint32_t puct_q __attribute__((ext_vector_type(4), aligned(4)));     // four words of a row: any word boundary
typedef uint32_t puct_q16 __attribute__((ext_vector_type(4), aligned(16)));  // four words on a 16-byte boundary

struct PuctAdvanceArgs {
  PuctArgs t;                // the tree; t.I = C, the capacity (leaf, move, leaf_id, priors, values unused)
  const int32_t *actions;    // [R] the action played at each root, -1 = none
  const uint32_t *next;      // [R][5N+1] the root's board after its action (read where a fresh tree is made)
  int32_t *remap;            // [R][C+1] scratch: the new id of every node, -1 = dropped
  int32_t *kept;             // [R] nodes kept (0: a fresh tree), may be NULL
};

constexpr int kPuctGroup = 4;   // kept nodes whose loads are in flight together (about 13 KB per wave at 19x19)

// Q * 64 dwordx4 and up to 3 single words per lane: a row of at most 256 Q + 3 words
template <int Q>
struct PuctRow {
  puct_q q[Q];
  uint32_t t;
};

template <int Q>
__device__ __forceinline__ void puct_row_load(PuctRow<Q> &v, const uint32_t *src, int words, int lane, bool on) {
  const int nq = words >> 2;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int q = lane + i * kWave;
    v.q[i] = puct_q{~0u, ~0u, ~0u, ~0u};
    if (on && q < nq) v.q[i] = *reinterpret_cast<const puct_q *>(src + 4 * q);
  }
  const int tw = 4 * nq + lane;   // (the words after the last whole four: lanes 0 .. words % 4 - 1)
  v.t = ~0u;
  if (on && tw < words) v.t = src[tw];
}

template <int Q>
__device__ __forceinline__ void puct_row_store(const PuctRow<Q> &v, uint32_t *dst, int words, int lane, bool on) {
  const int nq = words >> 2;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int q = lane + i * kWave;
    if (on && q < nq) *reinterpret_cast<puct_q *>(dst + 4 * q) = v.q[i];
  }
  const int tw = 4 * nq + lane;
  if (on && tw < words) dst[tw] = v.t;
}

// a child entry of node x under the renumbering: negative entries stay, a child id in (x, m) becomes its new id, anything
// else (only with corrupt buffers) -1.  The gather has no branch - an entry without a child reads remap[k], which is inside
// the tree - so that all the gathers of a turn are in flight together.
__device__ __forceinline__ uint32_t puct_new_child(uint32_t e, int x, int k, int m, const int32_t *rm) {
  const int c = (int)e;
  const bool inside = c > x && c < m;
  const uint32_t id = (uint32_t)rm[inside ? c : k];
  const uint32_t neg = (uint32_t)(c >> 31), in = 0u - (uint32_t)inside;   // all ones / zero: the choice below stays arithmetic
  return (e & neg) | ((id | ~in) & ~neg);
}

// p[0 .. words) = value: single words up to the first 16-byte boundary, dwordx4 from there, single words for the rest
__device__ __forceinline__ void puct_fill(uint32_t *p, int64_t words, uint32_t value, int lane) {
  if (words <= 0) return;
  const int64_t head = min(words, (int64_t)((4 - (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3));
  if (lane < head) p[lane] = value;
  p += head;
  words -= head;
  const int64_t nq = words >> 2;
  puct_q16 *q = reinterpret_cast<puct_q16 *>(p);
  const puct_q16 v = {value, value, value, value};
  for (int64_t i = lane; i < nq; i += kWave) q[i] = v;
  const int64_t tw = 4 * nq + lane;
  if (tw < words) p[tw] = value;
}

static __global__ __launch_bounds__(4 * kWave) void k_puct_advance(PuctAdvanceArgs b) {
  static_assert(5 * GG_MAX_BOARD + 1 <= 4 * kWave + 3 && GG_MAX_BOARD * GG_MAX_BOARD + 1 <= 8 * kWave + 3,
                "a board fits PuctRow<1>, a child or prior row PuctRow<2>");
  const PuctArgs &a = b.t;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, A = N * N + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    uint32_t *bd = a.boards + r * NN * W;
    uint32_t *ch = reinterpret_cast<uint32_t *>(a.child) + r * NN * A;
    uint32_t *pr = reinterpret_cast<uint32_t *>(a.prior) + r * NN * A;   // (priors move as bit patterns)
    int32_t *ln = a.links + r * NN * 2;
    PuctStat *st = a.stats + r * NN;
    int32_t *rm = b.remap + r * NN;
    const int m = __builtin_amdgcn_readfirstlane(max(1, min(a.nodes[r], NN)));   // (1 <= m <= C + 1: every index below stays inside the tree)
    const int act = b.actions[r];
    int k = -1;   // the node that becomes the root: 0 = the root stays, -1 = none (a fresh tree)
    if (act == -1) {
      k = 0;
    } else if (act >= 0 && act < A) {
      const int c0 = (int)ch[act];
      if (c0 >= 1 && c0 < m) k = c0;
    }
    k = __builtin_amdgcn_readfirstlane(k);
    if (k == 0) {   // not a byte of the tree changes
      if (lane == 0 && b.kept) b.kept[r] = m;
      continue;
    }
    int cnt = 0;   // kept nodes so far
    if (k > 0) {
      const int base0 = k & ~(kWave - 1);   // (nodes below k are dropped: their remap entries are never read)
      // MARK
      for (int base = base0; base < m; base += kWave) {
        const int x = base + lane;
        const int p = x < m ? ln[2 * (int64_t)x] : -1;
        int state = 0, ptr = 0;   // 0: dropped, 1: kept, 2: as the parent, which is lane ptr of this chunk
        if (x == k) {
          state = 1;
        } else if (x > k && x < m && p >= k && p < x) {   // (parents have smaller ids; below k nothing is kept)
          if (p >= base) {
            state = 2;
            ptr = p - base;
          } else {
            state = rm[p] >= 0 ? 1 : 0;
          }
        }
        // an unresolved lane points at a lower lane: the lowest of them resolves in every turn, jumping halves the chains
        while (__ballot(state == 2)) {
          const int s = __shfl(state, ptr), pp = __shfl(ptr, ptr);
          if (state == 2) {
            if (s != 2) state = s;
            else ptr = pp;
          }
        }
        const unsigned long long mask = __ballot(state == 1);
        if (x < m) rm[x] = state == 1 ? cnt + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
        cnt += __popcll(mask);
        puct_handover();   // the next chunk's lanes read remap entries that other lanes stored here
      }
      // MOVE
      for (int base = base0; base < m; base += kWave) {
        const int x = base + lane;
        const int id = x < m ? rm[x] : -1;
        unsigned long long mask = __ballot(id >= 0);
        while (mask) {
          int xs[kPuctGroup], ns[kPuctGroup];
          PuctRow<1> vb[kPuctGroup];
          PuctRow<2> vc[kPuctGroup], vp[kPuctGroup];
          int32_t lp[kPuctGroup], la[kPuctGroup];
          puct_q16 vs[kPuctGroup];   // the stat records as four words: w (two), n, v
#pragma unroll
          for (int i = 0; i < kPuctGroup; ++i) {
            xs[i] = -1;
            ns[i] = 0;
            if (mask) {
              const int bit = __ffsll(mask) - 1;
              xs[i] = base + bit;
              ns[i] = max(0, min(__shfl(id, bit), xs[i]));   // (new(x) <= x)
              mask &= mask - 1ull;
            }
          }
#pragma unroll
          for (int i = 0; i < kPuctGroup; ++i) {   // every load of the turn
            const bool on = xs[i] >= 0;
            const int64_t x64 = on ? xs[i] : 0;
            puct_row_load(vc[i], ch + x64 * A, A, lane, on);
            puct_row_load(vp[i], pr + x64 * A, A, lane, on);
            puct_row_load(vb[i], bd + x64 * W, W, lane, on);
            lp[i] = ln[2 * x64];   // (every lane the same words, no branch: only lane 0 stores them)
            la[i] = ln[2 * x64 + 1];
            vs[i] = *reinterpret_cast<const puct_q16 *>(st + x64);
          }
#pragma unroll
          for (int i = 0; i < kPuctGroup; ++i) {   // the renumbering: child entries and the parent
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              vc[i].q[j].x = puct_new_child(vc[i].q[j].x, xs[i], k, m, rm);
              vc[i].q[j].y = puct_new_child(vc[i].q[j].y, xs[i], k, m, rm);
              vc[i].q[j].z = puct_new_child(vc[i].q[j].z, xs[i], k, m, rm);
              vc[i].q[j].w = puct_new_child(vc[i].q[j].w, xs[i], k, m, rm);
            }
            vc[i].t = puct_new_child(vc[i].t, xs[i], k, m, rm);
            const bool below = lp[i] >= k && lp[i] < xs[i];   // (a kept node other than k has its parent in [k, x))
            const int32_t np = rm[below ? lp[i] : k];
            lp[i] = xs[i] == k || !below ? -1 : np;
            la[i] = xs[i] == k ? -1 : la[i];   // the new root
            vs[i].w = 0u;   // v
          }
#pragma unroll
          for (int i = 0; i < kPuctGroup; ++i) {   // every store of the turn (after every load: the assumption stated above)
            const bool on = xs[i] >= 0;
            const int64_t n64 = ns[i];
            puct_row_store(vc[i], ch + n64 * A, A, lane, on);
            puct_row_store(vp[i], pr + n64 * A, A, lane, on);
            puct_row_store(vb[i], bd + n64 * W, W, lane, on);
            if (on && lane == 0) {
              ln[2 * n64] = lp[i];
              ln[2 * n64 + 1] = la[i];
              *reinterpret_cast<puct_q16 *>(st + n64) = vs[i];
            }
          }
        }
      }
    } else {   // a fresh tree: node 0 = next[r]
      const uint32_t *nx = b.next + r * W;
      for (int i = lane; i < W; i += kWave) bd[i] = nx[i];
    }
    puct_handover();   // RESET: every row above has been read
    const int lo = cnt;   // (0 for a fresh tree: node 0 gets begin's rows as well, all but its board)
    puct_fill(ch + (int64_t)lo * A, (int64_t)(m - lo) * A, ~0u, lane);
    puct_fill(pr + (int64_t)lo * A, (int64_t)(m - lo) * A, 0u, lane);
    puct_fill(reinterpret_cast<uint32_t *>(ln) + (int64_t)lo * 2, (int64_t)(m - lo) * 2, ~0u, lane);
    puct_fill(reinterpret_cast<uint32_t *>(st) + (int64_t)lo * 4, (int64_t)(m - lo) * 4, 0u, lane);
    puct_fill(bd + (int64_t)max(lo, 1) * W, (int64_t)(m - max(lo, 1)) * W, 0u, lane);
    if (lane == 0) {
      a.nodes[r] = max(cnt, 1);
      if (b.kept) b.kept[r] = cnt;
    }
  }
}

// ---------------------------------------------------------------- self-play: noise into the root's priors, the move and the policy target
// k_puct_root_noise / k_puct_root_policy (gg_puct_root_noise / gg_puct_root_policy of include/gymgo_amd.h, which holds the
// normative text).  Both run outside a round (every v = 0) on node 0 of every tree, one wave per root as everywhere in this
// file, the lanes striding over the A actions with legality from the root board's invalid rows - k_puct_select's rule.  No
// atomics, no LDS, nothing read back.
//   NOISE   an applicable root (todo set, node 0 evaluated, game not over) gets prior_0[a] = keep prior_0[a] + eps z[a] on its
//           legal actions (float32, two products and one sum, no contraction; z = the noise with NaN / negatives / -0 as +0;
//           a NaN result as the one quiet NaN) and +0 elsewhere; todo[r] = 0.  Every other root keeps all its bytes.
//   POLICY  the lanes gather the visits of the root's children (kPuctStrides per lane, kept in registers), the wave sums them
//           (S) and takes the argmax (ties to the lowest action); with sample[r] and S > 0 one step of the root's generator
//           gives k in [0, S) and the action is the first one, ascending, whose running sum exceeds k: per stride an inclusive
//           scan over the lanes on top of the strides before it, the first lane past k from a ballot.  pi = n_a / S.

struct PuctRootArgs {
  PuctArgs t;                // the tree; t.I = C, the capacity (leaf, move, leaf_id, priors, values unused)
  const float *noise;        // [R][A] (noise)
  uint8_t *todo;             // [R] read and written (noise)
  float eps;                 // (noise)
  const uint8_t *sample;     // [R] 1 = draw the action in proportion to the visits; NULL = all 0 (policy)
  uint64_t *rng;             // [R] gg_rng_seed's generator, advanced once per draw (policy)
  int32_t *actions;          // [R] (policy)
  float *pi;                 // [R][A], may be NULL (policy)
  float *value;              // [R], may be NULL (policy)
};

constexpr int kPuctStrides = (GG_MAX_BOARD * GG_MAX_BOARD + 1 + kWave - 1) / kWave;   // 6 actions per lane at 19x19

__device__ __forceinline__ float puct_mix(float keep, float p, float eps, float z) {
#pragma clang fp contract(off)
  const float a = __fmul_rn(keep, p);
  const float b = __fmul_rn(eps, z);
  const float s = __fadd_rn(a, b);
  return s == s ? s : __uint_as_float(0x7FC00000u);   // (0 times an infinite value: one NaN, whatever the hardware's payload)
}

static __global__ __launch_bounds__(4 * kWave) void k_puct_root_noise(PuctRootArgs b) {
  const PuctArgs &a = b.t;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, A = N * N + 1, NN = a.I + 1;
  const float keep = __fsub_rn(1.0f, b.eps);
  for (int64_t r = wave; r < a.R; r += nwaves) {
    if (b.todo[r] == 0) continue;
    const uint32_t *g = a.boards + r * NN * W;   // node 0
    const uint32_t flag = g[5 * N];
    if ((flag & 4u) || a.stats[r * NN].n <= 0) continue;   // the game has ended, or the root is not evaluated yet: not a byte changes
    const float *z = b.noise + r * A;
    float *pr = a.prior + r * NN * A;   // node 0's row
    for (int act = lane; act < A; act += kWave) {
      const bool legal = puct_legal(g, act, N);
      const float zv = z[act];
      const float v = puct_mix(keep, pr[act], b.eps, zv > 0.f ? zv : 0.f);   // (NaN, negatives, -0 -> +0)
      pr[act] = legal ? v : 0.f;
    }
    if (lane == 0) b.todo[r] = 0;
  }
}

static __global__ __launch_bounds__(4 * kWave) void k_puct_root_policy(PuctRootArgs b) {
  const PuctArgs &a = b.t;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *g = a.boards + r * NN * W;   // node 0
    const int32_t *ch = a.child + r * NN * A;    // node 0's row
    const PuctStat *st = a.stats + r * NN;
    float *pi = b.pi ? b.pi + r * A : nullptr;
    const uint32_t flag = __builtin_amdgcn_readfirstlane(g[5 * N]);
    if (flag & 4u) {   // the game has ended: no action, an all-zero row, the generator untouched
      if (pi)
        for (int act = lane; act < A; act += kWave) pi[act] = 0.f;
      if (lane == 0) {
        b.actions[r] = -1;
        if (b.value) b.value[r] = 0.f;
      }
      continue;
    }
    const int nodes = max(1, min(a.nodes[r], NN));   // (1 <= nodes <= C + 1: every index below stays inside the tree)
    uint32_t na[kPuctStrides];   // the visits under this lane's actions, 0 where illegal or without a child
    uint32_t legal = 0u;         // bit i: the action of stride i is legal
    uint32_t sum = 0u;
    int32_t best = -1;
    int besta = A;
#pragma unroll
    for (int i = 0; i < kPuctStrides; ++i) {
      const int act = i * kWave + lane;
      na[i] = 0u;
      if (act < A) {
        if (puct_legal(g, act, N)) {
          legal |= 1u << i;
          const int c = ch[act];
          if (c > 0 && c < nodes) {
            const int32_t n = st[c].n;
            na[i] = n < 0 ? 0u : (uint32_t)n;
          }
          sum += na[i];
          if ((int32_t)na[i] > best) {   // (this lane's actions ascend: the first of equal counts stays)
            best = (int32_t)na[i];
            besta = act;
          }
        }
      }
    }
    // S, and the wave's argmax with ties to the lowest action (a lane without a legal action holds -1 / A and loses every tie)
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o);
      const int32_t ob = __shfl_xor(best, o);
      const int oa = __shfl_xor(besta, o);
      if (ob > best || (ob == best && oa < besta)) {
        best = ob;
        besta = oa;
      }
    }
    const uint32_t S = sum;
    int action = besta < A ? besta : P;   // (the pass is always legal: the fallback only with corrupt buffers)
    const bool draw = b.sample && b.sample[r] != 0 && S > 0u;
    if (draw) {
      uint64_t x = b.rng[r];
      const uint64_t u = splitmix_next(x);
      const uint32_t k = (uint32_t)(((u >> 32) * (uint64_t)S) >> 32);   // in [0, S)
      uint32_t base = 0u;   // the visits of the strides before this one
#pragma unroll
      for (int i = 0; i < kPuctStrides; ++i) {
        uint32_t run = na[i];   // inclusive scan over the lanes: the actions of a stride ascend with the lane
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
          const uint32_t up = __shfl_up(run, o);
          if (lane >= o) run += up;
        }
        const unsigned long long past = __ballot(base + run > k);
        if (past) {
          action = i * kWave + (__ffsll(past) - 1);
          break;
        }
        base += __shfl(run, kWave - 1);
      }
      if (lane == 0) b.rng[r] = x;
    }
    if (pi) {
      const float fs = (float)S;
#pragma unroll
      for (int i = 0; i < kPuctStrides; ++i) {
        const int act = i * kWave + lane;
        if (act < A) pi[act] = S > 0u && ((legal >> i) & 1u) ? __fdiv_rn((float)na[i], fs) : 0.f;
      }
    }
    if (lane == 0) {
      b.actions[r] = action;
      if (b.value) {
        const PuctStat k0 = st[0];
        const double s = (flag & 1u) ? -1.0 : 1.0;
        b.value[r] = k0.n > 0 ? (float)(s * k0.w / (double)k0.n) : 0.f;
      }
    }
  }
}

}  // namespace gg
