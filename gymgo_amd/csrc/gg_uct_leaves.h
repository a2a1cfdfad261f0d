// gg_uct_leaves.h - the UCT search with several leaves per root and round, chosen under virtual loss (gg_uct_select_leaves[_rave],
// gg_uct_backup_leaves[_rave], gg_uct_prior_expand_leaves of include/gymgo_amd_uct_leaves.h, which holds the normative text).
//
// The tree is gg_uct.h's with C + 1 nodes, C = rounds * L, plus virt = int32 [R][C+1]: v_x = the leaves handed out in the current
// round whose path goes through x.  Slot j of root r is row r L + j of leaf / move / leaf_id / counts / sums / amaf.  One wave per
// root, the L slots of a root strictly in order inside the wave; later slots read the child entries, links, stat words and v that
// lane 0 stored for earlier ones, so every slot starts with a release / acquire fence pair (uct_handover).  No atomics: a tree
// belongs to one wave.  No LDS and no scratch in the select and the backup.
//
// WHY THE BODIES STAND HERE A SECOND TIME.  k_uct_select_leaves is k_uct_select's walk and k_uct_backup_leaves k_uct_backup's body
// around a slot loop, and k_move_priors_leaves is k_move_priors' tree form with the tree taken from row / L.  Sharing one body
// with the one-leaf kernels (a `bool VL` on a common function) compiles k_uct_select, k_uct_backup and k_move_priors to other
// instruction schedules than they have; the one-leaf path is to stay the machine code it is, so gg_uct.h and gg_prior.h are
// untouched and the differences are marked here, each with `VL:`.  The scores are NOT restated: uct_score and rave_score of
// gg_uct.h are the only float expressions, so with every v = 0 a slot chooses what k_uct_select chooses, bit for bit.
// A FIX TO gg_uct.h's WALK OR FOLD, OR TO k_move_priors, IS A FIX HERE TOO (follow-up); leaves=1 against leaves=None in
// tests/test_gpu_uct_leaves.py fails when only one side was changed.
#pragma once
#include "gg_uct.h"
#include "gg_prior.h"

namespace gg {

// lane 0's stores above become visible to every lane's loads below (one wave; the scope is the workgroup's, which contains it)
__device__ __forceinline__ void uct_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool RAVE>
static __global__ __launch_bounds__(4 * kWave) void k_uct_select_leaves(UctArgs a, int32_t *virt, int32_t L) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *bd = a.boards + r * NN * W;
    int32_t *ch = a.child + r * NN * A;
    int32_t *st = a.stats + r * NN * 4;
    int32_t *ln = a.links + r * NN * 2;
    int32_t *vt = virt + r * NN;
    // VL: nodes lives in a register over the slots and is stored once (1 <= nodes <= I + 1: every index below stays inside the tree)
    int nodes = max(1, min(a.nodes[r], NN));
    bool open = true;   // VL: false from the slot that met a collision on
    for (int j = 0; j < L; ++j) {
      int x = 0, mv = -1, y = -1;
      if (open) {
        uct_handover();   // VL: the links, child entries, stats and v of the slots before this one
        // every step goes to a child with a larger id: at most I steps (the bound also stops a walk over corrupt links)
        for (int depth = 0; depth <= a.I; ++depth) {
          const int32_t nx0 = st[4 * x];
          if (x > 0 && nx0 <= 0) {   // VL: created earlier in this round, no board yet: a collision, before any read of x's board
            open = false;
            y = -1;
            break;
          }
          const uint32_t *g = bd + (int64_t)x * W;
          const uint32_t flag = g[5 * N];
          y = x;
          if (flag & 4u) break;   // the game has ended at x: x is the leaf, nothing is added
          const int t = nx0 / a.K + vt[x];   // VL: + v_x (n_x is a multiple of K, at most I K; v_x <= L)
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
                n = q.x + a.K * vt[c];   // VL: a virtual visit is K playouts, none of them won (n_c + K v_c <= I K)
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
              u = uct_score(white ? s.z : s.y, s.w, s.x + a.K * vt[c], lx, a.c);   // VL: + K v_c
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
              }
              ++nodes;
            }
            break;
          }
          if (nx <= x || nx >= nodes) break;   // (only with corrupt buffers: stop here)
          x = nx;
          y = x;
        }
      }
      if (y < 0) {
        x = 0;   // VL: an empty slot hands the root's board out
      } else if (lane == 0) {   // VL: the hand-over - one more leaf through every node from y up to the root
        for (int z = y, depth = 0; depth <= a.I; ++depth) {   // (parents have smaller ids: at most I + 1 nodes)
          vt[z] += 1;
          const int p = ln[2 * z];
          if (p < 0 || p >= z) break;
          z = p;
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
    if (lane == 0) a.nodes[r] = nodes;
  }
}

template <bool RAVE>
static __global__ __launch_bounds__(4 * kWave) void k_uct_backup_leaves(UctArgs a, int32_t *virt, int32_t L) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, NN = a.I + 1, P = N * N;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    int32_t *st = a.stats + r * NN * 4;
    const int32_t *ln = a.links + r * NN * 2;
    int32_t *vt = virt + r * NN;
    for (int j = 0; j < L; ++j) {   // VL: the slots in ascending order
      const int64_t row = r * L + j;
      const int y = a.leaf_id[row];
      if (y < 0 || y >= NN) continue;   // VL: an empty slot (-1), or a leaf id outside the tree
      // VL: the fence pair every slot starts with.  Nothing below depends on it across lanes - stats, v and totals are lane 0's
      // alone, a point's pair is read and rewritten by the lane that owns the point in every slot, and no board stored here is
      // read again in this launch - so it only keeps the slots' memory operations apart, as the rule's text asks
      uct_handover();
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
          vt[x] = max(vt[x] - 1, 0);   // VL: the leaf is no longer out
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

// k_move_priors<R, true, true> with need_move, for the R L rows of a round: in = leaf uint32 [B][5N+1], last = move, node =
// leaf_id, B = R L.  Row b seeds node leaf_id[b] of tree b / L of out = node_amaf [R][I+1][N^2][2]; a row with move < 0 or a leaf id
// outside [0, I] is skipped.  The rows of a tree that are not skipped name different nodes - each is a node of its own, made in
// this round -, so no two boards add to the same words.
template <int R>
static __global__ __launch_bounds__(kWave) void k_move_priors_leaves(const uint32_t *__restrict__ in, const int32_t *__restrict__ last,
                                                                     const int32_t *__restrict__ weights, uint32_t *__restrict__ out,
                                                                     const int32_t *__restrict__ node, int I, int L, int64_t B, int N) {
  using Q = Prior<R>;
  constexpr int LPB = Q::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[Q::kLdsWords];
  PlaneFrame<R> f(N);
  const uint32_t full = f.full;
  const bool top = f.r == 0, bot = f.r == N - 1;
  const uint32_t tf = top ? full : 0u, bf = bot ? full : 0u;
  const uint32_t edge = (top || bot) ? full : (1u | (1u << (N - 1)));
  const int P = N * N;
  uint32_t wv[kPriorTerms], ws[kPriorTerms];   // visits, 2 wins: the units of (n~, s~)
#pragma unroll
  for (int k = 0; k < kPriorTerms; ++k) {
    wv[k] = (uint32_t)weights[2 * k];
    ws[k] = 2u * (uint32_t)weights[2 * k + 1];
  }
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl, wh, inv, fl;
    plane_load<R, true>(in, nullptr, f, B, N, lds, bl, wh, inv, fl);
    uint32_t cls[4];
    feat_groups<R, false>(bl, wh, full, cls);
    const bool white = (fl & 1u) != 0, done = (fl & 4u) != 0;
    const uint32_t me = white ? wh : bl, op = white ? bl : wh;
    const uint32_t M = B3(cls[1], cls[2], cls[3], T_OR3);   // the stones of groups with >= 2 liberties
    // (the DPP moves run in every lane, outside any select: a lane masked off while its neighbour reads it would hand over zero)
    const uint32_t aboveM = lat_above<LPB>(me), belowM = lat_below<LPB>(me);
    const uint32_t aboveO = lat_above<LPB>(op), belowO = lat_below<LPB>(op);
    const uint32_t aboveC = lat_above<LPB>(M), belowC = lat_below<LPB>(M);
    const uint32_t meU = aboveM | tf, meD = belowM | bf;
    uint32_t Cr, Er;
    tactical_rows(me, op, M, meU, meD, aboveO, belowO, aboveC | tf, belowC | bf, full, Cr, Er);
    const uint32_t valid = done ? 0u : (full & ~inv);
    const uint32_t Xr = valid & eye_row(me, op, meU, meD, aboveO, belowO, full, edge, N);   // valid & ~F: the mover's own eyes
    uint32_t Pr = 0u;
    if (f.on && f.r < N && !done) {
      const uint32_t uM = top ? ~0u : pattern_pad(aboveM, N), uO = top ? ~0u : pattern_pad(aboveO, N);
      const uint32_t dM = bot ? ~0u : pattern_pad(belowM, N), dO = bot ? ~0u : pattern_pad(belowO, N);
      Pr = pattern_row(uM, uO, pattern_pad(me, N), pattern_pad(op, N), dM, dO, N) & full & ~(me | op);
    }
    // the previous point: a point of the board or nothing
    const int64_t b = f.on ? f.b_first + f.j : 0;
    const int la = f.on ? last[b] : -1;
    uint32_t near = 0u;
    if ((uint32_t)la < (uint32_t)P) {
      const int pr = la / N, pc = la - pr * N;
      if (f.r >= pr - 1 && f.r <= pr + 1) near = ((7u << pc) >> 1) & ~(f.r == pr ? 1u << pc : 0u);
    }
    const uint32_t rows[kPriorTerms] = {valid, Cr & valid, Er & valid, Pr & valid, valid & ~Xr & Pr & near, Xr};
    // this lane's destination: its board's node, in the tree of its row (VL: b / L)
    const int y = f.on ? node[b] : 0;
    const bool go = f.on && y >= 0 && y <= I && la >= 0;
    const uint32_t *dst = out + (((b / L) * (int64_t)(I + 1) + (go ? y : 0)) * P) * 2;
    const int so = f.j * Q::kSegWords;   // the segment inside LDS
    const int mo = (int)(((uintptr_t)dst & 15u) >> 2);
    WAVE_SYNC();
    if (go && f.r < N) {
      uint32_t *w = lds + so + mo + f.r * 2 * N;
      for (int c = 0; c < N; ++c) {
        uint32_t v = 0u, s = 0u;
#pragma unroll
        for (int k = 0; k < kPriorTerms; ++k) {
          const uint32_t m = 0u - ((rows[k] >> c) & 1u);
          v += m & wv[k];
          s += m & ws[k];
        }
        w[2 * c] = v;
        w[2 * c + 1] = s;
      }
    }
    WAVE_SYNC();
    // board by board, the whole wave: every lane works the destination out again from the board's own words
    for (int j = 0; j < f.nb; ++j) {
      const int64_t bj = f.b_first + j;
      const int yj = node[bj];
      if (yj < 0 || yj > I || last[bj] < 0) continue;
      uint32_t *dj = out + (((bj / L) * (int64_t)(I + 1) + yj) * P) * 2;
      prior_store<true>(dj, lds + j * Q::kSegWords, (int)(((uintptr_t)dj & 15u) >> 2), 2 * P, f.lane);
    }
    WAVE_SYNC();
  }
}

}  // namespace gg
