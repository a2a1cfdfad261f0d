// gg_gumbel.h - the Gumbel root rule of the PUCT search (gg_gumbel_begin / gg_gumbel_select_leaves / gg_gumbel_root of
// include/gymgo_amd_gumbel.h, which holds the normative text): "Policy improvement by planning with Gumbel" (Danihelka et al.,
// ICLR 2022) at node 0 of every tree of gg_puct.h - m actions drawn without replacement by the Gumbel-top-k trick (the caller's
// base = g + logit), the move's n simulations spread over them by sequential halving (the caller's schedule seq), the action
// of the largest g + logit + sigma(q).  Everything below node 0 is the walk of gg_puct.h, the SAME code: the select kernel is
// k_puct_select<true, GumbelRoot>, and GumbelRoot::choose stands where step d stands at node 0.
//
// Per search on the device: base float32 [R][A] (NaN counts as -inf; entries of illegal actions are never read), seen int32
// [R][A] (n of node 0's child under a when the search of this move began, 0 without a child), done int32 [R] (this move's
// simulations handed out through the root rule), seq int32 [S], c_visit and c_scale float64.
//
// THE ROOT PASS (gumbel_gather, one wave, A <= 362: at most kPuctStrides = 6 actions a lane): legality from the root board's
// invalid rows, one 16-byte gather of each child's record, and per action in registers
//   n_c, w_c, v_c  the child's record (0 without a child, negatives as 0; v_c = 0 in the read-out)
//   k_a  = max(0, n_c + v_c - seen[a])          this move's simulations of a, those in flight included
//   qh_a = n_c > 0 ? s w_c / n_c : q0           q0 = s w_0 / n_0 (0.0 at n_0 = 0); virtual visits do not enter
// then maxn (the largest n_c) and kmax (the largest k_a) by two max reductions over the wave.  THE CHOICE (gumbel_argmax):
// E = the legal actions with k_a = need when there are any (a ballot), else those with k_a = kmax;
//   m1 = c_visit + (double)maxn;  m2 = m1 c_scale;  sigma = m2 qh_a;  G = (double)base[a] + sigma
// in float64, each operation rounded to nearest in this order, no contraction (NaN counts as -inf), and the wave's argmax of G
// over E with ties to the lowest action - the reduction of k_puct_select.  No LDS, no atomics, vector stores only, every index
// bounded by the tree (child ids in (0, nodes)).  In the select the records' v words are those lane 0 stored for the slots
// before this one: the hand-over fence at the head of every slot (puct_handover in k_puct_select) covers them.
#pragma once
#include "gg_puct.h"

namespace gg {

struct GumbelArgs {
  const float *base;         // [R][A] g + logit
  const int32_t *seen;       // [R][A] (begin: written)
  int32_t *done;             // [R] (begin: written; select: read and written; root: unused)
  const int32_t *seq;        // [S] the schedule (select)
  int32_t S;
  double c_visit, c_scale;
  int32_t *actions;          // [R] (root)
  float *q;                  // [R][A], may be NULL (root)
  int32_t *visits;           // [R][A], may be NULL (root)
  float *value;              // [R], may be NULL (root)
};

// what a lane keeps of its actions (stride i: action i * kWave + lane), and the wave's two maxima
struct GumbelLane {
  int32_t nc[kPuctStrides], ka[kPuctStrides];
  double qh[kPuctStrides];
  uint32_t legal;   // bit i: the action of stride i is legal
  int32_t maxn, kmax;
  double q0;
};

// g: node 0's board (its game has not ended), ch: node 0's child row, st: the root's records, sn: the root's seen row
template <bool VL>
__device__ __forceinline__ void gumbel_gather(GumbelLane &v, const uint32_t *g, const int32_t *ch, const PuctStat *st, int nodes,
                                              const int32_t *sn, double s, int N, int A, int lane) {
#pragma clang fp contract(off)
  const PuctStat k0 = st[0];
  v.q0 = k0.n > 0 ? s * k0.w / (double)k0.n : 0.0;
  v.legal = 0u;
  v.maxn = 0;
  v.kmax = 0;
#pragma unroll
  for (int i = 0; i < kPuctStrides; ++i) {
    const int act = i * kWave + lane;
    v.nc[i] = 0;
    v.ka[i] = 0;
    v.qh[i] = v.q0;
    if (act < A && puct_legal(g, act, N)) {
      v.legal |= 1u << i;
      const int c = ch[act];
      double wc = 0.0;
      int32_t nc = 0, vc = 0;
      if (c > 0 && c < nodes) {   // (children always have larger ids than their parent)
        const PuctStat k = st[c];
        wc = k.w;
        nc = k.n < 0 ? 0 : k.n;
        if (VL) vc = k.v < 0 ? 0 : k.v;
      }
      const int64_t k = (int64_t)nc + vc - sn[act];
      v.nc[i] = nc;
      v.ka[i] = (int32_t)(k < 0 ? 0 : (k > 0x7FFFFFFF ? 0x7FFFFFFF : k));
      if (nc > 0) v.qh[i] = s * wc / (double)nc;
      v.maxn = max(v.maxn, nc);
      v.kmax = max(v.kmax, v.ka[i]);
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    v.maxn = max(v.maxn, __shfl_xor(v.maxn, o));
    v.kmax = max(v.kmax, __shfl_xor(v.kmax, o));
  }
}

// the action of the largest G among the legal actions with k_a = need (need < 0, or no such action: k_a = kmax), ties to the
// lowest action, A without a legal action; bs: the root's base row
__device__ __forceinline__ int gumbel_argmax(const GumbelLane &v, int need, const float *bs, double c_visit, double c_scale, int A,
                                             int lane) {
#pragma clang fp contract(off)
  bool has = false;
#pragma unroll
  for (int i = 0; i < kPuctStrides; ++i) has = has || (((v.legal >> i) & 1u) && v.ka[i] == need);
  const bool any = __ballot(has) != 0ull;   // "E is non-empty", over the wave
  const int target = need >= 0 && any ? need : v.kmax;
  const double m1 = c_visit + (double)v.maxn;
  const double m2 = m1 * c_scale;
  double best = -__builtin_inf();
  int besta = A;
#pragma unroll
  for (int i = 0; i < kPuctStrides; ++i) {
    if (!((v.legal >> i) & 1u) || v.ka[i] != target) continue;
    const int act = i * kWave + lane;
    const double sigma = m2 * v.qh[i];
    const double sum = (double)bs[act] + sigma;
    const double G = sum == sum ? sum : -__builtin_inf();
    if (G > best || besta == A) {   // (this lane's actions ascend: the first of equal scores stays)
      best = G;
      besta = act;
    }
  }
  // the wave's argmax, ties to the lowest action (a lane without an action of E holds -inf / A and loses every tie)
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int oa = __shfl_xor(besta, o);
    if (ob > best || (ob == best && oa < besta)) {
      best = ob;
      besta = oa;
    }
  }
  return besta;
}

// the root rule of k_puct_select (gg_puct.h): the tree's arguments with the rule's behind them
struct GumbelSelectArgs : PuctArgs {
  GumbelArgs b;
};

struct GumbelRoot {
  static constexpr bool kOn = true;
  using Args = GumbelSelectArgs;
  static __device__ __forceinline__ int begin(const Args &a, int64_t r) { return __builtin_amdgcn_readfirstlane(a.b.done[r]); }
  static __device__ __forceinline__ int choose(const Args &a, int64_t r, int t, const uint32_t *g, const int32_t *ch, const PuctStat *st,
                                               int nodes, double s, int N, int A, int lane) {
    GumbelLane v;
    gumbel_gather<true>(v, g, ch, st, nodes, a.b.seen + r * A, s, N, A, lane);
    const int need = t >= 0 && t < a.b.S ? a.b.seq[t] : -1;
    return gumbel_argmax(v, need, a.b.base + r * A, a.b.c_visit, a.b.c_scale, A, lane);
  }
  static __device__ __forceinline__ void end(const Args &a, int64_t r, int t, int lane) {
    if (lane == 0) a.b.done[r] = t;
  }
};

// seen = n of node 0's children (0 without a child, negatives as 0), done = 0
static __global__ __launch_bounds__(4 * kWave) void k_gumbel_begin(PuctArgs a, int32_t *seen, int32_t *done) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int A = a.N * a.N + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const int32_t *ch = a.child + r * NN * A;   // node 0's row
    const PuctStat *st = a.stats + r * NN;
    const int nodes = max(1, min(a.nodes[r], NN));   // (1 <= nodes <= C + 1: every index below stays inside the tree)
    for (int act = lane; act < A; act += kWave) {
      const int c = ch[act];
      int32_t n = 0;
      if (c > 0 && c < nodes) n = max(st[c].n, 0);
      seen[r * A + act] = n;
    }
    if (lane == 0) done[r] = 0;
  }
}

// the read-out, outside a round (every v = 0, none is read): the action, q, the visits, the root value
static __global__ __launch_bounds__(4 * kWave) void k_gumbel_root(PuctArgs a, GumbelArgs b) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int N = a.N, W = 5 * N + 1, P = N * N, A = P + 1, NN = a.I + 1;
  for (int64_t r = wave; r < a.R; r += nwaves) {
    const uint32_t *g = a.boards + r * NN * W;   // node 0
    float *q = b.q ? b.q + r * A : nullptr;
    int32_t *vis = b.visits ? b.visits + r * A : nullptr;
    const uint32_t flag = __builtin_amdgcn_readfirstlane(g[5 * N]);
    if (flag & 4u) {   // the game has ended: no action, all-zero rows
      for (int act = lane; act < A; act += kWave) {
        if (q) q[act] = 0.f;
        if (vis) vis[act] = 0;
      }
      if (lane == 0) {
        b.actions[r] = -1;
        if (b.value) b.value[r] = 0.f;
      }
      continue;
    }
    const int nodes = max(1, min(a.nodes[r], NN));   // (1 <= nodes <= C + 1: every index below stays inside the tree)
    const double s = (flag & 1u) ? -1.0 : 1.0;
    GumbelLane v;
    gumbel_gather<false>(v, g, a.child + r * NN * A, a.stats + r * NN, nodes, b.seen + r * A, s, N, A, lane);
    const int besta = gumbel_argmax(v, -1, b.base + r * A, b.c_visit, b.c_scale, A, lane);
#pragma unroll
    for (int i = 0; i < kPuctStrides; ++i) {
      const int act = i * kWave + lane;
      if (act < A) {
        const bool legal = (v.legal >> i) & 1u;
        if (q) q[act] = legal ? (float)v.qh[i] : 0.f;
        if (vis) vis[act] = v.nc[i];   // (0 where illegal)
      }
    }
    if (lane == 0) {
      b.actions[r] = besta < A ? besta : P;   // (the pass is always legal: the fallback only with corrupt buffers)
      if (b.value) b.value[r] = (float)v.q0;
    }
  }
}

}  // namespace gg
