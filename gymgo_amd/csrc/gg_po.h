// gg_po.h - batched Monte Carlo playouts to the end of the game (gg_playouts_begin / gg_playouts_advance): the FILL and
// HARVEST kernels around the tracked multi-ply rollout.
//
// J = R K jobs (K playouts of each of R roots) run on S working boards ("slots", tracked format).  The host side queues
// rollout chunks of `chunk_plies` plies on all slots (gg_batch_rollout_tracked, auto_reset = 0, the per-slot ply counter
// in steps_done), each followed by one harvest launch: every slot whose game has ended (flag bit 2) or that has played
// max_plies is scored (Tromp-Taylor areas, gym_go/gogame.py:275-300), added to its root's integer counters with vector
// atomics and refilled with the next job of the queue (one returning atomicAdd per wave; the wave's free slots take
// consecutive ids in lane order).  A slot the queue cannot refill is marked finished and stays frozen in later chunks.
// Refills happen between launches only, so a board's live plies remain a prefix of every rollout launch (gg_v5.h) and
// the rollout kernels need no change.
//
// Layout: one row per lane, one board per LPB lanes (gg_lat.h): the areas are lat_areas' two floods of the empty points,
// here also returned as owned rows for the per-point ownership counts.
//
// Flat Monte Carlo (gg_move_playouts_plan / _begin / _advance): the same kernel with MpArgs.  The plan (k_mp_counts, the
// scan of k_children_order_scan, k_mp_plan) lists the legal (root, action) pairs; a refill plays the pair's action on the
// root with lat_play_full (the five-flood ply) before it stores the child, so the first move also happens between launches.
#pragma once
#include <type_traits>

#include "gg_lat.h"

namespace gg {

struct PoArgs {
  const uint32_t *roots;   // [R][5N+1] tracked roots
  uint32_t *slots;         // [S][5N+1] working boards
  uint64_t *rng;           // [S]
  int64_t *plies;          // [S] plies of the slot's current job (steps_done of the rollout launches)
  int64_t *job;            // [S] local job id of the slot, -1 = empty
  int64_t *counter;        // [2] next job id, its value once every job is done (J + min(S, J))
  int32_t *counts;         // [R][4] black wins, white wins, draws, unfinished
  int64_t *sums;           // [R][2] sum of (black - white), sum of plies
  int32_t *own;            // [R][2][N][N] or null
  int64_t S, J, first_job;
  uint64_t base_seed;
  int32_t K, max_plies;
  float komi;
};

// generator of global job p: gg_rng_seed(base_seed, first_game = p) (k_rng_seed, gg_common.h)
__device__ __forceinline__ uint64_t po_seed(uint64_t base_seed, int64_t p) {
  uint64_t x = base_seed ^ ((uint64_t)p * 0xD1342543DE82EF95ull);
  splitmix_next(x);
  return x;
}

// lat_areas with the owned rows as well: black owns bl | (flood from black & ~flood from white), white alike
template <int R>
__device__ __forceinline__ void lat_areas_owned(uint32_t bl, uint32_t wh, uint32_t full, uint32_t &own_b, uint32_t &own_w,
                                                uint32_t &area_b, uint32_t &area_w) {
  constexpr int LPB = Lat<R>::LPB;
  uint32_t fb, fw;
  lat_area_floods<R>(bl, wh, full, fb, fw);
  own_b = bl | (fb & ~fw);
  own_w = wh | (fw & ~fb);
  const uint32_t sum = lat_board_sum<LPB>((uint32_t)__popc(own_b) | ((uint32_t)__popc(own_w) << 16));   // (<= 361 each)
  area_b = sum & 0xFFFFu;
  area_w = sum >> 16;
}

// First-move playouts (gg_move_playouts_*): the jobs of a legal (root, action) pair are K playouts from the child.  The plan
// lists the T legal pairs as r A + a (A = N^2 + 1); local job q is playout j = q % K of pair plan[q / K], global job
// ((first_root + r) A + a) K + j.  A slot's job word holds the pair, not q: the counters are indexed by it.
struct MpArgs : PoArgs {  // J = T K; first_job and own unused
  const int32_t *plan;    // [T] r A + a
  int64_t first_pair;     // first_root A
  int32_t A;
};

// AMAF playouts (gg_playouts_advance_amaf, include/gymgo_amd_amaf.h): the chunks log their moves (the log variants of
// the rollout kernels), and every harvest folds the new entries of every live slot into the slot's first-play rows - the points
// black / white played first in the slot's current job - before anything else; a finished slot adds them to its root's counters
// with the scored outcome, a refilled or emptied slot starts from zero rows.
struct AmafArgs : PoArgs {
  const uint16_t *log;   // [S][chunk_plies] the actions of the last chunk, entry t = the ply t of that launch
  uint32_t *first;       // [S][2][N] rows of the points black / white played first in the slot's current job
  int64_t *mark;         // [S] plies of the slot's job at the last harvest
  int32_t *amaf;         // [R][2][3][N][N] per root and colour: first plays, those in black wins, those in white wins
  int32_t chunk_plies;
};

// The pattern policy's queues (gg_playouts_advance_policy3, gg_move_playouts_advance_policy3, include/gymgo_amd_pattern.h,
// DESIGN 36): the chunks read and write `last`, the previous action of every slot, and the harvest sets last[s] = -1 for every
// slot it refills or empties - a job's first playout ply has no previous point, whatever the slot played before.
template <class Base>
struct LastArgs : Base {
  int32_t *last;   // [S]
};

// FILL (gg_playouts_begin): slot s takes job s (an empty, frozen board from s = J on) and the counter is set to
// {min(S, J), J + min(S, J)}.  HARVEST (gg_playouts_advance, after every rollout chunk): see the file's header.
// MOVE (gg_move_playouts_*): a refill loads the pair's root into the registers of the ply (as env_step_lat_body does), plays
// the pair's action with lat_play_full - wave-collective, so before the finished boards part from the others - and stores
// the child in the tracked layout; the counters are per pair.
template <int R, bool FULLN, bool FILL, typename Args = PoArgs>
__global__ __launch_bounds__(kWave) void k_po_harvest(Args a, int N) {
  constexpr bool MOVE = std::is_base_of<MpArgs, Args>::value;
  constexpr bool AMAF = std::is_same<Args, AmafArgs>::value;
  constexpr bool LAST = std::is_same<Args, LastArgs<PoArgs>>::value || std::is_same<Args, LastArgs<MpArgs>>::value;
  static_assert(!(LAST && FILL), "the pattern policy's queues are filled by the plain fill");
  static_assert(!(AMAF && FILL), "the AMAF queue is filled by the plain fill");
  using L = Lat<R>;
  constexpr int LPB = L::LPB, NBW = L::NBW;
  if (FULLN) N = R;
  const int lane = threadIdx.x & (kWave - 1);
  const int r = lane & (LPB - 1), j = lane / LPB;
  const int W = 5 * N + 1;
  const uint32_t full = r < N ? (1u << N) - 1u : 0u;
  if (FILL && blockIdx.x == 0 && lane == 0) {   // every harvested job pulls one id: all are done when word 0 reaches word 1
    a.counter[0] = a.J < a.S ? a.J : a.S;
    a.counter[1] = a.J + a.counter[0];
  }
  const int64_t ngroups = (a.S + NBW - 1) / NBW;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t s = g * NBW + j;
    const bool valid = s < a.S;
    uint32_t *slot = a.slots + (valid ? s : 0) * W;
    int64_t jid = -1;
    uint32_t flag = 0;
    bool fin = valid;
    if (!FILL) {
      if (valid) {
        jid = a.job[s];
        flag = slot[5 * N];
      }
      fin = valid && jid >= 0 && ((flag & 4u) != 0 || a.plies[s] >= a.max_plies);
    }
    // AMAF: the fold.  The lane of row r takes the new log entries of its slot - the plies since the last harvest, t < plies[s] -
    // mark[s] <= chunk_plies - that fall in its row and are in neither row yet; ply i of a job is played by the root's mover,
    // flipped for every earlier ply (passes included).  The entries come LPB at a time: lane i of the board loads entry t0 + i (one
    // coalesced 2-byte load per lane), and the board walks them in ply order by ds_bpermute - every lane of the wave takes part in
    // the walk, an entry beyond the board's count reads as 0xFFFF, which lies in no row.
    uint32_t fb = 0, fw = 0;
    if constexpr (AMAF) {
      const bool livejob = valid && jid >= 0;
      int64_t mk = 0;
      int nt = 0;
      uint32_t col0 = 0;
      uint32_t *fr = a.first + (2 * (valid ? s : 0) * N + (r < N ? r : 0));
      if (livejob) {
        mk = a.mark[s];
        const int64_t np = a.plies[s] - mk;
        nt = np < 0 ? 0 : (np > a.chunk_plies ? a.chunk_plies : (int)np);
        col0 = (a.roots[(jid / a.K) * W + 5 * N] ^ (uint32_t)mk) & 1u;
        if (r < N) {
          fb = fr[0];
          fw = fr[N];
        }
      }
      int ntw = nt;   // the longest walk of the wave's boards
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) ntw = max(ntw, __shfl_xor(ntw, o));
      const uint16_t *lg = a.log + (valid ? s : 0) * (int64_t)a.chunk_plies;
      const int lo = r * N, hi = r < N ? lo + N : lo;
      const int lane_b0 = lane & ~(LPB - 1);
      for (int t0 = 0; t0 < ntw; t0 += LPB) {
        const int mine = t0 + r < nt ? (int)lg[t0 + r] : 0xFFFF;
        const int lim = ntw - t0 < LPB ? ntw - t0 : LPB;
        for (int k = 0; k < lim; ++k) {
          const int act = __shfl(mine, lane_b0 + k);
          if (act >= lo && act < hi) {
            const uint32_t bit = 1u << (act - lo);
            if (!((fb | fw) & bit)) {
              if ((col0 ^ (uint32_t)(t0 + k)) & 1u) fw |= bit;
              else fb |= bit;
            }
          }
        }
      }
      if (livejob && !fin) {   // (a finished slot's rows go to amaf below and are zeroed with the refill)
        if (r < N) {
          fr[0] = fb;
          fr[N] = fw;
        }
        if (r == 0) a.mark[s] = mk + nt;
      }
    }
    const uint64_t lead = __ballot(fin && r == 0);   // one bit per finished board, at its first lane
    if (lead == 0) continue;
    int64_t next;
    if (FILL) {
      next = s;
    } else {
      // score: every lane takes part in the floods (rows of the other boards are zero)
      uint32_t bl = 0, wh = 0;
      if (fin && r < N) {
        bl = slot[r];
        wh = slot[N + r];
      }
      uint32_t ob, ow, ab, aw;
      lat_areas_owned<R>(bl, wh, full, ob, ow, ab, aw);
      if (fin) {
        const int64_t root = MOVE ? jid : jid / a.K;   // (MOVE: the pair r A + a)
        if (r == 0) {
          const int d = (int)ab - (int)aw;
          const float x = (float)d - a.komi;
          atomicAdd(a.counts + 4 * root + (x > 0.f ? 0 : (x < 0.f ? 1 : 2)), 1);
          if (!(flag & 4u)) atomicAdd(a.counts + 4 * root + 3, 1);
          atomicAdd(reinterpret_cast<unsigned long long *>(a.sums + 2 * root), (unsigned long long)(int64_t)d);
          atomicAdd(reinterpret_cast<unsigned long long *>(a.sums + 2 * root + 1), (unsigned long long)a.plies[s]);
        }
        if (!MOVE && a.own && r < N) {
          int32_t *pb = a.own + (2 * root * N + r) * N, *pw = pb + N * N;
          for (uint32_t m = ob; m; m &= m - 1) atomicAdd(pb + __builtin_ctz(m), 1);
          for (uint32_t m = ow; m; m &= m - 1) atomicAdd(pw + __builtin_ctz(m), 1);
        }
        if constexpr (AMAF) {   // the finished job's first plays, with the outcome scored above: one vector atomic per set bit
          if (r < N) {
            const float x = (float)((int)ab - (int)aw) - a.komi;
            const int win = x > 0.f ? 1 : (x < 0.f ? 2 : 0);
            const int64_t PP = (int64_t)N * N;
            int32_t *qb = a.amaf + 6 * root * PP + r * N, *qw = qb + 3 * PP;
            for (uint32_t m = fb; m; m &= m - 1) {
              atomicAdd(qb + __builtin_ctz(m), 1);
              if (win) atomicAdd(qb + win * PP + __builtin_ctz(m), 1);
            }
            for (uint32_t m = fw; m; m &= m - 1) {
              atomicAdd(qw + __builtin_ctz(m), 1);
              if (win) atomicAdd(qw + win * PP + __builtin_ctz(m), 1);
            }
          }
        }
      }
      // the wave's finished boards: one returning atomicAdd takes their job ids (ids from J on: none left; every
      // harvested job pulls exactly one id, so the same word counts the jobs done)
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(reinterpret_cast<unsigned long long *>(a.counter), (unsigned long long)__popcll(lead));
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base), hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
      next = (int64_t)(((uint64_t)hi << 32) | lo) + __popcll(lead & ((1ull << (j * LPB)) - 1ull));
    }
    if constexpr (MOVE) {
      const bool refill = fin && next < a.J;
      uint32_t me = 0, op = 0, M = 0, inv = 0, fl = 0, Q = 0;
      bool pass = false;
      int64_t pair = 0, gjob = 0;
      if (refill) {   // the root's rows in the registers of the ply, the action as Q / pass
        const int64_t c = next / a.K;
        pair = a.plan[c];
        const int64_t root = pair / a.A;
        const int act = (int)(pair - root * a.A);
        gjob = (a.first_pair + pair) * a.K + (next - c * a.K);
        const uint32_t *src = a.roots + root * W;
        fl = src[5 * N] & 7u;
        uint32_t bl = 0, wh = 0;
        if (r < N) {
          bl = src[r]; wh = src[N + r]; inv = src[2 * N + r];
          M = src[3 * N + r] | src[4 * N + r];
        }
        me = (fl & 1u) ? wh : bl;
        op = (fl & 1u) ? bl : wh;
        pass = act == N * N;
        const int ar = pass ? 0 : act / N;
        Q = (!pass && r == ar) ? (1u << (act - ar * N)) : 0u;
      }
      if (__ballot(refill)) lat_play_full<R>(me, op, M, inv, fl, Q, pass, refill ? ~0u : 0u, full);
      if (refill) {   // the child, tracked: a fresh generator, the ply count from zero (the first move is not counted)
        const uint32_t bl = (fl & 1u) ? op : me, wh = (fl & 1u) ? me : op;
        if (r < N) {
          slot[r] = bl; slot[N + r] = wh; slot[2 * N + r] = inv;
          slot[3 * N + r] = M & bl; slot[4 * N + r] = M & wh;
        }
        if (r == 0) {
          slot[5 * N] = fl;
          a.rng[s] = po_seed(a.base_seed, gjob);
          a.plies[s] = 0;
          a.job[s] = pair;
          if constexpr (LAST) a.last[s] = -1;   // (the first move is the root's business: the playout starts without a previous point)
        }
        continue;
      }
    }
    if (!fin) continue;
    if constexpr (AMAF) {   // a refilled or emptied slot starts from zero rows
      if (r < N) {
        a.first[2 * s * N + r] = 0u;
        a.first[(2 * s + 1) * N + r] = 0u;
      }
      if (r == 0) a.mark[s] = 0;
    }
    if constexpr (LAST) {   // a refilled or emptied slot has no previous point
      if (r == 0) a.last[s] = -1;
    }
    if (next < a.J) {   // refill: the root's words, a fresh generator, the ply count from zero
      const int64_t root = next / a.K;
      const uint32_t *src = a.roots + root * W;
      if (r < N) {
#pragma unroll
        for (int p = 0; p < 5; ++p) slot[p * N + r] = src[p * N + r];
      }
      if (r == 0) {
        slot[5 * N] = src[5 * N];
        a.rng[s] = po_seed(a.base_seed, a.first_job + next);
        a.plies[s] = 0;
        a.job[s] = next;
      }
    } else {            // the queue is empty: an empty board with the game-over bit, frozen from now on
      if (r < N) {
#pragma unroll
        for (int p = 0; p < 5; ++p) slot[p * N + r] = 0u;
      }
      if (r == 0) {
        slot[5 * N] = 4u;
        a.plies[s] = 0;
        a.job[s] = -1;
      }
    }
  }
}

// The plan of gg_move_playouts_plan, step 1: per tracked root, the number of legal first moves (the points whose invalid bit
// is clear + the pass; none once the game has ended), one thread per root.  Step 2 is k_children_order_scan (gg_v2.h).
static __global__ void k_mp_counts(const uint32_t *__restrict__ roots, int32_t *__restrict__ counts, int64_t R, int N) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= R) return;
  const uint32_t *g = roots + i * (5 * N + 1);
  const uint32_t full = (1u << N) - 1u;
  int c = 1;
  for (int y = 0; y < N; ++y) c += __popc(full & ~g[2 * N + y]);
  counts[i] = (g[5 * N] & 4u) ? 0 : c;
}

// step 3: root r's legal actions in ascending order (the pass last) at plan[offsets[r] ..], one wave per root: 64 points
// per round, the rank of each legal point by a ballot prefix.
static __global__ void k_mp_plan(const uint32_t *__restrict__ roots, const int32_t *__restrict__ offsets,
                                 int32_t *__restrict__ plan, int64_t R, int N) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (gridDim.x * (int64_t)blockDim.x) / kWave;
  const int P = N * N, A = P + 1;
  for (int64_t r = wave; r < R; r += nwaves) {
    const uint32_t *g = roots + r * (5 * N + 1);
    if (g[5 * N] & 4u) continue;
    int32_t *out = plan + offsets[r];
    const int32_t base = (int32_t)r * A;
    int k = 0;
    for (int p0 = 0; p0 < P; p0 += kWave) {
      const int p = p0 + lane;
      const int y = p / N;
      const bool ok = p < P && !((g[2 * N + (p < P ? y : 0)] >> (p - y * N)) & 1u);
      const uint64_t m = __ballot(ok);
      if (ok) out[k + __popcll(m & ((1ull << lane) - 1ull))] = base + p;
      k += __popcll(m);
    }
    if (lane == 0) out[k] = base + P;
  }
}

}  // namespace gg
