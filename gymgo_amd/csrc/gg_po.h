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
#pragma once
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
  using L = Lat<R>;
  constexpr int LPB = L::LPB, FW = L::FW, K = L::NF >= 2 ? 1 : 2;
  const uint32_t E = full & ~(bl | wh);
  const uint32_t sb = lat_dilate<LPB>(bl) & E, sw = lat_dilate<LPB>(wh) & E;
  uint32_t F[K], Mk[K], Mkr[K];
  if (K == 1) {
    F[0] = sb | (sw << (FW & 31));
    Mk[0] = E | (E << (FW & 31));
  } else {
    F[0] = sb; F[K - 1] = sw;
    Mk[0] = E; Mk[K - 1] = E;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) Mkr[k] = __brev(Mk[k]);
  lat_flood<LPB, K>(F, Mk, Mkr);
  const uint32_t fb = K == 1 ? (F[0] & L::FM) : F[0], fw = K == 1 ? (F[0] >> (FW & 31)) : F[K - 1];
  own_b = bl | (fb & ~fw);
  own_w = wh | (fw & ~fb);
  const uint32_t sum = lat_board_sum<LPB>((uint32_t)__popc(own_b) | ((uint32_t)__popc(own_w) << 16));   // (<= 361 each)
  area_b = sum & 0xFFFFu;
  area_w = sum >> 16;
}

// FILL (gg_playouts_begin): slot s takes job s (an empty, frozen board from s = J on) and the counter is set to
// {min(S, J), J + min(S, J)}.  HARVEST (gg_playouts_advance, after every rollout chunk): see the file's header.
template <int R, bool FULLN, bool FILL>
__global__ __launch_bounds__(kWave) void k_po_harvest(PoArgs a, int N) {
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
        const int64_t root = jid / a.K;
        if (r == 0) {
          const int d = (int)ab - (int)aw;
          const float x = (float)d - a.komi;
          atomicAdd(a.counts + 4 * root + (x > 0.f ? 0 : (x < 0.f ? 1 : 2)), 1);
          if (!(flag & 4u)) atomicAdd(a.counts + 4 * root + 3, 1);
          atomicAdd(reinterpret_cast<unsigned long long *>(a.sums + 2 * root), (unsigned long long)(int64_t)d);
          atomicAdd(reinterpret_cast<unsigned long long *>(a.sums + 2 * root + 1), (unsigned long long)a.plies[s]);
        }
        if (a.own && r < N) {
          int32_t *pb = a.own + (2 * root * N + r) * N, *pw = pb + N * N;
          for (uint32_t m = ob; m; m &= m - 1) atomicAdd(pb + __builtin_ctz(m), 1);
          for (uint32_t m = ow; m; m &= m - 1) atomicAdd(pw + __builtin_ctz(m), 1);
        }
      }
      // the wave's finished boards: one returning atomicAdd takes their job ids (ids from J on: none left; every
      // harvested job pulls exactly one id, so the same word counts the jobs done)
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(reinterpret_cast<unsigned long long *>(a.counter), (unsigned long long)__popcll(lead));
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base), hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
      next = (int64_t)(((uint64_t)hi << 32) | lo) + __popcll(lead & ((1ull << (j * LPB)) - 1ull));
    }
    if (!fin) continue;
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

}  // namespace gg
