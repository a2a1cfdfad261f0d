// gg_ladder.h - LADDER PLANES (gg_batch_ladder, gg_batch_ladder_tracked of include/gymgo_amd.h): the chains a
// ladder captures, the ataris that work and the moves that escape, by a BOUNDED SEARCH per board on the device.
//
// Layout: gg_feat.h's - ONE ROW PER LANE, a board is the 16 lanes of a DPP row (R <= 13, four boards per wave) or 32 lanes
// (R = 19, two boards per wave), rows are bit masks in registers, one single-wave workgroup per wave of boards.
//
// The definition (the header; tests/ladder_expect.py) is a minimax over two kinds of nodes - D: the defender moves, the prey
// has one liberty; A: the attacker moves, the prey has two - with a budget of 4 N plies and 16 N nodes per root query.  Here
// every board walks it as a STATE MACHINE stepped by one wave-wide loop; the control state (depth, node count, the last
// option tried, the ko point, what a child returned) is the same in all lanes of a board, the boards of a wave are wherever
// their own search is, a board that is done idles.  A ROUND, for every board that has work:
//   0. a board whose node has returned takes the last move back (the record below) and hands the value to the parent - until
//      the parent goes on with its next option, or the root has its answer;
//   1. a board between two chains seeds the next chain with one or two liberties (feat_groups has filed them);
//   2. the prey is flooded from its seed stone and its liberties are dilate & empty;
//   3. the node's next option after the last one tried, in the definition's order: A - the prey's two liberties; D - the
//      prey's liberty, then the liberties of the attacker's chains in atari next to the prey (each flooded and counted,
//      seed-and-flood over the prey's neighbours), row-major;
//   4. the option is played: the stone's own chain and the opponent's chains at its four neighbours are flooded in
//      lock-step (five floods, one register each), the opponent's without a liberty leave, the own chain's liberties, the
//      number of captured stones and the chain's size - three 6-bit fields of one board sum - give legality and the next ko
//      point, the prey's liberties after the move the outcome;
//   5. decide: the option fails (the node stays, the move is dropped: the position is only committed on a descent), it
//      escapes (D returns), or the search descends - the record is pushed, or, past either bound, the query is aborted: the
//      root position comes back from registers and the query gets its conservative answer.
// The root of a query is a node of depth 0 of the same kind (A for a two-liberty chain, D for a one-liberty chain) that
// tries EVERY option, files each answer in the planes and starts each with a fresh budget.
//
// TAKE-BACK: one 32-bit word per lane and level in LDS - the captured stones of the lane's row (bits 0 - 18), the played
// point (column in bits 19 - 23, bit 24 in the lane of its row) and the ko point before the move (bits 25 - 29, bit 30).
// A lane reads and writes its own words only: 4 N levels x 64 lanes x 4 B = 19 KB at 19x19, half of what the two colour
// rows per level take, and it is LDS per wave that bounds the waves per compute unit here.
// Every loop is bounded by construction: a round tries an option (a node has at most 1 + the number of attacker chains
// options and a query at most 16 N nodes), pops a level (at most 4 N) or takes a chain off the board's list.
// EMISSION: k_life's (plane_emit of gg_planes.h) - an LDS bit-string per wave, aligned 16-byte vectors inside the wave's slice, single elements at the
// ragged ends, nothing outside the slice.
#pragma once
#include "gg_feat.h"

namespace gg {

constexpr int kLadderPlanes = 4;

template <int R>
struct Ladder {
  using F_ = Feat<R>;
  static constexpr int LPB = F_::LPB, NBW = F_::NBW;
  static constexpr int kLevels = 4 * R;                                             // GG_LADDER_DEPTH(R): one record per ply
  static constexpr int kBsWords = plane_bs_words<R>(kLadderPlanes, 15);
  static constexpr int kIoWords = kBsWords > F_::kIoWords ? kBsWords : F_::kIoWords;  // (the staged input is dead by then)
  static constexpr int kLdsWords = kIoWords + kLevels * kWave;
  // THE ROUNDS OF A BOARD.  In every round a board that has work takes a chain off its list, tries one option or finds its
  // node spent.  A query enters at most 16 N nodes, every other one a D node; an A node tries two options and is spent once,
  // a D node tries the prey's liberty and at most N^2 / 2 capturing points (each needs an attacker chain and an empty point
  // of its own) and is spent once: at most (8 N + 1) (N^2 / 2 + 5) rounds below the root.  A board has at most N^2 chains;
  // a two-liberty chain has two queries, a one-liberty chain one and one per attacker chain next to it, and a planar
  // adjacency has at most three pairs per chain: at most 5 N^2 queries, and two more rounds per chain (fetched, spent).
  // 5 N^2 ((8 N + 1) (N^2 / 2 + 5) + 1) + 2 N^2 + 1 grows with N and at N = R is 1.35 M, 7.9 M and 51.2 M against
  // 32 R^5 = 1.89 M, 11.9 M and 79.2 M, so the loop's bound is not reached; a board that did reach it would report 255
  // aborted queries next to its incomplete planes.
  static constexpr int kRounds = 32 * R * R * R * R * R;
};

// the lowest point (row-major) of a row set of the board: the lowest bit of the first lane that holds one, zero elsewhere
template <int LPB> __device__ __forceinline__ uint32_t lad_first(uint32_t x) {
  const uint32_t incl = lat_board_scan<LPB>(x ? 1u : 0u);
  return (x != 0u && incl == 1u) ? (x & (0u - x)) : 0u;
}
// the points after the point p (one bit on the board, or none: then nothing) in row-major order
template <int LPB> __device__ __forceinline__ uint32_t lad_after(uint32_t p) {
  const uint32_t incl = lat_board_scan<LPB>(p ? 1u : 0u);
  return p ? ~(p | (p - 1u)) : (incl ? 0xFFFFFFFFu : 0u);
}
// one row set flooded through the mask m
template <int LPB> __device__ __forceinline__ uint32_t lad_flood(uint32_t seed, uint32_t m) {
  uint32_t F[1] = {seed}, Mk[1] = {m}, Mkr[1] = {__brev(m)};
  lat_flood<LPB, 1>(F, Mk, Mkr);
  return F[0];
}
__device__ __forceinline__ uint32_t lad_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// the take-back record of a lane: captured row, played point, ko point before
__device__ __forceinline__ uint32_t lad_pack(uint32_t cap, uint32_t q, uint32_t ko) {
  uint32_t w = cap;
  if (q) w |= (1u << 24) | ((uint32_t)(__ffs((int)q) - 1) << 19);
  if (ko) w |= (1u << 30) | ((uint32_t)(__ffs((int)ko) - 1) << 25);
  return w;
}

// gg_batch_ladder / gg_batch_ladder_tracked: out [B][4][N][N] of elements of 1 << esh bytes (`one`: the bit pattern of 1),
// aligned to its element; aborted uint8 [B] or null; orient int32 [B] or null (feat_orient on the loaded rows: the planes of
// the turned position).  One single-wave workgroup per NBW boards (grid-stride).
template <int R, bool TRACKED>
__global__ __launch_bounds__(kWave) void k_ladder(const void *__restrict__ in, const int32_t *__restrict__ orient,
                                                  uint8_t *__restrict__ out, uint8_t *__restrict__ aborted, int esh, uint32_t one,
                                                  int64_t B, int N) {
  using L_ = Ladder<R>;
  constexpr int LPB = L_::LPB;
  __shared__ __attribute__((aligned(16))) uint32_t lds[L_::kLdsWords];
  uint32_t *stack = lds + L_::kIoWords;
  PlaneFrame<R> f(N);
  const int lane = f.lane;
  const uint32_t full = f.full;
  const int max_depth = GG_LADDER_DEPTH(N), max_nodes = GG_LADDER_NODES(N);
  for (int64_t g = blockIdx.x; g < f.groups(B); g += gridDim.x) {
    f.at(g, B);
    uint32_t bl0, wh0, inv, fl;
    plane_load<R, TRACKED>(in, orient, f, B, N, lds, bl0, wh0, inv, fl);
    const bool white = (fl & 1u) != 0, over = (fl & 4u) != 0;
    uint32_t remq, ko0;
    {
      uint32_t cls[4];
      feat_groups<R, false>(bl0, wh0, full, cls);
      remq = cls[0] | cls[1];                                           // the chains with one or two liberties, either colour
      const uint32_t E0 = full & ~(bl0 | wh0);
      ko0 = over ? 0u : (E0 & inv & lat_dilate<LPB>((white ? bl0 : wh0) & cls[0]));   // plane 11 of the feature planes
    }
    // ---- the search: rows
    uint32_t bl = bl0, wh = wh0, ko = 0, rootko = 0, seed = 0, last = 0, rlast = 0;
    uint32_t lad = 0, p2 = 0, p3 = 0;
    // ---- the search: control, the same in every lane of a board
    int st = 0;                   // 0: between chains, 1: at a node, 2: done
    bool defw = false;            // the defender is white
    int kind = 1;                 // liberties of the root chain: 1 (the root is a D node) or 2 (an A node)
    int d = 0, nodes = 0;
    bool anyres = false;          // some work(c, Li) / some esc(c, o) of the chain
    bool pend = false, pv = false;   // the node has returned pv (captured) and has not been popped
    uint32_t nab = 0;
#pragma unroll 1
    for (int round = 0; round < L_::kRounds; ++round) {
      if (__ballot(st != 2) == 0ull) break;
      // a root answer of the current chain: good = work / esc of the option rlast
#define GG_LAD_FILE(COND, GOOD)                                                                 \
      {                                                                                         \
        const bool c_ = (COND), g_ = c_ && (GOOD);                                              \
        anyres = anyres || g_;                                                                  \
        if (g_ && kind == 2 && defw != white) p2 |= rlast;                                      \
        if (g_ && kind == 1 && defw == white) p3 |= rlast;                                      \
        if (c_) nodes = 0;                                                                      \
      }
      // 0. returns: take the move back, the parent reacts
#pragma unroll 1
      for (int it = 0; it < L_::kLevels; ++it) {
        if (__ballot(pend) == 0ull) break;
        const int lv = d > 0 ? d - 1 : 0;
        const uint32_t rec = stack[lv * kWave + lane];
        const bool parent_d = ((lv & 1) == 0) == (kind == 1);
        const bool mover_w = parent_d ? defw : !defw;
        const uint32_t Q = pend && (rec & (1u << 24)) ? 1u << ((rec >> 19) & 31u) : 0u;
        const uint32_t cap = pend ? rec & 0x7FFFFu : 0u;
        const uint32_t kob = (rec & (1u << 30)) ? 1u << ((rec >> 25) & 31u) : 0u;
        if (mover_w) { wh &= ~Q; bl |= cap; }
        else { bl &= ~Q; wh |= cap; }
        if (pend) {
          d = lv;
          last = Q;
          ko = lv == 0 ? rootko : kob;
        }
        const bool at_root = pend && lv == 0;
        GG_LAD_FILE(at_root, kind == 2 ? pv : !pv)
        const bool goes_on = pv == parent_d;    // A after a D that escaped, D after an A that captured: the next option
        if (pend && !at_root && !goes_on) pv = !parent_d;
        else pend = false;
      }
      // 1. the next chain
      const bool fetch = st == 0;
      const uint32_t s0 = lad_first<LPB>(fetch ? remq : 0u);
      const uint32_t sflags = lat_board_sum<LPB>((s0 ? 1u : 0u) | ((s0 & wh0) ? 64u : 0u));
      const bool fetched = fetch && (sflags & 63u) != 0u;
      if (fetch) {
        seed = s0;
        defw = (sflags >> 6) != 0u;
        st = fetched ? 1 : 2;
        d = 0; nodes = 0; anyres = false; last = 0; rlast = 0;
      }
      const bool node = st == 1;
      // 2. the prey and its liberties
      const uint32_t def = defw ? wh : bl, att = defw ? bl : wh;
      const uint32_t E = full & ~(bl | wh);
      const uint32_t Pr = lad_flood<LPB>(node ? seed : 0u, def);
      const uint32_t libs = lat_dilate<LPB>(Pr) & E;
      if (__ballot(fetched) != 0ull) {
        const uint32_t nl = lat_board_sum<LPB>(lad_min((uint32_t)__popc(libs), 3u));
        if (fetched) {
          kind = nl == 1u ? 1 : 2;
          remq &= ~Pr;
          const bool first_w = kind == 2 ? !defw : defw;
          rootko = first_w == white ? ko0 : 0u;
          ko = rootko;
        }
      }
      const bool is_d = ((d & 1) == 0) == (kind == 1);
      // 3. the next option
      const uint32_t lflags = lat_board_sum<LPB>((last ? 1u : 0u) | ((last & libs) ? 64u : 0u));
      const bool any_last = (lflags & 63u) != 0u, last_is_l = (lflags >> 6) != 0u;
      uint32_t caps = 0;
      {
        uint32_t rem = node && is_d && any_last ? lat_dilate<LPB>(Pr) & att : 0u;
#pragma unroll 1
        for (int it = 0; it < 2 * R * R; ++it) {   // (a round takes a chain off every board that still has one)
          if (__ballot(rem != 0u) == 0ull) break;
          const uint32_t G = lad_flood<LPB>(lad_first<LPB>(rem), att);
          const uint32_t lb = lat_dilate<LPB>(G) & E;
          const uint32_t n = lat_board_sum<LPB>(lad_min((uint32_t)__popc(lb), 2u));
          if (n == 1u) caps |= lb;
          rem &= ~G;
        }
      }
      const uint32_t after = lad_after<LPB>(last);
      const uint32_t cand_d = any_last ? (caps & ~libs & (last_is_l ? 0xFFFFFFFFu : after)) : libs;
      const uint32_t cand_a = any_last ? (libs & after) : libs;
      const uint32_t Q = lad_first<LPB>(node ? (is_d ? cand_d : cand_a) : 0u);
      // 4. the move
      const bool mover_w = is_d ? defw : !defw;
      const uint32_t me = mover_w ? wh : bl, op = mover_w ? bl : wh;
      const uint32_t me1 = me | Q;
      uint32_t F[5] = {lat_below<LPB>(Q) & op, lat_above<LPB>(Q) & op, (Q >> 1) & op, shl1(Q) & op, Q};
      {
        const uint32_t opr = __brev(op);
        const uint32_t Mk[5] = {op, op, op, op, me1}, Mkr[5] = {opr, opr, opr, opr, __brev(me1)};
        lat_flood<LPB, 5>(F, Mk, Mkr);
      }
      const uint32_t E1 = full & ~(me1 | op);
      uint32_t w1 = (Q ? 1u << 24 : 0u) | ((Q & ko) ? 1u << 26 : 0u);   // (one lane holds Q: one bit each)
#pragma unroll
      for (int k = 0; k < 4; ++k) w1 |= (lat_dilate<LPB>(F[k]) & E1) ? 1u << (6 * k) : 0u;
      const uint32_t S1 = lat_board_sum<LPB>(w1);
      const bool has_q = ((S1 >> 24) & 1u) != 0u, on_ko = ((S1 >> 26) & 1u) != 0u;
      uint32_t C = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) C |= ((S1 >> (6 * k)) & 63u) == 0u ? F[k] : 0u;
      const uint32_t G = F[4], EG = E1 | C;
      const uint32_t S2 = lat_board_sum<LPB>(lad_min((uint32_t)__popc(lat_dilate<LPB>(G) & EG), 3u) |
                                             (lad_min((uint32_t)__popc(C), 2u) << 7) | (lad_min((uint32_t)__popc(G), 2u) << 14) |
                                             ((G & Pr) ? 1u << 21 : 0u));
      const uint32_t own_libs = S2 & 127u, ncap = (S2 >> 7) & 127u, gsz = (S2 >> 14) & 127u;
      const bool touches = (S2 >> 21) != 0u;
      const bool legal = has_q && !on_ko && own_libs != 0u;
      const uint32_t ko_next = (ncap == 1u && gsz == 1u && own_libs == 1u) ? C : 0u;
      // the prey after a defender's move: merged with the stone's chain, or the same stones with the captured points free
      const uint32_t Pn = touches ? G : Pr;
      const uint32_t n = lat_board_sum<LPB>(lad_min((uint32_t)__popc(lat_dilate<LPB>(Pn) & EG), 3u));
      // 5. decide
      const bool tried = node && has_q, spent = node && !has_q;
      const bool escapes = tried && is_d && legal && n >= 3u;
      const bool descend = tried && legal && (!is_d || n == 2u);
      const bool abort_q = descend && (d + 1 > max_depth || nodes + 1 > max_nodes);
      const bool push = descend && !abort_q;
      const bool fails = tried && !escapes && !descend;
      if (tried && d == 0) rlast = Q;
      // the record of the level (a lane's own word); an index past the stack is an aborted query's: not written
      if (push) stack[d * kWave + lane] = lad_pack(C, Q, d == 0 ? 0u : ko);
      if (push) {
        if (mover_w) { wh = me1; bl = op & ~C; }
        else { bl = me1; wh = op & ~C; }
        ko = ko_next;
        d += 1;
        nodes += 1;
        last = 0;
      }
      if (abort_q) {
        bl = bl0; wh = wh0;
        d = 0;
        ko = rootko;
        last = rlast;
        nab = lad_min(nab + 1u, 255u);
      }
      GG_LAD_FILE(abort_q, kind == 1)                                   // "not captured" / "escapes"
      const bool root_now = (escapes || fails) && d == 0 && !abort_q;   // an answer without a search below it
      GG_LAD_FILE(root_now, kind == 1 && escapes)
      if (escapes || fails) last = Q;
      if (escapes && d > 0) { pend = true; pv = false; }                // D returns "not captured"
      if (spent) {
        if (d == 0) {   // the chain has its answers
          const bool laddered = kind == 2 ? anyres : !anyres;
          if (laddered) lad |= Pr;
          st = 0;
        } else {        // D without an escape is captured, A without a working atari is not
          pend = true;
          pv = is_d;
        }
      }
#undef GG_LAD_FILE
    }
    if (st != 2) nab = 255u;   // out of rounds (Ladder<R>::kRounds: not reached): say so
    if (aborted && f.on && f.r == 0) aborted[f.b_first + f.j] = (uint8_t)nab;
    const uint32_t own0 = white ? wh0 : bl0, opp0 = white ? bl0 : wh0;
    const uint32_t rows[kLadderPlanes] = {lad & own0, lad & opp0, over ? 0u : p2, over ? 0u : p3};
    WAVE_SYNC();   // (the stack's last reads before the string is zeroed)
    plane_emit<R, kLadderPlanes>(out, esh, one, rows, lds, f, N);
  }
}

}  // namespace gg
