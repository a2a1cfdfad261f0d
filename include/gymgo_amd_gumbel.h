/*
 * gymgo_amd_gumbel.h - the Gumbel root rule of the PUCT search of libgymgo_amd.so: the C ABI of the Gumbel family, a header of
 * its own beside include/gymgo_amd.h, whose types (gg_puct_stat), error codes (GG_E_*) and conventions it takes over.  The
 * entry points below are additive: GG_ABI_VERSION and the list of entry points of gymgo_amd.h do not change.
 */
#ifndef GYMGO_AMD_GUMBEL_H
#define GYMGO_AMD_GUMBEL_H
#include "gymgo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Gumbel root search by sequential halving: "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR
 * 2022) at node 0 of the trees of gg_puct_select_leaves / gg_puct_backup_leaves.  The tree, its buffers, legality, s (+1 if
 * black is to move at node 0, else -1), the stat record {w, n, v} and the slot / collision rules are those of
 * gg_puct_select_leaves in include/gymgo_amd.h; L = 1 is allowed and is the one-leaf search.  gg_puct_begin,
 * gg_puct_backup_leaves, gg_puct_legal, gg_puct_advance and every plane launch are used with it unchanged.  A = N * N + 1.
 *
 * Per search, caller-owned, on the device:
 *   base  float32 [R][A]   g(a) + logit(a), the caller's.  A NaN counts as -infinity.  Entries of illegal actions are never read.
 *   seen  int32 [R][A]     the visits n of node 0's child under a when the search of this move began, 0 without a child.
 *   done  int32 [R]        the simulations of this move handed out through the root rule.
 *   seq   int32 [S]        the schedule.
 * and the scalars c_visit, c_scale: float64, finite, >= 0.
 *
 * THE SCHEDULE seq(m, n), m >= 1 considered actions and n >= 1 simulations, in integers only (gg_gumbel_sequence, host memory,
 * no device work): m = 1: seq[t] = t.  Otherwise lg = ceil(log2 m), k = m, v[0 .. m-1] = 0, and while fewer than n entries
 * exist:  1. e = max(1, floor(n / (lg k)));  2. e times: append v[0 .. k-1], then v[i] += 1 for i < k;  3. k = max(2, floor(k / 2)).
 * Truncated to n entries.  seq(4, 8) = 0,0,0,0,1,1,2,2;  seq(16, 32) = sixteen 0s, eight 1s, four 2s, four 3s;
 * seq(3, 7) = 0,0,0,1,1,2,2;  seq(2, 4) = 0,0,1,1;  seq(16, 16) = sixteen 0s.  Entry t says how many of this move's simulations
 * the action that gets simulation t must have had: with distinct base values the m largest get one each, then the better
 * half of them one more each, and so on.
 *
 * THE ROOT RULE replaces step d of gg_puct_select_leaves at node 0 only, when node 0 is evaluated (n_0 > 0) and its game has
 * not ended; steps a to c come first, unchanged.  For every legal action a let n_c, w_c, v_c be the record of the child under a
 * (all three 0 without a child, negatives clamped to 0 as in the select).  Then
 *   k_a  = max(0, n_c + v_c - seen[r][a])      this move's simulations of a, the ones in flight included
 *   maxn = the largest n_c over the legal actions (real visits only, those from before this move included)
 *   q0   = s * w_0 / n_0                       a float64 division
 *   qh_a = n_c > 0 ? s * w_c / n_c : q0        virtual visits do not enter
 *   m1 = c_visit + (double)maxn;  m2 = m1 * c_scale;  sigma_a = m2 * qh_a;  G_a = (double)base[r][a] + sigma_a
 * each operation a float64 operation rounded to nearest, in this order, no fused multiply-add; a NaN G counts as -infinity.
 * The slot then chooses: t = done[r]; need = seq[t] if 0 <= t < S, else none.  E = {legal a : k_a = need}; if E is empty or
 * need is none, E = {legal a : k_a = kmax}, kmax the largest k_a.  a* = the action of E with the largest G_a, ties to the
 * lowest action (also when every G is -infinity).  From a* the walk goes on exactly as after step d: descend, or expand, or
 * the no-room rule; every node below the root keeps U'.  When a slot in which the root rule chose ends non-empty,
 * done[r] = t + 1.  A collision leaves done, v and everything else as gg_puct_select_leaves says; a slot that stops at node 0
 * itself (round 0 of a fresh root, an ended root) is not a simulation of this count.
 *
 * THE READ-OUT (gg_gumbel_root) is defined outside a round, when every v = 0 (none is read).  A root whose game has ended:
 * actions[r] = -1, the q row +0, the visits row 0, value[r] = +0.  Otherwise k_a, maxn, qh_a and G_a are as above with v = 0
 * and q0 = 0.0 when n_0 = 0;  actions[r] = the legal a with k_a = kmax and the largest G_a, ties to the lowest action;
 * q[r][a] = (float)qh_a on legal actions, +0 elsewhere;  visits[r][a] = n_c on legal actions, 0 elsewhere;
 * value[r] = (float)q0.  The improved policy softmax(logit + sigma(completed q)) is the caller's to make from q and visits (a
 * float sum would depend on its order; gymgo_amd.gogame.PuctSearch.gumbel_root does it in torch).
 *
 *   gg_gumbel_sequence        writes seq(m, n) to seq int32 [n] in HOST memory.  GG_E_BADARG: m < 1 or n < 1; GG_E_NULLPTR.
 *   gg_gumbel_begin           seen[r][a] = n of node 0's child under a (0 without a child; every a, legal or not), done[r] = 0.
 *                             Outside a round: at the start of every move's search, after gg_puct_begin or gg_puct_advance.
 *   gg_gumbel_select_leaves   gg_puct_select_leaves with the root rule: same buffers, same outputs, done updated.
 *   gg_gumbel_root            the read-out.  q, visits and value may be NULL.
 *
 * Checks, all before any device work, in this order: GG_E_BADSIZE for N outside [2, GG_MAX_BOARD] or R < 0; GG_E_BADARG for
 * C < 1, C = 2^31 - 1, c negative or not finite, L < 1, L > C, S < 1, c_visit or c_scale negative or not finite (each where
 * the entry point has that parameter); R = 0 returns 0; GG_E_NULLPTR for a NULL pointer other than q, visits, value;
 * GG_E_BADARG for stats not on a 16-byte boundary (a record is read as one 16-byte access).  Every call but
 * gg_gumbel_sequence queues ONE launch on hip_stream and never synchronises; one wave per root, no atomics, vector stores
 * only, every index bounded by the tree; root r's results depend on root r alone.
 */
int32_t gg_gumbel_sequence(int32_t m, int32_t n, int32_t *seq);
int32_t gg_gumbel_begin(int64_t R, int32_t N, int32_t C, const int32_t *child, const gg_puct_stat *stats, const int32_t *nodes,
                        int32_t *seen, int32_t *done, void *hip_stream);
int32_t gg_gumbel_select_leaves(int64_t R, int32_t N, int32_t C, int32_t L, double c, const uint32_t *boards, int32_t *child,
                                const float *prior, int32_t *links, gg_puct_stat *stats, int32_t *nodes, const float *base,
                                const int32_t *seen, int32_t *done, const int32_t *seq, int32_t S, double c_visit, double c_scale,
                                uint32_t *leaf, int32_t *move, int32_t *leaf_id, void *hip_stream);
int32_t gg_gumbel_root(int64_t R, int32_t N, int32_t C, const uint32_t *boards, const int32_t *child, const gg_puct_stat *stats,
                       const int32_t *nodes, const float *base, const int32_t *seen, double c_visit, double c_scale,
                       int32_t *actions, float *q, int32_t *visits, float *value, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_GUMBEL_H */
