/*
 * gymgo_amd_uct_leaves.h - the UCT search of libgymgo_amd.so with several leaves per root and round, chosen under virtual
 * loss: a header of its own beside include/gymgo_amd.h, whose types, error codes (GG_E_*) and conventions it takes over; the
 * tree is that of gg_uct_begin (gymgo_amd.h), with RAVE that of gymgo_amd_amaf.h, with priors that of gymgo_amd_prior.h.  The
 * entry points below are additive: GG_ABI_VERSION and the entry points of the other headers do not change, and every existing
 * call queues what it queued.
 */
#ifndef GYMGO_AMD_UCT_LEAVES_H
#define GYMGO_AMD_UCT_LEAVES_H
#include "gymgo_amd.h"
#include "gymgo_amd_amaf.h"
#include "gymgo_amd_prior.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * THE RULE.  This text is normative: the kernels (gymgo_amd/csrc/gg_uct.h, gg_prior.h) and the host restatement
 * (tests/mc_uct_leaves_expect.py) both implement it.
 *
 * THE TREE.  R roots, T rounds, L >= 1 leaves per root and round.  A tree has C + 1 nodes, C = T L.  Every buffer of
 * gg_uct_begin / gg_uct_select[_rave] / gg_uct_backup[_rave] keeps its layout with C where it has I: boards, child, links, stats,
 * nodes, node_amaf; log_table is double [C + 1], log(t K).  gg_uct_begin and gg_uct_prior_begin are called with I = C.
 * Bounds: C K < 2^31; RAVE: 2 C K < 2^31; with priors the bound of gymgo_amd_prior.h with C for I.
 * One more caller-owned buffer: virt int32 [R][C + 1].  v_x is the number of leaves handed out in the current round whose path
 * goes through node x.  The caller zero-fills it before the search; it is 0 outside a round.
 * Slot j of root r is ROW r L + j of leaf, move, leaf_id, counts, sums and amaf: all of them have R L rows.
 *
 * SELECT (gg_uct_select_leaves[_rave]).  A root's slots j = 0 .. L - 1 run strictly in order.  Each walks from x = 0 and tests, in
 * this order:
 *   1. Collision.  x > 0 and n_x = 0: x was created earlier in this round and has no board yet.  This slot and every later slot
 *      of the root are EMPTY: leaf_id = -1, move = -1, leaf = a copy of the root's board, and nothing is added to any v.  The
 *      test comes before any read of x's board.
 *   2. Ended node.  The game has ended at x: x is the leaf.  An ended node may be taken by several slots of a round.
 *   3. The action of x.  With t_x = n_x / K + v_x clamped to [0, C] and, for a child c, ne_c = n_c + K v_c:
 *        plain  the lowest legal action without a child is expanded; if there is none, the legal action of the largest
 *               U = (2 w_c + d_c) / (2 ne_c) + c sqrt(log_table[t_x] / ne_c), ties to the lowest action;
 *        RAVE   the largest U of gymgo_amd_amaf.h over every legal action, with ne_c for n (0 where there is no child) and
 *               log_table[t_x]; a winner without a child is expanded.
 *      One virtual visit is K playouts lost by the side that chose the child: it enters the denominator and the argument of
 *      the logarithm, never the wins.  With every v = 0 both are the scores of gg_uct_select[_rave] bit for bit: the same two
 *      functions compute them, there is no other float expression.
 *      Expansion and the case without room are gg_uct_select's: y = nodes++, the child entry, the links and zero stats are
 *      written; with nodes = C + 1 already, x is evaluated as it stands, move = -1.  A chosen child is descended into.
 *   4. Hand over.  A slot that found its leaf y adds 1 to v from y up to the root, then writes row r L + j: leaf = the board of
 *      the node the walk stopped at (the new node's parent, or the node itself), move = the expanded action or -1, leaf_id = y.
 *
 * HAND OUT.  gg_batch_play_moves_tracked on the R L rows (T = 1).  With priors, gg_uct_prior_expand_leaves: row r L + j seeds
 * node leaf_id of tree r; rows with move < 0 - the empty ones among them - and leaf ids outside [0, C] are skipped.  Then the
 * playout queue on the R L rows as roots: gg_playouts_begin / _advance* with R L for R (under RAVE with amaf int32 [R L][2][3][N][N]),
 * first_root L for first_root.  Empty rows are evaluated like any other row and ignored by the backup.
 *
 * BACKUP (gg_uct_backup_leaves[_rave]).  The slots of a root in ascending order, empty ones (leaf_id outside [0, C]) skipped.
 * Per slot, gg_uct_backup[_rave]'s work with row r L + j of counts / sums (and amaf): leaf is stored as the board of node leaf_id
 * when move >= 0; K, the wins and the draws are added along the parent chain; totals [R][2] (nullable) += unfinished, plies; RAVE:
 * the fold of gymgo_amd_amaf.h along the path.  On the same chain v -= 1, never below 0.  Afterwards every v is 0.
 *
 * CONSEQUENCES.  L = 1 never collides and grows gg_uct_select's tree exactly.  The root's n grows by K times the non-empty slots of
 * a round.  No walk passes through a node without a board, so the fold reads only boards that were stored.  A select past the
 * capacity writes nothing beyond a tree.
 *
 * PARAMETERS: each call takes its namesake's list with L (after I, which is C here); select and backup also take virt, behind
 * nodes (select) and stats / node_amaf (backup).
 * CHECKS, in this order: GG_E_BADSIZE: N outside [2, 19], R < 0; GG_E_BADARG: C < 1, K < 1, c negative or not finite, L < 1
 * (gg_uct_prior_expand_leaves: C < 1, C = 2^31 - 1, L < 1); GG_E_BADSIZE: C K > 2^31 - 1, R L > 2^63 - 1; RAVE: GG_E_BADSIZE: 2 C K >
 * 2^31 - 1, GG_E_BADARG: rave_equiv not positive and finite, fpu not finite; GG_E_NULLPTR: any pointer but totals NULL, virt
 * included; R = 0 is no work; gg_uct_prior_expand_leaves: GG_E_BADARG: node_amaf not aligned to an int32.
 *
 * Every call queues ONE launch on hip_stream and never synchronises.  One wave owns a tree: no atomics, no LDS in the select and
 * the backup; every index is bounded by the tree (nodes clamped to [1, C + 1], child ids larger than their parent's and below
 * nodes, walks of at most C + 1 steps) and by the R L rows.
 */
int32_t gg_uct_select_leaves(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, double c, const double *log_table,
                             const uint32_t *boards, int32_t *child, int32_t *links, int32_t *stats, int32_t *nodes, int32_t *virt,
                             uint32_t *leaf, int32_t *move, int32_t *leaf_id, void *hip_stream);
int32_t gg_uct_backup_leaves(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, const int32_t *counts, const int64_t *sums,
                             int64_t *totals, uint32_t *boards, const int32_t *links, int32_t *stats, int32_t *virt,
                             const uint32_t *leaf, const int32_t *move, const int32_t *leaf_id, void *hip_stream);
int32_t gg_uct_select_leaves_rave(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, double c, double rave_equiv, double fpu,
                                  const double *log_table, const uint32_t *boards, int32_t *child, int32_t *links, int32_t *stats,
                                  const int32_t *node_amaf, int32_t *nodes, int32_t *virt, uint32_t *leaf, int32_t *move,
                                  int32_t *leaf_id, void *hip_stream);
int32_t gg_uct_backup_leaves_rave(int64_t R, int32_t N, int32_t I, int32_t L, int32_t K, const int32_t *counts, const int64_t *sums,
                                  const int32_t *amaf, int64_t *totals, uint32_t *boards, const int32_t *links, int32_t *stats,
                                  int32_t *node_amaf, int32_t *virt, const uint32_t *leaf, const int32_t *move,
                                  const int32_t *leaf_id, void *hip_stream);
int32_t gg_uct_prior_expand_leaves(int64_t R, int32_t N, int32_t I, int32_t L, const int32_t *weights, const uint32_t *leaf,
                                   const int32_t *move, const int32_t *leaf_id, int32_t *node_amaf, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_UCT_LEAVES_H */
