/*
 * gymgo_amd_prior.h - heuristic priors for the nodes of the RAVE search of libgymgo_amd.so, from the sets of the tactical and the
 * pattern playout policy: a header of its own beside include/gymgo_amd.h, whose types, error codes (GG_E_*) and conventions it
 * takes over; the sets are those of gymgo_amd_tactics.h and gymgo_amd_pattern.h, the tree is that of gymgo_amd_amaf.h.  The entry
 * points below are additive: GG_ABI_VERSION and the list of entry points of gymgo_amd.h do not change, and every existing call
 * queues what it queued.
 */
#ifndef GYMGO_AMD_PRIOR_H
#define GYMGO_AMD_PRIOR_H
#include "gymgo_amd.h"
#include "gymgo_amd_tactics.h"
#include "gymgo_amd_pattern.h"
#include "gymgo_amd_amaf.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * THE RULE, exact, in integers.
 *
 * Weights.  A prior is six pairs (visits, wins) of int32, in this order: even, capture, escape, pattern, local, eye_fill -
 * `weights`, int32 [12] in DEVICE memory.  The contract is 0 <= wins <= visits for every pair; the library cannot look at device
 * memory before the launch and does not check it.
 *
 * Sets.  For a board with mover m: `valid`, `C`, `E` and `F` are those of gymgo_amd_tactics.h (nothing is valid on a board
 * whose game has ended), `P`, `prev` and `L` those of gymgo_amd_pattern.h - prev from `last`: a point of the board, or no
 * previous point for -1, the pass N^2, any other int32, or last = NULL.  X = valid and not F: the mover's own eyes.
 *
 *   pair(p) = even + [p in C] capture + [p in E] escape + [p in P and valid] pattern + [p in L] local + [p in X] eye_fill
 *             for p in valid, and (0, 0) for every other point.
 *
 * Units.  What is stored or added per point is (visits(p), 2 wins(p)): the units of the (n~, s~) pairs of gymgo_amd_amaf.h, where
 * s~ is twice the wins plus the draws.  The pass has no pair: node_amaf has no slot for it, its value in the select stays q or
 * fpu.
 *
 * Bound.  n~ and s~ are int32: a search of I iterations of K playouts with priors needs
 * 2 (I K + the sum of the six visits) < 2^31; the caller sees to it.
 *
 * THE RULE ON ITS OWN.
 *   gg_batch_move_priors           states uint8 [B][6][N][N] -> out int32 [B][N^2][2], every pair STORED
 *   gg_batch_move_priors_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                                  gg_batch_track_states(s) and s (the class rows of a tracked board are not read)
 * last: NULL, or int32 [B], the previous action of every board; any value is allowed, and one that is no point of the board
 * indexes nothing.  out needs the alignment of an int32 only.  Checks, in this order: GG_E_BADSIZE: N outside [2, 19], B < 0;
 * B = 0 is no work; GG_E_NULLPTR: states / tracked, weights or out NULL; GG_E_BADARG: out not aligned to an int32.
 *
 * IN THE TREE.  node_amaf is that of gg_uct_select_rave / gg_uct_backup_rave, int32 [R][I+1][N^2][2], zero-filled by the caller
 * before the search; both calls ADD to it, as the backup does - integer additions commute, so only the select that reads a
 * node's pairs has to come after the call that seeds them.
 *   gg_uct_prior_begin    after gg_uct_begin: node 0 of every tree gets pair() of roots[r] (tracked boards uint32 [R][5N+1]) with
 *                         prev from last_actions[r] (NULL: no root has a previous point).
 *   gg_uct_prior_expand   after the gg_batch_play_moves_tracked of an iteration: for every root with move[r] >= 0 and leaf_id[r]
 *                         in [0, I], leaf[r] is the board of the new node leaf_id[r] and move[r] its previous action (the pass
 *                         N^2: no previous point); that node gets pair().  Every other root is skipped.
 * Checks, in this order: GG_E_BADSIZE: N outside [2, 19], R < 0; GG_E_BADARG: I < 1 or I = 2^31 - 1; GG_E_NULLPTR: roots / leaf,
 * weights, move, leaf_id or node_amaf NULL (last_actions may be); R = 0 is no work; GG_E_BADARG: node_amaf not aligned to an int32.
 *
 * Every call queues ONE launch on hip_stream and never synchronises; no flood but the one that counts liberties, no atomics;
 * every store lies inside out / the rows of node_amaf it names, the inputs - weights included - are only read.
 */
int32_t gg_batch_move_priors(const uint8_t *states, const int32_t *last, const int32_t *weights, int32_t *out, int64_t B, int32_t N,
                             void *hip_stream);
int32_t gg_batch_move_priors_tracked(const uint32_t *tracked, const int32_t *last, const int32_t *weights, int32_t *out, int64_t B,
                                     int32_t N, void *hip_stream);
int32_t gg_uct_prior_begin(const uint32_t *roots, const int32_t *last_actions, int64_t R, int32_t N, int32_t I, const int32_t *weights,
                           int32_t *node_amaf, void *hip_stream);
int32_t gg_uct_prior_expand(int64_t R, int32_t N, int32_t I, const int32_t *weights, const uint32_t *leaf, const int32_t *move,
                            const int32_t *leaf_id, int32_t *node_amaf, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_PRIOR_H */
