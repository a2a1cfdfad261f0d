/*
 * gymgo_amd_amaf.h - all-moves-as-first (AMAF) statistics of the Monte Carlo playouts of libgymgo_amd.so and RAVE in its UCT
 * search: a header of its own beside include/gymgo_amd.h, whose types, error codes (GG_E_*), policies and conventions it takes
 * over (GG_POLICY_TACTICAL: gymgo_amd_tactics.h).  The entry points below are additive: GG_ABI_VERSION and the list of entry
 * points of gymgo_amd.h do not change, and every existing call queues what it queued.
 */
#ifndef GYMGO_AMD_AMAF_H
#define GYMGO_AMD_AMAF_H
#include "gymgo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * DEFINITIONS.
 * - The FIRST-PLAY MAP of a move sequence gives point p the colour of the first move of the sequence played at p, if any.
 *   Passes give nothing.  A later play at p gives nothing, whatever became of the first stone: a point that is captured and
 *   played again, by either colour, stays with the colour that played it first.
 * - Colours: 0 black, 1 white.  The colour of ply i of a playout is the starting colour (flag bit 0 of its root), flipped for
 *   every earlier ply, passes included.
 *
 * THE MOVE LOG.  gg_batch_rollout_tracked_log is gg_batch_rollout_tracked_policy2 with auto_reset = 0 and policy 0 / 1 / 2:
 * tracked, rng, last_actions and steps_done end bit for bit as that call leaves them.  log is uint16 [B][plies]: entry [b][t] is
 * the action board b played at ply t of THIS launch - a point 0 .. N^2 - 1, or N^2 for the pass.  Board b writes exactly the
 * entries t < the number of plies it played in this launch (its live plies are a prefix of the launch); every other entry keeps
 * the caller's bytes, a board whose game has ended writes nothing.  Checks, in this order: GG_E_BADARG: plies outside
 * [0, 4096], policy outside [0, 2]; then the size and pointer checks of gg_batch_rollout_tracked (B = 0 and plies = 0 are no
 * work); GG_E_NULLPTR: rng or log NULL.  One launch on hip_stream, never synchronises.  The kernels are the log variants of the
 * two families gg_batch_rollout_tracked_policy2 runs on, chosen as that call chooses for policies 1 and 2; the band the uniform
 * path gives to the sixteen-board kernel goes to the one-row-per-lane kernel.
 *
 * THE QUEUE.  gg_playouts_advance_amaf takes the parameters of gg_playouts_advance_policy2 (after gg_playouts_begin with the
 * same buffers) plus four caller-owned buffers:
 *   log    uint16 [S][chunk_plies]   the move log of the last chunk
 *   first  uint32 [S][2][N]          the rows of the points black / white played first in the slot's current job; zero-filled
 *                                    by the caller after gg_playouts_begin, opaque afterwards
 *   mark   int64  [S]                the slot's ply count at the last harvest; zero-filled likewise
 *   amaf   int32  [R][2][3][N][N]    the output, ADDED to: the caller zeroes it before the first advance call of a run
 * amaf[r][c][0][p] is the number of playouts of root r whose first-play map gives p to colour c; amaf[r][c][1][p] and
 * amaf[r][c][2][p] count how many of those the harvest scored as a black / a white win (draws are the remainder).  Every
 * playout counts, with the outcome that goes into counts, those cut off by max_plies included.  The chunks are launches of the
 * log variants; every harvest folds the new log entries of every live slot into its rows of `first`, a finished slot adds one
 * vector atomic per set bit to amaf, and a refilled or emptied slot starts from zero rows.  chunk_plies divides max_plies, so a
 * job starts on a chunk boundary and the log index is the ply's index in the launch.  Results do not depend on S or
 * chunk_plies.  Checks: those of gg_playouts_advance_policy2 in its order, then GG_E_BADARG: chunk_plies > 4096, then
 * GG_E_NULLPTR: log, first, mark or amaf NULL.
 *
 * RAVE.  gg_uct_select_rave / gg_uct_backup_rave take the buffers of gg_uct_select / gg_uct_backup (after gg_uct_begin) plus
 *   node_amaf  int32 [R][I+1][N^2][2]   zero-filled by the caller before the search
 *   amaf       int32 [R][2][3][N][N]    the iteration's output of gg_playouts_advance_amaf, zeroed before its playouts
 * For node x with mover m, node_amaf[x][p] = (n~, s~): the simulations through x in which m played p first after x, and twice
 * m's wins plus the draws among them.
 * SELECT.  At node x, for every legal action a: n, w, d from the child's stats (n = 0 without a child), s = 2 w + d for x's
 * mover; n~, s~ from node_amaf (0 for the pass).  In float64, each operation rounded to nearest in the order written, no
 * contraction: q = s / (2 n), q~ = s~ / (2 n~), beta = n~ / (n + n~ + (n n~) / rave_equiv); the value v is
 * (1 - beta) q + beta q~ when both counts are positive, q or q~ when one is, fpu when neither; U = v + c sqrt(L[n_x / K] / n)
 * when n > 0, else U = v.  The largest U wins, ties to the lowest action.  A winner without a child is expanded into node
 * nodes[r]++ (its node_amaf rows stay zero); with no room left x is evaluated as it is; an ended node is the leaf - both as in
 * gg_uct_select.  Checks: gg_uct_select's, with GG_E_BADSIZE also for 2 I K >= 2^31 and GG_E_BADARG unless rave_equiv > 0 and
 * finite and fpu finite; GG_E_NULLPTR: node_amaf NULL.
 * BACKUP.  The stats go up the parent chain as in gg_uct_backup.  With x_0 = root .. x_d = leaf the path, m_j the action of x_j:
 * for every i in 0 .. d, c the mover of x_i, S = 2 (c's wins) + draws of `counts`, T_i the points among m_(i+1) .. m_d:
 *   p in T_i whose first occurrence m_j was played by c (j - i odd):  node_amaf[x_i][p] += (K, S)
 *   p not in T_i:  node_amaf[x_i][p] += (amaf[r][c][0][p], 2 amaf[r][c][1 + c][p] + amaf[r][c][0][p] - amaf[r][c][1][p]
 *                                                          - amaf[r][c][2][p])
 * - the first-play map of "the tree moves below x_i, then the playout", in integers.  Checks: gg_uct_backup's, GG_E_BADSIZE also
 * for 2 I K >= 2^31, GG_E_NULLPTR: amaf or node_amaf NULL.  One launch each, one wave per root, no atomics.
 */
int32_t gg_batch_rollout_tracked_log(uint32_t *tracked, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B,
                                     int32_t N, int32_t plies, int32_t policy, uint16_t *log, void *hip_stream);
int32_t gg_playouts_advance_amaf(const uint32_t *roots, int64_t R, int32_t N, int32_t K, int64_t first_root, uint64_t base_seed,
                                 int32_t max_plies, int32_t chunk_plies, float komi, int32_t chunks, int32_t policy,
                                 uint32_t *slots, uint64_t *rng, int64_t *plies, int64_t *job, int64_t S, int64_t *counter,
                                 int32_t *counts, int64_t *sums, int32_t *ownership, uint16_t *log, uint32_t *first,
                                 int64_t *mark, int32_t *amaf, void *hip_stream);
int32_t gg_uct_select_rave(int64_t R, int32_t N, int32_t I, int32_t K, double c, double rave_equiv, double fpu,
                           const double *log_table, const uint32_t *boards, int32_t *child, int32_t *links, int32_t *stats,
                           const int32_t *node_amaf, int32_t *nodes, uint32_t *leaf, int32_t *move, int32_t *leaf_id,
                           void *hip_stream);
int32_t gg_uct_backup_rave(int64_t R, int32_t N, int32_t I, int32_t K, const int32_t *counts, const int64_t *sums,
                           const int32_t *amaf, int64_t *totals, uint32_t *boards, const int32_t *links, int32_t *stats,
                           int32_t *node_amaf, const uint32_t *leaf, const int32_t *move, const int32_t *leaf_id,
                           void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_AMAF_H */
