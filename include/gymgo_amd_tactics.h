/*
 * gymgo_amd_tactics.h - the capture- and atari-aware playout policy of libgymgo_amd.so and its plane family: a header of its
 * own beside include/gymgo_amd.h, whose types, error codes (GG_E_*), dtype codes (GG_W_*, GG_FEAT_U8), policies
 * (GG_POLICY_UNIFORM, GG_POLICY_NO_EYE_FILL) and conventions it takes over.  The entry points below are additive:
 * GG_ABI_VERSION and the list of entry points of gymgo_amd.h do not change, and the three _policy entry points of gymgo_amd.h
 * keep answering GG_E_BADARG for anything but their two policies.
 */
#ifndef GYMGO_AMD_TACTICS_H
#define GYMGO_AMD_TACTICS_H
#include "gymgo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * THE RULE.  GG_POLICY_TACTICAL = 2.  The rule applies to a live board, from the mover's view.
 *
 * Definitions:
 * - `low` = the stones of either colour whose group has fewer than two liberties.  Groups and liberties are as in
 *   gg_batch_group_liberties.  This is the complement, within the stones, of the class rows a tracked board carries.
 * - `valid` = points whose invalid bit is clear.  `eye` is as in GG_POLICY_NO_EYE_FILL.
 * - `C` (capture points) = valid points orthogonally next to an opponent stone in `low`.  Such a point is that group's last
 *   liberty, so the move captures.  The ko point is not valid, so it is not in `C`.
 * - `E` (escape points) = valid points orthogonally next to a mover's stone in `low`, with at least two empty orthogonal
 *   neighbours on the board.  The chain the move makes has at least those two liberties.
 * - `F` = the candidates of no_eye_fill: valid and not an eye.
 * - No point of `C` or `E` is an eye of the mover.  An eye has no opponent neighbour and no empty neighbour.  So neither set
 *   needs the eye term.
 *
 * The ply:
 * - It advances the generator exactly once, as the other two policies do.
 * - Let `u` be the high 32 bits of that draw, the word the kernels already keep.
 * - The gate is open when `(u & 3) != 0`.
 * - The set drawn from is `C` if the gate is open and `C` is not empty.  Otherwise it is `E` if the gate is open and `E` is
 *   not empty.  Otherwise it is `F`.
 * - With `n` points in that set, the action is the pass if `n = 0`, which can only happen with `F`.  Otherwise it is the
 *   `floor(u n / 2^32)`-th point of the set in ascending order.
 *
 * Unchanged from GG_POLICY_NO_EYE_FILL:
 * - A board that is reset on this ply plays on the empty board: all three sets come from an empty position.
 * - A finished game without auto-reset draws nothing.
 * - The live-prefix invariant holds, and the generator after a launch is `x0 + played c`.
 * - First moves (gg_move_playouts_*) and the trees keep every legal action.
 *
 * (Without the gate - always capture when a capture exists - playouts fall into take-and-retake cycles, they have no superko:
 * one 19x19 game in four never ended.  With it every game of every size tried ended)
 *
 * The planes: T = gg_tactics_planes() = 3 planes per board, out [B][3][N][N], every element exactly 0 or 1, all zero for a game
 * that has ended:
 *   0  C   1  E   2  F
 *   gg_batch_tactics           states uint8 [B][6][N][N] -> out of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8
 *   gg_batch_tactics_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                              gg_batch_track_states(s) and s (every group is counted from the stones; the class rows of a
 *                              tracked board are not read)
 * orient (NULL, or int32 [B], only orient[b] & 7 is read; gg_batch_symmetry's orientations): the planes are geometric, out[b]
 * is view orient[b] of the unoriented result; the board is turned in registers after the load.
 * Alignment (out needs that of its element only), stores and the checks with their order and codes: gg_batch_life's
 * (GG_E_BADSIZE: N outside [2, 19], B < 0, an unknown dtype; B = 0 is no work; GG_E_NULLPTR: states / tracked or out NULL;
 * GG_E_BADARG: out not aligned to its element).  Every call queues ONE launch on hip_stream and never synchronises; no global
 * atomics; every store lies inside the B rows of out.
 *
 * The policy in the playouts: the three calls below take the parameter lists of their _policy namesakes of gymgo_amd.h and
 * accept policies 0, 1 and 2.  Policies 0 and 1 queue what the namesake queues, launch for launch; every other policy but 2
 * gives GG_E_BADARG; all other checks and their order are the namesake's.
 */
#define GG_POLICY_TACTICAL 2
int32_t gg_tactics_planes(void);
int32_t gg_batch_tactics(const uint8_t *states, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                         void *hip_stream);
int32_t gg_batch_tactics_tracked(const uint32_t *tracked, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                                 void *hip_stream);
int32_t gg_batch_rollout_tracked_policy2(uint32_t *tracked, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B,
                                         int32_t N, int32_t plies, int32_t auto_reset, int32_t policy, void *hip_stream);
int32_t gg_playouts_advance_policy2(const uint32_t *roots, int64_t R, int32_t N, int32_t K, int64_t first_root, uint64_t base_seed,
                                    int32_t max_plies, int32_t chunk_plies, float komi, int32_t chunks, int32_t policy,
                                    uint32_t *slots, uint64_t *rng, int64_t *plies, int64_t *job, int64_t S, int64_t *counter,
                                    int32_t *counts, int64_t *sums, int32_t *ownership, void *hip_stream);
int32_t gg_move_playouts_advance_policy2(const uint32_t *roots, int64_t R, int32_t N, const int32_t *plan, int64_t T, int32_t K,
                                         int64_t first_root, uint64_t base_seed, int32_t max_plies, int32_t chunk_plies,
                                         float komi, int32_t chunks, int32_t policy, uint32_t *slots, uint64_t *rng,
                                         int64_t *plies, int64_t *job, int64_t S, int64_t *counter, int32_t *counts,
                                         int64_t *sums, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_TACTICS_H */
