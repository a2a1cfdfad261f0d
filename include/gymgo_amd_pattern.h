/*
 * gymgo_amd_pattern.h - the 3x3-pattern local-response playout policy of libgymgo_amd.so and its plane family: a header of its
 * own beside include/gymgo_amd.h and include/gymgo_amd_tactics.h, whose types, error codes (GG_E_*), dtype codes (GG_W_*,
 * GG_FEAT_U8), policies (GG_POLICY_UNIFORM, GG_POLICY_NO_EYE_FILL, GG_POLICY_TACTICAL) and conventions it takes over.  The entry
 * points below are additive: GG_ABI_VERSION and the list of entry points of gymgo_amd.h do not change, and the _policy and
 * _policy2 entry points keep answering GG_E_BADARG for anything but their policies.
 */
#ifndef GYMGO_AMD_PATTERN_H
#define GYMGO_AMD_PATTERN_H
#include "gymgo_amd.h"
#include "gymgo_amd_tactics.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * THE RULE.  GG_POLICY_PATTERN = 3.  The rule applies to a live board, from the mover's view.
 *
 * Neighbour states.  Each of the eight neighbours of an empty point is empty, black, white or off the board.
 *
 * Pattern notation.  A pattern is three strings of three characters, rows top to bottom.  The centre is the point.
 *   X  a stone of one colour
 *   O  a stone of the other colour
 *   .  empty
 *   #  off the board
 *   ?  anything, off the board included
 *   x  anything but X (empty, O, off)
 *   o  anything but O (empty, X, off)
 * A point matches a pattern if some of the eight views of the pattern (four rotations, with and without a mirror) matches under
 * either assignment of black and white to X and O.  So the set does not depend on who is to move.
 *
 * The thirteen patterns.
 *    1 XOX/.../???    2 XO./.../?.?    3 XO?/X../x.?    4 .O./X../...
 *    5 XO?/O.o/?o?    6 XO?/O.X/???    7 ?X?/O.O/ooo    8 OX?/o.O/???
 *    9 X.?/O.?/###   10 OX?/X.O/###   11 ?X?/x.O/###   12 ?XO/x.x/###
 *   13 ?OX/X.O/###
 *
 * Checksum of a restatement.  Over all 4^8 assignments of the eight neighbours, 15 828 match some pattern.  Per pattern the
 * counts are 504, 256, 768, 8, 4 544, 3 392, 2 812, 10 304, 240, 64, 608, 504, 64.
 *
 * Sets.
 * - `P` = the empty points that match.
 * - `prev` = the board's previous action if it is a point of the board, in [0, N^2).  Otherwise there is no previous point.  That
 *   covers -1, the pass N^2 and any other int32.
 * - `L` = `F` and `P` and (the up to eight on-board neighbours of `prev`).  `L` is empty without a previous point.  `F`, `C`, `E`,
 *   `valid` and `eye` are as in gymgo_amd_tactics.h.
 *
 * The ply.  The generator advances exactly once.  The gate and `u` are as for GG_POLICY_TACTICAL.
 * - With the gate open, the ply draws from the first non-empty set of `C`, `E`, `L`, `F`.
 * - With the gate closed, it draws from `F`.
 * - It passes when the set is empty, else takes the set's floor(u n / 2^32)-th point in ascending order.
 *
 * No previous point.  These plies have none:
 * - a reset ply;
 * - the first ply after a pass;
 * - a job's first playout ply in either queue, including after the first move of a move-playout job.
 *
 * Resets, frozen boards, the live-prefix invariant and `x0 + played c` are as for GG_POLICY_NO_EYE_FILL.
 *
 * The planes: gg_pattern_planes() = 2 planes per board, out [B][2][N][N], every element exactly 0 or 1, both all zero for a game
 * that has ended:
 *   0  P   1  L
 *   gg_batch_patterns           states uint8 [B][6][N][N] -> out of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8
 *   gg_batch_patterns_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                               gg_batch_track_states(s) and s (the class rows of a tracked board are not read)
 * last (NULL, or int32 [B]): the previous action of every board, of the UNTURNED board; any value is allowed, and one that is
 * no point of the board indexes nothing.  `L` is all zero when last is NULL.
 * orient (NULL, or int32 [B], only orient[b] & 7 is read; gg_batch_symmetry's orientations): the planes are geometric, out[b]
 * is view orient[b] of the unoriented result; the board - and the previous point with it - is turned in registers after the load.
 * Alignment (out needs that of its element only), stores and the checks with their order and codes: gg_batch_life's
 * (GG_E_BADSIZE: N outside [2, 19], B < 0, an unknown dtype; B = 0 is no work; GG_E_NULLPTR: states / tracked or out NULL;
 * GG_E_BADARG: out not aligned to its element).  Every call queues ONE launch on hip_stream and never synchronises; no flood, no
 * global atomics; every store lies inside the B rows of out.
 *
 * The policy in the playouts: the three calls below accept policies 0, 1, 2 and 3; every other policy gives GG_E_BADARG; all
 * other checks and their order are the _policy2 namesake's.  Policies 0, 1 and 2 queue what the namesake queues, launch for
 * launch.
 *   gg_batch_rollout_tracked_policy3   the parameter list of _policy2.  For policies 0 - 2 last_actions stays an output and may be
 *       NULL.  Policy 3 needs it: NULL gives GG_E_NULLPTR (where the namesake looks at rng).  It is READ as the previous action
 *       of every board - any int32; a value outside [0, N^2) means no previous point and indexes nothing - and written as ever:
 *       the last action of the launch, or -1 for a board that did not play.  Carried from launch to launch, launches of any
 *       lengths give the boards one launch of the total length gives.
 *   gg_playouts_advance_policy3, gg_move_playouts_advance_policy3   the parameter lists of _policy2 plus `last`, int32 [S], before
 *       the stream: the previous action of every slot.  The caller fills it with -1 after _begin; afterwards it is opaque.  It is
 *       ignored, and may be NULL, for policies 0 - 2; policy 3 without it gives GG_E_NULLPTR (after the policy check).  The chunks
 *       run with it in and out, and the harvest sets last[s] = -1 for every slot it refills or empties: results depend on neither
 *       S nor chunk_plies.
 */
#define GG_POLICY_PATTERN 3
int32_t gg_pattern_planes(void);
int32_t gg_batch_patterns(const uint8_t *states, const int32_t *last, const int32_t *orient, void *out, int32_t out_dtype, int64_t B,
                          int32_t N, void *hip_stream);
int32_t gg_batch_patterns_tracked(const uint32_t *tracked, const int32_t *last, const int32_t *orient, void *out, int32_t out_dtype,
                                  int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_rollout_tracked_policy3(uint32_t *tracked, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B,
                                         int32_t N, int32_t plies, int32_t auto_reset, int32_t policy, void *hip_stream);
int32_t gg_playouts_advance_policy3(const uint32_t *roots, int64_t R, int32_t N, int32_t K, int64_t first_root, uint64_t base_seed,
                                    int32_t max_plies, int32_t chunk_plies, float komi, int32_t chunks, int32_t policy,
                                    uint32_t *slots, uint64_t *rng, int64_t *plies, int64_t *job, int64_t S, int64_t *counter,
                                    int32_t *counts, int64_t *sums, int32_t *ownership, int32_t *last, void *hip_stream);
int32_t gg_move_playouts_advance_policy3(const uint32_t *roots, int64_t R, int32_t N, const int32_t *plan, int64_t T, int32_t K,
                                         int64_t first_root, uint64_t base_seed, int32_t max_plies, int32_t chunk_plies,
                                         float komi, int32_t chunks, int32_t policy, uint32_t *slots, uint64_t *rng,
                                         int64_t *plies, int64_t *job, int64_t S, int64_t *counter, int32_t *counts,
                                         int64_t *sums, int32_t *last, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_PATTERN_H */
