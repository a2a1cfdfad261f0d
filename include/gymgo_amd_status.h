/*
 * gymgo_amd_status.h - stone status and the final score from playout ownership of libgymgo_amd.so: the C ABI of the status
 * family, a header of its own beside include/gymgo_amd.h, whose types, error codes (GG_E_*), dtype codes (GG_W_*, GG_FEAT_U8)
 * and conventions it takes over.  The entry points below are additive: GG_ABI_VERSION and the list of entry points of
 * gymgo_amd.h do not change.
 */
#ifndef GYMGO_AMD_STATUS_H
#define GYMGO_AMD_STATUS_H
#include "gymgo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GG_STATUS_MAX_PLAYOUTS (1 << 20) /* the largest K */
#define GG_STATUS_MAX_DEN 1024           /* the largest denominator of the threshold */

/*
 * Stone status and final areas: which chains the playouts of a position call alive, dead or unsettled, and the
 * Tromp-Taylor areas (gg_batch_area's rule) of the board once the dead chains are taken off - the step between
 * gg_playouts_* with ownership and a final score, bit-exact against tests/status_expect.py.
 *
 * THE RULE.  own (int32 [B][2][N][N]): own[b][0][p] / own[b][1][p] = in how many of K = playouts playouts point p ended in
 * black's / white's area, in the board's stored frame (the ownership of gg_playouts_advance).  The caller's contract:
 * 0 <= own <= K and own[b][0][p] + own[b][1][p] <= K.  num / den: the threshold.  For every chain C (4-connected stones of
 * one colour c) with |C| stones, D(C) = the sum over its stones p of own[b][1 - c][p] and A(C) = that of own[b][c][p]:
 *   C is dead       iff D den >= num K |C|,
 *   else alive      iff A den >= num K |C|,
 *   else unsettled.
 * Every product is a 64-bit integer and no floating point appears: the result is bit-defined.  With D + A <= K |C| and
 * 2 num > den a chain cannot be both.  Values outside the contract give an unspecified status for their chain and nothing
 * else: no address and no loop bound depends on a value.  own on empty points is never read into a result.  After the vote
 * the dead chains of both colours are taken off, and the areas are those of what remains; unsettled chains stay on the
 * board, so the shared liberties of a seki are neutral.
 *
 * side = 0 (black's view) or 1 (white's): me / op = that side / the other.  S = gg_status_planes() = 9 planes per board,
 * out [B][9][N][N], every element exactly 0 or 1:
 *   0 / 1 / 2   my stones whose chain is alive / dead / unsettled
 *   3 / 4 / 5   op's stones whose chain is alive / dead / unsettled
 *   6 / 7 / 8   my area / op's area / neutral points, after the dead stones are gone
 * Planes 0 - 5 partition the stones, planes 6 - 8 the board.  counts (NULL, or int32 [B][4]): counts[b] = the number of
 * points of plane 6, of plane 7, of plane 1 and of plane 4.  Only planes 0 and 1 of the states and the turn flag are read (of
 * a tracked board the two stone row sets and the turn bit).
 *   gg_batch_status           states uint8 [B][6][N][N] -> out of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8
 *   gg_batch_status_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                             gg_batch_track_states(s) and s
 * side (NULL, or uint8 [B]) and orient (NULL, or int32 [B], only orient[b] & 7 is read): gg_batch_area's.  own is always in
 * the stored frame of the board, whatever orient says: out[b] is view orient[b] of the unoriented result (the analysis runs
 * unturned and the nine result rows are turned in registers).  The counts do not turn.
 *
 * Checks, in this order and before any device work: N outside [2, 19], B < 0 or an out_dtype other than the four ->
 * GG_E_BADSIZE; playouts outside [1, GG_STATUS_MAX_PLAYOUTS], num < 1, num > den, den > GG_STATUS_MAX_DEN or 2 num <= den
 * -> GG_E_BADARG; B == 0 -> 0, no work; own or counts not 4-byte aligned -> GG_E_BADARG; the boards, own or out NULL ->
 * GG_E_NULLPTR (orient, side and counts may be NULL); out not aligned to its element -> GG_E_BADARG.  Every call queues ONE
 * launch on hip_stream and never synchronises; no global atomics; every load lies inside the B rows of the inputs and every
 * store inside the B rows of out and of counts; own is not written.
 */
int32_t gg_status_planes(void);
int32_t gg_batch_status(const uint8_t *states, const int32_t *orient, const uint8_t *side, const int32_t *own, int32_t playouts,
                        int32_t num, int32_t den, void *out, int32_t *counts, int32_t out_dtype, int64_t B, int32_t N,
                        void *hip_stream);
int32_t gg_batch_status_tracked(const uint32_t *tracked, const int32_t *orient, const uint8_t *side, const int32_t *own,
                                int32_t playouts, int32_t num, int32_t den, void *out, int32_t *counts, int32_t out_dtype, int64_t B,
                                int32_t N, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_STATUS_H */
