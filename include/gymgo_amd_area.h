/*
 * gymgo_amd_area.h - the area ownership planes of libgymgo_amd.so: the C ABI of the area family, a header of its own beside
 * include/gymgo_amd.h, whose types, error codes (GG_E_*), dtype codes (GG_W_*, GG_FEAT_U8) and conventions it takes over.
 * The entry points below are additive: GG_ABI_VERSION and the list of entry points of gymgo_amd.h do not change.
 */
#ifndef GYMGO_AMD_AREA_H
#define GYMGO_AMD_AREA_H
#include "gymgo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Area ownership planes: the points Tromp-Taylor scoring counts for each colour, and those it counts for neither -
 * the per-point form of gg_batch_areas (gym_go/gogame.py:275-300), bit-exact against tests/area_expect.py.
 * With black stones b and white stones w, E = the empty points, Rb = the empty points connected through E (4-neighbourhood)
 * to an empty point next to a black stone, Rw alike for white.  side = 0 (black's view) or 1 (white's): me / op = the stones
 * of that side / the other.  A = gg_area_planes() = 3 planes per board, out [B][3][N][N], every element exactly 0 or 1:
 *   0  own_area   me | (R_me & ~R_op)
 *   1  opp_area   op | (R_op & ~R_me)
 *   2  neutral    E & ~(plane 0 | plane 1): empty points whose region touches both colours, or neither (a board without
 *                 stones is all neutral)
 * The three planes partition the board.  counts (NULL, or int32 [B][2]): counts[b] = the number of points of plane 0 and of
 * plane 1; with side 0 exactly what gg_batch_areas gives for the board.  Only planes 0 and 1 of the states and the turn flag
 * are read (of a tracked board the two stone row sets and the turn bit): plane 3, pass and done do not matter, an ended
 * position is treated like any other.
 *   gg_batch_area           states uint8 [B][6][N][N] -> out of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8
 *   gg_batch_area_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                           gg_batch_track_states(s) and s
 * side (NULL, or uint8 [B]): NULL = every board's own turn flag, the mover's view of every other plane family; else
 * side[b] == 0 is black's view of board b and anything else white's, whatever its turn flag says - the view a training target
 * needs, where the final position of a game is seen by the mover of a sampled one.
 * orient (NULL, or int32 [B], only orient[b] & 7 is read; gg_batch_symmetry's orientations): the planes are geometric, so
 * out[b] is view orient[b] of the unoriented result and also the result of the turned position; the board is turned in
 * registers after the load.  The counts do not turn.
 * Alignment (out needs that of its element only), stores and the checks with their order and codes: gg_batch_life's; orient,
 * side and counts may be NULL, out may not.  Every call queues ONE launch on hip_stream and never synchronises; no global
 * atomics; every store lies inside the B rows of out and of counts.
 */
int32_t gg_area_planes(void);
int32_t gg_batch_area(const uint8_t *states, const int32_t *orient, const uint8_t *side, void *out, int32_t *counts,
                      int32_t out_dtype, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_area_tracked(const uint32_t *tracked, const int32_t *orient, const uint8_t *side, void *out, int32_t *counts,
                              int32_t out_dtype, int64_t B, int32_t N, void *hip_stream);


#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_AREA_H */
