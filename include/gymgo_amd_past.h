/*
 * gymgo_amd_past.h - the history input planes of libgymgo_amd.so: the C ABI of the past family, a header of its own beside
 * include/gymgo_amd.h, whose types, error codes (GG_E_*), dtype codes (GG_W_*, GG_FEAT_U8) and conventions it takes over.
 * The entry points below are additive: GG_ABI_VERSION and the list of entry points of gymgo_amd.h do not change.
 */
#ifndef GYMGO_AMD_PAST_H
#define GYMGO_AMD_PAST_H
#include "gymgo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GG_PAST_MAX_POSITIONS 8

/*
 * History input planes: the stones of the last T positions of a game and the points of its last T - 1 moves, as
 * the player to move now sees them - AlphaGo Zero's history planes (T = 8, moves = 0, plus the colour plane gg_batch_features
 * has) and KataGo's recent-move planes (moves = 1) from one family, bit-exact against tests/past_expect.py.
 *
 * THE RING of a batch of games: rows uint32 [B][H][2][N] and count int32 [B], H >= 1.  An entry is a position as row masks,
 * the N black rows and then the N white rows, bit c of a row = column c, as in tracked boards.  The ring holds the positions
 * strictly BEFORE the current one: the caller pushes a position before it plays on it, one push per ply, passes included.
 *   gg_past_push           states uint8 [B][6][N][N]: where mask[b] != 0 (mask NULL: everywhere) entry count[b] mod H of board b
 *                          becomes the position (planes 0 and 1 of the states) and count[b] goes up by one; every other board
 *                          keeps every byte of its ring and its count
 *   gg_past_push_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)] (their two stone row sets)
 * So position t >= 1 plies ago is entry (count - t) mod H, and it exists iff t <= min(max(count, 0), H).
 *
 * THE PLANES: T positions (1 .. GG_PAST_MAX_POSITIONS; position 0 is the current one), moves 0 or 1;
 * P = gg_past_planes(T, moves) = 2 T + (moves ? T - 1 : 0) planes per board (at most 23; -1 outside that domain),
 * out [B][P][N][N], every element exactly 0 or 1.  With me = the colour to move at position 0 (the turn flag of the board
 * given) and op = the other, whoever was to move back then:
 *   2 t      (t = 0 .. T-1)   the stones of me at position t
 *   2 t + 1                   the stones of op at position t
 *   2 T + t  (t = 0 .. T-2)   only with moves: occ_t & ~occ_{t+1}, occ = the occupied points, where position t + 1 exists, else
 *                             empty - the point of the move played t plies ago (a move adds one stone and removes captured
 *                             ones, and suicide is illegal), nothing for a pass
 * A position that does not exist gives empty planes.  Only planes 0 and 1 and the turn flag of the board given are read (of
 * a tracked board the two stone row sets and the turn bit), and the rings; every row read from a ring is masked to the
 * board, so a ring that holds garbage cannot set an element outside it.
 *   gg_batch_past           states uint8 [B][6][N][N] -> out of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8
 *   gg_batch_past_tracked   the same from tracked boards: the same bytes for gg_batch_track_states(s) and s
 * rows and count may BOTH be NULL: every earlier position is then absent (H is not looked at).  One alone may not.
 * orient (NULL, or int32 [B], only orient[b] & 7 is read; gg_batch_symmetry's orientations): every position of board b is
 * turned alike, in registers after the loads; out[b] is view orient[b] of the unoriented result and also the result of the
 * turned game.
 *
 * THE TREE: gg_puct_past gives the planes of the played leaves of a gg_puct_select / gg_puct_select_leaves launch (after
 * gg_batch_play_moves_tracked): leaf uint32 [R L][gg_tracked_words(N)], leaf_id int32 [R L], row i = slot i mod L of root
 * r = i / L, boards uint32 [R][C + 1][gg_tracked_words(N)] and links int32 [R][C + 1][2] of the tree, out [R L][P][N][N].
 * Position 0 is leaf[i].  From x = leaf_id[i] the walk takes the parent p = links[r][x][0] while 0 <= p < x (gg_puct_superko's
 * bound: corrupt links can neither loop nor leave root r's slice), at most T - 1 times: d = the ancestors found.  Position
 * t <= d is boards[r][the t-th ancestor], position t > d is position t - d of root r's ring (rows [R][H][2][N], count [R]: the
 * positions before node 0; the pair may be NULL as above).  A row whose leaf_id lies outside [0, C] - an empty slot - has
 * d = 0; its output is defined and to be ignored, like that of every other family.  A slot's ancestors are nodes evaluated
 * in earlier rounds, so their boards are in the tree (collision rule a of gg_puct_select_leaves); the new node's own links
 * entry is written by the select launch.  Nothing in the tree is written.  orient: int32 [R L] or NULL.
 *
 * Checks, all before any device work, in this order: GG_E_BADSIZE for N outside [2, GG_MAX_BOARD], B (R) < 0 or an out_dtype
 * that is none of the four; GG_E_BADARG for T outside [1, 8], moves other than 0 / 1, H < 1 with a ring given (gg_past_push:
 * always), and for gg_puct_past C < 1, C == INT32_MAX, L < 1 or L > C; B (R) == 0 returns 0; GG_E_NULLPTR for a NULL states /
 * tracked / leaf / leaf_id / boards / links / out, for a NULL rows or count of gg_past_push, and for exactly one of rows and count
 * elsewhere; GG_E_BADARG for an out not aligned to its element or any other pointer but states and mask not aligned to 4
 * bytes.  Every call queues ONE launch on hip_stream and never synchronises; no global atomics; every store is a vector
 * store inside the B rows of out, or - the pushes - inside entry count[b] mod H of board b's ring and count[b], of the boards
 * whose mask byte is set.
 */
int32_t gg_past_planes(int32_t T, int32_t moves);
int32_t gg_past_push(const uint8_t *states, const uint8_t *mask, uint32_t *rows, int32_t *count, int32_t H, int64_t B, int32_t N,
                     void *hip_stream);
int32_t gg_past_push_tracked(const uint32_t *tracked, const uint8_t *mask, uint32_t *rows, int32_t *count, int32_t H, int64_t B,
                             int32_t N, void *hip_stream);
int32_t gg_batch_past(const uint8_t *states, const uint32_t *rows, const int32_t *count, int32_t H, int32_t T, int32_t moves,
                      const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_past_tracked(const uint32_t *tracked, const uint32_t *rows, const int32_t *count, int32_t H, int32_t T,
                              int32_t moves, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                              void *hip_stream);
int32_t gg_puct_past(int64_t R, int32_t N, int32_t C, int32_t L, const uint32_t *boards, const int32_t *links, const uint32_t *rows,
                     const int32_t *count, int32_t H, int32_t T, int32_t moves, const uint32_t *leaf, const int32_t *leaf_id,
                     const int32_t *orient, void *out, int32_t out_dtype, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_PAST_H */
