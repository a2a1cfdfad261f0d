/*
 * gymgo_amd.h - C-ABI of the MI355X (gfx950) batched Go step path.
 *
 * The reference (huangeddie/GymGo) is pure Python and has no FFI seam; its boundary for this path
 * is the function API of gym_go/gogame.py + gym_go/state_utils.py.  Each entry point below is what
 * a ctypes binding of that API binds to (the stub is shown in INTEGRATION.md); the reference
 * function it replaces is cited as path:line relative to the reference root.
 *
 * Conventions (all entry points):
 *   - States are contiguous uint8 [B][6][N][N], values in {0,1}; channels per gym_go/govars.py:4-9
 *     (0 black, 1 white, 2 turn, 3 invalid moves for the side to move, 4 previous move was a pass,
 *     5 game over).  Planes 2, 4 and 5 are uniform by construction (the reference only ever writes
 *     them whole: gym_go/gogame.py:49-56, gym_go/state_utils.py:241); the kernels read one byte of each.
 *   - Every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, reads one environment
 *     variable (GYMGO_AMD_CUS, see gg_device_cus: performance only) and never synchronises: work is enqueued on `hip_stream` (a hipStream_t of the device that owns the
 *     buffers, NULL = its default stream) and the call returns immediately.  The kernels run on the device that owns
 *     the first buffer argument, whatever the calling thread's current device is (it is restored before the call
 *     returns).
 *   - Global state.  No result depends on anything but the arguments.  The library keeps three pieces of mutable state,
 *     all performance-only: a per-device cache of the CU count (relaxed atomics; racing first callers store the same value), a
 *     per-(device, kernel) cache of kernel occupancy (behind a mutex) and, in device memory, the "FairShare" progress
 *     boards of the fused multi-ply kernels (two of 512 KB per device - one per translation unit of the library: the
 *     fused rollouts with drawn moves, and the replay / env-step launches; waves of the other unit's kernels are
 *     "foreign" to a board, like another stream's - every wave of such a launch publishes the ply it has reached and
 *     reads its SIMD-mates' words to set its own issue priority; stale or foreign words only shift priorities).  Every entry point is re-entrant and
 *     thread-safe: concurrent calls from several threads on several streams are supported
 *     (tests/test_gpu_threads.py; tools/sanitize.sh: the host side under ASan / UBSan / TSan).
 *   - CPU twins.  SURVEY 8(b) sketched `_cpu`-suffixed entry points with host pointers next to these.  They are
 *     deliberately NOT exported: the CPU restatement of the path is test infrastructure (oracle/gg_oracle.c,
 *     `gg_oracle_*`, linked by tests and the bench's cpu_baseline only), and a product library that could fall back
 *     to it would void every parity claim.  A missing GPU is an error (hipErrorNoDevice / GymGoNativeError).
 *   - Which kernel serves a call depends on its arguments only (board size, batch size, plies per launch).
 *   - Alignment.  Boards may start at any byte offset, but HBM is only touched with naturally aligned 16-byte accesses:
 *     a state / children / tracked buffer must be READABLE from its start rounded down to 16 bytes to its end rounded
 *     up to 16 bytes (always true for a whole allocation and for any slice of one; bytes outside the buffer are read,
 *     never written).
 *   - 2 <= N <= 19.  Actions are int32 in [0, N*N]; N*N = pass (gym_go/gogame.py:40-42).
 *   - Return value: 0 on success, a hipError_t (> 0) for launch/runtime errors, or a negative
 *     GG_E_* code for bad arguments.  Re-entrant; safe from several threads / one process per GPU.
 */
#ifndef GYMGO_AMD_H
#define GYMGO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_ABI_VERSION 5
#define GG_MAX_BOARD 19
#define GG_NUM_CHNLS 6

#define GG_E_BADSIZE (-1)  /* N outside [2, 19] or B < 0 */
#define GG_E_NULLPTR (-2)  /* a required pointer is NULL */
#define GG_E_BADARG (-3)   /* other argument out of range */

/* element type of policy weights (gg_batch_sample_weighted*, gg_batch_env_step_tracked_weighted) */
#define GG_W_F32 0  /* float32 */
#define GG_W_BF16 1 /* bfloat16: the upper half of a float32 */
#define GG_W_F16 2  /* IEEE float16 */

/* per-game status written by gg_batch_next_states */
#define GG_STATUS_OK 0
#define GG_STATUS_ILLEGAL 1 /* point has INVD set / action out of range: the reference raises
                               AssertionError (gym_go/gogame.py:59, :117); the row is copied through */

int32_t gg_version(void);

/* Number of compute units the library sizes its grids for: those of the calling thread's current device (0 if no device),
   or the value of the environment variable GYMGO_AMD_CUS (1 ... 4096, read once per process) - for a partition of the GPU
   or a GPU shared with other work.  Results never depend on it (tests/test_gpu_cus.py). */
int32_t gg_device_cus(void);

/*
 * gogame.batch_next_states(batch_states, batch_action1d, canonical)   gym_go/gogame.py:90-150
 * with the per-game semantics of gogame.next_state                      gym_go/gogame.py:34-87
 * (place / pass, state_utils.update_pieces capture resolution :159-180, ko :72-75,
 * state_utils.compute_invalid_moves :24-83, state_utils.set_turn :235-241, optional
 * canonical_form :313-321) for EVERY game - the reference's batch path mis-aligns games when the
 * batch contains passes (gym_go/state_utils.py:187-193); that defect is not reproduced.
 * `in` and `out` must not overlap.  `status` may be NULL.
 */
int32_t gg_batch_next_states(const uint8_t *in, const int32_t *actions, uint8_t *out, int32_t *status,
                             int64_t B, int32_t N, int32_t canonical, void *hip_stream);

/*
 * gogame.batch_next_states with a caller-owned WORKSPACE                gym_go/gogame.py:90-150
 * Same arguments, results and status as gg_batch_next_states, plus `workspace`: uint32 [B][gg_tracked_words(N)], zero-filled
 * before its first use and otherwise opaque.  The call leaves in it the tracked form (stones + liberty classes) of every
 * position it wrote to `out`; the next call takes the liberty classes of game b from there when planes 0 / 1 of in[b]
 * equal the workspace's stones EXACTLY (checked per board, every call) and analyses the board from scratch otherwise.
 * A loop that feeds each output batch back as the next input - a rollout through the step API - therefore pays the
 * full liberty analysis once; results never depend on the workspace content.
 */
int32_t gg_batch_next_states_ws(const uint8_t *in, const int32_t *actions, uint8_t *out, int32_t *status, uint32_t *workspace,
                                int64_t B, int32_t N, int32_t canonical, void *hip_stream);

/*
 * state_utils.batch_compute_invalid_moves                              gym_go/state_utils.py:86-156
 * Recomputes plane 3 (invalid moves for the side to move, plane 2) from planes 0-2:
 * mask[b] = compute_invalid_moves(states[b], player = 1 - turn(states[b]), ko[b]).
 * `ko` (nullable) holds a flat point index per game or -1.  mask is uint8 [B][N][N].
 */
int32_t gg_batch_invalid_mask(const uint8_t *states, const int32_t *ko, uint8_t *mask, int64_t B, int32_t N,
                              void *hip_stream);

/*
 * gogame.batch_areas                                                   gym_go/gogame.py:303-310
 * (gogame.areas :275-300, Tromp-Taylor): black[b], white[b] = area of each colour, as int32
 * (the reference returns the same integers as float64).
 */
int32_t gg_batch_areas(const uint8_t *states, int32_t *black, int32_t *white, int64_t B, int32_t N,
                       void *hip_stream);

/*
 * gogame.children(state, canonical, padded=True) for every state      gym_go/gogame.py:175-186
 * children is uint8 [B][N*N+1][6][N][N]; slot a = next_state(states[b], a, canonical) when action a
 * is valid (plane 3 clear, or a = pass), all zeros otherwise (gym_go/tests/test_basics.py:209-223).
 */
int32_t gg_batch_children(const uint8_t *states, uint8_t *children, int64_t B, int32_t N, int32_t canonical,
                          void *hip_stream);

/* gogame.children(state, canonical, padded=False) (gym_go/gogame.py:175-180: the un-padded result is what the reference
 * computes first, :179; GoEnv.children forwards the flag, gym_go/envs/go_env.py:105-109) for a whole batch, in two calls:
 *   1. gg_batch_children_offsets: offsets int32 [B+1] = exclusive prefix sums of the number of children valid_moves() keeps
 *      per parent (:153-161: the points whose plane-3 byte is 0, + the pass; ALL N*N+1 actions once the game has ended),
 *      offsets[B] = the total.  The caller reads offsets[B] back and allocates children: uint8 [offsets[B]][6][N][N].
 *      order (int32 [B], may be NULL): the parents sorted by falling child count - the order in which the expansion should
 *      hand them to the machine (a parent's work grows with its children; heaviest first keeps the launch's tail short).
 *      Parents with equal counts come in ANY order, which may differ from one call to the next (like the slot a playout of
 *      gg_playouts_* lands in, it is settled by an atomic: it decides which work item a parent is, never what is written;
 *      these two are the outputs of the library that are not functions of the arguments alone).
 *      B = 0 is not "no work" for offsets: offsets[B] = the total holds there too, so offsets[0] = 0 is written (and no
 *      other byte).
 *      GG_E_BADSIZE if B * (N*N+1) does not fit an int32.
 *   2. gg_batch_children_compact: parent b's children at children[offsets[b] .. offsets[b+1]), ascending action order - exactly
 *      the non-zero-padded slots of gg_batch_children, i.e. children_padded[b][valid_moves(states[b]) == 1] (a kept slot whose
 *      move the reference would have refused - an ended game, plane 3 clear on a stone - is all zero, as in the padded form).
 *      order: what gg_batch_children_offsets wrote for the same states (any permutation of 0 .. B-1 gives the same result),
 *      or NULL: index order.
 * On mid-game 19x19 parents a third of the 362 slots is kept: a third of the bytes of the padded expansion. */
int32_t gg_batch_children_offsets(const uint8_t *states, int32_t *offsets, int32_t *order, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_children_compact(const uint8_t *states, const int32_t *offsets, const int32_t *order, uint8_t *children, int64_t B,
                                  int32_t N, int32_t canonical, void *hip_stream);

/*
 * Uniform-random rollout, `plies` steps per game, IN PLACE, board resident on-chip between plies:
 * per ply and game  a ~ Uniform{valid actions incl. pass}  (GoEnv.uniform_random_action,
 * gym_go/envs/go_env.py:78-81; gogame.random_action gym_go/gogame.py:395-404), then
 * state = next_state(state, a).  A finished game (plane 5 set) is reset to zeros first when
 * auto_reset != 0, otherwise it is left frozen and draws nothing.
 * rng: uint64 [B] per-game generator state (see gg_rng_seed), advanced once per ply played.
 * last_actions (nullable): int32 [B], the last action applied during this call (-1 if the game was frozen throughout).
 * steps_done (nullable): int64 [B], incremented by the number of plies actually played.
 * Sampler (build-defined, mirrored by oracle/gg_oracle.c): x += 0x9E3779B97F4A7C15;
 * u = splitmix64_finalise(x); k = ((u >> 32) * n_valid) >> 32; action = k-th valid action ascending.
 */
int32_t gg_batch_rollout(uint8_t *states, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B,
                         int32_t N, int32_t plies, int32_t auto_reset, void *hip_stream);

/*
 * gg_batch_rollout with a caller-owned WORKSPACE
 * Same arguments, results (states, rng, last_actions, steps_done) and kernel dispatch as gg_batch_rollout, plus `workspace`:
 * uint32 [B][gg_tracked_words(N)], zero-filled before its first use and otherwise opaque.  A launch of the thirty-two-board
 * kernel on byte planes leaves in it the stones and liberty classes of every position it wrote to `states`; the next call
 * takes the liberty classes of game b from there when planes 0 / 1 of states[b] equal the workspace's stones EXACTLY
 * (checked per board, every call) and analyses the board from scratch otherwise.  A loop that calls the rollout again and
 * again on one resident buffer therefore pays the full liberty analysis once, whatever else edits some of the boards in
 * between; results never depend on the workspace content.  Launches served by any other kernel (small batches, short
 * launches) neither read nor write the workspace.
 */
int32_t gg_batch_rollout_ws(uint8_t *states, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, uint32_t *workspace,
                            int64_t B, int32_t N, int32_t plies, int32_t auto_reset, void *hip_stream);

/*
 * GoEnv.step for every game of a batched env, IN PLACE, one launch            gym_go/envs/go_env.py:49-76
 *   1. auto_reset != 0: a finished game (plane 5 set) is reset first (GoEnv.reset, :40-47); auto_reset == 0: it
 *      is refused (status 1, row untouched; the reference asserts `not self.done`, :53).
 *   2. the action: actions[b] (0 .. N*N, N*N = pass) or, when actions == NULL, drawn uniformly over the valid
 *      actions with rng[b] exactly like gg_batch_rollout / gg_batch_sample_actions (uniform_random_action, :78-81).
 *   3. legality (gogame.py:59): out of range or on a set point of plane 3 -> status 1, row untouched.
 *   4. state = gogame.next_state(state, action)  (:34-87), dones[b] = game_ended (:189-196).
 *   5. rewards[b] = GoEnv.reward() (:128-149) from black's perspective with Tromp-Taylor areas (gogame.py:275-300)
 *      of the resulting position: GG_REWARD_REAL  done ? sign(black - white - komi) : 0;
 *      GG_REWARD_HEURISTIC  done ? (margin > 0 ? +N*N : -N*N) : margin.
 * rng: uint64 [B], required when actions == NULL (advanced once per game that draws).  rewards float32 [B], dones
 * uint8 [B], status int32 [B], taken_actions int32 [B] (the action used): each nullable.
 */
#define GG_REWARD_REAL 0
#define GG_REWARD_HEURISTIC 1
int32_t gg_batch_env_step(uint8_t *states, const int32_t *actions, uint64_t *rng, float *rewards, uint8_t *dones,
                          int32_t *status, int32_t *taken_actions, int64_t B, int32_t N, float komi,
                          int32_t reward_method, int32_t auto_reset, void *hip_stream);

/*
 * gg_batch_env_step + the score of every resulting position, ONE launch         gym_go/envs/go_env.py:49-76, :128-149
 * areas: int32 [B][2] (required) = gogame.areas (gym_go/gogame.py:275-300) of the position each game is left in: black, white -
 * what GoEnv.reward / winning / winner read after the step.  Everything else as gg_batch_env_step (the reward follows
 * `reward_method`).  GoEnv.step of the Python package is this call at B = 1 on a record in pinned, device-mapped host
 * memory (hipHostMalloc: the kernel reads the action and writes state, areas, status and done in place - no copy either way);
 * like every entry point it accepts any device-accessible pointer whose 16-byte-aligned superset is readable.
 */
int32_t gg_batch_env_step_scored(uint8_t *states, const int32_t *actions, uint64_t *rng, float *rewards, uint8_t *dones,
                                 int32_t *status, int32_t *taken_actions, int32_t *areas, int64_t B, int32_t N, float komi,
                                 int32_t reward_method, int32_t auto_reset, void *hip_stream);

/*
 * One sampling pass only (no step): actions[b] ~ Uniform{valid actions of states[b] incl. pass},
 * same generator as gg_batch_rollout (advances rng[b] once).  Finished games: reset is NOT applied;
 * every action counts as valid there (gogame.invalid_moves returns zeros once ended, :155-156).
 */
int32_t gg_batch_sample_actions(const uint8_t *states, uint64_t *rng, int32_t *actions, int64_t B, int32_t N,
                                void *hip_stream);

/*
 * state_utils.update_pieces / batch_update_pieces                       gym_go/state_utils.py:159-211
 * Stand-alone capture resolution (inside gg_batch_next_states it is fused), with the reference's own inputs:
 * adj is int32 [B][K] - the locations whose opponent groups are examined, as flat indices r * N + c (the reference
 * passes the on-board neighbours of the stone just placed: adj_locs of state_utils.adj_data, :214-223, so K = 4;
 * entries outside [0, N*N) are unused) - and players[b] is the side that moved.  Every group of the OTHER colour that
 * holds one of these locations and has no empty point next to it - liberties are taken on the position as given,
 * before any removal, like `empties` at :164 - is removed IN PLACE (planes 0/1) and marked in killed
 * (uint8 [B][N][N], nullable).  The position need not be reachable by legal play.
 */
int32_t gg_batch_update_pieces(uint8_t *states, const int32_t *adj, int32_t K, const int32_t *players, uint8_t *killed,
                               int64_t B, int32_t N, void *hip_stream);

/*
 * Auto-reset of a batched env (build-side policy; the reference has one game per GoEnv and resets by hand,
 * gym_go/envs/go_env.py:40-47): every game whose game-over plane is set becomes gogame.init_state (all zeros).
 */
int32_t gg_batch_reset_finished(uint8_t *states, int64_t B, int32_t N, void *hip_stream);

/*
 * Bit-packed state format for replay buffers / checkpoints / the wire (no reference counterpart; the reference
 * stores 0/1 in float64, gym_go/gogame.py:22-25).  One board = gg_packed_words(N) = 3 N + 1 uint32:
 * N row masks (bit c = column c) of plane 0, of plane 1, of plane 3, then a flag word (bit 0 turn, bit 1 previous
 * move was a pass, bit 2 game over).  unpack(pack(s)) == s for every state whose planes 2/4/5 are uniform.
 */
int32_t gg_packed_words(int32_t N);
int32_t gg_batch_pack_states(const uint8_t *states, uint32_t *packed, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_unpack_states(const uint32_t *packed, uint8_t *states, int64_t B, int32_t N, void *hip_stream);

/*
 * The step path on PACKED boards (uint32 [B][gg_packed_words(N)], the format of gg_batch_pack_states): same semantics,
 * arguments and error behaviour as the byte-plane entry points of the same name, with `packed` in place of `states`.
 * A board is 232 B instead of 2 166 B at 19x19 and the kernels skip the byte <-> bit conversions - for search trees and
 * replay buffers that keep states packed and unpack only what goes to a network.
 *   gg_batch_next_states_packed   gogame.batch_next_states         gym_go/gogame.py:90-150   (in / out must not overlap)
 *   gg_batch_rollout_packed       loop of uniform_random_action + step  gym_go/envs/go_env.py:49-81   (in place)
 *   gg_batch_env_step_packed      GoEnv.step + reward + reset      gym_go/envs/go_env.py:40-76, :128-149   (in place)
 *   gg_batch_children_packed      gogame.children per state        gym_go/gogame.py:175-186
 *                                 children: uint32 [B][N*N+1][gg_packed_words(N)], slots of invalid actions all zero
 */
int32_t gg_batch_next_states_packed(const uint32_t *in, const int32_t *actions, uint32_t *out, int32_t *status, int64_t B,
                                    int32_t N, int32_t canonical, void *hip_stream);
int32_t gg_batch_rollout_packed(uint32_t *packed, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B,
                                int32_t N, int32_t plies, int32_t auto_reset, void *hip_stream);
int32_t gg_batch_env_step_packed(uint32_t *packed, const int32_t *actions, uint64_t *rng, float *rewards, uint8_t *dones,
                                 int32_t *status, int32_t *taken_actions, int64_t B, int32_t N, float komi,
                                 int32_t reward_method, int32_t auto_reset, void *hip_stream);
int32_t gg_batch_children_packed(const uint32_t *packed, uint32_t *children, int64_t B, int32_t N, int32_t canonical,
                                 void *hip_stream);

/*
 * Replay of given move sequences, IN PLACE, the boards resident on-chip for all T moves (one launch instead of T):
 * for t = 0 .. T-1: states[b] = gogame.next_state(states[b], moves[b][t])      gym_go/gogame.py:34-87
 * i.e. a loop of GoEnv.step (gym_go/envs/go_env.py:49-76) over recorded games, search lines or a policy's action buffer.
 * moves: int32 [B][T] (N*N = pass).  A game stops at its first move that is out of range, on an invalid point
 * (gogame.py:59) or made after the game has ended (go_env.py:53) and keeps the state before that move;
 * played (nullable): int32 [B] = number of moves applied (T if all were).  _packed: the same on packed boards.
 */
int32_t gg_batch_play_moves(uint8_t *states, const int32_t *moves, int32_t *played, int64_t B, int32_t N, int32_t T,
                            void *hip_stream);
int32_t gg_batch_play_moves_packed(uint32_t *packed, const int32_t *moves, int32_t *played, int64_t B, int32_t N, int32_t T,
                                   void *hip_stream);

/*
 * TRACKED boards: uint32 [B][gg_tracked_words(N) = 5 N + 1] = the packed board (rows of planes 0 / 1 / 3) + two more
 * row sets - the black / the white stones whose group has >= 2 liberties - + the flag word (bit 0 turn, bit 1 previous
 * move was a pass, bit 2 game over).  A board that carries its liberty classes needs no analysis when a launch starts,
 * so stepping it ONE ply per launch (a policy network choosing every move) runs at the fused kernel's rate.
 *   gg_batch_track_states       uint8 [B][6][N][N] -> tracked (classes by one analysis)
 *   gg_batch_untrack_states     tracked -> uint8 [B][6][N][N]
 *   gg_batch_rollout_tracked    as gg_batch_rollout, in place on tracked boards
 *   gg_batch_play_moves_tracked as gg_batch_play_moves, in place on tracked boards (T = 1: one GoEnv.step per game)
 * The class rows must belong to the position: boards edited by the caller go through untrack / track again.
 */
int32_t gg_tracked_words(int32_t N);
int32_t gg_batch_track_states(const uint8_t *states, uint32_t *tracked, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_untrack_states(const uint32_t *tracked, uint8_t *states, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_rollout_tracked(uint32_t *tracked, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B,
                                 int32_t N, int32_t plies, int32_t auto_reset, void *hip_stream);
int32_t gg_batch_play_moves_tracked(uint32_t *tracked, const int32_t *moves, int32_t *played, int64_t B, int32_t N, int32_t T,
                                    void *hip_stream);

/*
 * GoEnv.step for every game of a batched env whose boards are kept TRACKED, IN PLACE, one launch
 * (gym_go/envs/go_env.py:49-76): the same steps 1-5, arguments and outputs as gg_batch_env_step, on boards that carry
 * their liberty classes - no per-ply analysis, so a policy-driven env steps at the multi-ply kernel's per-ply rate.
 * states_out (nullable): uint8 [B][6][N][N], the resulting position of EVERY game as byte planes - the observation
 * GoEnv.step returns (:66), written by the same launch (pass NULL to keep only the tracked boards current).
 * steps_done (nullable): int64 [B], += 1 for every game whose step was played (status GG_STATUS_OK).
 * GG_REWARD_REAL scores a game only when it ends (a rare path); GG_REWARD_HEURISTIC scores every game every step.
 */
int32_t gg_batch_env_step_tracked(uint32_t *tracked, const int32_t *actions, uint64_t *rng, float *rewards, uint8_t *dones,
                                  int32_t *status, int32_t *taken_actions, uint8_t *states_out, int64_t *steps_done,
                                  int64_t B, int32_t N, float komi, int32_t reward_method, int32_t auto_reset,
                                  void *hip_stream);

/*
 * gg_batch_env_step_tracked with the move of every game DRAWN FROM POLICY WEIGHTS by the same launch:
 * gogame.random_weighted_action (gym_go/gogame.py:385-392) fused into GoEnv.step (gym_go/envs/go_env.py:49-76).
 * weights: [B][N*N+1] of float32 / bfloat16 / float16 (weight_dtype = GG_W_*; one weight per action, the pass last; the
 * 16-bit forms are widened exactly and halve the bytes this launch reads).  Per game: a finished game is reset first when
 * auto_reset; the weights are masked by the game's invalid-move rows (the pass is always playable), L1-normalised and
 * drawn from as gg_batch_sample_weighted describes, with rng[b] (which advances once; a frozen game - finished,
 * auto_reset == 0 - draws nothing and is refused).  A game whose playable weights are all zero is refused
 * (status GG_STATUS_ILLEGAL, taken action -1) - np.random.choice raises for such a vector.  Other arguments and
 * outputs as gg_batch_env_step_tracked; taken_actions receives the drawn moves.
 */
int32_t gg_batch_env_step_tracked_weighted(uint32_t *tracked, const void *weights, int32_t weight_dtype, uint64_t *rng, float *rewards,
                                           uint8_t *dones, int32_t *status, int32_t *taken_actions, uint8_t *states_out,
                                           int64_t *steps_done, int64_t B, int32_t N, float komi, int32_t reward_method,
                                           int32_t auto_reset, void *hip_stream);

/*
 * gogame.random_weighted_action(move_weights)                           gym_go/gogame.py:385-392
 * gogame.random_action(state) = the same with weights 1 - invalid       gym_go/gogame.py:395-404
 * for every game: actions[b] ~ weights[b] / sum(weights[b]) over the playable actions.  The reference normalises in
 * float64 and draws from NumPy's global generator; so that device and oracle agree bit for bit the draw is defined in
 * integers: (1) each weight (float32, or bfloat16 / float16 widened exactly: weight_dtype = GG_W_*) is clamped to
 * [+0, FLT_MAX] on its float32 bit pattern (anything with the sign bit set, -NaN included -> 0; +NaN / +inf -> FLT_MAX)
 * and zeroed where plane 3 of states[b] is set (the reference ASSUMES invalid moves have weight 0, :387; the pass is
 * never masked, a finished game masks nothing, gym_go/gogame.py:155-156; states == NULL: no mask); (2) with E = max(the
 * largest weight's biased exponent, 24), q[a] = trunc(w[a] * 2^(148 - E)) < 2^22: the weights as 22-bit fixed point
 * relative to the largest; (3) T = sum q, k = floor((u >> 32) * T / 2^32) with u the next output of rng[b]
 * (gg_rng_seed's generator, advanced once per game per call); (4) the action is the first one, in the interleaved order
 * a = i + 16 j (i = 0..15 outer), whose running sum of q exceeds k, so P(a) = q[a] / T.  T == 0 gives actions[b] = -1.
 */
int32_t gg_batch_sample_weighted(const uint8_t *states, const void *weights, int32_t weight_dtype, uint64_t *rng,
                                 int32_t *actions, int64_t B, int32_t N, void *hip_stream);

/* The same draw for row-mask boards: planes = 3 (packed, gg_batch_pack_states) or 5 (tracked, gg_batch_track_states). */
int32_t gg_batch_sample_weighted_rows(const uint32_t *boards, int32_t planes, const void *weights, int32_t weight_dtype,
                                      uint64_t *rng, int32_t *actions, int64_t B, int32_t N, void *hip_stream);

/*
 * gogame.all_symmetries(image) / gogame.random_symmetry(image)          gym_go/gogame.py:340-382
 * for a batch: in is uint8 [B][C][N][N] (any C >= 1 with C*N*N <= 8192: states, observations, per-point targets).
 * orient: int32 [B], the orientation of each game in 0..7 composed exactly as the reference does (bit 0 flip the columns,
 * then bit 1 flip the rows, then bit 2 np.rot90 over the board axes) -> out is [B][C][N][N]; orient == NULL: all eight
 * views of every game, out is [B][8][C][N][N] in the order of all_symmetries.  in and out must not overlap.
 */
int32_t gg_batch_symmetry(const uint8_t *in, const int32_t *orient, uint8_t *out, int64_t B, int32_t C, int32_t N,
                          void *hip_stream);

/*
 * The same on row-mask boards (planes = 3 packed / 5 tracked; uint32 [B][planes*N+1]): every row plane is transformed
 * (a column flip is a bit reversal, a row flip a row permutation, the rotation a bit transpose), the flag word copied -
 * liberty classes and the invalid-move rows (ko point included) are geometric, so the result is a valid board of the
 * same format.  out is [B][W] (orient given) or [B][8][W].
 */
int32_t gg_batch_symmetry_rows(const uint32_t *in, int32_t planes, const int32_t *orient, uint32_t *out, int64_t B,
                               int32_t N, void *hip_stream);

/* rng[b] = initial generator state for (base_seed, game index first_game + b). */
int32_t gg_rng_seed(uint64_t *rng, uint64_t base_seed, int64_t first_game, int64_t B, void *hip_stream);

/*
 * Batched Monte Carlo playouts to the end of the game, scored and reduced per root.  Composes the loop of
 * GoEnv.uniform_random_action + step (gym_go/envs/go_env.py:78-81; gogame.next_state gym_go/gogame.py:34-87) until the
 * game ends, then gogame.winning (:225-230) on gogame.areas (Tromp-Taylor, :275-300) of the final position.
 * Playout j of local root r is global job p = (first_root + r) * K + j: its generator starts as gg_rng_seed(base_seed,
 * first_game = p), it plays the sampler of gg_batch_rollout from roots[r] with auto_reset = 0 until the game-over flag is
 * set or max_plies plies have been played (a root that has ended plays none) and is scored as it stands: b, w = areas,
 * outcome = sign(b - w - komi) (komi as float32).  Per root (integer sums: no result depends on S, chunk_plies or the
 * order in which the device finishes the jobs):
 *   counts    int32 [R][4]: black wins, white wins, draws, unfinished (playouts cut off by max_plies)
 *   sums      int64 [R][2]: sum of (b - w), sum of plies played
 *   ownership int32 [R][2][N][N] (nullable): per point, the number of playouts that ended with it in black's / white's area
 * roots: tracked boards uint32 [R][gg_tracked_words(N)] (gg_batch_track_states), read only.  S working slots, caller-owned
 * and otherwise opaque: slots uint32 [S][gg_tracked_words(N)], rng uint64 [S], plies int64 [S], job int64 [S];
 * counter int64 [2] = {next job id, the value it reaches once every job is done}: counter[1] - counter[0] = jobs outstanding
 * (every harvested playout takes one id from the queue, ids from R K on refill nothing).
 *   gg_playouts_begin    zeroes counts / sums / ownership, sets counter = {m, R K + m} with m = min(S, R K) and fills the
 *                        first m slots with jobs 0, 1, ... (the other slots: empty, frozen boards).  R = 0 is NOT "no work"
 *                        here: it makes the empty queue - counter = {0, 0}, every slot empty -, which a driver that polls
 *                        counter relies on (gg_move_playouts_begin with T = 0 likewise); an advance on it is no work.
 *                        Which slot a job lands in is settled by an atomic on counter: the slots are opaque, and two runs of
 *                        the same calls hold the same jobs in other slots.  counts / sums / ownership do not depend on it.
 *   gg_playouts_advance  queues `chunks` x (gg_batch_rollout_tracked of chunk_plies plies on all S slots + one harvest
 *                        launch that scores every slot whose playout has ended, adds it to its root and refills the slot
 *                        from the queue).  The work is done once counter[0] == counter[1]; a playout takes at most
 *                        max_plies / chunk_plies chunks, so (ceil(R K / S) + 1) * max_plies / chunk_plies chunks always suffice.
 * Both calls take the same arguments (komi and chunks: advance only) and must be given them unchanged between a begin
 * and the advances that follow it.  GG_E_BADSIZE: N outside [2, 19], R < 0, S < 1; GG_E_BADARG: K < 1, chunk_plies < 1,
 * max_plies < 1 or not a multiple of chunk_plies, first_root < 0, chunks < 0; GG_E_NULLPTR: a buffer other than
 * ownership is NULL.
 */
int32_t gg_playouts_begin(const uint32_t *roots, int64_t R, int32_t N, int32_t K, int64_t first_root, uint64_t base_seed,
                          int32_t max_plies, int32_t chunk_plies, uint32_t *slots, uint64_t *rng, int64_t *plies, int64_t *job,
                          int64_t S, int64_t *counter, int32_t *counts, int64_t *sums, int32_t *ownership, void *hip_stream);
int32_t gg_playouts_advance(const uint32_t *roots, int64_t R, int32_t N, int32_t K, int64_t first_root, uint64_t base_seed,
                            int32_t max_plies, int32_t chunk_plies, float komi, int32_t chunks, uint32_t *slots, uint64_t *rng,
                            int64_t *plies, int64_t *job, int64_t S, int64_t *counter, int32_t *counts, int64_t *sums,
                            int32_t *ownership, void *hip_stream);

/*
 * Flat Monte Carlo: the playouts above per legal FIRST MOVE.  A = N*N + 1.  Action a is legal at root r when the root's game
 * has not ended and a is the pass (a = N*N) or point a's invalid bit is clear: exactly the moves the tracked step accepts.
 * A root whose game has ended has NO legal first move (unlike gg_batch_children, which keeps all A slots of such a parent).
 * Playout j of the legal pair (r, a) is global job p = ((first_root + r) A + a) K + j: it starts from the child
 * next_state(roots[r], a) with the generator gg_rng_seed(base_seed, first_game = p) and is then played and scored exactly as
 * a playout of gg_playouts_* (max_plies counts the plies AFTER the first move; a first move that ends the game - a pass
 * after a pass - gives a finished playout of 0 plies).  So row (r, a) equals gg_playouts_* of that child alone with
 * first_root = (first_root + r) A + a.  No ownership output.
 *   gg_move_playouts_plan     offsets int32 [R+1] = exclusive prefix sums of the number of legal first moves per root
 *                             (offsets[R] = T, the number of legal pairs: read it back before the calls below; R = 0
 *                             writes offsets[0] = 0 and nothing else);
 *                             plan int32 [R*A]: plan[offsets[r] + k] = r A + a_k, a_k root r's k-th legal action in
 *                             ascending order (the pass last); only the first T entries are written.
 *                             GG_E_BADSIZE: N outside [2, 19], R < 0, R*A does not fit an int32; GG_E_NULLPTR.
 *   gg_move_playouts_begin / gg_move_playouts_advance: the protocol of gg_playouts_begin / advance on J = T K jobs.  Local
 *                             job q is playout q % K of the pair plan[q / K].  Outputs per pair, indexed by r A + a, zero for
 *                             the illegal ones: counts int32 [R][A][4], sums int64 [R][A][2] (as above; Σ plies without the
 *                             first move).  (ceil(T K / S) + 1) * max_plies / chunk_plies chunks always suffice.
 * The argument checks are those of gg_playouts_*, in the same order, with GG_E_BADSIZE also for R*A beyond an int32 and
 * T outside [0, R*A]; plan is required.
 */
int32_t gg_move_playouts_plan(const uint32_t *roots, int64_t R, int32_t N, int32_t *offsets, int32_t *plan, void *hip_stream);
int32_t gg_move_playouts_begin(const uint32_t *roots, int64_t R, int32_t N, const int32_t *plan, int64_t T, int32_t K,
                               int64_t first_root, uint64_t base_seed, int32_t max_plies, int32_t chunk_plies, uint32_t *slots,
                               uint64_t *rng, int64_t *plies, int64_t *job, int64_t S, int64_t *counter, int32_t *counts,
                               int64_t *sums, void *hip_stream);
int32_t gg_move_playouts_advance(const uint32_t *roots, int64_t R, int32_t N, const int32_t *plan, int64_t T, int32_t K,
                                 int64_t first_root, uint64_t base_seed, int32_t max_plies, int32_t chunk_plies, float komi,
                                 int32_t chunks, uint32_t *slots, uint64_t *rng, int64_t *plies, int64_t *job, int64_t S,
                                 int64_t *counter, int32_t *counts, int64_t *sums, void *hip_stream);

/*
 * UCT tree search over the playouts above, R independent searches of I iterations, the trees on the device.  A = N*N + 1.
 * Each root r has a tree with room for I + 1 nodes (node 0 = the root); a node holds its tracked board, parent / action
 * (-1 at the root), integer stats n / black wins / white wins / draws and a child table child[a] (-1: not expanded).
 * The legal actions of node x: none once x's game has ended, else the pass and every point whose invalid bit is clear.
 * Iteration i, per root:
 *   1. select (gg_uct_select): from x = 0, while x's game has not ended: if some legal a has no child, the lowest such a
 *      is expanded - node y = nodes[r]++ with parent x, action a, zero stats, child_x[a] = y - and y is the leaf;
 *      otherwise x = child_x[a*], a* the legal action of the largest U (ties to the lowest action) with, for c = child_x[a]
 *      and w = black wins of c if black is to move at x (flag bit 0 clear), else white wins of c:
 *        U = (2 w + d_c) / (2 n_c) + C * sqrt(log_table[n_x / K] / n_c)
 *      in float64, each operation rounded to nearest in this order, no fused multiply-add.  A node whose game has ended
 *      is the leaf itself.  Writes leaf[r] = the board of the node the walk stopped at (the new node's parent, or the
 *      ended node), move[r] = the expanded action (-1: none), leaf_id[r] = the leaf.
 *   2. the caller plays move on leaf (gg_batch_play_moves_tracked(leaf, move, NULL, R, N, T = 1): -1 is out of range, the
 *      board stays put) and evaluates leaf with gg_playouts_begin / _advance (roots = leaf, K playouts per root).
 *   3. backup (gg_uct_backup): stores leaf[r] as node y's board when move[r] >= 0, then adds K to n and counts[r][0..2] to
 *      the black wins / white wins / draws of every node from leaf_id[r] up to the root; totals (nullable, int64 [R][2],
 *      zeroed by the caller) += counts[r][3] (unfinished), sums[r][1] (plies).
 * Buffers, caller-owned (W = gg_tracked_words(N)): boards uint32 [R][I+1][W], child int32 [R][I+1][A], links int32 [R][I+1][2]
 * (parent, action; -1 / -1 at unused nodes), stats int32 [R][I+1][4] (n, black wins, white wins, draws), nodes int32 [R];
 * leaf uint32 [R][W], move int32 [R], leaf_id int32 [R]; log_table double [I+1] = log(t K), t = 0 .. I.
 *   gg_uct_begin   node 0 = roots[r] (tracked, read only), every child table -1, links -1, stats 0, nodes = 1.
 * A select without room (more than I selects after a begin) evaluates the node it stopped at: no write beyond a tree.
 * The argument checks come before any device work, in the order of gg_playouts_*: GG_E_BADSIZE: N outside [2, 19],
 * R < 0; GG_E_BADARG: I < 1, K < 1, C negative or not finite (select); GG_E_BADSIZE: I K >= 2^31; GG_E_NULLPTR: a buffer
 * other than totals is NULL.  R = 0 is no work.  The same R, N, I, K go to every call of one search.
 */
int32_t gg_uct_begin(const uint32_t *roots, int64_t R, int32_t N, int32_t I, int32_t K, uint32_t *boards, int32_t *child,
                     int32_t *links, int32_t *stats, int32_t *nodes, void *hip_stream);
int32_t gg_uct_select(int64_t R, int32_t N, int32_t I, int32_t K, double c, const double *log_table, const uint32_t *boards,
                      int32_t *child, int32_t *links, int32_t *stats, int32_t *nodes, uint32_t *leaf, int32_t *move,
                      int32_t *leaf_id, void *hip_stream);
int32_t gg_uct_backup(int64_t R, int32_t N, int32_t I, int32_t K, const int32_t *counts, const int64_t *sums, int64_t *totals,
                      uint32_t *boards, const int32_t *links, int32_t *stats, const uint32_t *leaf, const int32_t *move,
                      const int32_t *leaf_id, void *hip_stream);

/*
 * Playout policies: what a ply of the tracked rollout - and so of every playout above - draws from.
 *   GG_POLICY_UNIFORM      the sampler of gg_batch_rollout: every legal point and the pass with equal probability
 *   GG_POLICY_NO_EYE_FILL  never fill your own eye, pass only when nothing else is left.  A point p is an EYE OF THE MOVER
 *                          when p is empty, every orthogonal neighbour of p on the board holds a stone of the mover and, with
 *                          D = the diagonal neighbours of p on the board that hold an opponent stone, D = 0 if p lies on the
 *                          first or last row or column, else D <= 1.  The candidates are the points whose invalid bit is
 *                          clear and that are not eyes of the mover, in ascending order, n of them.  A ply advances the
 *                          generator exactly once as the uniform sampler does, whether or not the draw is used; the action
 *                          is the pass if n = 0, else the floor((u >> 32) n / 2^32)-th candidate.
 * First moves (gg_move_playouts_*) and the tree (gg_uct_*) keep all legal actions: the policy governs playout plies only.
 *   gg_batch_eye_mask                mask uint8 [B][N][N] = the mover's eyes of byte-plane boards uint8 [B][6][N][N] (all
 *                                    zero for a game that has ended); checks as gg_batch_invalid_mask
 *   gg_batch_rollout_tracked_policy  gg_batch_rollout_tracked with the policy (GG_POLICY_UNIFORM forwards to it)
 *   gg_playouts_advance_policy, gg_move_playouts_advance_policy: the _advance calls with `policy` after `chunks`
 * GG_E_BADARG for a policy other than the two above, checked with the other arguments before any device work.
 */
#define GG_POLICY_UNIFORM 0
#define GG_POLICY_NO_EYE_FILL 1
int32_t gg_batch_eye_mask(const uint8_t *states, uint8_t *mask, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_rollout_tracked_policy(uint32_t *tracked, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B,
                                        int32_t N, int32_t plies, int32_t auto_reset, int32_t policy, void *hip_stream);
int32_t gg_playouts_advance_policy(const uint32_t *roots, int64_t R, int32_t N, int32_t K, int64_t first_root, uint64_t base_seed,
                                   int32_t max_plies, int32_t chunk_plies, float komi, int32_t chunks, int32_t policy,
                                   uint32_t *slots, uint64_t *rng, int64_t *plies, int64_t *job, int64_t S, int64_t *counter,
                                   int32_t *counts, int64_t *sums, int32_t *ownership, void *hip_stream);
int32_t gg_move_playouts_advance_policy(const uint32_t *roots, int64_t R, int32_t N, const int32_t *plan, int64_t T, int32_t K,
                                        int64_t first_root, uint64_t base_seed, int32_t max_plies, int32_t chunk_plies,
                                        float komi, int32_t chunks, int32_t policy, uint32_t *slots, uint64_t *rng,
                                        int64_t *plies, int64_t *job, int64_t S, int64_t *counter, int32_t *counts,
                                        int64_t *sums, void *hip_stream);

/*
 * PUCT tree search with priors and a caller-supplied evaluator (the AlphaZero search), R independent searches of I
 * iterations, the trees on the device.  A = N*N + 1.  Each root r has a tree with room for I + 1 nodes (node 0 = the root); a
 * node holds its tracked board, parent / action (-1 at the root), a stat record {w: float64 sum of the backed-up values FROM
 * BLACK'S POINT OF VIEW, n: int32 visits}, float32 priors prior[a] (all zero until the node is evaluated) and a child table
 * child[a] (-1: no child).  The legal actions of node x are those of gg_uct_*: none once x's game has ended, else the pass
 * and every point whose invalid bit is clear.  Nothing in the tree draws random numbers; root r's results depend on root r
 * alone.  Iteration i, per root:
 *   1. select (gg_puct_select): from x = 0.  If x's game has ended or n_x = 0 (not evaluated yet: only the root, at i = 0),
 *      x is the leaf and move = -1.  Otherwise a* = the legal action of the largest U (ties to the lowest action); without a
 *      child under a*, node y = nodes[r]++ with parent x, action a*, child_x[a*] = y is the leaf and move = a*; else
 *      x = child_x[a*] and the walk goes on.  With s = +1 if black is to move at x (flag bit 0 clear), else -1, and n_c, w_c
 *      the record of the child under a (n_c = 0 without a child):
 *        q = n_c == 0 ? 0 : s * w_c / n_c;  t1 = C * prior_x[a];  t2 = sqrt(n_x);  t3 = t1 * t2;  t4 = t3 / (1 + n_c);  U = q + t4
 *      in float64, each operation rounded to nearest in this order, no fused multiply-add; a U that is NaN (C = 0 times an
 *      infinite prior) counts as -infinity.  n_x counts the node's own evaluation (n_x = 1 + the sum of n_c), so the first
 *      selection below a fresh node sees sqrt(1) and follows the priors.  Writes leaf[r] = the board of the node the walk
 *      stopped at (the new node's parent, or the leaf itself), move[r], leaf_id[r] = the leaf.
 *   2. the caller plays move on leaf (gg_batch_play_moves_tracked(leaf, move, NULL, R, N, T = 1): -1 is out of range, the
 *      board stays put), turns leaf into byte planes (gg_batch_untrack_states) and has them evaluated: priors float32 [R][A]
 *      and values float32 [R], the value from the point of view of the player to move at the leaf.  Priors are NOT
 *      renormalised here (a float sum would depend on its order): that is the evaluator's job.
 *   3. backup (gg_puct_backup): stores leaf[r] as node y's board when move[r] >= 0.  If n_y = 0, prior_y[a] = priors[r][a]
 *      where a is legal at y and priors[r][a] > 0, else 0 (NaN, negatives, illegal actions -> 0).  If y's game has ended,
 *      v = sign(b - w - komi) of its Tromp-Taylor areas (komi as float32, as gg_playouts_*) and the evaluator's row is
 *      ignored; else v = s_y * clamp(values[r], -1, 1) with NaN -> 0.  Every node from y up to the root: n += 1, w += v (one
 *      float64 add per node and iteration, in iteration order).
 * Buffers, caller-owned (W = gg_tracked_words(N)): boards uint32 [R][I+1][W], child int32 [R][I+1][A], prior float [R][I+1][A],
 * links int32 [R][I+1][2] (parent, action; -1 / -1 at unused nodes), stats gg_puct_stat [R][I+1], nodes int32 [R];
 * leaf uint32 [R][W], move int32 [R], leaf_id int32 [R].  4 W + 8 A + 24 bytes per node.
 *   gg_puct_begin   node 0 = roots[r] (tracked, read only), every child table -1, priors 0, links -1, stats 0, nodes = 1.
 * A select without room (all I + 1 nodes in use: I selects use I of them) evaluates the node it stopped at, with move = -1:
 * no write beyond a tree.
 * The argument checks come before any device work, in the order of gg_uct_*: GG_E_BADSIZE: N outside [2, 19], R < 0;
 * GG_E_BADARG: I < 1 or I = 2^31 - 1 (I + 1 nodes are counted in an int32), C negative or not finite (select), komi not
 * finite (backup); GG_E_NULLPTR: a buffer is NULL.  R = 0 is no work.  The same R, N, I go to every call of one search.
 */
typedef struct {
  double w;         /* sum of the backed-up values, black's point of view */
  int32_t n;        /* visits, the node's own evaluation included */
  int32_t reserved; /* 0 on the one-leaf path; v, the virtual visits, of gg_puct_*_leaves: 0 outside a round */
} gg_puct_stat;
int32_t gg_puct_begin(const uint32_t *roots, int64_t R, int32_t N, int32_t I, uint32_t *boards, int32_t *child, float *prior,
                      int32_t *links, gg_puct_stat *stats, int32_t *nodes, void *hip_stream);
int32_t gg_puct_select(int64_t R, int32_t N, int32_t I, double c, const uint32_t *boards, int32_t *child, const float *prior,
                       int32_t *links, const gg_puct_stat *stats, int32_t *nodes, uint32_t *leaf, int32_t *move, int32_t *leaf_id,
                       void *hip_stream);
int32_t gg_puct_backup(int64_t R, int32_t N, int32_t I, float komi, const float *priors, const float *values, uint32_t *boards,
                       float *prior, const int32_t *links, gg_puct_stat *stats, const uint32_t *leaf, const int32_t *move,
                       const int32_t *leaf_id, void *hip_stream);

/*
 * PUCT with several leaves per root per round and virtual loss: a second select / backup pair on the SAME tree (same
 * buffers, same bytes; gg_puct_begin is reused unchanged with I = C).  R roots, T rounds, L >= 1 slots per root and round;
 * the tree has room for C + 1 nodes, C = T * L.  Each node has n, w and priors as above plus v, an int32 count of virtual
 * visits: the reserved word of gg_puct_stat, 0 outside a round.  Slot j of root r is row r * L + j of leaf / move /
 * leaf_id / priors / values.  One round, per root:
 *   1. select (gg_puct_select_leaves) runs slots j = 0 .. L - 1 strictly in order.  Each slot walks from x = 0 and tests, in
 *      this order:
 *      a. n_x = 0 and v_x > 0: x was handed out earlier in this round and is not evaluated yet - a collision.  This slot and
 *         every later slot of this root are EMPTY: leaf_id = -1, move = -1, leaf = a copy of node 0's board; selection for
 *         this root ends, nothing is added to any v.  The test comes before any read of x's board (a node created in this
 *         round has no board in the tree until its backup).
 *      b. the game has ended at x: x is the leaf, move = -1.  An ended node may be taken by several slots of one round.
 *      c. n_x = 0 (and v_x = 0): x is the leaf, move = -1 (the root in round 0).
 *      d. otherwise a* = the legal action of the largest U', ties to the lowest action.  With s = +-1 for the mover at x and
 *         n_c, w_c, v_c all 0 without a child:
 *           ne = n_c + v_c;  q = ne == 0 ? 0 : (s * w_c - (double)v_c) / (double)ne;  t1 = c * prior_x[a];
 *           t2 = sqrt((double)(n_x + v_x));  t3 = t1 * t2;  t4 = t3 / (double)(1 + ne);  U' = q + t4
 *         in float64, in this order, no fused multiply-add, NaN counts as -infinity: one virtual visit is one loss for the
 *         side that chose the child.  With every v = 0 this is U of gg_puct_select bit for bit.  No child under a*: with room,
 *         node y = nodes[r]++ is linked in and is the leaf, move = a*; without room (only when driven past C leaves) x is
 *         the leaf as it is, move = -1.  A child under a*: descend.
 *      After a slot has found its leaf, v += 1 on every node from the leaf up to the root.
 *   2. the caller plays the R * L moves (gg_batch_play_moves_tracked(leaf, move, NULL, R * L, N, T = 1)), untracks the
 *      boards and may take the legality mask from gg_puct_legal; rows of empty slots are evaluated like any other and ignored.
 *   3. backup (gg_puct_backup_leaves) runs the slots in ascending order and skips leaf_id = -1.  Each slot does exactly step 3
 *      of gg_puct_backup with row r * L + j, and v -= 1 (never below 0) on the same chain.  The float64 additions into w
 *      happen in slot order.  After a backup every v of the tree is 0.
 * So root n = the number of non-empty slots so far (at most T * L), round 0 evaluates the root alone, and L = 1 never
 * collides and grows the tree of gg_puct_select / gg_puct_backup exactly.
 * Buffers: the tree as above with C where I stood; leaf uint32 [R*L][W], move / leaf_id int32 [R*L], priors float [R*L][A],
 * values float [R*L].  The argument checks come before any device work, in the order above: GG_E_BADSIZE, then
 * GG_E_BADARG (the conditions of gg_puct_select / gg_puct_backup on C, or L < 1, or L > C), then GG_E_NULLPTR.
 *   gg_puct_legal   from B played tracked boards leaf [B][W] and leaf_id [B]: legal uint8 [B][A] (1 = the pass and every
 *                   point whose invalid bit is clear; all 0 once the game has ended) and live uint8 [B] (1 where
 *                   leaf_id >= 0), in one launch.  GG_E_BADSIZE: N outside [2, 19], B < 0; GG_E_NULLPTR; B = 0 is no work.
 */
int32_t gg_puct_select_leaves(int64_t R, int32_t N, int32_t C, int32_t L, double c, const uint32_t *boards, int32_t *child,
                              const float *prior, int32_t *links, gg_puct_stat *stats, int32_t *nodes, uint32_t *leaf,
                              int32_t *move, int32_t *leaf_id, void *hip_stream);
int32_t gg_puct_backup_leaves(int64_t R, int32_t N, int32_t C, int32_t L, float komi, const float *priors, const float *values,
                              uint32_t *boards, float *prior, const int32_t *links, gg_puct_stat *stats, const uint32_t *leaf,
                              const int32_t *move, const int32_t *leaf_id, void *hip_stream);
int32_t gg_puct_legal(const uint32_t *leaf, const int32_t *leaf_id, int64_t B, int32_t N, uint8_t *legal, uint8_t *live,
                      void *hip_stream);

/*
 * Tree reuse across moves: every root plays one action and the subtree under it becomes the tree, in place.  The tree is
 * the one of gg_puct_* above with room for C + 1 nodes (C where I stood), on either path.  The call is only defined outside
 * a round (after a backup, or before the first select), when every v = 0.  actions int32 [R]; next uint32 [R][W], the
 * tracked board of each root after its action (what gg_batch_play_moves_tracked(.., T = 1) makes of node 0's board; read
 * only where a fresh tree is made); remap int32 [R][C+1], caller-owned scratch whose contents afterwards are unspecified;
 * kept int32 [R], may be NULL.  Per root r, with a = actions[r], m = nodes[r] clamped to [1, C + 1] and child_0 the root's
 * child table:
 *   a = -1                                  k = 0: the root stays (a game that has ended, a root the caller does not move)
 *   0 <= a < A and 1 <= child_0[a] < m      k = child_0[a]
 *   anything else                           k = -1
 * k = 0: no byte of the tree changes (nodes[r] included); kept[r] = m.
 * k > 0: the kept set K is k and every node whose parent chain reaches k: ascending over x in (k, m), x is kept when its
 *   parent p satisfies k <= p < x and p is kept (parents have smaller ids, so one pass decides it).  new(x) = the number of
 *   kept nodes below x, an order-preserving renumbering with new(k) = 0.  Node new(x) receives x's board, its prior row (as
 *   bit patterns), n and w, and v = 0; its links become (new(parent_x), action_x), (-1, -1) at the new root; in its child
 *   row a negative entry stays, an entry c with x < c < m becomes new(c) - a child of a kept node is kept - and any other
 *   entry (only with corrupt buffers) -1, as does an entry whose node was not kept.  nodes[r] = kept[r] = |K|.  Every node
 *   in [|K|, m) is put back into gg_puct_begin's state - child -1, prior +0, links -1 / -1, stats all-zero bytes - and its
 *   board words are set to 0.
 * k = -1: node 0 = next[r] with child -1, prior +0, links -1 / -1, stats zero; the nodes in [1, m) as above;
 *   nodes[r] = 1, kept[r] = 0: what gg_puct_begin leaves for that root.
 * Nodes >= m are not touched.  (gg_puct_begin does not write the boards of unused nodes: they are unspecified until an
 * advance zeroes them, and nothing reads the board of a node >= nodes[r].)
 * So n_x = 1 + the sum of n_c still holds in the kept tree, the new root is already evaluated (the next select scores at
 * once; root visits start at the child's n), child ids stay larger than their parent's and below nodes[r], and root r's
 * result depends on root r alone.  A kept tree may be full: selects then fall under the no-room rule above.
 * Alignment: stats must start on a 16-byte boundary - a record is read and written as one 16-byte access, as by
 * gg_puct_select_leaves / gg_puct_backup_leaves -; every other buffer needs the 4 bytes of its element type and no more
 * (rows are moved and reset with 16-byte accesses at any word address, single words up to a boundary where it matters).
 * The argument checks come before any device work, in the order above: GG_E_BADSIZE: N outside [2, 19], R < 0;
 * GG_E_BADARG: C < 1 or C = 2^31 - 1; GG_E_NULLPTR: any pointer but kept is NULL.  R = 0 is no work.
 */
int32_t gg_puct_advance(const int32_t *actions, const uint32_t *next, int64_t R, int32_t N, int32_t C, uint32_t *boards,
                        int32_t *child, float *prior, int32_t *links, gg_puct_stat *stats, int32_t *nodes, int32_t *remap,
                        int32_t *kept, void *hip_stream);

/*
 * Self-play on the kept tree: noise into the root's priors, the move drawn from the visit counts, the policy target.  The
 * tree is the one of gg_puct_* above with room for C + 1 nodes (C where I stood), on either path.  Both calls are only
 * defined outside a round (after a backup, after an advance, or before the first select), when every v = 0; both run one
 * wave per root, use no atomics and read nothing back; root r's results depend on root r alone.  The legal actions of the
 * root are those of gg_puct_select at node 0: none once its game has ended, else the pass and every point whose invalid bit
 * is clear.
 *   gg_puct_root_noise   noise float32 [R][A]; todo uint8 [R], read and written; eps float32 in [0, 1].  Root r is APPLICABLE
 *     when todo[r] != 0, node 0 is evaluated (n_0 > 0) and the root's game has not ended.  An applicable root gets, with
 *     keep = 1.0f - eps in float32 and z = noise[r][a] where NaN, negatives and -0 count as +0:
 *       a legal:    prior_0[a] = (keep * prior_0[a]) + (eps * z)
 *       a illegal:  prior_0[a] = +0
 *     the two float32 products and the one float32 sum each rounded to nearest in this order, no fused multiply-add; a sum
 *     that is NaN (0 times an infinite z or prior) is stored as the quiet NaN 0x7FC00000, which the selects count as
 *     -infinity like any NaN score; and todo[r] = 0.  Every other root keeps all its bytes and its todo value.  The noise is
 *     NOT normalised here (the rule of the priors above: a float sum would depend on its order): a Dirichlet sample over the
 *     legal actions is the caller's to make.  The todo protocol reaches both kinds of root without a host read: one call
 *     before round 0 changes the kept roots (already evaluated) and clears their todo, the same call again after round 0
 *     changes the fresh roots that round 0 has just evaluated; ended roots are never touched, and a root is changed once.
 *   gg_puct_root_policy   sample uint8 [R], NULL = all 0; rng uint64 [R], the generator of gg_rng_seed, required when sample
 *     is not NULL; actions int32 [R]; pi float32 [R][A], may be NULL; value float32 [R], may be NULL.  Per root, n_a = the
 *     visits of the child under the legal action a (0 without a child) and S = the sum of the n_a as an int32.
 *     The root's game has ended: actions[r] = -1, the pi row all +0, value[r] = +0, rng[r] untouched.  Otherwise:
 *       pi[r][a] = float(n_a) / float(S), one float32 division rounded to nearest; +0 on illegal actions; the whole row +0
 *         when S = 0.
 *       value[r] = float(s * w_0 / n_0), the float64 division first, then the conversion to float32, s = +1 if black is to
 *         move at the root (flag bit 0 clear), else -1: the root's mean value for the player to move; +0 when n_0 = 0.
 *       sample[r] = 0, or S = 0: actions[r] = the legal action of the largest n_a, ties to the lowest action; rng[r] untouched.
 *       otherwise the ply step of the sampler above: x += 0x9E3779B97F4A7C15; u = splitmix64_finalise(x);
 *         k = ((u >> 32) * S) >> 32 in 64-bit integers; actions[r] = the first legal action, ascending, whose running sum of
 *         n_a exceeds k; rng[r] = x (advanced once).
 *     So a root draws with P(a) = n_a / S up to 2^-32, and only the two rules exist - the most visits, and in proportion to
 *     the visits: the temperatures 0 and 1 of the AlphaZero schedule.  A general temperature needs pow and could not be
 *     bit-exact: it is out of scope.
 * The argument checks come before any device work, in the order above: GG_E_BADSIZE: N outside [2, 19], R < 0;
 * GG_E_BADARG: C < 1 or C = 2^31 - 1, eps outside [0, 1] or NaN (root_noise); R = 0 is no work and returns 0 before any
 * pointer is looked at; GG_E_NULLPTR: any pointer but sample, rng, pi, value is NULL, or sample is given without rng.
 */
int32_t gg_puct_root_noise(int64_t R, int32_t N, int32_t C, float eps, const float *noise, uint8_t *todo, const uint32_t *boards,
                           float *prior, const gg_puct_stat *stats, const int32_t *nodes, void *hip_stream);
int32_t gg_puct_root_policy(int64_t R, int32_t N, int32_t C, const uint8_t *sample, uint64_t *rng, const uint32_t *boards,
                            const int32_t *child, const gg_puct_stat *stats, const int32_t *nodes, int32_t *actions, float *pi,
                            float *value, void *hip_stream);

/*
 * Network input planes with per-group liberty counts: what an evaluator of gg_puct_* is fed, from byte planes or from the
 * tracked leaf boards, in one launch.  A GROUP is a maximal orthogonally connected set of stones of one colour, its
 * LIBERTIES are the distinct empty points orthogonally adjacent to any of its stones.  OWN = the player to move (plane 2 /
 * flag bit 0), OPPONENT = the other colour.  F = gg_feature_planes() = 16 planes per board, out [B][16][N][N], every
 * element exactly 0 or 1:
 *    0       own stone
 *    1       opponent stone
 *    2 - 5   own stone whose group has exactly 1 / exactly 2 / exactly 3 / >= 4 liberties (a stone of a hand-made group
 *            without liberties sets none of them)
 *    6 - 9   the same for opponent stones
 *   10       legal point: empty, plane 3 (invalid) clear, game not over
 *   11       ko point: empty, plane 3 set, game not over, and some orthogonally adjacent OPPONENT group has exactly one
 *            liberty (this point) - the ko is the only reason the rules refuse a capturing move (gym_go/gogame.py:72-75),
 *            so this tells it from suicide
 *   12       capturing point: plane 10 set and some adjacent opponent group has exactly one liberty
 *   13       every point, iff the mover is black
 *   14       every point, iff the previous move was a pass
 *   15       every point
 * Plane 3 of the input (the invalid row set of a tracked board) is taken as given, not recomputed.  Every group is counted
 * by a flood of its own whatever the input form - the class rows of a tracked board are not read - so
 * gg_batch_features_tracked of gg_batch_track_states(s) equals gg_batch_features(s) bit for bit.
 *   gg_batch_group_liberties   libs uint8 [B][N][N] = the number of liberties of the group of the stone at each point,
 *                              saturated at 255; 0 at empty points.  The per-group counterpart of gogame.liberties /
 *                              num_liberties (gym_go/gogame.py:231-262), which count per colour.
 *   gg_batch_features          states uint8 [B][6][N][N] -> out [B][16][N][N] of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16
 *                              or GG_FEAT_U8 (0 and 1 are exact in all four)
 *   gg_batch_features_tracked  the same from tracked boards uint32 [B][gg_tracked_words(N)]
 * out must be 16-byte aligned (a board's planes are a multiple of 16 bytes long: every store is an aligned 16-byte store;
 * GG_E_BADARG otherwise).  Checks as gg_batch_eye_mask: GG_E_BADSIZE for N outside [2, 19], B < 0 or an out_dtype other
 * than the four; B = 0 is no work; GG_E_NULLPTR.  Every call queues one launch on hip_stream and never synchronises.
 */
#define GG_FEAT_U8 3 /* uint8 elements (after GG_W_F32 / GG_W_BF16 / GG_W_F16) */
int32_t gg_feature_planes(void);
int32_t gg_batch_group_liberties(const uint8_t *states, uint8_t *libs, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_features(const uint8_t *states, void *out, int32_t out_dtype, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_features_tracked(const uint32_t *tracked, void *out, int32_t out_dtype, int64_t B, int32_t N, void *hip_stream);

/*
 * Symmetry-aware network input and output: the planes a network reads in one of the eight orientations of
 * gg_batch_symmetry, vectors over the actions turned forward and back, and the draw of the orientations.  Orientation o:
 * bit 0 flips the columns, then bit 1 flips the rows, then bit 2 rotates by 90 degrees; only o & 7 is read.
 *
 *   gg_batch_features_oriented / gg_batch_features_tracked_oriented    orient int32 [B]
 *     out[b] is view orient[b] of gg_batch_features(states)[b] (gg_batch_features_tracked(tracked)[b]): every one of the
 *     sixteen planes turned alike, as gg_batch_symmetry turns a uint8 image of sixteen channels.  All sixteen planes are
 *     geometric, plane 3 of the input is taken as given and the ko point moves with the board, so out[b] is ALSO
 *     gg_batch_features of the turned position: of gg_batch_symmetry(states, orient)[b], and of
 *     gg_batch_symmetry_rows(tracked, 5, orient)[b].  The inputs are not changed.  One launch: the boards are turned in
 *     registers after the load.  Checks: those of gg_batch_features, the same codes in the same order, GG_E_NULLPTR also
 *     for orient.
 *
 *   gg_batch_symmetry_policy    in, out: [B][A] elements of elem_size bytes, A = N*N + 1; orient int32 [B]
 *     Rows over the actions - priors, legal masks, visit-count targets - moved as bit patterns (elem_size 1, 2 or 4: bool,
 *     uint8, float16, bfloat16, float32, int32; NaN payloads survive).  With T(a) = the action that marks on view
 *     orient[b] the point action a marks on the board (the pass stays the pass):
 *       inverse == 0:  out[b][T(a)] = in[b][a]   - the first N*N elements turned as a one-plane image by gg_batch_symmetry's
 *                                                  rule, element N*N kept: a vector over the board becomes one over the view
 *       inverse != 0:  out[b][a] = in[b][T(a)]   - a vector over the view comes back to the board
 *     in and out must not overlap; neither needs any alignment (every access to memory is an aligned 16-byte access or a
 *     single byte inside the rows).  GG_E_BADSIZE for N outside [2, 19], B < 0 or an elem_size other than 1, 2, 4; B = 0 is
 *     no work; GG_E_NULLPTR.  One launch.
 *
 *   gg_batch_draw_orient        rng uint64 [B] (gg_rng_seed's generator), orient int32 [B]
 *     orient[b] = u >> 61 with u the generator's next output - one ply step, rng[b] advances once: gg_puct_root_policy's
 *     draw ((u >> 32) * S) >> 32 with S = 8.  GG_E_BADSIZE for B < 0; B = 0 is no work; GG_E_NULLPTR.  One launch.
 * Every call queues its launch on hip_stream and never synchronises.
 */
int32_t gg_batch_features_oriented(const uint8_t *states, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                                   void *hip_stream);
int32_t gg_batch_features_tracked_oriented(const uint32_t *tracked, const int32_t *orient, void *out, int32_t out_dtype, int64_t B,
                                           int32_t N, void *hip_stream);
int32_t gg_batch_symmetry_policy(const void *in, const int32_t *orient, void *out, int32_t elem_size, int32_t inverse, int64_t B,
                                 int32_t N, void *hip_stream);
int32_t gg_batch_draw_orient(uint64_t *rng, int32_t *orient, int64_t B, void *hip_stream);

/*
 * Pass-alive (Benson) life planes: the stones that can never be captured, whatever the opponent plays and even
 * if their owner always passes, and the points they decide - exact, all integers and sets, no reading.  For a colour X:
 * S = the points holding a stone of X, O = the other colour's stones, E = the empty points; adjacency is orthogonal and on
 * the board.  CHAINS are the connected components of S, REGIONS the connected components of the complement of S (E and O
 * together).  A region r is VITAL to a chain c when r contains an empty point and every empty point of r is adjacent to a
 * stone of c (a region without an empty point is vital to nothing); r BORDERS c when some point of r is adjacent to a
 * stone of c.  Start with A = all chains and Q = all regions and repeat until neither changes:
 *   1. drop from A every chain with fewer than two regions of Q vital to it;
 *   2. drop from Q every region that borders a chain of X not in A.
 * alive(X) = the stones of the chains left in A; safe(X) = the points (empty or O) of every region left in Q that is vital
 * to at least one chain left in A; both empty when X has no stones.  Only planes 0, 1 and 2 of a state are read (of a
 * tracked board: the two stone row sets and the turn flag): an ended game gets its planes like any other, a hand-made chain
 * without liberties simply follows the definition.  L = gg_life_planes() = 4 planes per board, out [B][4][N][N], every
 * element exactly 0 or 1, OWN = the player to move:
 *    0  alive(own)      1  alive(opponent)      2  safe(own)      3  safe(opponent)
 * settled (NULL, or uint8 [B]): settled[b] = 1 iff every point of board b lies in plane 0 | 1 | 2 | 3, else 0 (the empty board
 * is not settled).  orient (NULL, or int32 [B], only orient[b] & 7 is read; gg_batch_symmetry's orientations): out[b] is view
 * orient[b] of the unoriented result, which is also the result of the turned position; settled does not depend on it.
 *   gg_batch_life           states uint8 [B][6][N][N] -> out of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8
 *   gg_batch_life_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                           gg_batch_track_states(s) and s
 * out needs the alignment of its element only (4 N^2 elements are no multiple of 16 bytes for odd N in uint8): the stores
 * are aligned 16-byte vectors inside a wave's slice of out and single elements at its two ragged ends; nothing outside
 * out [B][4][N][N] and settled [B] is written.  Checks, in this order: GG_E_BADSIZE for N outside [2, 19], B < 0 or an
 * out_dtype other than the four; B = 0 is no work and returns 0; GG_E_NULLPTR for a NULL input or out; GG_E_BADARG for an
 * out not aligned to its element size.  Every call queues ONE launch on hip_stream and never synchronises.
 */
int32_t gg_life_planes(void);
int32_t gg_batch_life(const uint8_t *states, const int32_t *orient, void *out, uint8_t *settled, int32_t out_dtype, int64_t B,
                      int32_t N, void *hip_stream);
int32_t gg_batch_life_tracked(const uint32_t *tracked, const int32_t *orient, void *out, uint8_t *settled, int32_t out_dtype,
                              int64_t B, int32_t N, void *hip_stream);

/*
 * Ladder planes: the first tactical fact that needs reading - a bounded search per board, all integers and
 * sets, bit-exact against tests/ladder_expect.py.
 * TERMS.  Colours, chains and liberties as for the feature planes; points are ordered row-major.  The PREY is a chain, the
 * DEFENDER its colour, the ATTACKER the other colour.  A search is a sequence of legal moves on a copy of the position:
 * captures as in the rules (the opponent chains next to the played stone that are left without a liberty go first); a
 * move is legal when the point is empty, is not the current ko point and, after captures, the played stone's chain has a
 * liberty; a move that captures exactly one stone and whose own chain is then that single stone with exactly one liberty
 * makes the captured point the ko point for the next move only.  At the root the ko point of the position (plane 11 of the
 * feature planes) applies exactly when the first player of the search is the player to move, otherwise there is none.
 * NODE D(pos, c): the defender moves, c has exactly one liberty L.  Options, in order: 1. L; 2. the sole liberty of each
 * attacker chain adjacent to c that has exactly one liberty - distinct points in row-major order, L skipped.  A legal
 * option leaves the chain c' that holds c's stones with n liberties: n >= 3: the option escapes; n <= 1: it fails;
 * n == 2: it escapes iff A(pos', c') is false.  D is true (captured) iff no option escapes; evaluation stops at the first.
 * NODE A(pos, c): the attacker moves, c has exactly two liberties L1 < L2.  For each Li in order that is legal for the
 * attacker the option works iff D(pos', c) is true.  A is true iff some option works; evaluation stops at the first.
 * BOUNDS.  Every entry into D or A counts one node; its depth is the number of moves played on the copy.  A root query that
 * would enter a node at depth > GG_LADDER_DEPTH(N) = 4 N, or a node beyond number GG_LADDER_NODES(N) = 16 N, is ABORTED:
 * its answer is "not captured" for an attacker query and "escapes" for a defender query, whatever had been found.  (The
 * principal line of a ladder across the board's diagonal is below 4 N plies; a wrong atari costs about two nodes before the
 * prey has three liberties, so 16 N leaves a factor above the clean ladder and bounds the launch.)  The evaluation order is
 * part of the definition: it decides what an aborted query had counted.
 * ROOT QUERIES, one budget each, independent of one another.  For every chain c with exactly two liberties and each Li:
 * work(c, Li) iff Li is legal for the attacker and D of the resulting position is true (false if aborted).  For every chain
 * c with exactly one liberty and each option o of D: esc(c, o) iff o is legal and escapes (true if aborted).
 * laddered(c): some work(c, Li) for a two-liberty chain, no esc(c, o) for a one-liberty chain; chains with none or with three
 * and more liberties never.  Whose turn it is does not enter but through the root ko.
 * out [B][GG_LADDER_PLANES][N][N], every element exactly 0 or 1, OWN = the player to move:
 *    0  own stones of laddered chains             1  opponent stones of laddered chains
 *    2  ladder captures: the points Li with work(c, Li) for an opponent two-liberty chain c
 *    3  ladder escapes: the points o with esc(c, o) for an own one-liberty chain c
 * A board whose game is over gets planes 2 and 3 clear.  aborted (NULL, or uint8 [B]): min(aborted root queries of the
 * board, 255).  orient (NULL, or int32 [B], only orient[b] & 7 is read; gg_batch_symmetry's orientations): out[b] and
 * aborted[b] are those of the TURNED position - turned first, then searched (the planes are geometric up to the row-major
 * tie-breaks, which only matter inside aborted queries).
 *   gg_batch_ladder           states uint8 [B][6][N][N] -> out of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 / GG_FEAT_U8
 *   gg_batch_ladder_tracked   the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                             gg_batch_track_states(s) and s
 * Alignment, stores and the checks with their order and codes: gg_batch_life's.  Every call queues ONE launch on hip_stream
 * and never synchronises; no global atomics.
 */
#define GG_LADDER_PLANES 4
#define GG_LADDER_DEPTH(N) (4 * (N))
#define GG_LADDER_NODES(N) (16 * (N))
int32_t gg_batch_ladder(const uint8_t *states, const int32_t *orient, void *out, uint8_t *aborted, int32_t out_dtype, int64_t B,
                        int32_t N, void *hip_stream);
int32_t gg_batch_ladder_tracked(const uint32_t *tracked, const int32_t *orient, void *out, uint8_t *aborted, int32_t out_dtype,
                                int64_t B, int32_t N, void *hip_stream);

/*
 * Move-outcome planes: what a move WOULD do, for every point the mover may play - exact, all integers and
 * sets, bit-exact against tests/outcome_expect.py.  Everything is from the mover's point of view; colours, chains and
 * liberties as for the feature planes.
 * A CANDIDATE is a point that is empty, has plane 3 clear, and lies on a board whose game has not ended: exactly the legal
 * plane (plane 10) of gg_batch_features.  For a candidate p, from the stones alone (planes 0 and 1; of a tracked board
 * the two stone row sets - its class rows are not read):
 *   1. put a stone of the mover on p;
 *   2. remove every opponent chain that now has no liberty: captured(p) = the number of stones removed;
 *   3. take the chain that contains p: libs(p) = the number of its liberties, size(p) = the number of its stones;
 *   4. if libs(p) == 0 (a suicide: it is a candidate only when the caller's plane 3 is not the true mask), then
 *      libs(p) = captured(p) = size(p) = 0.
 * At every point that is no candidate all three are 0.  The position is assumed to hold no chain without liberties; what a
 * point next to such a chain gets is not specified (as for the ladder planes).
 *   gg_batch_move_counts          states uint8 [B][6][N][N] -> out uint8 [B][GG_MOVE_COUNTS][N][N] =
 *                                 min(libs, 255), min(captured, 255), min(size, 255)
 *   gg_batch_move_planes          states -> out [B][GG_MOVE_PLANES][N][N] of out_dtype: GG_W_F32 / GG_W_BF16 / GG_W_F16 /
 *                                 GG_FEAT_U8, every element exactly 0 or 1:
 *                                    0 -  3  libs     == 1 / == 2 / == 3 / >= 4
 *                                    4 -  7  captured == 1 / == 2 / == 3 / >= 4
 *                                    8 - 11  libs == 1 and size == 1 / == 2 / == 3 / >= 4: a self-atari, by the size of the
 *                                            chain it puts into atari
 *   gg_batch_move_planes_tracked  the same from tracked boards uint32 [B][gg_tracked_words(N)]: the same bytes for
 *                                 gg_batch_track_states(s) and s
 * orient (NULL, or int32 [B], only orient[b] & 7 is read; gg_batch_symmetry's orientations): the planes are geometric, so
 * out[b] is view orient[b] of the unoriented result and also the result of the turned position; the board is turned in
 * registers after the load.  Alignment (out needs that of its element only), stores and the checks with their order and
 * codes: gg_batch_life's.  Every call queues ONE launch on hip_stream and never synchronises; no global atomics.
 */
#define GG_MOVE_PLANES 12
#define GG_MOVE_COUNTS 3
int32_t gg_batch_move_planes(const uint8_t *states, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                             void *hip_stream);
int32_t gg_batch_move_planes_tracked(const uint32_t *tracked, const int32_t *orient, void *out, int32_t out_dtype, int64_t B,
                                     int32_t N, void *hip_stream);
int32_t gg_batch_move_counts(const uint8_t *states, uint8_t *out, int64_t B, int32_t N, void *hip_stream);

/*
 * Position hashes and positional superko: a 64-bit Zobrist hash of every board, the hash of the position after
 * every move of the mover without building the child, and the moves that would recreate a position of the board's history.
 * THE KEYS.  key(c, y, x), c = 0 black / 1 white, 0 <= y, x < 19, is output number i + 1, i = c * 361 + y * 19 + x, of the
 * splitmix64 generator (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; output z ^ z >> 31) started at state GG_HASH_SEED.  They do not depend on N; the
 * 722 keys are distinct and non-zero; key(0, 0, 0) = 0xc8a43d929c6a465e, key(1, 18, 18) = 0x345c2fd1bcdda841.  The library
 * holds them as a constant table of its code object: there is no initialisation call and no state.
 * THE POSITION HASH.  hash(position) = the XOR of key(colour, y, x) over its stones, as int64.  It is POSITIONAL: the turn, the
 * pass, ko and game-over flags do not enter, and the empty board hashes to 0.
 * THE MOVE HASHES.  move_hash(position, a) for a in [0, N*N]: for a CANDIDATE point (empty, plane 3 clear, game not over: the
 * candidates of the move-outcome planes) the hash of the position after the mover plays there and the opponent chains left
 * without a liberty are removed (the played chain itself is never removed); for the pass and every point that is no
 * candidate, hash(position).  Every slot is written.  The position is assumed to hold no chain without liberties; of a
 * tracked board the class rows ARE read (they say which opponent stones are in atari) and must belong to the position.
 * THE REPEAT MASK.  history int64 [B][H], count int32 [B]: board b's valid entries are its first min(max(count[b], 0), H).
 * repeat[b][a] = 1 iff a is a candidate point and move_hash(b, a) equals a valid entry, else 0; the pass is never a repeat.
 * Equal 64-bit hashes are TAKEN AS equal positions: two different positions collide with probability about 2^-64 per
 * comparison, and a collision forbids a legal move; it never allows a repetition.
 *   gg_batch_hash                 states uint8 [B][6][N][N] -> out int64 [B]
 *   gg_batch_hash_tracked         the same from tracked boards uint32 [B][gg_tracked_words(N)]
 *   gg_batch_move_hashes          states -> any of hashes int64 [B][N*N+1], repeat uint8 [B][N*N+1] and rows uint32 [B][N]
 *                                 (the repeat points as row masks, bit x of rows[b][y]: the form a tracked board's invalid
 *                                 rows take); each may be NULL, not all three
 *   gg_batch_move_hashes_tracked  the same from tracked boards
 * history and count may be NULL only when repeat and rows both are; they are not read then.  Checks, in this order and
 * before any device work: N outside [2, 19] or B < 0 -> GG_E_BADSIZE; H < 0 -> GG_E_BADARG; B == 0 -> 0; the boards, every
 * output, or a needed history / count NULL -> GG_E_NULLPTR; out / hashes / history not 8-byte aligned, rows / count not
 * 4-byte aligned -> GG_E_BADARG.  Every call queues ONE launch on hip_stream and never synchronises; no global atomics; every
 * store lies inside the outputs' B rows.
 */
#define GG_HASH_SEED 0x676F2D6861736821ull
int32_t gg_batch_hash(const uint8_t *states, int64_t *out, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_hash_tracked(const uint32_t *tracked, int64_t *out, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_move_hashes(const uint8_t *states, const int64_t *history, const int32_t *count, int32_t H, int64_t *hashes,
                             uint8_t *repeat, uint32_t *rows, int64_t B, int32_t N, void *hip_stream);
int32_t gg_batch_move_hashes_tracked(const uint32_t *tracked, const int64_t *history, const int32_t *count, int32_t H,
                                     int64_t *hashes, uint8_t *repeat, uint32_t *rows, int64_t B, int32_t N, void *hip_stream);

/*
 * Positional superko AT EVERY NODE of a PUCT tree: one launch between gg_batch_play_moves_tracked and the
 * evaluation of a round's leaves.  THE RULE: at node y of root r's tree a board move a is illegal if the position after a has
 * the hash of a valid entry of game r's history, or of the position of any node on the parent chain of y, from y's parent up
 * to node 0.  Equality is that of the 64-bit hashes (above); the pass is never forbidden; a node whose game has ended has no
 * candidates.  The tree is a tree, so a node's chain never changes: the rule is applied ONCE, when the node is made - the
 * forbidden points are ORed into the invalid rows of the new node's tracked board before it is evaluated and stored, and
 * select, gg_puct_legal, the prior mask of the first evaluation, the feature planes, gg_puct_root_policy and
 * gg_puct_root_noise, which all read legality from the board, follow.  After gg_puct_advance the marks of a kept node stay
 * right: it was marked against (old history + its old chain), and that set equals (new history + its new chain) as long as the
 * history has dropped no entry - the old root and the node under the action played have moved from the chain into the history.
 * links int32 [R][C+1][2]: the tree's own.  node_hash int64 [R][C+1]: the position hash of every evaluated node.  history int64
 * [R][H], count int32 [R]: the repeat mask's (root r's valid entries are its first min(max(count[r], 0), H)); both may be NULL
 * - no game history, H is ignored -, one alone may not.  leaf uint32 [R*L][W], move and leaf_id int32 [R*L]: the outputs of the
 * select launch AFTER gg_batch_play_moves_tracked; the one-leaf path passes L = 1.  Row i belongs to root r = i / L; y =
 * leaf_id[i], m = move[i]:
 *   y < 1, y > C or m < 0   the row is SKIPPED: no byte of leaf[i] and no entry of node_hash is written (an empty slot, a node
 *                           evaluated again - its board carries its marks already -, the root of round 0 - that is
 *                           gg_batch_move_hashes_tracked's `rows` -, a select without room);
 *   otherwise               node_hash[r][y] = hash(leaf[i]), and every candidate point of leaf[i] (empty, invalid bit clear,
 *                           game not over) whose move hash is in the forbidden set gets its bit set in words [2N, 3N) of
 *                           leaf[i].  The forbidden set: the valid entries of history[r] and node_hash[r][x] for x =
 *                           parent(y), parent(parent(y)), .. down to node 0.  No other word of leaf changes.
 * THE WALK IS BOUNDED: it goes on only while the parent p of x satisfies 0 <= p < x, and takes at most C steps - corrupt links
 * can neither loop nor leave root r's slice of links and node_hash.
 * WHO FILLS node_hash: the caller fills node_hash[r][0] (gg_batch_hash_tracked of the roots), and after gg_puct_advance the
 * entries of the kept nodes (one gg_batch_hash_tracked over the boards buffer does both).  The launch reads node_hash only at
 * ancestors, which are evaluated nodes of earlier rounds, and writes it only at nodes made in this round; such a node is never
 * on another slot's path (collision rule a of gg_puct_select_leaves), and an ended node that several slots take has m = -1
 * and is skipped: the slots of one root do not race.
 * Checks, in this order and before any device work: N outside [2, 19] or R < 0 -> GG_E_BADSIZE; C < 1, C = 2^31 - 1, L < 1,
 * L > C or H < 0 -> GG_E_BADARG; R == 0 -> 0; a NULL pointer other than the history pair, or exactly one of the pair NULL ->
 * GG_E_NULLPTR; node_hash or history not 8-byte aligned, any other buffer not 4-byte aligned -> GG_E_BADARG.  ONE launch on
 * hip_stream, no synchronisation, no global atomics; every store is a vector store inside the rows named above.
 */
int32_t gg_puct_superko(int64_t R, int32_t N, int32_t C, int32_t L, const int32_t *links, int64_t *node_hash,
                        const int64_t *history, const int32_t *count, int32_t H, uint32_t *leaf, const int32_t *move,
                        const int32_t *leaf_id, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMGO_AMD_H */
