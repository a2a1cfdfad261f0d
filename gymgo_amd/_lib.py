"""ctypes loader of the in-tree HIP library (gymgo_amd/libgymgo_amd.so) + tensor plumbing.

There is NO CPU fallback: if the shared library is missing, or a tensor is not a contiguous
ROCm device tensor of the dtype its parameter takes, the call raises.  PyTorch is used only for device
memory and the current HIP stream; every entry point of include/gymgo_amd.h is bound here with plain
pointers, from ONE table (ABI) that tests/test_host_abi.py holds against the header, and reached through
call().  A new entry point is one declaration in the header and one entry in the table.  The area family has a header of
its own, include/gymgo_amd_area.h, and a table of its own, ABI_AREA, bound and called the same way; so have the past family
(include/gymgo_amd_past.h, ABI_PAST), the Gumbel root rule of the PUCT search (include/gymgo_amd_gumbel.h, ABI_GUMBEL), the
tactical playout policy with its planes (include/gymgo_amd_tactics.h, ABI_TACTICS), the AMAF statistics of the playouts with
RAVE in the UCT search (include/gymgo_amd_amaf.h, ABI_AMAF), the pattern playout policy with its planes
(include/gymgo_amd_pattern.h, ABI_PATTERN), the move priors of the RAVE search (include/gymgo_amd_prior.h, ABI_PRIOR), stone
status with the final score from playout ownership (include/gymgo_amd_status.h, ABI_STATUS) and the UCT search with several
leaves per root and round (include/gymgo_amd_uct_leaves.h, ABI_UCT_LEAVES).  ABI_ALL is the ten merged: the one lookup lib(),
call(), ptrs() and PARAMS (the parameter names of every entry point, in order) are made from.
"""
import collections
import ctypes
import os
import threading

import torch  # must be imported before the library so both share ONE HIP runtime (libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgymgo_amd.so')   # always the in-tree build: no override, no search path
ABI_VERSION = 5                                      # GG_ABI_VERSION of include/gymgo_amd.h

Param = collections.namedtuple('Param', 'name kind')
Param.__doc__ = """One parameter of an entry point, under the name include/gymgo_amd.h gives it.  kind: the ctypes type of a scalar
(c_void_p for hip_stream), or - a pointer to device memory - the torch dtype a tensor passed there must have, or a tuple of
them where the header says `void *` / `uint8_t *` and the entry point takes several."""

_vp, _i32, _i64, _u64, _f32, _f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double
_U8, _I32, _I64, _F32 = torch.uint8, torch.int32, torch.int64, torch.float32     # uint32_t * / uint64_t * are int32 / int64 tensors
_PLANES = (torch.float32, torch.bfloat16, torch.float16, torch.uint8)           # GG_W_* / GG_FEAT_U8 outputs
_WEIGHTS = (torch.float32, torch.bfloat16, torch.float16)                       # GG_W_*
_ROWS = (torch.bool, torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.int32)   # elem_size 1, 2, 4
_FLAGS = (torch.bool, torch.uint8)


def _params(kind, *names):
    return tuple(Param(n, kind) for n in names)


# parameter runs that several entry points share, as the header spells them
_STREAM = _params(_vp, 'hip_stream')
_BN = _params(_i64, 'B') + _params(_i32, 'N') + _STREAM
_BNC = _params(_i64, 'B') + _params(_i32, 'N', 'canonical') + _STREAM
_BNT = _params(_i64, 'B') + _params(_i32, 'N', 'T') + _STREAM
_ROLL = _params(_I64, 'rng') + _params(_I32, 'last_actions') + _params(_I64, 'steps_done')
_PLIES = _params(_i64, 'B') + _params(_i32, 'N', 'plies', 'auto_reset')
_STEP = (_params(_I32, 'actions') + _params(_I64, 'rng') + _params(_F32, 'rewards') + _params(_U8, 'dones')
         + _params(_I32, 'status', 'taken_actions'))
_REWARD = _params(_i64, 'B') + _params(_i32, 'N') + _params(_f32, 'komi') + _params(_i32, 'reward_method', 'auto_reset') + _STREAM
_OUT = _params(_PLANES, 'out')
_OUT_BN = _params(_i32, 'out_dtype') + _BN
_WEIGHTED = _params(_WEIGHTS, 'weights') + _params(_i32, 'weight_dtype')
_JOBS = (_params(_i64, 'R') + _params(_i32, 'N', 'K') + _params(_i64, 'first_root') + _params(_u64, 'base_seed')
         + _params(_i32, 'max_plies', 'chunk_plies'))
_MOVE_JOBS = (_params(_i64, 'R') + _params(_i32, 'N') + _params(_I32, 'plan') + _params(_i64, 'T') + _params(_i32, 'K')
              + _params(_i64, 'first_root') + _params(_u64, 'base_seed') + _params(_i32, 'max_plies', 'chunk_plies'))
_CHUNKS = _params(_f32, 'komi') + _params(_i32, 'chunks')
_QUEUE = (_params(_I32, 'slots') + _params(_I64, 'rng', 'plies', 'job') + _params(_i64, 'S') + _params(_I64, 'counter')
          + _params(_I32, 'counts') + _params(_I64, 'sums'))
_OWN = _params(_I32, 'ownership') + _STREAM
_LEAF = _params(_I32, 'leaf', 'move', 'leaf_id') + _STREAM
_RNI = _params(_i64, 'R') + _params(_i32, 'N', 'I')
_RNC = _params(_i64, 'R') + _params(_i32, 'N', 'C')
_PUCT_TREE = (_params(_I32, 'boards', 'child') + _params(_F32, 'prior') + _params(_I32, 'links', 'stats', 'nodes'))   # gg_puct_stat: 4 words
_PUCT_BACK = (_params(_f32, 'komi') + _params(_F32, 'priors', 'values') + _params(_I32, 'boards') + _params(_F32, 'prior')
              + _params(_I32, 'links', 'stats') + _LEAF)

_MOVE_HASHES = (_params(_I64, 'history') + _params(_I32, 'count') + _params(_i32, 'H') + _params(_I64, 'hashes')
                + _params(_U8, 'repeat') + _params(_I32, 'rows') + _BN)

# THE description of the C ABI on the Python side: one entry per function of include/gymgo_amd.h, in header order, one Param
# per parameter.  EXPORTS, the ctypes argtypes lib() sets and the marshalling of call() all come from here.
ABI = {
    'gg_version': (),
    'gg_device_cus': (),
    'gg_batch_next_states': _params(_U8, 'in') + _params(_I32, 'actions') + _params(_U8, 'out') + _params(_I32, 'status') + _BNC,
    'gg_batch_next_states_ws': (_params(_U8, 'in') + _params(_I32, 'actions') + _params(_U8, 'out')
                                + _params(_I32, 'status', 'workspace') + _BNC),
    'gg_batch_invalid_mask': _params(_U8, 'states') + _params(_I32, 'ko') + _params(_U8, 'mask') + _BN,
    'gg_batch_areas': _params(_U8, 'states') + _params(_I32, 'black', 'white') + _BN,
    'gg_batch_children': _params(_U8, 'states', 'children') + _BNC,
    'gg_batch_children_offsets': _params(_U8, 'states') + _params(_I32, 'offsets', 'order') + _BN,
    'gg_batch_children_compact': _params(_U8, 'states') + _params(_I32, 'offsets', 'order') + _params(_U8, 'children') + _BNC,
    'gg_batch_rollout': _params(_U8, 'states') + _ROLL + _PLIES + _STREAM,
    'gg_batch_rollout_ws': _params(_U8, 'states') + _ROLL + _params(_I32, 'workspace') + _PLIES + _STREAM,
    'gg_batch_env_step': _params(_U8, 'states') + _STEP + _REWARD,
    'gg_batch_env_step_scored': _params(_U8, 'states') + _STEP + _params(_I32, 'areas') + _REWARD,
    'gg_batch_sample_actions': _params(_U8, 'states') + _params(_I64, 'rng') + _params(_I32, 'actions') + _BN,
    'gg_batch_update_pieces': (_params(_U8, 'states') + _params(_I32, 'adj') + _params(_i32, 'K') + _params(_I32, 'players')
                               + _params(_U8, 'killed') + _BN),
    'gg_batch_reset_finished': _params(_U8, 'states') + _BN,
    'gg_packed_words': _params(_i32, 'N'),
    'gg_batch_pack_states': _params(_U8, 'states') + _params(_I32, 'packed') + _BN,
    'gg_batch_unpack_states': _params(_I32, 'packed') + _params(_U8, 'states') + _BN,
    'gg_batch_next_states_packed': _params(_I32, 'in', 'actions', 'out', 'status') + _BNC,
    'gg_batch_rollout_packed': _params(_I32, 'packed') + _ROLL + _PLIES + _STREAM,
    'gg_batch_env_step_packed': _params(_I32, 'packed') + _STEP + _REWARD,
    'gg_batch_children_packed': _params(_I32, 'packed', 'children') + _BNC,
    'gg_batch_play_moves': _params(_U8, 'states') + _params(_I32, 'moves', 'played') + _BNT,
    'gg_batch_play_moves_packed': _params(_I32, 'packed', 'moves', 'played') + _BNT,
    'gg_tracked_words': _params(_i32, 'N'),
    'gg_batch_track_states': _params(_U8, 'states') + _params(_I32, 'tracked') + _BN,
    'gg_batch_untrack_states': _params(_I32, 'tracked') + _params(_U8, 'states') + _BN,
    'gg_batch_rollout_tracked': _params(_I32, 'tracked') + _ROLL + _PLIES + _STREAM,
    'gg_batch_play_moves_tracked': _params(_I32, 'tracked', 'moves', 'played') + _BNT,
    'gg_batch_env_step_tracked': (_params(_I32, 'tracked') + _STEP + _params(_U8, 'states_out') + _params(_I64, 'steps_done')
                                  + _REWARD),
    'gg_batch_env_step_tracked_weighted': (_params(_I32, 'tracked') + _WEIGHTED + _STEP[1:] + _params(_U8, 'states_out')
                                           + _params(_I64, 'steps_done') + _REWARD),
    'gg_batch_sample_weighted': _params(_U8, 'states') + _WEIGHTED + _params(_I64, 'rng') + _params(_I32, 'actions') + _BN,
    'gg_batch_sample_weighted_rows': (_params(_I32, 'boards') + _params(_i32, 'planes') + _WEIGHTED + _params(_I64, 'rng')
                                      + _params(_I32, 'actions') + _BN),
    'gg_batch_symmetry': (_params(_U8, 'in') + _params(_I32, 'orient') + _params(_U8, 'out') + _params(_i64, 'B')
                          + _params(_i32, 'C', 'N') + _STREAM),
    'gg_batch_symmetry_rows': _params(_I32, 'in') + _params(_i32, 'planes') + _params(_I32, 'orient', 'out') + _BN,
    'gg_rng_seed': _params(_I64, 'rng') + _params(_u64, 'base_seed') + _params(_i64, 'first_game', 'B') + _STREAM,
    'gg_playouts_begin': _params(_I32, 'roots') + _JOBS + _QUEUE + _OWN,
    'gg_playouts_advance': _params(_I32, 'roots') + _JOBS + _CHUNKS + _QUEUE + _OWN,
    'gg_move_playouts_plan': (_params(_I32, 'roots') + _params(_i64, 'R') + _params(_i32, 'N') + _params(_I32, 'offsets', 'plan')
                              + _STREAM),
    'gg_move_playouts_begin': _params(_I32, 'roots') + _MOVE_JOBS + _QUEUE + _STREAM,
    'gg_move_playouts_advance': _params(_I32, 'roots') + _MOVE_JOBS + _CHUNKS + _QUEUE + _STREAM,
    'gg_uct_begin': (_params(_I32, 'roots') + _RNI + _params(_i32, 'K') + _params(_I32, 'boards', 'child', 'links', 'stats', 'nodes')
                     + _STREAM),
    'gg_uct_select': (_RNI + _params(_i32, 'K') + _params(_f64, 'c') + _params(torch.float64, 'log_table')
                      + _params(_I32, 'boards', 'child', 'links', 'stats', 'nodes') + _LEAF),
    'gg_uct_backup': (_RNI + _params(_i32, 'K') + _params(_I32, 'counts') + _params(_I64, 'sums', 'totals')
                      + _params(_I32, 'boards', 'links', 'stats') + _LEAF),
    'gg_batch_eye_mask': _params(_U8, 'states', 'mask') + _BN,
    'gg_batch_rollout_tracked_policy': _params(_I32, 'tracked') + _ROLL + _PLIES + _params(_i32, 'policy') + _STREAM,
    'gg_playouts_advance_policy': _params(_I32, 'roots') + _JOBS + _CHUNKS + _params(_i32, 'policy') + _QUEUE + _OWN,
    'gg_move_playouts_advance_policy': _params(_I32, 'roots') + _MOVE_JOBS + _CHUNKS + _params(_i32, 'policy') + _QUEUE + _STREAM,
    'gg_puct_begin': _params(_I32, 'roots') + _RNI + _PUCT_TREE + _STREAM,
    'gg_puct_select': _RNI + _params(_f64, 'c') + _PUCT_TREE + _LEAF,
    'gg_puct_backup': _RNI + _PUCT_BACK,
    'gg_puct_select_leaves': _RNC + _params(_i32, 'L') + _params(_f64, 'c') + _PUCT_TREE + _LEAF,
    'gg_puct_backup_leaves': _RNC + _params(_i32, 'L') + _PUCT_BACK,
    'gg_puct_legal': (_params(_I32, 'leaf', 'leaf_id') + _params(_i64, 'B') + _params(_i32, 'N') + _params(torch.bool, 'legal', 'live')
                      + _STREAM),
    'gg_puct_advance': _params(_I32, 'actions', 'next') + _RNC + _PUCT_TREE + _params(_I32, 'remap', 'kept') + _STREAM,
    'gg_puct_root_noise': (_RNC + _params(_f32, 'eps') + _params(_F32, 'noise') + _params(_FLAGS, 'todo') + _params(_I32, 'boards')
                           + _params(_F32, 'prior') + _params(_I32, 'stats', 'nodes') + _STREAM),
    'gg_puct_root_policy': (_RNC + _params(_FLAGS, 'sample') + _params(_I64, 'rng') + _params(_I32, 'boards', 'child', 'stats', 'nodes', 'actions')
                            + _params(_F32, 'pi', 'value') + _STREAM),
    'gg_feature_planes': (),
    'gg_batch_group_liberties': _params(_U8, 'states', 'libs') + _BN,
    'gg_batch_features': _params(_U8, 'states') + _OUT + _OUT_BN,
    'gg_batch_features_tracked': _params(_I32, 'tracked') + _OUT + _OUT_BN,
    'gg_batch_features_oriented': _params(_U8, 'states') + _params(_I32, 'orient') + _OUT + _OUT_BN,
    'gg_batch_features_tracked_oriented': _params(_I32, 'tracked', 'orient') + _OUT + _OUT_BN,
    'gg_batch_symmetry_policy': (_params(_ROWS, 'in') + _params(_I32, 'orient') + _params(_ROWS, 'out')
                                 + _params(_i32, 'elem_size', 'inverse') + _BN),
    'gg_batch_draw_orient': _params(_I64, 'rng') + _params(_I32, 'orient') + _params(_i64, 'B') + _STREAM,
    'gg_life_planes': (),
    'gg_batch_life': _params(_U8, 'states') + _params(_I32, 'orient') + _OUT + _params(_U8, 'settled') + _OUT_BN,
    'gg_batch_life_tracked': _params(_I32, 'tracked', 'orient') + _OUT + _params(_U8, 'settled') + _OUT_BN,
    'gg_batch_ladder': _params(_U8, 'states') + _params(_I32, 'orient') + _OUT + _params(_U8, 'aborted') + _OUT_BN,
    'gg_batch_ladder_tracked': _params(_I32, 'tracked', 'orient') + _OUT + _params(_U8, 'aborted') + _OUT_BN,
    'gg_batch_move_planes': _params(_U8, 'states') + _params(_I32, 'orient') + _OUT + _OUT_BN,
    'gg_batch_move_planes_tracked': _params(_I32, 'tracked', 'orient') + _OUT + _OUT_BN,
    'gg_batch_move_counts': _params(_U8, 'states', 'out') + _BN,
    'gg_batch_hash': _params(_U8, 'states') + _params(_I64, 'out') + _BN,
    'gg_batch_hash_tracked': _params(_I32, 'tracked') + _params(_I64, 'out') + _BN,
    'gg_batch_move_hashes': _params(_U8, 'states') + _MOVE_HASHES,
    'gg_batch_move_hashes_tracked': _params(_I32, 'tracked') + _MOVE_HASHES,
    'gg_puct_superko': (_RNC + _params(_i32, 'L') + _params(_I32, 'links') + _params(_I64, 'node_hash', 'history')
                        + _params(_I32, 'count') + _params(_i32, 'H') + _LEAF),
}
# ... and of include/gymgo_amd_area.h, the area family's header, in its order: a table of its own, so that ABI stays the
# description of include/gymgo_amd.h alone (tests/test_area_host.py holds this one against its header the same way)
ABI_AREA = {
    'gg_area_planes': (),
    'gg_batch_area': (_params(_U8, 'states') + _params(_I32, 'orient') + _params(_FLAGS, 'side') + _OUT + _params(_I32, 'counts')
                      + _OUT_BN),
    'gg_batch_area_tracked': (_params(_I32, 'tracked', 'orient') + _params(_FLAGS, 'side') + _OUT + _params(_I32, 'counts')
                              + _OUT_BN),
}
# ... and of include/gymgo_amd_past.h, the past family's header, in its order (tests/test_past_host.py holds it against its header)
_RING = _params(_I32, 'rows', 'count') + _params(_i32, 'H')
_PAST = _RING + _params(_i32, 'T', 'moves') + _params(_I32, 'orient') + _OUT + _OUT_BN
ABI_PAST = {
    'gg_past_planes': _params(_i32, 'T', 'moves'),
    'gg_past_push': _params(_U8, 'states') + _params(_FLAGS, 'mask') + _RING + _BN,
    'gg_past_push_tracked': _params(_I32, 'tracked') + _params(_FLAGS, 'mask') + _RING + _BN,
    'gg_batch_past': _params(_U8, 'states') + _PAST,
    'gg_batch_past_tracked': _params(_I32, 'tracked') + _PAST,
    'gg_puct_past': (_RNC + _params(_i32, 'L') + _params(_I32, 'boards', 'links') + _RING + _params(_i32, 'T', 'moves')
                     + _params(_I32, 'leaf', 'leaf_id', 'orient') + _OUT + _params(_i32, 'out_dtype') + _STREAM),
}
# ... and of include/gymgo_amd_gumbel.h, the Gumbel root rule's header, in its order (tests/test_gumbel_host.py holds it against its
# header).  seq of gg_gumbel_sequence is HOST memory: call() passes the int address it is given
_GUMBEL_TREE = _params(_I32, 'child', 'stats', 'nodes')
ABI_GUMBEL = {
    'gg_gumbel_sequence': _params(_i32, 'm', 'n') + _params(_I32, 'seq'),
    'gg_gumbel_begin': _RNC + _GUMBEL_TREE + _params(_I32, 'seen', 'done') + _STREAM,
    'gg_gumbel_select_leaves': (_RNC + _params(_i32, 'L') + _params(_f64, 'c') + _PUCT_TREE + _params(_F32, 'base')
                                + _params(_I32, 'seen', 'done', 'seq') + _params(_i32, 'S') + _params(_f64, 'c_visit', 'c_scale')
                                + _LEAF),
    'gg_gumbel_root': (_RNC + _params(_I32, 'boards') + _GUMBEL_TREE + _params(_F32, 'base') + _params(_I32, 'seen')
                       + _params(_f64, 'c_visit', 'c_scale') + _params(_I32, 'actions') + _params(_F32, 'q') + _params(_I32, 'visits')
                       + _params(_F32, 'value') + _STREAM),
}
# ... and of include/gymgo_amd_tactics.h, the tactical playout policy's header, in its order (tests/test_tactics_host.py holds it
# against its header): the planes, and the three _policy calls of ABI under the names that accept GG_POLICY_TACTICAL too
ABI_TACTICS = {
    'gg_tactics_planes': (),
    'gg_batch_tactics': _params(_U8, 'states') + _params(_I32, 'orient') + _OUT + _OUT_BN,
    'gg_batch_tactics_tracked': _params(_I32, 'tracked', 'orient') + _OUT + _OUT_BN,
    'gg_batch_rollout_tracked_policy2': ABI['gg_batch_rollout_tracked_policy'],
    'gg_playouts_advance_policy2': ABI['gg_playouts_advance_policy'],
    'gg_move_playouts_advance_policy2': ABI['gg_move_playouts_advance_policy'],
}
# ... and of include/gymgo_amd_amaf.h, the AMAF / RAVE header, in its order (tests/test_amaf_host.py holds it against its header).
# uint16_t * (the move log) is an int16 tensor, as uint32_t * is an int32 one
_I16 = torch.int16
ABI_AMAF = {
    'gg_batch_rollout_tracked_log': (_params(_I32, 'tracked') + _ROLL + _params(_i64, 'B') + _params(_i32, 'N', 'plies', 'policy')
                                     + _params(_I16, 'log') + _STREAM),
    'gg_playouts_advance_amaf': (_params(_I32, 'roots') + _JOBS + _CHUNKS + _params(_i32, 'policy') + _QUEUE
                                 + _params(_I32, 'ownership') + _params(_I16, 'log') + _params(_I32, 'first') + _params(_I64, 'mark')
                                 + _params(_I32, 'amaf') + _STREAM),
    'gg_uct_select_rave': (_RNI + _params(_i32, 'K') + _params(_f64, 'c', 'rave_equiv', 'fpu') + _params(torch.float64, 'log_table')
                           + _params(_I32, 'boards', 'child', 'links', 'stats', 'node_amaf', 'nodes') + _LEAF),
    'gg_uct_backup_rave': (_RNI + _params(_i32, 'K') + _params(_I32, 'counts') + _params(_I64, 'sums') + _params(_I32, 'amaf')
                           + _params(_I64, 'totals') + _params(_I32, 'boards', 'links', 'stats', 'node_amaf') + _LEAF),
}
# ... and of include/gymgo_amd_pattern.h, the pattern playout policy's header, in its order (tests/test_pattern_host.py holds it
# against its header): the planes, and the three _policy2 calls under the names that accept GG_POLICY_PATTERN too - the two queue
# calls with the slots' previous actions in front of the stream
ABI_PATTERN = {
    'gg_pattern_planes': (),
    'gg_batch_patterns': _params(_U8, 'states') + _params(_I32, 'last', 'orient') + _OUT + _OUT_BN,
    'gg_batch_patterns_tracked': _params(_I32, 'tracked', 'last', 'orient') + _OUT + _OUT_BN,
    'gg_batch_rollout_tracked_policy3': ABI_TACTICS['gg_batch_rollout_tracked_policy2'],
    'gg_playouts_advance_policy3': ABI_TACTICS['gg_playouts_advance_policy2'][:-1] + _params(_I32, 'last') + _STREAM,
    'gg_move_playouts_advance_policy3': ABI_TACTICS['gg_move_playouts_advance_policy2'][:-1] + _params(_I32, 'last') + _STREAM,
}
# ... and of include/gymgo_amd_prior.h, the move priors of the RAVE search, in its order (tests/test_prior_host.py holds it against
# its header).  weights is DEVICE memory: int32 [12], six (visits, wins) pairs
_PRIOR_OUT = _params(_I32, 'weights', 'out') + _BN
ABI_PRIOR = {
    'gg_batch_move_priors': _params(_U8, 'states') + _params(_I32, 'last') + _PRIOR_OUT,
    'gg_batch_move_priors_tracked': _params(_I32, 'tracked', 'last') + _PRIOR_OUT,
    'gg_uct_prior_begin': _params(_I32, 'roots', 'last_actions') + _RNI + _params(_I32, 'weights', 'node_amaf') + _STREAM,
    'gg_uct_prior_expand': _RNI + _params(_I32, 'weights', 'leaf', 'move', 'leaf_id', 'node_amaf') + _STREAM,
}
# ... and of include/gymgo_amd_status.h, stone status and the final score from playout ownership, in its order
# (tests/test_status_host.py holds it against its header)
_STATUS = (_params(_FLAGS, 'side') + _params(_I32, 'own') + _params(_i32, 'playouts', 'num', 'den') + _OUT + _params(_I32, 'counts')
           + _OUT_BN)
ABI_STATUS = {
    'gg_status_planes': (),
    'gg_batch_status': _params(_U8, 'states') + _params(_I32, 'orient') + _STATUS,
    'gg_batch_status_tracked': _params(_I32, 'tracked', 'orient') + _STATUS,
}
# ... and of include/gymgo_amd_uct_leaves.h, the UCT search with several leaves per root and round, in its order
# (tests/test_uct_leaves_host.py holds it against its header): each call is its namesake's list with L behind I and - select and
# backup - virt behind nodes / behind stats or node_amaf (and lands in its namesake's checked body and kernel, with L = 1 and no
# virt from the namesake: gg_kernels.hip, gg_prior.hip)
def _with_leaves(ps, virt_after=None):
    out = []
    for p in ps:
        out.append(p)
        if p.name == 'I':
            out += _params(_i32, 'L')
        if p.name == virt_after:
            out += _params(_I32, 'virt')
    return tuple(out)


ABI_UCT_LEAVES = {
    'gg_uct_select_leaves': _with_leaves(ABI['gg_uct_select'], 'nodes'),
    'gg_uct_backup_leaves': _with_leaves(ABI['gg_uct_backup'], 'stats'),
    'gg_uct_select_leaves_rave': _with_leaves(ABI_AMAF['gg_uct_select_rave'], 'nodes'),
    'gg_uct_backup_leaves_rave': _with_leaves(ABI_AMAF['gg_uct_backup_rave'], 'node_amaf'),
    'gg_uct_prior_expand_leaves': _with_leaves(ABI_PRIOR['gg_uct_prior_expand']),
}
EXPORTS = tuple(ABI)
EXPORTS_AREA = tuple(ABI_AREA)
EXPORTS_PAST = tuple(ABI_PAST)
EXPORTS_GUMBEL = tuple(ABI_GUMBEL)
EXPORTS_TACTICS = tuple(ABI_TACTICS)
EXPORTS_AMAF = tuple(ABI_AMAF)
EXPORTS_PATTERN = tuple(ABI_PATTERN)
EXPORTS_PRIOR = tuple(ABI_PRIOR)
EXPORTS_STATUS = tuple(ABI_STATUS)
EXPORTS_UCT_LEAVES = tuple(ABI_UCT_LEAVES)
_signatures = lambda table: {f: ([p.kind if isinstance(p.kind, type) else _vp for p in ps], _i32) for f, ps in table.items()}
_SIGNATURES = _signatures(ABI)   # argtypes, restype
_SIGNATURES_AREA = _signatures(ABI_AREA)
_SIGNATURES_PAST = _signatures(ABI_PAST)
_SIGNATURES_GUMBEL = _signatures(ABI_GUMBEL)
_SIGNATURES_TACTICS = _signatures(ABI_TACTICS)
_SIGNATURES_AMAF = _signatures(ABI_AMAF)
_SIGNATURES_PATTERN = _signatures(ABI_PATTERN)
_SIGNATURES_PRIOR = _signatures(ABI_PRIOR)
_SIGNATURES_STATUS = _signatures(ABI_STATUS)
_SIGNATURES_UCT_LEAVES = _signatures(ABI_UCT_LEAVES)
# every entry point of the ten headers in ONE lookup: what lib() binds and what call(), ptrs() and the plane launches of gogame
# (PARAMS: the parameter names in order) look an entry point up in, whichever header declares it
ABI_ALL = {**ABI, **ABI_AREA, **ABI_PAST, **ABI_GUMBEL, **ABI_TACTICS, **ABI_AMAF, **ABI_PATTERN, **ABI_PRIOR, **ABI_STATUS,
           **ABI_UCT_LEAVES}
PARAMS = {f: {p.name: i for i, p in enumerate(ps)} for f, ps in ABI_ALL.items()}   # the parameter names in order -> position
# call(): the number of parameters and (index, dtypes, name) of every pointer to device memory
_POINTERS = {f: (len(ps), tuple((i, p.kind if isinstance(p.kind, tuple) else (p.kind,), p.name)
                                for i, p in enumerate(ps) if not isinstance(p.kind, type)))
             for f, ps in ABI_ALL.items()}

_lib = None


class GymGoNativeError(RuntimeError):
    pass


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    import glob
    import subprocess
    csrc = os.path.join(_HERE, 'csrc')
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.hip', '.h'))]
    srcs += glob.glob(os.path.join(os.path.dirname(_HERE), 'include', 'gymgo_amd*.h'))
    stale = not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(f) for f in srcs)
    if force or stale:
        subprocess.check_call(['make', '-C', os.path.join(_HERE, 'csrc'), '-s', '-B', '-j3'])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GymGoNativeError(
                'HIP library %s not built (run `make -C gymgo_amd/csrc` or __graft_entry__.build()); '
                'gymgo_amd has no CPU fallback' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _signatures(ABI_ALL).items():
            fn = getattr(L, name)  # AttributeError if the .so does not export what the header declares
            fn.argtypes, fn.restype = argtypes, restype
        if L.gg_version() != ABI_VERSION:
            raise GymGoNativeError('%s has ABI version %d, this package binds version %d: rebuild it '
                                   '(make -C gymgo_amd/csrc)' % (LIB_PATH, L.gg_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(code, what):
    if code != 0:
        raise GymGoNativeError('%s failed with code %d (%s)' % (
            what, code, 'bad argument' if code < 0 else 'hipError_t'))


_stream_override = threading.local()   # .raw: a hipStream_t that replaces torch's current stream (GoVecEnvParts)


def stream_ptr(device=None):
    """torch's current stream on `device` as a hipStream_t: launches go where the caller's torch work goes.  (A
    GoVecEnvParts sub-batch steps on its own stream: it names that stream here for the duration of its call instead of
    switching torch's current stream, which costs more host time than the launch.)"""
    raw = getattr(_stream_override, 'raw', None)
    if raw is not None:
        dev = getattr(_stream_override, 'device', None)     # the override names a stream of ONE device
        if dev is None or _device_index(device) == dev:
            return raw
    return current_raw_stream(device)


def _device_index(device):
    if isinstance(device, str):
        device = torch.device(device)
    idx = device.index if isinstance(device, torch.device) else device
    return torch.cuda.current_device() if idx is None else idx


def current_raw_stream(device=None):
    """hipStream_t of torch's current stream on `device` (an int; 0 = the null stream)."""
    try:
        if isinstance(device, str):           # 'cuda' / 'cuda:1', as torch's own factory functions accept
            device = torch.device(device)
        idx = device.index if isinstance(device, torch.device) else device
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)
    except (AttributeError, TypeError):   # an older / newer torch without the raw getter
        return torch.cuda.current_stream(device).cuda_stream
    except RuntimeError:
        if torch.cuda.is_available():
            raise
        # (a call() site names its stream before call() looks at the tensors: without a device that is where it ends)
        raise GymGoNativeError('no ROCm device visible; gymgo_amd has no CPU path') from None


class stream_override:
    """with stream_override(raw, device): every launch of this thread ON `device` goes to the hipStream_t `raw` (launches on
    another device keep torch's current stream there; device None = whatever device the launch is on)."""

    def __init__(self, raw, device=None):
        self.raw = raw
        self.device = None if device is None else _device_index(device)

    def __enter__(self):
        self.prev = (getattr(_stream_override, 'raw', None), getattr(_stream_override, 'device', None))
        _stream_override.raw, _stream_override.device = self.raw, self.device

    def __exit__(self, *exc):
        _stream_override.raw, _stream_override.device = self.prev


_hip = None


def hip_runtime():
    """The HIP runtime torch and the library already share, bound for the three stream-ordering calls GoVecEnvParts
    makes per step (torch's Stream.wait_stream creates and destroys an event per call: 8 us of host time against 2) and the
    stream wait of GoEnv.step."""
    global _hip
    if _hip is None:
        # The runtime ALREADY in the process (torch's and the library's): its path is read from /proc/self/maps and that exact
        # file is opened - dlopen by soname could bring in a second runtime when a torch wheel bundles its own copy under
        # another name, and events created in one runtime mean nothing to streams of the other.
        H, paths = None, []
        try:
            with open('/proc/self/maps') as f:
                for line in f:
                    # (the path is everything from the first '/' on: it may hold spaces; a '(deleted)' suffix cannot be opened)
                    path = line[line.index('/'):].rstrip('\n') if '/' in line else ''
                    if path.endswith(' (deleted)'):
                        continue
                    if 'libamdhip64' in os.path.basename(path) and path not in paths:
                        paths.append(path)
        except OSError:
            pass
        for name in paths + ['libamdhip64.so']:
            try:
                H = ctypes.CDLL(name)
                break
            except OSError:
                continue
        if H is None:
            raise GymGoNativeError('libamdhip64.so not found (it is loaded with torch)')
        H.hipEventCreateWithFlags.argtypes, H.hipEventCreateWithFlags.restype = [ctypes.POINTER(_vp), ctypes.c_uint], _i32
        H.hipEventRecord.argtypes, H.hipEventRecord.restype = [_vp, _vp], _i32
        H.hipStreamWaitEvent.argtypes, H.hipStreamWaitEvent.restype = [_vp, _vp, ctypes.c_uint], _i32
        H.hipEventDestroy.argtypes, H.hipEventDestroy.restype = [_vp], _i32
        H.hipStreamQuery.argtypes, H.hipStreamQuery.restype = [_vp], _i32
        H.hipStreamSynchronize.argtypes, H.hipStreamSynchronize.restype = [_vp], _i32
        H.hipStreamIsCapturing.argtypes, H.hipStreamIsCapturing.restype = [_vp, ctypes.POINTER(ctypes.c_int)], _i32
        if torch.cuda.is_available():
            # the same runtime as torch's: a torch stream must be a stream it knows.  Probed with hipStreamIsCapturing,
            # which is legal on a capturing stream (hipStreamQuery would invalidate the capture) and reports an unknown
            # handle (400 hipErrorInvalidHandle / 709 hipErrorContextIsDestroyed) - any other code (a sticky asynchronous
            # error of earlier work, say) is not a statement about the runtime and is left to the call that caused it
            cap = ctypes.c_int(0)
            rc = H.hipStreamIsCapturing(current_raw_stream(None), ctypes.byref(cap))
            if rc in (400, 709):
                raise GymGoNativeError('the HIP runtime opened for stream ordering (%s) does not know torch\'s stream '
                                       '(hipStreamIsCapturing -> %d): two runtimes in one process?' % (getattr(H, '_name', '?'), rc))
        _hip = H
    return _hip


def hip_event():
    """A HIP event without timing (usable inside a stream capture)."""
    ev = _vp()
    check(hip_runtime().hipEventCreateWithFlags(ctypes.byref(ev), 2), 'hipEventCreateWithFlags')   # hipEventDisableTiming
    return ev


def dev_ptr(t, dtype, name):
    """Pointer of a contiguous device tensor of `dtype` (one dtype, or a tuple of those allowed); raises instead of silently
    copying."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GymGoNativeError('%s must be a ROCm device tensor (got %r); gymgo_amd has no CPU path'
                               % (name, type(t) if not isinstance(t, torch.Tensor) else t.device))
    # (call() tests these same four conditions in line before it comes here: change them in both places)
    if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype) or not t.is_contiguous():
        raise GymGoNativeError('%s must be contiguous %s (got %s, contiguous=%s)'
                               % (name, dtype, t.dtype, t.is_contiguous()))
    return t.data_ptr()


def ptrs(fn, **tensors):
    """dev_ptr of every tensor as the parameter of entry point `fn` it is named after - dtype(s) from the table -, in the order
    given: for the paths that check their buffers once and hand call() the pointers from then on."""
    kinds = {p.name: p.kind for p in ABI_ALL[fn]}
    return tuple(dev_ptr(t, kinds[n], n) for n, t in tensors.items())


def launch(fn, *args):
    """fn(...) plus check and nothing else, for the paths whose every pointer is already an address (ptrs()) and whose host
    time per launch is their cost: what call() does after it has looked at its arguments."""
    code = getattr(_lib or lib(), fn)(*args)
    if code:
        check(code, fn)


def call(fn, *args):
    """Call entry point `fn` of the library and raise GymGoNativeError unless it returns 0.  args: one per parameter of
    ABI[fn], the stream (stream_ptr / current_raw_stream: the caller's choice) last.  A pointer parameter takes None (NULL),
    an int (a pointer the caller has prepared: ptrs(), or pinned host memory) or a tensor, which goes through dev_ptr with the
    table's dtype(s) and the header's parameter name; scalars pass as they are."""
    count, pointers = _POINTERS[fn]
    if len(args) != count:
        raise TypeError('%s takes %d arguments (%d given)' % (fn, count, len(args)))
    args = list(args)
    for i, dtypes, name in pointers:
        a = args[i]
        if a is None or type(a) is int:
            continue
        if type(a) is torch.Tensor and a.is_cuda and a.dtype in dtypes and a.is_contiguous():   # what dev_ptr asks, without the call
            args[i] = a.data_ptr()
        else:           # (a tensor subclass, or what dev_ptr refuses: its verdict, its message)
            args[i] = dev_ptr(a, dtypes if len(dtypes) > 1 else dtypes[0], name)
    code = getattr(_lib or lib(), fn)(*args)
    if code:
        check(code, fn)
