"""The case table of tests/test_gpu_guarded.py: which entry points of the C ABI run between guards, at which board sizes,
batch sizes and start residues, and how each of their buffers is made.

A Case names an entry point of gymgo_amd/_lib.py's binding tables, a board size, a batch size, the ROLE of every device
pointer ('in': declared const by the header and registered read-only; 'out': every element is written by the call;
'inout': read and written; 'null': NULL, where the header allows it) and the options its builder reads.  The table is plain
data and needs no device (tests/test_guard_cases_host.py holds it against the binding tables and the headers); build() and
run_case() need one.

Batch sizes: the rollout cells are rollout_cells(n) of tests/test_gpu_dispatch_sizes.py, each at the batch size below it
that the same kernel family serves at one compute unit (a short last wave); the other calls take the B = 12 / 24 / 200 / 256
of that file's child script, ragged the same way.  Positions: its positions(): oracle-made mid-game and late boards, every
fourth from a game played on until most have ended.
"""
import collections
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import guard_arena                                   # noqa: E402
from test_gpu_dispatch_sizes import rollout_cells   # noqa: E402

SIZES = (2, 3, 6, 9, 11, 13, 16, 19)    # every full size, one partial size per row capacity, an even N, the two smallest records
U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
W_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}

Case = collections.namedtuple('Case', 'fn n b roles dtypes opts')
Out = collections.namedtuple('Out', 'shape dtype')     # an `out` buffer: no content of the caller's, every element written

# Entry points whose EVERY written buffer already stands between sentinels in an existing test (file::test), read by hand
# for this list: the one `out` of the policy turn and of the past planes, leaf and node_hash of the superko launch, out and
# counts of the area planes, and the whole-tree buffers and per-round outputs of the advance, leaves and self-play calls.
GUARDED_ELSEWHERE = {
    'gg_batch_symmetry_policy': 'test_gpu_symmetry_io.py::test_policy_turn',
    'gg_puct_superko': 'test_gpu_puct_superko.py::test_the_launch_alone_on_planted_cases',
    'gg_puct_advance': 'test_gpu_puct_advance.py::test_entry_point_on_own_buffers_shards_stream_numpy_and_check',
    'gg_puct_select_leaves': 'test_gpu_puct_leaves.py::test_leaves_virtual_visits_and_select_past_capacity_on_own_buffers',
    'gg_puct_backup_leaves': 'test_gpu_puct_leaves.py::test_leaves_virtual_visits_and_select_past_capacity_on_own_buffers',
    'gg_puct_root_noise': 'test_gpu_puct_selfplay.py::test_entry_points_on_own_buffers_with_sentinels',
    'gg_puct_root_policy': 'test_gpu_puct_selfplay.py::test_entry_points_on_own_buffers_with_sentinels',
    'gg_batch_area': 'test_gpu_area.py::test_sub_batches_between_sentinels',
    'gg_batch_area_tracked': 'test_gpu_area.py::test_sub_batches_between_sentinels',
    'gg_batch_past': 'test_gpu_past.py::test_dtypes_sub_batches_between_sentinels_and_a_ring_of_garbage',
    'gg_batch_past_tracked': 'test_gpu_past.py::test_dtypes_sub_batches_between_sentinels_and_a_ring_of_garbage',
}
# gg_gumbel_sequence takes HOST memory (seq is written by the host, no launch): there is nothing for a device arena to guard.
EXEMPT = {'gg_gumbel_sequence': 'seq is host memory, written by the host'}
# What the headers let a caller pass as NULL, per entry point of the table (include/gymgo_amd.h: "nullable", "may be NULL",
# "NULL = ..."; rng of an env step: "required when actions == NULL"): each is NULL in at least one case.
_ROLL_NULLS = ('last_actions', 'steps_done')
_STEP_NULLS = ('actions', 'rng', 'rewards', 'dones', 'status', 'taken_actions')
NULLABLE = {
    'gg_batch_next_states': ('status',), 'gg_batch_next_states_ws': ('status',), 'gg_batch_next_states_packed': ('status',),
    'gg_batch_invalid_mask': ('ko',), 'gg_batch_children_offsets': ('order',), 'gg_batch_children_compact': ('order',),
    'gg_batch_rollout': _ROLL_NULLS, 'gg_batch_rollout_ws': _ROLL_NULLS, 'gg_batch_rollout_packed': _ROLL_NULLS,
    'gg_batch_rollout_tracked': _ROLL_NULLS, 'gg_batch_rollout_tracked_policy': _ROLL_NULLS, 'gg_batch_rollout_tracked_policy2': _ROLL_NULLS,
    'gg_batch_env_step': _STEP_NULLS, 'gg_batch_env_step_scored': _STEP_NULLS, 'gg_batch_env_step_packed': _STEP_NULLS,
    'gg_batch_env_step_tracked': _STEP_NULLS + ('states_out', 'steps_done'),
    'gg_batch_env_step_tracked_weighted': ('rewards', 'dones', 'status', 'taken_actions', 'states_out', 'steps_done'),
    'gg_batch_update_pieces': ('killed',), 'gg_batch_play_moves': ('played',), 'gg_batch_play_moves_packed': ('played',),
    'gg_batch_play_moves_tracked': ('played',), 'gg_batch_sample_weighted': ('states',), 'gg_batch_symmetry': ('orient',),
    'gg_batch_symmetry_rows': ('orient',),
    'gg_batch_life': ('orient', 'settled'), 'gg_batch_life_tracked': ('orient', 'settled'), 'gg_batch_ladder': ('orient', 'aborted'),
    'gg_batch_ladder_tracked': ('orient', 'aborted'), 'gg_batch_move_planes': ('orient',), 'gg_batch_move_planes_tracked': ('orient',),
    'gg_batch_tactics': ('orient',), 'gg_batch_tactics_tracked': ('orient',), 'gg_past_push': ('mask',), 'gg_past_push_tracked': ('mask',),
    'gg_batch_move_hashes': ('history', 'count', 'hashes', 'repeat', 'rows'),
    'gg_batch_move_hashes_tracked': ('history', 'count', 'hashes', 'repeat', 'rows'),
    'gg_playouts_begin': ('ownership',), 'gg_playouts_advance': ('ownership',), 'gg_playouts_advance_policy': ('ownership',),
    'gg_playouts_advance_policy2': ('ownership',), 'gg_uct_backup': ('totals',), 'gg_gumbel_root': ('q', 'visits', 'value'),
    'gg_puct_past': ('rows', 'count', 'orient'),
}


def tables():
    from gymgo_amd import _lib
    return (_lib.ABI, _lib.ABI_AREA, _lib.ABI_PAST, _lib.ABI_GUMBEL, _lib.ABI_TACTICS)


def params(fn):
    for t in tables():
        if fn in t:
            return t[fn]
    raise KeyError(fn)


def pointer_params(fn):
    """[(name, kind)] of the device pointers of an entry point, in order; the stream is no pointer argument."""
    return [(p.name, p.kind) for p in params(fn) if not isinstance(p.kind, type)]


def pointer_dtype(case, name):
    kind = dict(pointer_params(case.fn))[name]
    return case.dtypes[name] if isinstance(kind, tuple) else kind


def pointer_align(case, name):
    """The alignment a pointer of a case gets: that of its element, or what the case names (opts['align']: the natural alignment
    of a record - gg_puct_stat starts with a double -, or the 16 bytes a header demands)."""
    return case.opts.get('align', {}).get(name, guard_arena.element_size(pointer_dtype(case, name)))


def tracked_words(n):
    return 5 * n + 1


def packed_words(n):
    return 3 * n + 1


# ------------------------------------------------------------------------------------------------ the table

def ragged(n, B, plies):
    """The batch size just below the cell's that the cell's kernel family still serves at one compute unit, for both values of
    auto_reset: a short last wave, a last pair of one board."""
    import bench
    for cand in (B - 1, B - 3):
        if cand >= 1 and all(bench.rollout_kernel_name(n, cand, plies, 1, a) == bench.rollout_kernel_name(n, B, plies, 1, a)
                             for a in (True, False)):
            return cand
    return B


_LAYOUT_OF = {'states': 'bytes', 'packed': 'packed', 'tracked': 'tracked', 'in': 'bytes'}
_NULLS = ((), ('last_actions',), ('steps_done',), ('last_actions', 'steps_done'))


def _case(fn, n, b, roles, opts, dtypes=None):
    names = [name for name, _ in pointer_params(fn)]
    assert sorted(roles) == sorted(names), (fn, sorted(roles), sorted(names))
    return Case(fn, n, b, roles, dtypes or {}, opts)


def _rollout(fn, n, B, plies, auto, k, policy=None):
    first = params(fn)[0].name
    roles = {first: 'inout', 'rng': 'inout', 'last_actions': 'out', 'steps_done': 'inout'}
    if fn == 'gg_batch_rollout_ws':
        roles['workspace'] = 'inout'
    for name in _NULLS[k % 4]:
        roles[name] = 'null'
    opts = dict(build='rollout', plies=plies, auto=int(auto), seed=7 * B + plies + k, oracle='rollout' if not policy else None)
    if policy is not None:
        opts['policy'] = policy
    return _case(fn, n, B, roles, opts)


def _step_roles(fn, k, given, no_rng=False):
    """Roles of an env-step call, variant k: one nullable output after the other is NULL, every sixth variant has them all."""
    names = [name for name, _ in pointer_params(fn)]
    roles = {names[0]: 'inout', 'rng': 'inout'}
    if 'actions' in names:
        roles['actions'] = 'in' if given else 'null'
        if given and no_rng:
            roles['rng'] = 'null'            # rng is required only when the moves are drawn
    if 'weights' in names:
        roles['weights'] = 'in'
    outs = [m for m in ('rewards', 'dones', 'status', 'taken_actions', 'states_out', 'steps_done') if m in names]
    for j, m in enumerate(outs):
        roles[m] = 'inout' if m == 'steps_done' else 'out'
        if k % (len(outs) + 1) == j + 1:
            roles[m] = 'null'
    if 'areas' in names:
        roles['areas'] = 'out'               # required
    return roles


def cases(n):
    """The cases of board size n, in a fixed order."""
    A, out, k = n * n + 1, [], 0
    # ---- rollouts: every cell of rollout_cells(n), both values of auto_reset, last_actions / steps_done given and NULL in turn
    for B0, plies in rollout_cells(n):
        B = ragged(n, B0, plies)
        for auto in (1, 0):
            out.append(_rollout('gg_batch_rollout', n, B, plies, auto, k))
            out.append(_rollout('gg_batch_rollout_ws', n, B, plies, auto, k + 1))
            k += 1
    for B, plies in ((23, 1), (24, 3), (23, 9), (16, 1), (15, 3), (199, 1), (200, 3), (199, 9)):
        out.append(_rollout('gg_batch_rollout_tracked', n, B, plies, k % 2, k))
        k += 1
    for B, plies in ((199, 5), (29, 5), (30, 2), (200, 5), (30, 5), (29, 2)):
        out.append(_rollout('gg_batch_rollout_packed', n, B, plies, k % 2, k))
        k += 1
    for B, plies in ((23, 9), (199, 9), (200, 3)):     # the policy draws: k_rollout_lat_pol / _tac, k_rollout5_pol / _tac at 9 / 13 / 19
        for policy in (0, 1, 2):
            if policy < 2:
                out.append(_rollout('gg_batch_rollout_tracked_policy', n, B, plies, k % 2, k, policy))
            out.append(_rollout('gg_batch_rollout_tracked_policy2', n, B, plies, (k + 1) % 2, k + 2, policy))
            k += 1
    # ---- next states: straight, pipelined, sixteen boards per wave; through a workspace; packed
    for B in (11, 199, 256):
        for canonical in (0, 1):
            st = 'null' if k % 3 == 0 else 'out'
            out.append(_case('gg_batch_next_states', n, B, {'in': 'in', 'actions': 'in', 'out': 'out', 'status': st},
                             dict(build='next_states', canonical=canonical, oracle='next_states')))
            out.append(_case('gg_batch_next_states_ws', n, B, {'in': 'in', 'actions': 'in', 'out': 'out', 'status': 'out' if st == 'null' else 'null',
                                                               'workspace': 'inout'},
                             dict(build='next_states', canonical=canonical, oracle='next_states')))
            out.append(_case('gg_batch_next_states_packed', n, B, {'in': 'in', 'actions': 'in', 'out': 'out', 'status': st},
                             dict(build='next_states', canonical=canonical, layout='packed', oracle='next_states')))
            k += 1
    # ---- the env steps: given and drawn moves, both reward methods, auto_reset on and off, each nullable output NULL in turn
    for fn, sizes in (('gg_batch_env_step', (11, 199, 256)), ('gg_batch_env_step_scored', (11, 199, 256)),
                      ('gg_batch_env_step_packed', (11, 199, 256)), ('gg_batch_env_step_tracked', (23, 199, 200))):
        for B in sizes:
            for v in range(4):
                given = v % 2 == 0
                out.append(_case(fn, n, B, _step_roles(fn, k, given, v == 2), dict(build='env_step', given=given, method=(v // 2 + k) % 2,
                                                                           auto=int(k % 3 != 0), seed=k)))
                k += 1
    for B in (23, 199):
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            out.append(_case('gg_batch_env_step_tracked_weighted', n, B, _step_roles('gg_batch_env_step_tracked_weighted', k, False),
                             dict(build='env_step', given=False, method=k % 2, auto=int(k % 3 != 0), seed=k), {'weights': dt}))
            k += 1
    # ---- the other board calls
    for B in (199, 256):
        for ko in ('in', 'null'):
            out.append(_case('gg_batch_invalid_mask', n, B, {'states': 'in', 'ko': ko, 'mask': 'out'}, dict(build='invalid_mask', oracle='invalid_mask')))
        out.append(_case('gg_batch_areas', n, B - 1, {'states': 'in', 'black': 'out', 'white': 'out'}, dict(build='areas', oracle='areas')))
        out.append(_case('gg_batch_eye_mask', n, B, {'states': 'in', 'mask': 'out'}, dict(build='board_plane', planes=1)))
        out.append(_case('gg_batch_group_liberties', n, B, {'states': 'in', 'libs': 'out'}, dict(build='board_plane', planes=1)))
        out.append(_case('gg_batch_move_counts', n, B, {'states': 'in', 'out': 'out'}, dict(build='board_plane', planes=3)))
        out.append(_case('gg_batch_sample_actions', n, B, {'states': 'in', 'rng': 'inout', 'actions': 'out'}, dict(build='sample', seed=k)))
        out.append(_case('gg_batch_reset_finished', n, B - 1, {'states': 'inout'}, dict(build='reset')))
        out.append(_case('gg_batch_pack_states', n, B, {'states': 'in', 'packed': 'out'}, dict(build='convert', src='bytes', dst='packed')))
        out.append(_case('gg_batch_unpack_states', n, B, {'packed': 'in', 'states': 'out'}, dict(build='convert', src='packed', dst='bytes')))
        out.append(_case('gg_batch_track_states', n, B, {'states': 'in', 'tracked': 'out'}, dict(build='convert', src='bytes', dst='tracked')))
        out.append(_case('gg_batch_untrack_states', n, B, {'tracked': 'in', 'states': 'out'}, dict(build='convert', src='tracked', dst='bytes')))
        for Bu, killed in ((B - 1, 'out'), (B // 8, 'out' if B == 199 else 'null'), (B // 16, 'out')):
            out.append(_case('gg_batch_update_pieces', n, Bu, {'states': 'inout', 'adj': 'in', 'players': 'in', 'killed': killed},
                             dict(build='update_pieces', seed=k + Bu, oracle='update_pieces')))
        out.append(_case('gg_rng_seed', n, B - 1, {'rng': 'out'}, dict(build='rng_seed', seed=k)))
        out.append(_case('gg_batch_draw_orient', n, B - 1, {'rng': 'inout', 'orient': 'out'}, dict(build='draw_orient', seed=k)))
        out.append(_case('gg_puct_legal', n, B - 1, {'leaf': 'in', 'leaf_id': 'in', 'legal': 'out', 'live': 'out'}, dict(build='puct_legal', seed=k)))
        k += 1
    for B in (11, 23, 199):
        out.append(_case('gg_batch_sample_actions', n, B, {'states': 'in', 'rng': 'inout', 'actions': 'out'}, dict(build='sample', seed=k)))
        k += 1
    for B in (23, 200):
        for j, dt in enumerate((torch.float32, torch.bfloat16, torch.float16)):
            roles = {'states': 'null' if j == 1 else 'in', 'weights': 'in', 'rng': 'inout', 'actions': 'out'}
            out.append(_case('gg_batch_sample_weighted', n, B, roles, dict(build='sample_weighted', seed=k), {'weights': dt}))
            out.append(_case('gg_batch_sample_weighted_rows', n, B, {'boards': 'in', 'weights': 'in', 'rng': 'inout', 'actions': 'out'},
                             dict(build='sample_weighted', seed=k, planes=3 + 2 * (j % 2)), {'weights': dt}))
            k += 1
    # ---- children: padded on two dozen parents, the two calls of the un-padded form, packed
    for canonical in (0, 1):
        out.append(_case('gg_batch_children', n, 23, {'states': 'in', 'children': 'out'}, dict(build='children', canonical=canonical, oracle='children')))
        out.append(_case('gg_batch_children_packed', n, 23, {'packed': 'in', 'children': 'out'}, dict(build='children', canonical=canonical, layout='packed')))
        for B in (23, 199):
            order = 'null' if (canonical + (B == 199)) % 2 else 'out'
            out.append(_case('gg_batch_children_offsets', n, B, {'states': 'in', 'offsets': 'out', 'order': order},
                             dict(build='children_offsets', oracle='children_offsets', by_rule=('order',), empty_writes='offsets')))
            out.append(_case('gg_batch_children_compact', n, B if B == 23 else 47,
                             {'states': 'in', 'offsets': 'in', 'order': 'null' if order == 'out' else 'in', 'children': 'out'},
                             dict(build='children_compact', canonical=canonical, oracle='children_compact')))
    # ---- the replays (per pair of boards; sixteen boards per wave from 32 boards and two moves on), symmetry
    for B, T in ((23, 3), (199, 3), (24, 1), (200, 2)):
        for fn, first in (('gg_batch_play_moves', 'states'), ('gg_batch_play_moves_packed', 'packed'), ('gg_batch_play_moves_tracked', 'tracked')):
            out.append(_case(fn, n, B, {first: 'inout', 'moves': 'in', 'played': 'null' if k % 2 else 'out'}, dict(build='play_moves', T=T, seed=k)))
            k += 1
    for B in (37, 200):
        for orient in ('in', 'null'):
            out.append(_case('gg_batch_symmetry', n, B, {'in': 'in', 'orient': orient, 'out': 'out'}, dict(build='symmetry', seed=k)))
            out.append(_case('gg_batch_symmetry_rows', n, B, {'in': 'in', 'orient': orient, 'out': 'out'},
                             dict(build='symmetry', seed=k, planes=3 if orient == 'in' else 5)))
            k += 1
    out += plane_cases(n)
    out += search_cases(n)
    return out


# entry point -> (planes per board, the per-board flag output or None, orient: 'none' (no such parameter) / 'in' (required) /
# 'null' (may be NULL), whether the header demands a 16-byte aligned out)
_PLANE_CALLS = {
    'gg_batch_features': (16, None, 'none', True), 'gg_batch_features_tracked': (16, None, 'none', True),
    'gg_batch_features_oriented': (16, None, 'in', True), 'gg_batch_features_tracked_oriented': (16, None, 'in', True),
    'gg_batch_life': (4, 'settled', 'null', False), 'gg_batch_life_tracked': (4, 'settled', 'null', False),
    'gg_batch_ladder': (4, 'aborted', 'null', False), 'gg_batch_ladder_tracked': (4, 'aborted', 'null', False),
    'gg_batch_move_planes': (12, None, 'null', False), 'gg_batch_move_planes_tracked': (12, None, 'null', False),
    'gg_batch_tactics': (3, None, 'null', False), 'gg_batch_tactics_tracked': (3, None, 'null', False),
}
_PLANE_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def plane_cases(n):
    """The plane calls, the position hashes and the pushes of the history ring.  Their own files hold `out` between sentinels at a
    few offsets of an aligned base, but not the per-board flags (settled, aborted), not the hashes, not the ring, and the tracked
    and oriented forms only in part: here every buffer they write stands in the arena, at every residue."""
    out, rot = [], _PLANE_DTYPES[SIZES.index(n) % 3]
    for fn, (P, flag, orient, aligned) in _PLANE_CALLS.items():
        first = params(fn)[0].name
        for j, (B, dt) in enumerate(((199, U8), (37, U8), (256, rot))):
            if aligned and orient == 'none' and j == 1:
                continue
            roles = {first: 'in', 'out': 'out'}
            if orient != 'none':
                roles['orient'] = 'null' if orient == 'null' and j == 1 else 'in'
            if flag:
                roles[flag] = 'null' if j == 1 else 'out'
            opts = dict(build='planes', planes=P, seed=n + j)
            if aligned:
                opts.update(align={'out': 16}, demand=('out',))
            out.append(_case(fn, n, B, roles, opts, {'out': dt}))
    for j, B in enumerate((199, 256)):
        out.append(_case('gg_batch_hash', n, B - j, {'states': 'in', 'out': 'out'}, dict(build='hash')))
        out.append(_case('gg_batch_hash_tracked', n, B - 1 + j, {'tracked': 'in', 'out': 'out'}, dict(build='hash')))
    for fn, first in (('gg_batch_move_hashes', 'states'), ('gg_batch_move_hashes_tracked', 'tracked')):
        for j, (B, given) in enumerate(((199, ('hashes', 'repeat', 'rows')), (37, ('hashes',)), (256, ('repeat', 'rows')), (23, ('repeat',)))):
            ring = 'in' if given != ('hashes',) else 'null'        # history and count may be NULL only when repeat and rows both are
            roles = {first: 'in', 'history': ring, 'count': ring}
            roles.update({name: 'out' if name in given else 'null' for name in ('hashes', 'repeat', 'rows')})
            out.append(_case(fn, n, B, roles, dict(build='move_hashes', seed=n + j)))
    for j, (B, mask) in enumerate(((199, U8), (256, torch.bool), (37, U8), (23, None))):
        for fn, first in (('gg_past_push', 'states'), ('gg_past_push_tracked', 'tracked')):
            out.append(_case(fn, n, B, {first: 'in', 'mask': 'in' if mask else 'null', 'rows': 'inout', 'count': 'inout'},
                             dict(build='past_push', seed=n + j), {'mask': mask or U8}))
    return out


SEARCH_ROOTS = (0, 1, 3, 2, 7)      # of positions(): three mid-game boards, two from the games played on to their end
_SLOTS = ('slots', 'rng', 'plies', 'job')
_QUEUE_BUFFERS = _SLOTS + ('counter', 'counts', 'sums')
_TREE = ('boards', 'child', 'prior', 'links', 'stats', 'nodes')
_LEAF = ('leaf', 'move', 'leaf_id')


def _roles(fn, *groups):
    """{pointer: role} from (role, names) pairs; a name the entry point does not have is left out."""
    names = [name for name, _ in pointer_params(fn)]
    return {name: role for role, group in groups for name in group if name in names}


def search_cases(n):
    """The Monte Carlo queue and the tree searches on SEARCH_ROOTS: five roots, fewer slots than jobs (the slots are recycled),
    every buffer the call reads or writes in the arena.  A call in the middle of a protocol (an advance, a select, a backup)
    starts from the buffers the calls before it leave on plain tensors (the scenarios below); a buffer a call writes only in
    part - the boards of a tree, `plan` - is `inout` with content of the caller's.  stats (gg_puct_stat: a double first) stands
    on 8 bytes, and on the 16 the Gumbel header demands."""
    R, out = len(SEARCH_ROOTS), []
    for own in ('out', 'null'):
        roles = _roles('gg_playouts_begin', ('in', ('roots',)), ('out', _QUEUE_BUFFERS), (own, ('ownership',)))
        out.append(_case('gg_playouts_begin', n, R, roles, dict(build='playouts', stage='begin', empty_writes='queue')))
        for fn, policy in (('gg_playouts_advance', None), ('gg_playouts_advance_policy', 1), ('gg_playouts_advance_policy2', 2)):
            roles = _roles(fn, ('in', ('roots',)), ('inout', _QUEUE_BUFFERS + (('ownership',) if own == 'out' else ())),
                           ('null', ('ownership',) if own == 'null' else ()))
            out.append(_case(fn, n, R, roles, dict(build='playouts', stage='advance', policy=policy, slotwise=_SLOTS)))
    out.append(_case('gg_move_playouts_plan', n, R, {'roots': 'in', 'offsets': 'out', 'plan': 'inout'}, dict(build='move_playouts', stage='plan', empty_writes='offsets')))
    out.append(_case('gg_move_playouts_begin', n, R, _roles('gg_move_playouts_begin', ('in', ('roots', 'plan')), ('out', _QUEUE_BUFFERS)),
                     dict(build='move_playouts', stage='begin', empty={'T': 0}, empty_writes='queue')))
    for fn, policy in (('gg_move_playouts_advance', None), ('gg_move_playouts_advance_policy', 1), ('gg_move_playouts_advance_policy2', 2)):
        out.append(_case(fn, n, R, _roles(fn, ('in', ('roots', 'plan')), ('inout', _QUEUE_BUFFERS)),
                         dict(build='move_playouts', stage='advance', policy=policy, empty={'T': 0}, slotwise=_SLOTS)))
    out.append(_case('gg_uct_begin', n, R, {'roots': 'in', 'boards': 'inout', 'child': 'out', 'links': 'out', 'stats': 'out', 'nodes': 'out'},
                     dict(build='uct', stage='begin')))
    out.append(_case('gg_uct_select', n, R, _roles('gg_uct_select', ('in', ('log_table', 'boards')), ('inout', ('child', 'links', 'stats', 'nodes')),
                                                   ('out', _LEAF)), dict(build='uct', stage='select')))
    for totals in ('inout', 'null'):
        out.append(_case('gg_uct_backup', n, R, _roles('gg_uct_backup', ('in', ('counts', 'sums', 'links') + _LEAF), ('inout', ('boards', 'stats')),
                                                       (totals, ('totals',))), dict(build='uct', stage='backup')))
    a8 = {'stats': 8}
    out.append(_case('gg_puct_begin', n, R, _roles('gg_puct_begin', ('in', ('roots',)), ('inout', ('boards',)), ('out', _TREE[1:])),
                     dict(build='puct', stage='begin', align=a8)))
    out.append(_case('gg_puct_select', n, R, _roles('gg_puct_select', ('in', ('boards', 'prior', 'stats')), ('inout', ('child', 'links', 'nodes')),
                                                    ('out', _LEAF)), dict(build='puct', stage='select', align=a8)))
    out.append(_case('gg_puct_backup', n, R, _roles('gg_puct_backup', ('in', ('priors', 'values', 'links') + _LEAF), ('inout', ('boards', 'prior', 'stats'))),
                     dict(build='puct', stage='backup', align=a8)))
    for dt, ring, orient in ((U8, 'in', 'in'), (U8, 'null', 'in'), (torch.float16, 'in', 'null')):      # the leaves' history planes
        out.append(_case('gg_puct_past', n, R, {'boards': 'in', 'links': 'in', 'rows': ring, 'count': ring, 'leaf': 'in', 'leaf_id': 'in',
                                                'orient': orient, 'out': 'out'}, dict(build='puct_past'), {'out': dt}))
    a16 = {'stats': 16}
    out.append(_case('gg_gumbel_begin', n, R, {'child': 'in', 'stats': 'in', 'nodes': 'in', 'seen': 'out', 'done': 'out'},
                     dict(build='gumbel', stage='begin', align=a16, demand=('stats',))))
    out.append(_case('gg_gumbel_select_leaves', n, R,
                     _roles('gg_gumbel_select_leaves', ('in', ('boards', 'prior', 'base', 'seen', 'seq')),
                            ('inout', ('child', 'links', 'stats', 'nodes', 'done')), ('out', _LEAF)),
                     dict(build='gumbel', stage='select', align=a16, demand=('stats',))))
    for j in range(2):
        nulls = (('q', 'value'), ('visits',))[j]
        roles = _roles('gg_gumbel_root', ('in', ('boards', 'child', 'stats', 'nodes', 'base', 'seen')), ('out', ('actions', 'q', 'visits', 'value')))
        roles.update({name: 'null' for name in nulls})
        out.append(_case('gg_gumbel_root', n, R, roles, dict(build='gumbel', stage='root', align=a16, demand=('stats',))))
    return out


_TABLE = None


def table():
    """[(case, {pointer: residue})] over all SIZES, in a fixed order."""
    global _TABLE
    if _TABLE is None:
        every = [c for n in SIZES for c in cases(n)]
        _TABLE = list(zip(every, assign_residues(every)))
    return _TABLE


def assign_residues(every):
    """Start residues mod 16, rotated over the table: a pointer parameter of an entry point takes, of the residues its element
    size allows and no earlier pointer of the same call has, the one it has stood at least often so far (ties: the next one
    after its last) - so every parameter sees every residue it may have once it has been used often enough, and the pointers of
    one call that need the SAME alignment start in different residue classes while there are classes left (16 / that alignment).
    Pointers of different alignments are not held apart: a byte pointer and a word pointer of one call may both stand at 4."""
    stood, last, calls = collections.Counter(), {}, collections.Counter()
    res = []
    for c in every:
        r, taken = {}, collections.defaultdict(set)
        names = [name for name, _ in pointer_params(c.fn) if c.roles[name] != 'null']
        turn = calls[c.fn] % len(names)          # (the pointer that chooses first changes from case to case: nobody gets the leftovers)
        calls[c.fn] += 1
        for name in names[turn:] + names[:turn]:
            es = pointer_align(c, name)
            count = guard_arena.ALIGN // es
            if len(taken[es]) == count:
                taken[es].clear()
            first = last.get((c.fn, name), len(taken[es]) * es - es) // es + 1
            order = [(first + j) % count for j in range(count)]
            k = min((k for k in order if k not in taken[es]), key=lambda k: stood[c.fn, name, k * es])
            taken[es].add(k)
            r[name] = last[c.fn, name] = k * es
            stood[c.fn, name, k * es] += 1
        res.append(r)
    return res


# ------------------------------------------------------------------------------------------------ the buffers (device)

class Ctx:
    """The positions of one child process and the device they go to."""

    def __init__(self, device='cuda'):
        self.dev = device
        self._pos, self._dev_pos, self.scenarios = {}, {}, {}

    def pos(self, N):
        """positions(N) of tests/test_gpu_dispatch_sizes.py's child script: 256 boards the oracle makes, every fourth from a game
        played on until most have ended."""
        if N not in self._pos:
            from oracle import c_oracle
            B0 = 256
            z = np.zeros((B0, 6, N, N), np.uint8)
            mid, _, _ = c_oracle.batch_rollout_mt(z, c_oracle.rng_seed(100 + N, B0), N * N // 2 + 3, True, 16)
            late, _, _ = c_oracle.batch_rollout_mt(z[:B0 // 4], c_oracle.rng_seed(200 + N, B0 // 4), 3 * N * N, False, 16)
            mid[3::4] = late
            self._pos[N] = mid
            self._dev_pos[N] = torch.from_numpy(mid).to(self.dev)
        return self._pos[N]

    def boards(self, N, B, layout='bytes'):
        """A fresh copy of the first B positions as byte planes, packed or tracked boards."""
        from gymgo_amd import gogame
        self.pos(N)
        st = self._dev_pos[N][:B].clone()
        return st if layout == 'bytes' else gogame.batch_pack(st) if layout == 'packed' else gogame.batch_track(st)


def _layout(c):
    return c.opts.get('layout') or _LAYOUT_OF[params(c.fn)[0].name]


def _given(c, name):
    return c.roles[name] != 'null'


def _words(layout, N):
    return {'packed': packed_words(N), 'tracked': tracked_words(N)}[layout]


def _b_rollout(c, x):
    from gymgo_amd import gogame
    N, B, o = c.n, c.b, c.opts
    a = {params(c.fn)[0].name: x.boards(N, B, _layout(c)), 'rng': gogame.rng_seed(B, o['seed'], 0, x.dev),
         'last_actions': Out((B,), I32) if _given(c, 'last_actions') else None,
         'steps_done': (torch.arange(B, dtype=I64, device=x.dev) * 3 + 1) if _given(c, 'steps_done') else None,
         'B': B, 'N': N, 'plies': o['plies'], 'auto_reset': o['auto']}
    if 'workspace' in c.roles:
        a['workspace'] = torch.zeros((B, tracked_words(N)), dtype=I32, device=x.dev)
    if 'policy' in o:
        a['policy'] = o['policy']
    return a


def _moves(c, x, B, seed):
    """Moves for the first B positions: drawn uniformly from the legal ones, every fifth replaced by any action at all (many
    of them illegal) and every eleventh out of range."""
    from gymgo_amd import gogame
    N = c.n
    acts = gogame.batch_sample_actions(x.boards(N, B), gogame.rng_seed(B, 5 + seed, 0, x.dev)).cpu().numpy()
    rs = np.random.default_rng(1000 + seed)
    acts[::5] = rs.integers(0, N * N + 1, size=len(acts[::5]))
    acts[::11] = N * N + 1 + rs.integers(0, 3, size=len(acts[::11]))
    return torch.from_numpy(acts.astype(np.int32)).to(x.dev)


def _b_next_states(c, x):
    N, B = c.n, c.b
    layout = _layout(c)
    shape = (B, 6, N, N) if layout == 'bytes' else (B, _words(layout, N))
    a = {'in': x.boards(N, B, layout), 'actions': _moves(c, x, B, B), 'out': Out(shape, U8 if layout == 'bytes' else I32),
         'status': Out((B,), I32) if _given(c, 'status') else None, 'B': B, 'N': N, 'canonical': c.opts['canonical']}
    if 'workspace' in c.roles:
        a['workspace'] = torch.zeros((B, tracked_words(N)), dtype=I32, device=x.dev)
    return a


def _weights(c, x, B, seed):
    """Policy weights [B][N*N+1] of the case's dtype: positive, a quarter of them zero, every ninth row all zero (refused)."""
    A = c.n * c.n + 1
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((B, A), generator=g)
    w[torch.rand((B, A), generator=g) < 0.25] = 0
    w[::9] = 0
    return w.to(c.dtypes['weights']).to(x.dev)


def _b_env_step(c, x):
    from gymgo_amd import gogame
    N, B, o = c.n, c.b, c.opts
    first = params(c.fn)[0].name
    a = {first: x.boards(N, B, _layout(c)), 'rng': gogame.rng_seed(B, 6 + o['seed'], 0, x.dev) if _given(c, 'rng') else None,
         'B': B, 'N': N, 'komi': 0.5, 'reward_method': o['method'], 'auto_reset': o['auto']}
    if 'actions' in c.roles:
        a['actions'] = _moves(c, x, B, o['seed']) if o['given'] else None
    if 'weights' in c.roles:
        a['weights'], a['weight_dtype'] = _weights(c, x, B, o['seed']), W_CODES[c.dtypes['weights']]
    for name, shape, dt in (('rewards', (B,), F32), ('dones', (B,), U8), ('status', (B,), I32), ('taken_actions', (B,), I32),
                            ('areas', (B, 2), I32), ('states_out', (B, 6, N, N), U8)):
        if name in c.roles:
            a[name] = Out(shape, dt) if _given(c, name) else None
    if 'steps_done' in c.roles:
        a['steps_done'] = (torch.arange(B, dtype=I64, device=x.dev) * 5 + 2) if _given(c, 'steps_done') else None
    return a


def _b_invalid_mask(c, x):
    N, B = c.n, c.b
    ko = None
    if _given(c, 'ko'):
        rs = np.random.default_rng(N + B)
        k = rs.integers(-1, N * N, size=B).astype(np.int32)
        k[::3] = -1
        ko = torch.from_numpy(k).to(x.dev)
    return {'states': x.boards(N, B), 'ko': ko, 'mask': Out((B, N, N), U8), 'B': B, 'N': N}


def _b_areas(c, x):
    return {'states': x.boards(c.n, c.b), 'black': Out((c.b,), I32), 'white': Out((c.b,), I32), 'B': c.b, 'N': c.n}


def _b_board_plane(c, x):
    N, B, names = c.n, c.b, [name for name, _ in pointer_params(c.fn)]
    shape = (B, N, N) if c.opts['planes'] == 1 else (B, c.opts['planes'], N, N)
    return {'states': x.boards(N, B), names[1]: Out(shape, U8), 'B': B, 'N': N}


def _b_sample(c, x):
    from gymgo_amd import gogame
    return {'states': x.boards(c.n, c.b), 'rng': gogame.rng_seed(c.b, c.opts['seed'], 0, x.dev), 'actions': Out((c.b,), I32), 'B': c.b, 'N': c.n}


def _b_sample_weighted(c, x):
    from gymgo_amd import gogame
    N, B, o = c.n, c.b, c.opts
    a = {'weights': _weights(c, x, B, o['seed']), 'weight_dtype': W_CODES[c.dtypes['weights']], 'rng': gogame.rng_seed(B, o['seed'], 0, x.dev),
         'actions': Out((B,), I32), 'B': B, 'N': N}
    if 'boards' in c.roles:
        a['boards'], a['planes'] = x.boards(N, B, 'packed' if o['planes'] == 3 else 'tracked'), o['planes']
    else:
        a['states'] = x.boards(N, B) if _given(c, 'states') else None
    return a


def _b_reset(c, x):
    return {'states': x.boards(c.n, c.b), 'B': c.b, 'N': c.n}


def _b_convert(c, x):
    N, B, o = c.n, c.b, c.opts
    names = [name for name, _ in pointer_params(c.fn)]
    shape = (B, 6, N, N) if o['dst'] == 'bytes' else (B, _words(o['dst'], N))
    return {names[0]: x.boards(N, B, o['src']), names[1]: Out(shape, U8 if o['dst'] == 'bytes' else I32), 'B': B, 'N': N}


def _b_update_pieces(c, x):
    """The reference's inputs: the on-board neighbours of one point per board (off-board ones as -1), the side that moved."""
    N, B = c.n, c.b
    rs = np.random.default_rng(c.opts['seed'])
    p = rs.integers(0, N * N, size=B)
    r, q = p // N, p % N
    adj = np.stack([np.where(r > 0, p - N, -1), np.where(r < N - 1, p + N, -1), np.where(q > 0, p - 1, -1), np.where(q < N - 1, p + 1, -1)], axis=1)
    players = rs.integers(0, 2, size=B)
    return {'states': x.boards(N, B), 'adj': torch.from_numpy(adj.astype(np.int32)).to(x.dev), 'K': 4,
            'players': torch.from_numpy(players.astype(np.int32)).to(x.dev), 'killed': Out((B, N, N), U8) if _given(c, 'killed') else None,
            'B': B, 'N': N}


def _b_rng_seed(c, x):
    return {'rng': Out((c.b,), I64), 'base_seed': 1234567 + c.opts['seed'], 'first_game': 3 * c.n, 'B': c.b}


def _b_planes(c, x):
    N, B, o, dt = c.n, c.b, c.opts, c.dtypes['out']
    a = {params(c.fn)[0].name: x.boards(N, B, _layout(c)), 'out': Out((B, o['planes'], N, N), dt), 'out_dtype': OUT_CODES[dt], 'B': B, 'N': N}
    if 'orient' in c.roles:
        a['orient'] = torch.from_numpy(np.random.default_rng(o['seed']).integers(0, 8, size=B).astype(np.int32)).to(x.dev) if _given(c, 'orient') else None
    for flag in ('settled', 'aborted'):
        if flag in c.roles:
            a[flag] = Out((B,), U8) if _given(c, flag) else None
    return a


def _b_hash(c, x):
    return {params(c.fn)[0].name: x.boards(c.n, c.b, _layout(c)), 'out': Out((c.b,), I64), 'B': c.b, 'N': c.n}


def _b_move_hashes(c, x):
    """A history of garbage and of the boards' own hashes (so that nothing repeats by design, and the launch still compares)."""
    N, B, H, A = c.n, c.b, 3, c.n * c.n + 1
    rs = np.random.default_rng(c.opts['seed'])
    ring = _given(c, 'history')
    return {params(c.fn)[0].name: x.boards(N, B, _layout(c)), 'H': H, 'B': B, 'N': N,
            'history': torch.from_numpy(rs.integers(-2 ** 62, 2 ** 62, size=(B, H))).to(x.dev) if ring else None,
            'count': torch.from_numpy(rs.integers(-1, 6, size=B).astype(np.int32)).to(x.dev) if ring else None,
            'hashes': Out((B, A), I64) if _given(c, 'hashes') else None, 'repeat': Out((B, A), U8) if _given(c, 'repeat') else None,
            'rows': Out((B, N), I32) if _given(c, 'rows') else None}


def _b_past_push(c, x):
    """A ring of garbage with counts on either side of H, pushed where the mask byte is set (any non-zero byte of a uint8 mask)."""
    N, B, H = c.n, c.b, 3
    rs = np.random.default_rng(c.opts['seed'])
    mask = None
    if _given(c, 'mask'):
        m = rs.integers(0, 2, size=B) * (rs.integers(1, 256, size=B) if c.dtypes['mask'] == U8 else 1)
        mask = torch.from_numpy(m.astype(np.uint8)).to(x.dev).view(c.dtypes['mask'])
    return {params(c.fn)[0].name: x.boards(N, B, _layout(c)), 'mask': mask, 'H': H, 'B': B, 'N': N,
            'rows': torch.from_numpy(rs.integers(-2 ** 31, 2 ** 31, size=(B, H, 2, N)).astype(np.int32)).to(x.dev),
            'count': torch.from_numpy(rs.integers(0, 9, size=B).astype(np.int32)).to(x.dev)}


def _b_draw_orient(c, x):
    from gymgo_amd import gogame
    return {'rng': gogame.rng_seed(c.b, c.opts['seed'], 0, x.dev), 'orient': Out((c.b,), I32), 'B': c.b}


def _b_puct_legal(c, x):
    """Played leaf boards as a select round hands them on: tracked boards, a third of the slots empty (leaf_id -1)."""
    N, B = c.n, c.b
    ids = np.random.default_rng(c.opts['seed']).integers(0, 9, size=B).astype(np.int32)
    ids[::3] = -1
    return {'leaf': x.boards(N, B, 'tracked'), 'leaf_id': torch.from_numpy(ids).to(x.dev), 'B': B, 'N': N,
            'legal': Out((B, N * N + 1), torch.bool), 'live': Out((B,), torch.bool)}


def _b_children(c, x):
    N, B = c.n, c.b
    A, layout = N * N + 1, _layout(c)
    if layout == 'bytes':
        return {'states': x.boards(N, B), 'children': Out((B, A, 6, N, N), U8), 'B': B, 'N': N, 'canonical': c.opts['canonical']}
    return {'packed': x.boards(N, B, 'packed'), 'children': Out((B, A, packed_words(N)), I32), 'B': B, 'N': N, 'canonical': c.opts['canonical']}


def _b_children_offsets(c, x):
    return {'states': x.boards(c.n, c.b), 'offsets': Out((c.b + 1,), I32), 'order': Out((c.b,), I32) if _given(c, 'order') else None,
            'B': c.b, 'N': c.n}


def _b_children_compact(c, x):
    """offsets and order as gg_batch_children_offsets makes them for these states, on plain tensors."""
    from gymgo_amd import _lib
    N, B = c.n, c.b
    st = x.boards(N, B)
    offsets, order = torch.empty(B + 1, dtype=I32, device=x.dev), torch.empty(B, dtype=I32, device=x.dev)
    _lib.call('gg_batch_children_offsets', st, offsets, order, B, N, _lib.stream_ptr(x.dev))
    total = int(offsets[B])
    return {'states': st, 'offsets': offsets, 'order': order if _given(c, 'order') else None, 'children': Out((total, 6, N, N), U8),
            'B': B, 'N': N, 'canonical': c.opts['canonical']}


def _b_play_moves(c, x):
    N, B, T = c.n, c.b, c.opts['T']
    moves = torch.stack([_moves(c, x, B, c.opts['seed'] + t) for t in range(T)], dim=1).contiguous()
    return {params(c.fn)[0].name: x.boards(N, B, _layout(c)), 'moves': moves, 'played': Out((B,), I32) if _given(c, 'played') else None,
            'B': B, 'N': N, 'T': T}


def _b_symmetry(c, x):
    N, B, o = c.n, c.b, c.opts
    orient = None
    if _given(c, 'orient'):
        orient = torch.from_numpy(np.random.default_rng(o['seed']).integers(0, 8, size=B).astype(np.int32)).to(x.dev)
    views = () if orient is not None else (8,)
    if 'planes' in o:
        layout = 'packed' if o['planes'] == 3 else 'tracked'
        return {'in': x.boards(N, B, layout), 'planes': o['planes'], 'orient': orient, 'out': Out((B,) + views + (_words(layout, N),), I32),
                'B': B, 'N': N}
    return {'in': x.boards(N, B), 'orient': orient, 'out': Out((B,) + views + (6, N, N), U8), 'B': B, 'C': 6, 'N': N}


# ---- the Monte Carlo queue and the tree searches: scenarios on plain tensors, one per board size and child process

PO = dict(K=3, S=4, first_root=2, base_seed=99, max_plies=8, chunk_plies=4, komi=0.5, chunks=2)      # 15 jobs on 4 slots
MP = dict(K=2, S=4, first_root=1, base_seed=77, max_plies=8, chunk_plies=4, komi=0.5, chunks=2)      # 2 T jobs on 4 slots
UCT = dict(I=3, K=2, c=1.4)
PUCT = dict(I=4, c=1.25, komi=0.5)             # the tree the Gumbel calls run on too: C = 4 = 2 rounds of L = 2
GUMBEL = dict(L=2, c=1.25, S=4, c_visit=50.0, c_scale=1.0)


def _call(x, fn, *a):
    from gymgo_amd import _lib
    _lib.call(fn, *a, _lib.stream_ptr(x.dev))


def _search_roots(x, N):
    from gymgo_amd import gogame
    return gogame.batch_track(torch.from_numpy(x.pos(N)[list(SEARCH_ROOTS)]).to(x.dev))


def _zeros(x, shape, dtype=I32):
    return torch.zeros(shape, dtype=dtype, device=x.dev)


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


def _scenario(x, kind, N, make):
    key = (kind, N)
    if key not in x.scenarios:
        x.scenarios[key] = make(x, N)
        torch.cuda.synchronize()
    return x.scenarios[key]


def _queue_shapes(N, R, S, per_root):
    W = tracked_words(N)
    return {'slots': ((S, W), I32), 'rng': ((S,), I64), 'plies': ((S,), I64), 'job': ((S,), I64), 'counter': ((2,), I64),
            'counts': ((R,) + per_root + (4,), I32), 'sums': ((R,) + per_root + (2,), I64)}


def _s_playouts(x, N):
    """-> the roots and the queue's buffers as gg_playouts_begin leaves them."""
    R, p = len(SEARCH_ROOTS), PO
    roots = _search_roots(x, N)
    q = {name: _zeros(x, shape, dt) for name, (shape, dt) in _queue_shapes(N, R, p['S'], ()).items()}
    q['ownership'] = _zeros(x, (R, 2, N, N))
    _call(x, 'gg_playouts_begin', roots, R, N, p['K'], p['first_root'], p['base_seed'], p['max_plies'], p['chunk_plies'],
          q['slots'], q['rng'], q['plies'], q['job'], p['S'], q['counter'], q['counts'], q['sums'], q['ownership'])
    return {'roots': roots, 'begun': q}


def _b_playouts(c, x):
    N, R, p, o = c.n, c.b, PO, c.opts
    s = _scenario(x, 'playouts', N, _s_playouts)
    a = {'roots': s['roots'].clone(), 'R': R, 'N': N, 'K': p['K'], 'first_root': p['first_root'], 'base_seed': p['base_seed'],
         'max_plies': p['max_plies'], 'chunk_plies': p['chunk_plies'], 'S': p['S']}
    if o['stage'] == 'begin':
        a.update({name: Out(shape, dt) for name, (shape, dt) in _queue_shapes(N, R, p['S'], ()).items()})
        a['ownership'] = Out((R, 2, N, N), I32) if _given(c, 'ownership') else None
        return a
    a.update(_clone(s['begun']))
    if not _given(c, 'ownership'):
        a['ownership'] = None
    a.update(komi=p['komi'], chunks=p['chunks'])
    if o['policy'] is not None:
        a['policy'] = o['policy']
    return a


def _s_move_playouts(x, N):
    """-> the roots, offsets and plan of gg_move_playouts_plan, T, and the queue's buffers as gg_move_playouts_begin leaves them."""
    R, p, A = len(SEARCH_ROOTS), MP, N * N + 1
    roots = _search_roots(x, N)
    offsets, plan = _zeros(x, (R + 1,)), torch.full((R * A,), -1, dtype=I32, device=x.dev)
    _call(x, 'gg_move_playouts_plan', roots, R, N, offsets, plan)
    T = int(offsets[R])
    assert T * p['K'] > p['S'], 'fewer jobs than slots'
    q = {name: _zeros(x, shape, dt) for name, (shape, dt) in _queue_shapes(N, R, p['S'], (A,)).items()}
    _call(x, 'gg_move_playouts_begin', roots, R, N, plan, T, p['K'], p['first_root'], p['base_seed'], p['max_plies'], p['chunk_plies'],
          q['slots'], q['rng'], q['plies'], q['job'], p['S'], q['counter'], q['counts'], q['sums'])
    return {'roots': roots, 'plan': plan, 'T': T, 'begun': q}


def _b_move_playouts(c, x):
    N, R, p, o, A = c.n, c.b, MP, c.opts, c.n * c.n + 1
    s = _scenario(x, 'move_playouts', N, _s_move_playouts)
    if o['stage'] == 'plan':       # only the first T entries of plan are written: a buffer with content of the caller's
        return {'roots': s['roots'].clone(), 'R': R, 'N': N, 'offsets': Out((R + 1,), I32), 'plan': torch.full((R * A,), -7, dtype=I32, device=x.dev)}
    a = {'roots': s['roots'].clone(), 'R': R, 'N': N, 'plan': s['plan'].clone(), 'T': s['T'], 'K': p['K'], 'first_root': p['first_root'],
         'base_seed': p['base_seed'], 'max_plies': p['max_plies'], 'chunk_plies': p['chunk_plies'], 'S': p['S']}
    if o['stage'] == 'begin':
        a.update({name: Out(shape, dt) for name, (shape, dt) in _queue_shapes(N, R, p['S'], (A,)).items()})
        return a
    a.update(_clone(s['begun']))
    a.update(komi=p['komi'], chunks=p['chunks'])
    if o['policy'] is not None:
        a['policy'] = o['policy']
    return a


def _s_uct(x, N):
    """-> the tree after gg_uct_begin and one iteration (the state a select starts from), the leaves of the second select after
    their moves are played (the state a backup starts from), and made-up playout results."""
    R, I, K, A, W = len(SEARCH_ROOTS), UCT['I'], UCT['K'], N * N + 1, tracked_words(N)
    roots = _search_roots(x, N)
    t = {'boards': _zeros(x, (R, I + 1, W)), 'child': _zeros(x, (R, I + 1, A)), 'links': _zeros(x, (R, I + 1, 2)),
         'stats': _zeros(x, (R, I + 1, 4)), 'nodes': _zeros(x, (R,))}
    lf = {'leaf': _zeros(x, (R, W)), 'move': _zeros(x, (R,)), 'leaf_id': _zeros(x, (R,))}
    with np.errstate(divide='ignore'):
        log_table = torch.from_numpy(np.log(np.arange(I + 1, dtype=np.float64) * K)).to(x.dev)
    counts = torch.tensor([[1, 1, 0, 0], [2, 0, 0, 0], [0, 1, 1, 0], [0, 0, 1, 1], [1, 0, 0, 1]], dtype=I32, device=x.dev)[:R].contiguous()
    sums = torch.tensor([[3, 11], [-4, 16], [0, 9], [7, 12], [-1, 5]], dtype=I64, device=x.dev)[:R].contiguous()
    _call(x, 'gg_uct_begin', roots, R, N, I, K, t['boards'], t['child'], t['links'], t['stats'], t['nodes'])

    def select():
        _call(x, 'gg_uct_select', R, N, I, K, UCT['c'], log_table, t['boards'], t['child'], t['links'], t['stats'], t['nodes'],
              lf['leaf'], lf['move'], lf['leaf_id'])
        _call(x, 'gg_batch_play_moves_tracked', lf['leaf'], lf['move'], None, R, N, 1)

    select()
    _call(x, 'gg_uct_backup', R, N, I, K, counts, sums, None, t['boards'], t['links'], t['stats'], lf['leaf'], lf['move'], lf['leaf_id'])
    before_select = _clone(t)
    select()
    return {'roots': roots, 'log_table': log_table, 'counts': counts, 'sums': sums, 'select': before_select, 'backup': dict(_clone(t), **_clone(lf))}


def _b_uct(c, x):
    N, R, o, A, W, I, K = c.n, c.b, c.opts, c.n * c.n + 1, tracked_words(c.n), UCT['I'], UCT['K']
    s = _scenario(x, 'uct', N, _s_uct)
    a = {'R': R, 'N': N, 'I': I, 'K': K}
    if o['stage'] == 'begin':      # the boards of unused nodes are not written: content of the caller's
        a.update(roots=s['roots'].clone(), boards=torch.full((R, I + 1, W), 0x1234567, dtype=I32, device=x.dev), child=Out((R, I + 1, A), I32),
                 links=Out((R, I + 1, 2), I32), stats=Out((R, I + 1, 4), I32), nodes=Out((R,), I32))
    elif o['stage'] == 'select':
        a.update(_clone(s['select']))
        a.update(c=UCT['c'], log_table=s['log_table'].clone(), leaf=Out((R, W), I32), move=Out((R,), I32), leaf_id=Out((R,), I32))
    else:
        b = _clone(s['backup'])
        a.update(counts=s['counts'].clone(), sums=s['sums'].clone(), totals=_zeros(x, (R, 2), I64) + 5 if _given(c, 'totals') else None,
                 boards=b['boards'], links=b['links'], stats=b['stats'], leaf=b['leaf'], move=b['move'], leaf_id=b['leaf_id'])
    return a


def _s_puct(x, N):
    """-> the PUCT tree after gg_puct_begin and one iteration (what a select starts from), the played leaves of the second select
    (what a backup starts from) and the tree after two iterations (what the Gumbel calls start from), with a made-up evaluator."""
    R, I, A, W = len(SEARCH_ROOTS), PUCT['I'], N * N + 1, tracked_words(N)
    roots = _search_roots(x, N)
    g = torch.Generator().manual_seed(N)
    priors = torch.rand((R, A), generator=g).to(x.dev)
    priors = (priors / priors.sum(dim=1, keepdim=True)).contiguous()
    values = (torch.rand((R,), generator=g) * 2 - 1).to(x.dev)
    t = {'boards': _zeros(x, (R, I + 1, W)), 'child': _zeros(x, (R, I + 1, A)), 'prior': _zeros(x, (R, I + 1, A), F32),
         'links': _zeros(x, (R, I + 1, 2)), 'stats': _zeros(x, (R, I + 1, 4)), 'nodes': _zeros(x, (R,))}
    lf = {'leaf': _zeros(x, (R, W)), 'move': _zeros(x, (R,)), 'leaf_id': _zeros(x, (R,))}
    _call(x, 'gg_puct_begin', roots, R, N, I, *[t[k] for k in _TREE])

    def select():
        _call(x, 'gg_puct_select', R, N, I, PUCT['c'], *[t[k] for k in _TREE], *[lf[k] for k in _LEAF])
        _call(x, 'gg_batch_play_moves_tracked', lf['leaf'], lf['move'], None, R, N, 1)

    def backup():
        _call(x, 'gg_puct_backup', R, N, I, PUCT['komi'], priors, values, t['boards'], t['prior'], t['links'], t['stats'], *[lf[k] for k in _LEAF])

    select()
    backup()
    before_select = _clone(t)
    select()
    before_backup = dict(_clone(t), **_clone(lf))
    backup()
    return {'roots': roots, 'priors': priors, 'values': values, 'select': before_select, 'backup': before_backup, 'tree': _clone(t)}


def _b_puct(c, x):
    N, R, o, A, W, I = c.n, c.b, c.opts, c.n * c.n + 1, tracked_words(c.n), PUCT['I']
    s = _scenario(x, 'puct', N, _s_puct)
    a = {'R': R, 'N': N, 'I': I}
    if o['stage'] == 'begin':      # the boards of unused nodes are not written: content of the caller's
        a.update(roots=s['roots'].clone(), boards=torch.full((R, I + 1, W), 0x1234567, dtype=I32, device=x.dev), child=Out((R, I + 1, A), I32),
                 prior=Out((R, I + 1, A), F32), links=Out((R, I + 1, 2), I32), stats=Out((R, I + 1, 4), I32), nodes=Out((R,), I32))
    elif o['stage'] == 'select':
        a.update(_clone(s['select']))
        a.update(c=PUCT['c'], leaf=Out((R, W), I32), move=Out((R,), I32), leaf_id=Out((R,), I32))
    else:
        b = _clone(s['backup'])
        a.update(komi=PUCT['komi'], priors=s['priors'].clone(), values=s['values'].clone(), boards=b['boards'], prior=b['prior'], links=b['links'],
                 stats=b['stats'], leaf=b['leaf'], move=b['move'], leaf_id=b['leaf_id'])
    return a


PAST = dict(H=3, T=3, moves=1)           # gg_past_planes(3, 1) = 2 T + T - 1 = 8 planes
OUT_CODES = {**W_CODES, U8: 3}           # GG_FEAT_U8


def _b_puct_past(c, x):
    """The played leaves of the PUCT scenario's second select (L = 1) with the tree they come from, and a ring of garbage rows:
    every row read from a ring is masked to the board."""
    N, R, C, p = c.n, c.b, PUCT['I'], PAST
    b = _clone(_scenario(x, 'puct', N, _s_puct)['backup'])
    rs = np.random.default_rng(70 + N)
    ring = _given(c, 'rows')
    return {'R': R, 'N': N, 'C': C, 'L': 1, 'boards': b['boards'], 'links': b['links'], 'H': p['H'], 'T': p['T'], 'moves': p['moves'],
            'rows': torch.from_numpy(rs.integers(-2 ** 31, 2 ** 31, size=(R, p['H'], 2, N)).astype(np.int32)).to(x.dev) if ring else None,
            'count': torch.from_numpy(rs.integers(0, 6, size=R).astype(np.int32)).to(x.dev) if ring else None,
            'leaf': b['leaf'], 'leaf_id': b['leaf_id'],
            'orient': torch.from_numpy(rs.integers(0, 8, size=R).astype(np.int32)).to(x.dev) if _given(c, 'orient') else None,
            'out': Out((R, 2 * p['T'] + p['T'] - 1, N, N), c.dtypes['out']), 'out_dtype': OUT_CODES[c.dtypes['out']]}


def _s_gumbel(x, N):
    """-> base, the schedule seq(2, 4) and what gg_gumbel_begin leaves on the PUCT scenario's tree after two iterations."""
    R, C, A = len(SEARCH_ROOTS), PUCT['I'], N * N + 1
    t = _scenario(x, 'puct', N, _s_puct)['tree']
    base = torch.randn((R, A), generator=torch.Generator().manual_seed(50 + N)).to(x.dev)
    seq = torch.tensor([0, 0, 1, 1], dtype=I32, device=x.dev)
    seen, done = _zeros(x, (R, A)), _zeros(x, (R,)) + 9
    _call(x, 'gg_gumbel_begin', R, N, C, t['child'], t['stats'], t['nodes'], seen, done)
    return {'base': base, 'seq': seq, 'seen': seen, 'done': done}


def _b_gumbel(c, x):
    N, R, o, A, W, C, p = c.n, c.b, c.opts, c.n * c.n + 1, tracked_words(c.n), PUCT['I'], GUMBEL
    t = _clone(_scenario(x, 'puct', N, _s_puct)['tree'])
    s = _scenario(x, 'gumbel', N, _s_gumbel)
    a = {'R': R, 'N': N, 'C': C}
    if o['stage'] == 'begin':
        a.update(child=t['child'], stats=t['stats'], nodes=t['nodes'], seen=Out((R, A), I32), done=Out((R,), I32))
    elif o['stage'] == 'select':
        L = p['L']
        a.update(t)
        a.update(L=L, c=p['c'], base=s['base'].clone(), seen=s['seen'].clone(), done=s['done'].clone(), seq=s['seq'].clone(), S=p['S'],
                 c_visit=p['c_visit'], c_scale=p['c_scale'], leaf=Out((R * L, W), I32), move=Out((R * L,), I32), leaf_id=Out((R * L,), I32))
    else:
        a.update(boards=t['boards'], child=t['child'], stats=t['stats'], nodes=t['nodes'], base=s['base'].clone(), seen=s['seen'].clone(),
                 c_visit=p['c_visit'], c_scale=p['c_scale'], actions=Out((R,), I32), q=Out((R, A), F32) if _given(c, 'q') else None,
                 visits=Out((R, A), I32) if _given(c, 'visits') else None, value=Out((R,), F32) if _given(c, 'value') else None)
    return a


BUILDERS = {'planes': _b_planes, 'hash': _b_hash, 'move_hashes': _b_move_hashes, 'past_push': _b_past_push, 'puct_past': _b_puct_past, 'playouts': _b_playouts, 'move_playouts': _b_move_playouts, 'uct': _b_uct, 'puct': _b_puct, 'gumbel': _b_gumbel,
            'rollout': _b_rollout, 'next_states': _b_next_states, 'env_step': _b_env_step, 'invalid_mask': _b_invalid_mask, 'areas': _b_areas,
            'board_plane': _b_board_plane, 'sample': _b_sample, 'sample_weighted': _b_sample_weighted, 'reset': _b_reset, 'convert': _b_convert,
            'update_pieces': _b_update_pieces, 'rng_seed': _b_rng_seed, 'children': _b_children, 'children_offsets': _b_children_offsets,
            'children_compact': _b_children_compact, 'draw_orient': _b_draw_orient, 'puct_legal': _b_puct_legal, 'play_moves': _b_play_moves, 'symmetry': _b_symmetry}


# ------------------------------------------------------------------------------------------------ the oracle

def _as_bytes(c, t):
    from gymgo_amd import gogame
    layout = _layout(c)
    t = t.clone()               # (a plain allocation: the conversions are not the call under test)
    return (t if layout == 'bytes' else gogame.batch_unpack(t, c.n) if layout == 'packed' else gogame.batch_untrack(t)).cpu().numpy()


def _o_rollout(c, x, ins, got):
    from oracle import c_oracle
    first = params(c.fn)[0].name
    want, want_rng, want_last = c_oracle.batch_rollout(x.pos(c.n)[:c.b], ins['rng'].cpu().numpy().view(np.uint64), c.opts['plies'], bool(c.opts['auto']))
    bad = []
    if not np.array_equal(_as_bytes(c, got[first]), want):
        bad.append('boards != oracle')
    if not np.array_equal(got['rng'].cpu().numpy().view(np.uint64), want_rng):
        bad.append('generators != oracle')
    if 'last_actions' in got and not np.array_equal(got['last_actions'].cpu().numpy(), want_last):
        bad.append('last actions != oracle')
    return bad


def _o_next_states(c, x, ins, got):
    from oracle import c_oracle
    want, status = c_oracle.batch_next_states(x.pos(c.n)[:c.b], ins['actions'].cpu().numpy(), bool(c.opts['canonical']))
    bad = [] if np.array_equal(_as_bytes(c, got['out']), want) else ['next states != oracle']
    if 'status' in got and not np.array_equal(got['status'].cpu().numpy(), status):
        bad.append('status != oracle')
    return bad


def _o_invalid_mask(c, x, ins, got):
    from oracle import c_oracle
    host = x.pos(c.n)[:c.b]
    ko = ins['ko'].cpu().numpy() if 'ko' in ins else np.full(c.b, -1)
    want = np.stack([c_oracle.compute_invalid_moves(host[i], 1 - int(host[i, 2, 0, 0]), int(ko[i])) for i in range(c.b)])
    return [] if np.array_equal(got['mask'].cpu().numpy(), want) else ['mask != oracle']


def _o_areas(c, x, ins, got):
    from oracle import c_oracle
    wb, ww = c_oracle.batch_areas(x.pos(c.n)[:c.b])
    return [] if np.array_equal(got['black'].cpu().numpy(), wb) and np.array_equal(got['white'].cpu().numpy(), ww) else ['areas != oracle']


def _o_children(c, x, ins, got):
    from oracle import c_oracle
    want = c_oracle.batch_children(x.pos(c.n)[:c.b], bool(c.opts['canonical']))
    return [] if np.array_equal(got['children'].cpu().numpy(), want) else ['children != oracle']


def _kept(start):
    """valid_moves() per parent: the points whose plane-3 byte is 0 and the pass; all of them once the game has ended."""
    k = len(start)
    keep = np.concatenate([start[:, 3].reshape(k, -1) == 0, np.ones((k, 1), bool)], axis=1)
    keep[start[:, 5, 0, 0] == 1] = True
    return keep


def _o_children_offsets(c, x, ins, got):
    keep = _kept(x.pos(c.n)[:c.b])
    want = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    bad = [] if 'offsets' not in got or np.array_equal(got['offsets'].cpu().numpy(), want) else ['offsets != expectation']
    if 'order' in got:
        order, count = got['order'].cpu().numpy(), keep.sum(axis=1)
        if sorted(order.tolist()) != list(range(c.b)) or (np.diff(count[order]) > 0).any():
            bad.append('order is no permutation by falling child count')
    return bad


def _o_children_compact(c, x, ins, got):
    from oracle import c_oracle
    start = x.pos(c.n)[:c.b]
    want = c_oracle.batch_children(start, bool(c.opts['canonical']))[_kept(start)]
    return [] if np.array_equal(got['children'].cpu().numpy(), want) else ['un-padded children != oracle']


def _o_update_pieces(c, x, ins, got):
    from oracle import c_oracle
    start, adj, players = x.pos(c.n)[:c.b], ins['adj'].cpu().numpy(), ins['players'].cpu().numpy()
    want = [c_oracle.update_pieces(start[i], adj[i][adj[i] >= 0], int(players[i])) for i in range(c.b)]
    bad = [] if np.array_equal(got['states'].cpu().numpy(), np.stack([w[0] for w in want])) else ['states != oracle']
    if 'killed' in got and not np.array_equal(got['killed'].cpu().numpy(), np.stack([w[1] for w in want])):
        bad.append('killed != oracle')
    return bad


ORACLES = {'rollout': _o_rollout, 'next_states': _o_next_states, 'invalid_mask': _o_invalid_mask, 'areas': _o_areas, 'children': _o_children,
           'children_offsets': _o_children_offsets, 'children_compact': _o_children_compact, 'update_pieces': _o_update_pieces}


# ------------------------------------------------------------------------------------------------ one case on the device

def plain_prefill(shape, dtype, device):
    """What an `out` tensor of the plain run holds before the call: bytes 0x40 | ((i * 29) & 0x3F) - bit 7 clear where the arena's
    fill has it set, so an element neither run writes differs between the two."""
    n = guard_arena._numel(shape) * guard_arena.element_size(dtype)
    i = torch.arange(n, dtype=torch.int64, device=device)
    return (((i * 29) & 0x3F) | 0x40).to(U8).view(dtype).view(tuple(shape))


def _first_difference(a, b):
    d = (a.reshape(-1).view(U8) != b.reshape(-1).view(U8)).nonzero()
    return int(d[0]) // a.element_size() if d.numel() else None


def describe(c, res):
    opts = ' '.join('%s=%s' % kv for kv in sorted(c.opts.items()) if kv[0] not in ('build', 'oracle', 'seed', 'by_rule', 'slotwise', 'empty', 'empty_writes', 'align', 'demand'))
    ptrs = ' '.join('%s:%s' % (name, 'NULL' if c.roles[name] == 'null' else '%s@%d' % (c.roles[name], res[name])) for name, _ in pointer_params(c.fn))
    return '%s N=%d B=%d %s [%s]' % (c.fn, c.n, c.b, opts, ptrs)


def run_case(c, res, x, oracle=True):
    """One case on the device -> a list of findings (empty: the case holds).  1. the call on arena views returns 0; 2. no guard
    byte and no `in` region changed; 3. every `out` / `inout` region is bit-equal to the same call on plain, separately
    allocated tensors whose `out` tensors start from another fill (so every element of an `out` region was written: no case of
    this table declares an element that a call leaves alone); 4. where oracle/c_oracle.py has the call, the arena's outputs equal the
    oracle's bit for bit; 5. the same call with B = 0 returns 0 and changes no byte of the arena, regions included; 6. a pointer
    a header demands 16 bytes of (opts['demand']) is refused with GG_E_BADARG 8 bytes off.  Three options say where a header
    leaves an output open, and how it is held instead: by_rule (step 3), slotwise (after step 3), empty_writes (step 5)."""
    from gymgo_amd import _lib
    args = BUILDERS[c.opts['build']](c, x)
    ps = [p for p in params(c.fn) if p.name != 'hip_stream']
    assert sorted(args) == sorted(p.name for p in ps), (c.fn, sorted(args), [p.name for p in ps])
    pointers = [name for name, _ in pointer_params(c.fn)]
    shapes = {}
    for name in pointers:
        v = args[name]
        assert (v is None) == (c.roles[name] == 'null'), (c.fn, name)
        if v is not None:
            shapes[name] = (tuple(v.shape), v.dtype)
            assert v.dtype == pointer_dtype(c, name), (c.fn, name, v.dtype)
    demanded = [name for name in c.opts.get('demand', ()) if name in shapes]
    arena = guard_arena.Arena(sum(guard_arena.footprint(s, d) for s, d in shapes.values())
                              + sum(guard_arena.footprint(*shapes[name]) for name in demanded) + 64, x.dev)
    views, plain, ins = {}, {}, {}
    for name in pointers:
        if name not in shapes:
            continue
        v, role = args[name], c.roles[name]
        views[name] = arena.take(name, shapes[name][0], shapes[name][1], res[name], readonly=role == 'in')
        if isinstance(v, Out):
            assert role == 'out', (c.fn, name, role)
            plain[name] = plain_prefill(v.shape, v.dtype, x.dev)
        else:
            assert role in ('in', 'inout'), (c.fn, name, role)
            views[name].copy_(v)
            plain[name], ins[name] = v.clone(), v
    stream = _lib.stream_ptr(x.dev)

    def invoke(buffers, **scalars):
        try:
            _lib.call(c.fn, *[buffers.get(p.name) if p.name in pointers else scalars.get(p.name, args[p.name]) for p in ps], stream)
        except _lib.GymGoNativeError as e:
            return str(e)
        return None

    found = []
    arena.snapshot()
    err = invoke(views)
    torch.cuda.synchronize()
    if err:
        return ['the call between guards: ' + err]
    found += ['%s: %s changed at offset %d' % (name, {'before': 'the guard before it', 'after': 'the guard after it',
                                                         'inside': 'the read-only region'}[side], off)
              for name, side, off in arena.violations()]
    err = invoke(plain)
    torch.cuda.synchronize()
    if err:
        return found + ['the call on plain tensors: ' + err]
    got = {}
    for name in pointers:
        if name in views and c.roles[name] != 'in':
            got[name] = views[name]
            if name in c.opts.get('by_rule', ()):
                # the header defines this output by a rule that leaves ties open, and the kernel settles them with atomics
                # (`order` of gg_batch_children_offsets): two runs may differ, so the case's oracle holds BOTH runs against the
                # rule instead - which no element of either prefill satisfies, so every element was written
                assert c.opts.get('oracle')
                found += ['plain run: ' + f for f in ORACLES[c.opts['oracle']](c, x, ins, {name: plain[name]})]
                continue
            if name in c.opts.get('slotwise', ()):
                continue
            at = _first_difference(views[name], plain[name])
            if at is not None:
                row = guard_arena._numel(shapes[name][0][1:])
                found.append('%s differs from the plain run at element %d (row %d, element %d of the row)' % (name, at, at // row, at % row))
    if c.opts.get('slotwise'):
        # the working slots of the playout queue are opaque (include/gymgo_amd.h), and WHICH slot a job lands in is settled by an
        # atomic on the queue's counter (gg_po.h): two runs hold the same slots in another order.  A slot is its whole record -
        # job word (the job id, or the (root, move) pair in the first-move family, where several slots share one), generator,
        # ply count and board -, and the two runs must hold the same records as a multiset: compared always, after sorting the
        # records of each run.  Every result of the call (counter, counts, sums, ownership) is compared bit for bit above
        def records(buffers):
            cols = [buffers[name].reshape(buffers[name].shape[0], -1).to(torch.int64).cpu() for name in ('job', 'rng', 'plies', 'slots')]
            return sorted(tuple(row) for row in torch.cat(cols, dim=1).tolist())

        ra, rp = records(views), records(plain)
        if ra != rp:
            k = next(i for i, (u, v) in enumerate(zip(ra, rp)) if u != v)
            found.append('the slots are not those of the plain run in another order: sorted record %d starts %s / %s' % (k, ra[k][:3], rp[k][:3]))
    if oracle and c.opts.get('oracle'):
        found += ORACLES[c.opts['oracle']](c, x, ins, got)
    # the empty batch and the refused call: all pointers valid, no byte of the arena changes.  Every region the full call wrote
    # gets the arena's fill back first, so that a store of what is already there cannot go unseen
    # (the `inout` regions after the refused call only: should it not be refused, it runs on what the full call left)
    for name in views:
        if c.roles[name] == 'out':
            arena.refill(name)
        arena.set_readonly(name)
    # a pointer for which the header demands more than its element's alignment stands where the header wants it above; here, once,
    # 8 bytes off (an input with the same content, an output with the fill): GG_E_BADARG before any device work
    for name in demanded:
        off = arena.take(name + ' (8 bytes off)', shapes[name][0], shapes[name][1], 8, readonly=True)
        if not isinstance(args[name], Out):
            off.copy_(args[name])
        arena.snapshot()
        err = invoke(dict(views, **{name: off}))
        torch.cuda.synchronize()
        if err is None or 'code -3' not in err:
            found.append('%s 8 bytes off a 16-byte boundary: %s, not GG_E_BADARG' % (name, err or 'the call returned 0'))
        found += ['%s 8 bytes off: %s changed (%s, offset %d)' % ((name,) + v) for v in arena.violations()]
    # What a header defines for an empty batch is written, in the open (opts['empty_writes']: these regions stay writable, every
    # other region and every guard is held, and what they hold afterwards is asserted):
    #   'queue'    gg_playouts_begin / gg_move_playouts_begin make the queue whatever R is (counter = {m, R K + m}, m = min(S, R K),
    #              the other slots empty): R = 0 writes an EMPTY queue, which the drivers poll - counter must read {0, 0}
    #   'offsets'  gg_batch_children_offsets / gg_move_playouts_plan write offsets[B] = the total whatever B is: B = 0 writes
    #              offsets[0] = 0 and no other byte of offsets
    for name in views:
        if c.roles[name] == 'inout':
            arena.refill(name)
    kind = c.opts.get('empty_writes')
    for name in {'queue': _SLOTS + ('counter',), 'offsets': ('offsets',), None: ()}[kind]:
        arena.set_readonly(name, False)
    batch = 'B' if 'B' in args else 'R'
    arena.snapshot()
    before = {name: v.clone() for name, v in views.items()}
    err = invoke(views, **dict(c.opts.get('empty', {}), **{batch: 0}))
    torch.cuda.synchronize()
    if err:
        found.append('the empty batch: ' + err)
    if kind == 'queue' and views['counter'].tolist() != [0, 0]:
        found.append('the empty batch: counter is %s, not {0, 0}' % views['counter'].tolist())
    if kind == 'offsets':
        before['offsets'][0] = 0
        if not torch.equal(views['offsets'], before['offsets']):
            found.append('the empty batch: offsets is not the fill with offsets[0] = 0')
    found += ['the empty batch: %s changed (%s, offset %d)' % v for v in arena.violations()]
    return found
