"""`gogame`-compatible function library over the HIP kernels (mirrors gym_go/gogame.py:22-468:
same names, positional order, return shapes and error behaviour).

Containers
  * torch uint8 device tensors ([6,N,N] / [B,6,N,N]) are the native form: results are device tensors.
  * NumPy arrays (the reference's float64 states) are accepted everywhere for drop-in use: they are
    moved to the device, run through the same kernels, and the result comes back as a NumPy array of
    the input dtype.  Nothing is ever computed on the CPU.
Errors: an illegal move raises AssertionError (gym_go/gogame.py:59, :117); action_size() without
arguments raises RuntimeError (:196).
"""
import collections
import math
import os
import weakref

import numpy as np
import torch

from gymgo_amd import _lib, govars

_U8, _I32, _I64 = torch.uint8, torch.int32, torch.int64


def _device():
    if not torch.cuda.is_available():
        raise _lib.GymGoNativeError('no ROCm device visible; gymgo_amd has no CPU path')
    return torch.device('cuda', torch.cuda.current_device())


class _Box:
    """Remembers how the caller passed a state so results go back in the same form."""

    def __init__(self, x):
        self.numpy = not isinstance(x, torch.Tensor)
        if self.numpy:
            x = np.asarray(x)
            self.np_dtype = x.dtype if x.dtype != np.bool_ else np.dtype(np.uint8)
            self.t = torch.from_numpy(np.ascontiguousarray(x).astype(np.uint8, copy=False)).to(_device())
        else:
            if not x.is_cuda:
                raise _lib.GymGoNativeError('state tensors must live on the ROCm device')
            self.t = x.to(_U8).contiguous()

    def back(self, t, dtype=None):
        if self.numpy:
            return t.cpu().numpy().astype(dtype or self.np_dtype)
        return t


def _actions_tensor(actions, B, device):
    if isinstance(actions, torch.Tensor):
        a = actions.to(device=device, dtype=_I32).contiguous()
    else:
        a = torch.as_tensor(np.asarray(actions).astype(np.int32), device=device)
    if a.numel() != B:
        raise ValueError('need one action per state (%d != %d)' % (a.numel(), B))
    return a.reshape(B)


# ------------------------------------------------------------------ raw device calls

def next_states_workspace(batch_size, board_size, device=None):
    """A zero-filled workspace for batch_next_states(..., workspace=): int32 [B, 5N+1] on the device."""
    return torch.zeros((batch_size, tracked_words(board_size)), dtype=_I32, device=device or _device())


def _next_states_dev(states, actions, canonical, out=None, status=None, workspace=None):
    B, C, N, _ = states.shape
    if out is None:
        out = torch.empty_like(states)
    elif out.shape != states.shape:
        raise ValueError('out must have the shape of the states %s' % (tuple(states.shape),))
    if status is None:
        status = torch.empty(B, dtype=_I32, device=states.device)
    if workspace is not None and tuple(workspace.shape) != (B, 5 * N + 1):
        raise ValueError('workspace must be int32 [B, 5N+1] (gogame.next_states_workspace)')
    name, ws = ('gg_batch_next_states', ()) if workspace is None else ('gg_batch_next_states_ws', (workspace,))
    _lib.call(name, states, actions, out, status, *ws, B, N, int(bool(canonical)), _lib.stream_ptr(states.device))
    return out, status


def _children_dev(states, canonical, out=None):
    B, C, N, _ = states.shape
    if out is None:
        out = torch.empty((B, N * N + 1, C, N, N), dtype=_U8, device=states.device)
    elif tuple(out.shape) != (B, N * N + 1, C, N, N):
        raise ValueError('out must be [B, N*N+1, 6, N, N]')
    _lib.call('gg_batch_children', states, out, B, N, int(bool(canonical)), _lib.stream_ptr(states.device))
    return out


def _children_offsets_dev(states, offsets=None, order=None):
    """(offsets int32 [B+1], order int32 [B]) of gg_batch_children_offsets: exclusive prefix sums of the number of children
    valid_moves() keeps per state, and the states by falling count (the launch order of the expansion)."""
    B, C, N, _ = states.shape
    if offsets is None:
        offsets = torch.empty(B + 1, dtype=_I32, device=states.device)
    elif offsets.numel() < B + 1:          # the launch writes offsets[0 .. B]
        raise ValueError('offsets must hold at least B + 1 = %d int32 (got %d)' % (B + 1, offsets.numel()))
    if order is None:
        order = torch.empty(max(B, 1), dtype=_I32, device=states.device)
    elif order.numel() < B:
        raise ValueError('order must hold at least B = %d int32 (got %d)' % (B, order.numel()))
    _lib.call('gg_batch_children_offsets', states, offsets, order, B, N, _lib.stream_ptr(states.device))
    return offsets, order


def _children_compact_dev(states, canonical, offsets=None, out=None):
    """The un-padded children of every state, concatenated (gg_batch_children_compact) -> (children uint8 [total, 6, N, N],
    offsets int32 [B+1]).  `out`: a caller-owned buffer of at least offsets[B] boards; with the upper bound
    B * (N*N+1) no device -> host read of the total is needed and the launches can be captured in a graph, a smaller buffer
    is checked against the total (one host read) and refused when it is too short."""
    B, C, N, _ = states.shape
    offsets, order = _children_offsets_dev(states, offsets)
    if out is None:
        total = int(offsets[B].item())            # (the one host read of the un-padded form: the size of its result)
        out = torch.empty((total, C, N, N), dtype=_U8, device=states.device)
    elif out.dim() != 4 or tuple(out.shape[1:]) != (C, N, N):
        raise ValueError('out must be [n >= total children, 6, N, N]')
    elif out.shape[0] < B * (N * N + 1):
        # smaller than the upper bound: the true total has to be read back once, or the launch could write past the end
        total = int(offsets[B].item())
        if out.shape[0] < total:
            raise ValueError('out holds %d boards, the un-padded children of this batch are %d' % (out.shape[0], total))
    _lib.call('gg_batch_children_compact', states, offsets, order, out, B, N, int(bool(canonical)), _lib.stream_ptr(states.device))
    return out, offsets


def _areas_dev(states, out=None):
    B, C, N, _ = states.shape
    if out is None:
        black = torch.empty(B, dtype=_I32, device=states.device)
        white = torch.empty(B, dtype=_I32, device=states.device)
    else:
        black, white = out
    _lib.call('gg_batch_areas', states, black, white, B, N, _lib.stream_ptr(states.device))
    return black, white


def _invalid_mask_dev(states, ko=None):
    B, C, N, _ = states.shape
    mask = torch.empty((B, N, N), dtype=_U8, device=states.device)
    _lib.call('gg_batch_invalid_mask', states, ko, mask, B, N, _lib.stream_ptr(states.device))
    return mask


# ------------------------------------------------------------------ gogame API

def init_state(size, device=None):
    """gym_go/gogame.py:22-25.  NumPy float64 zeros like the reference, or a device uint8 tensor."""
    if device is None:
        return np.zeros((govars.NUM_CHNLS, size, size))
    return torch.zeros((govars.NUM_CHNLS, size, size), dtype=_U8, device=device)


def batch_init_state(batch_size, board_size, device=None):
    """gym_go/gogame.py:28-31."""
    if device is None:
        return np.zeros((batch_size, govars.NUM_CHNLS, board_size, board_size))
    return torch.zeros((batch_size, govars.NUM_CHNLS, board_size, board_size), dtype=_U8, device=device)


def next_state(state, action1d, canonical=False):
    """gym_go/gogame.py:34-87.  Input is never mutated; illegal point -> AssertionError."""
    box = _Box(state)
    N = box.t.shape[-1]
    actions = torch.tensor([int(action1d)], dtype=_I32, device=box.t.device)
    out, status = _next_states_dev(box.t[None], actions, canonical)
    if int(status[0]) != 0:
        a = int(action1d)
        raise AssertionError(('Invalid move', (a // N, a % N)))
    return box.back(out[0])


def batch_next_states(batch_states, batch_action1d, canonical=False, check=True, out=None, status=None, workspace=None):
    """gym_go/gogame.py:90-150, with next_state's semantics for every game (also when the batch
    contains passes, where the reference mis-aligns games: gym_go/state_utils.py:187-193).
    check=True (default) synchronises to raise AssertionError like :117 if any move is illegal;
    check=False returns (next_states, status) without a host sync - illegal rows pass through.
    out / status (device tensors, optional): caller-owned result buffers - a per-ply loop that ping-pongs two
    state tensors then allocates nothing per call.
    workspace (gogame.next_states_workspace(B, N), optional): lets a loop that feeds each output back as the next
    input skip the from-scratch liberty analysis (gg_batch_next_states_ws): the classes of the last outputs are kept
    there and reused for every board whose stones match exactly; results are identical with and without it."""
    if (out is not None and isinstance(batch_states, torch.Tensor) and isinstance(batch_action1d, torch.Tensor)
            and batch_states.dtype == _U8 and batch_action1d.dtype == _I32 and not check):
        # hot loop: device tensors in the native dtypes, nothing to convert
        return _next_states_dev(batch_states, batch_action1d, canonical, out, status, workspace)
    box = _Box(batch_states)
    B = box.t.shape[0]
    actions = _actions_tensor(batch_action1d, B, box.t.device)
    out, status = _next_states_dev(box.t, actions, canonical, out, status, workspace)
    if not check:
        return box.back(out), status
    if B and bool((status != 0).any()):
        raise AssertionError('Invalid move in batch at games %s' % torch.nonzero(status).flatten()[:8].tolist())
    return box.back(out)


def invalid_moves(state):
    """gym_go/gogame.py:153-157: plane 3 flattened + [0] for pass; all zeros once the game ended."""
    box = _Box(state)
    t = box.t
    n = t.shape[-1] * t.shape[-2] + 1
    res = torch.zeros(n, dtype=_U8, device=t.device)
    if not game_ended(t):
        res[:-1] = t[govars.INVD_CHNL].reshape(-1)
    return box.back(res, np.float64 if box.numpy else None)


def valid_moves(state):
    """gym_go/gogame.py:160-161."""
    return 1 - invalid_moves(state)


def batch_invalid_moves(batch_state):
    """gym_go/gogame.py:164-168 (no game-over special case, like the reference)."""
    box = _Box(batch_state)
    t = box.t
    n = t.shape[0]
    flat = t[:, govars.INVD_CHNL].reshape(n, -1)
    res = torch.cat([flat, torch.zeros((n, 1), dtype=_U8, device=t.device)], dim=1)
    return box.back(res, np.float64 if box.numpy else None)


def batch_valid_moves(batch_state):
    """gym_go/gogame.py:171-172."""
    return 1 - batch_invalid_moves(batch_state)


def children(state, canonical=False, padded=True):
    """gym_go/gogame.py:175-186.  padded=True -> [N*N+1, 6, N, N] with all-zero slots for invalid
    actions; padded=False -> only the valid actions' successors, ascending action order."""
    box = _Box(state)
    if not padded:      # gym_go/gogame.py:179: only the successors of the valid actions - written by the device as such
        return box.back(_children_compact_dev(box.t[None], canonical)[0])
    return box.back(_children_dev(box.t[None], canonical)[0])


def batch_children(batch_states, canonical=False, padded=True, out=None, offsets=None):
    """BASELINE.json config 5 (no reference counterpart: == stack(children(s) for s in states)).
    padded=True -> [B, N*N+1, 6, N, N]; out (optional): a caller-owned uint8 device tensor of that shape to expand into
    (6.4 GB at config 5).
    padded=False -> (children [total, 6, N, N], offsets int32 [B+1]): the un-padded children of every state concatenated
    (== cat(children(s, padded=False) for s in states)); state b's are children[offsets[b]:offsets[b+1]].  On mid-game
    19x19 positions a third of the padded bytes.  out / offsets (optional): caller-owned buffers (out: at least `total`
    boards, e.g. B * (N*N+1); then nothing is read back to the host)."""
    box = _Box(batch_states)
    if not padded:
        kids, offs = _children_compact_dev(box.t, canonical, offsets, out)
        if box.numpy:
            offs = offs.cpu().numpy()
            return box.back(kids[:int(offs[-1])]), offs
        return kids, offs
    return box.back(_children_dev(box.t, canonical, out))


def action_size(state=None, board_size: int = None):
    """gym_go/gogame.py:189-197."""
    if state is not None:
        m, n = state.shape[1:]
    elif board_size is not None:
        m, n = board_size, board_size
    else:
        raise RuntimeError('No argument passed')
    return m * n + 1


def _plane_any(state, chnl):
    if isinstance(state, torch.Tensor):
        return bool((state[chnl] == 1).any())
    return bool(np.max(np.asarray(state)[chnl] == 1))


def prev_player_passed(state):
    """gym_go/gogame.py:200-201."""
    return _plane_any(state, govars.PASS_CHNL)


def batch_prev_player_passed(batch_state):
    """gym_go/gogame.py:204-205."""
    if isinstance(batch_state, torch.Tensor):
        return batch_state[:, govars.PASS_CHNL].amax(dim=(1, 2)) == 1
    return np.max(batch_state[:, govars.PASS_CHNL], axis=(1, 2)) == 1


def game_ended(state):
    """gym_go/gogame.py:208-214: 0/1."""
    if isinstance(state, torch.Tensor):
        return int(bool((state[govars.DONE_CHNL] == 1).all()))
    m, n = state.shape[1:]
    return int(np.count_nonzero(np.asarray(state)[govars.DONE_CHNL] == 1) == m * n)


def batch_game_ended(batch_state):
    """gym_go/gogame.py:217-222."""
    if isinstance(batch_state, torch.Tensor):
        return batch_state[:, govars.DONE_CHNL].amax(dim=(1, 2))
    return np.max(batch_state[:, govars.DONE_CHNL], axis=(1, 2))


def areas(state):
    """gym_go/gogame.py:275-300 (Tromp-Taylor) -> (black_area, white_area)."""
    box = _Box(state)
    b, w = _areas_dev(box.t[None])
    if box.numpy:
        return np.float64(int(b[0])), np.float64(int(w[0]))
    return b[0], w[0]


def batch_areas(batch_state, out=None):
    """gym_go/gogame.py:303-310 -> two [B] arrays.  out (optional): (black, white) int32 device tensors to write into."""
    box = _Box(batch_state)
    b, w = _areas_dev(box.t, out)
    if box.numpy:
        return b.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    return b, w


def winning(state, komi=0):
    """gym_go/gogame.py:225-230: sign(black_area - white_area - komi)."""
    black_area, white_area = areas(state)
    if isinstance(black_area, torch.Tensor):
        return torch.sign(black_area.to(torch.float64) - white_area.to(torch.float64) - komi)
    return np.sign(black_area - white_area - komi)


def batch_winning(state, komi=0):
    """gym_go/gogame.py:233-238."""
    b, w = batch_areas(state)
    if isinstance(b, torch.Tensor):
        return torch.sign(b.to(torch.float64) - w.to(torch.float64) - komi)
    return np.sign(b - w - komi)


def turn(state):
    """gym_go/gogame.py:241-246."""
    if isinstance(state, torch.Tensor):
        return int(state[govars.TURN_CHNL].max())
    return int(np.max(np.asarray(state)[govars.TURN_CHNL]))


def batch_turn(batch_state):
    """gym_go/gogame.py:249-250."""
    if isinstance(batch_state, torch.Tensor):
        return batch_state[:, govars.TURN_CHNL].amax(dim=(1, 2)).to(_I64)
    return np.max(batch_state[:, govars.TURN_CHNL], axis=(1, 2)).astype(int)


def liberties(state):
    """gym_go/gogame.py:253-264: per colour, empty points next to ANY stone of that colour (a dilation
    of the whole colour, not per group).  Host-side convenience, tensor ops only."""
    box = _Box(state)
    t = box.t.to(torch.bool)
    empty = ~(t[govars.BLACK] | t[govars.WHITE])
    res = []
    for stones in (t[govars.BLACK], t[govars.WHITE]):
        grown = torch.zeros_like(stones)
        grown[1:] |= stones[:-1]
        grown[:-1] |= stones[1:]
        grown[:, 1:] |= stones[:, :-1]
        grown[:, :-1] |= stones[:, 1:]
        res.append(grown & empty)
    if box.numpy:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res[0], res[1]


def num_liberties(state):
    """gym_go/gogame.py:267-272."""
    b, w = liberties(state)
    return int(b.sum()), int(w.sum())


def canonical_form(state):
    """gym_go/gogame.py:313-321: a copy; colours swapped and turn cleared when white is to move."""
    if isinstance(state, torch.Tensor):
        s = state.clone()
        if turn(s) == govars.WHITE:
            s[[govars.BLACK, govars.WHITE]] = state[[govars.WHITE, govars.BLACK]]
            s[govars.TURN_CHNL] = 1 - s[govars.TURN_CHNL]
        return s
    s = np.copy(state)
    if turn(s) == govars.WHITE:
        s[[govars.BLACK, govars.WHITE]] = s[[govars.WHITE, govars.BLACK]]
        s[govars.TURN_CHNL] = 1 - s[govars.TURN_CHNL]
    return s


def batch_canonical_form(batch_state):
    """gym_go/gogame.py:324-337 (no host loop: one masked swap)."""
    if isinstance(batch_state, torch.Tensor):
        s = batch_state.clone()
        white = batch_state[:, govars.TURN_CHNL].amax(dim=(1, 2)) == govars.WHITE
        sel = white[:, None, None]
        s[:, govars.BLACK] = torch.where(sel, batch_state[:, govars.WHITE], batch_state[:, govars.BLACK])
        s[:, govars.WHITE] = torch.where(sel, batch_state[:, govars.BLACK], batch_state[:, govars.WHITE])
        s[:, govars.TURN_CHNL] = torch.where(sel, torch.zeros_like(s[:, govars.TURN_CHNL]), s[:, govars.TURN_CHNL])
        return s
    s = np.copy(batch_state)
    white = batch_turn(s) == govars.WHITE
    s[white, govars.BLACK], s[white, govars.WHITE] = batch_state[white, govars.WHITE], batch_state[white, govars.BLACK]
    s[white, govars.TURN_CHNL] = 0
    return s


def _orient(image, i):
    flip = torch.flip if isinstance(image, torch.Tensor) else (lambda x, dims: np.flip(x, dims[0]))
    rot = (lambda x: torch.rot90(x, 1, (1, 2))) if isinstance(image, torch.Tensor) else (
        lambda x: np.rot90(x, axes=(1, 2)))
    x = image
    if (i >> 0) % 2:
        x = flip(x, (2,))
    if (i >> 1) % 2:
        x = flip(x, (1,))
    if (i >> 2) % 2:
        x = rot(x)
    return x


def random_symmetry(image):
    """gym_go/gogame.py:340-359: one of the 8 dihedral views of a [C, N, N] image."""
    return _orient(image, int(np.random.randint(0, 8)))


def all_symmetries(image):
    """gym_go/gogame.py:362-382: all 8, same order (h-flip bit 0, v-flip bit 1, rot90 bit 2)."""
    return [_orient(image, i) for i in range(8)]


def random_weighted_action(move_weights):
    """gym_go/gogame.py:385-392: L1-normalise, then draw."""
    w = np.asarray(move_weights.cpu() if isinstance(move_weights, torch.Tensor) else move_weights, dtype=np.float64)
    w = w / np.abs(w).sum()
    return np.random.choice(np.arange(len(w)), p=w)


def random_action(state):
    """gym_go/gogame.py:395-404: uniform over plane-3-clear points and pass."""
    inv = state[govars.INVD_CHNL].reshape(-1)
    inv = inv.cpu().numpy() if isinstance(inv, torch.Tensor) else np.asarray(inv)
    return random_weighted_action(1 - np.append(inv, 0))


def str(state):
    """gym_go/gogame.py:407-468: Unicode board + turn / game state / areas footer."""
    s = state.cpu().numpy() if isinstance(state, torch.Tensor) else np.asarray(state)
    size = s.shape[1]
    rows = ['\t' + ''.join('{}'.format(i).ljust(2, ' ') for i in range(size))]
    for i in range(size):
        line = '{}\t'.format(i)
        for j in range(size):
            last = j == size - 1
            if s[0, i, j] == 1 or s[1, i, j] == 1:
                line += '○' if s[0, i, j] == 1 else '●'
                if not last:
                    line += '═' if i in (0, size - 1) else '─'
            elif i == 0:
                line += '╔═' if j == 0 else ('╗' if last else '╤═')
            elif i == size - 1:
                line += '╚═' if j == 0 else ('╝' if last else '╧═')
            else:
                line += '╟─' if j == 0 else ('╢' if last else '┼─')
        rows.append(line)
    black_area, white_area = areas(state)
    phase = 'END' if game_ended(state) else ('PASSED' if prev_player_passed(state) else 'ONGOING')
    rows.append('\tTurn: {}, Game State (ONGOING|PASSED|END): {}'.format('BLACK' if turn(state) == 0 else 'WHITE', phase))
    rows.append('\tBlack Area: {}, White Area: {}'.format(int(black_area), int(white_area)))
    return '\n'.join(rows) + '\n'


# ------------------------------------------------------------------ device rollout helpers (build-side)

def rng_seed(batch_size, base_seed=20260927, first_game=0, device=None):
    """Per-game generator states for batch_rollout / batch_sample_actions (include/gymgo_amd.h)."""
    device = device or _device()
    # uint64 storage as int64 tensor (torch has no general uint64 ops; only the bits matter)
    rng = torch.empty(batch_size, dtype=_I64, device=device)
    _lib.call('gg_rng_seed', rng, int(base_seed) & (2 ** 64 - 1), int(first_game), batch_size, _lib.stream_ptr(device))
    return rng


# Workspaces batch_rollout attaches to the state tensors it is called on again and again: id(tensor) -> [data_ptr, shape,
# device, workspace or None].  Entries leave with their tensor (weakref.finalize).
_ROLLOUT_WS = {}


def _rollout_workspace(t):
    """The workspace batch_rollout keeps for the device tensor `t` (uint32 [B][tracked_words(N)] as int32, zeroed), or None.
    The first call on a tensor object only records it - a one-shot call, or a slice made for one call, allocates nothing -,
    the second allocates.  An entry whose tensor no longer has the pointer, shape and device it was recorded with starts over."""
    if os.environ.get('GYMGO_AMD_ROLLOUT_WS', '1') == '0':
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != _U8 or t.dim() != 4 or not t.is_contiguous():
        return None
    key, sig = id(t), (t.data_ptr(), tuple(t.shape), t.device)
    ent = _ROLLOUT_WS.get(key)
    if ent is None or ent[0] != sig:
        if ent is None:
            weakref.finalize(t, _ROLLOUT_WS.pop, key, None)
        _ROLLOUT_WS[key] = [sig, None]
        return None
    if ent[1] is None:
        if torch.cuda.is_current_stream_capturing():      # no allocation inside a stream capture: this call goes without
            return None
        ent[1] = torch.zeros((t.shape[0], 5 * t.shape[2] + 1), dtype=_I32, device=t.device)
    return ent[1]


def batch_rollout(batch_states, rng, plies, auto_reset=True, last_actions=None, steps_done=None, workspace=None):
    """IN PLACE: `plies` uniform-random steps per game with the board resident on-chip (gg_batch_rollout).
    workspace: int32 [B][tracked_words(N)], zero-filled before its first use (gg_batch_rollout_ws: big launches take the liberty
    classes of every board that still is what the last call left from there, instead of analysing it again; results do not
    depend on it).  None: from its second call on the same tensor object on, the call keeps a workspace of its own for that
    tensor (388 B per 19x19 game, freed with the tensor; GYMGO_AMD_ROLLOUT_WS=0 switches that off)."""
    B, C, N, _ = batch_states.shape
    if workspace is None:
        workspace = _rollout_workspace(batch_states)
    elif tuple(workspace.shape) != (B, 5 * N + 1):
        raise ValueError('workspace must be int32 [%d][%d] (got %s)' % (B, 5 * N + 1, tuple(workspace.shape)))
    name, ws = ('gg_batch_rollout', ()) if workspace is None else ('gg_batch_rollout_ws', (workspace,))
    _lib.call(name, batch_states, rng, last_actions, steps_done, *ws, B, N, int(plies), int(bool(auto_reset)),
              _lib.stream_ptr(batch_states.device))
    return batch_states


REWARD_METHODS = {'real': 0, 'heuristic': 1}   # GG_REWARD_* of include/gymgo_amd.h (gym_go/envs/go_env.py:11-17)


def batch_env_step(batch_states, actions=None, rng=None, komi=0.0, reward_method='real', auto_reset=True, out=None):
    """IN PLACE GoEnv.step (gym_go/envs/go_env.py:49-76) of every game in ONE launch (gg_batch_env_step): auto-reset,
    the action (`actions`, or drawn uniformly with `rng` when None), legality, next_state, game_ended and
    GoEnv.reward (:128-149).  -> (rewards float32 [B], dones uint8 [B], status int32 [B], taken int32 [B]);
    `out` = such a 4-tuple to write into (no allocation: the call is then capturable in a hipGraph as is)."""
    B, C, N, _ = batch_states.shape
    dev = batch_states.device
    if actions is None and rng is None:
        raise ValueError('batch_env_step needs actions or an rng state to draw them with')
    if out is None:
        out = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=_U8, device=dev),
               torch.empty(B, dtype=_I32, device=dev), torch.empty(B, dtype=_I32, device=dev))
    rewards, dones, status, taken = out
    _lib.call('gg_batch_env_step', batch_states, actions, rng, rewards, dones, status, taken, B, N, float(komi),
              REWARD_METHODS[reward_method], int(bool(auto_reset)), _lib.stream_ptr(dev))
    return out


def batch_sample_actions(batch_states, rng):
    """actions[b] ~ Uniform{valid actions incl. pass} on the device (GoEnv.uniform_random_action,
    gym_go/envs/go_env.py:78-81, for every game at once)."""
    B, C, N, _ = batch_states.shape
    actions = torch.empty(B, dtype=_I32, device=batch_states.device)
    _lib.call('gg_batch_sample_actions', batch_states, rng, actions, B, N, _lib.stream_ptr(batch_states.device))
    return actions


def batch_reset_finished(batch_states):
    """IN PLACE: every finished game (plane 5 set) becomes init_state (GoVecEnv auto-reset, gg_batch_reset_finished)."""
    B, C, N, _ = batch_states.shape
    _lib.call('gg_batch_reset_finished', batch_states, B, N, _lib.stream_ptr(batch_states.device))
    return batch_states


def packed_words(board_size):
    """uint32 words per board of the bit-packed format (3 N + 1)."""
    return 3 * board_size + 1


def batch_pack(batch_states):
    """[B,6,N,N] uint8 device tensor -> [B, 3N+1] int32 device tensor (row masks of planes 0/1/3 + flag word);
    9.3x smaller at 19x19 - replay buffers, checkpoints, the wire (gg_batch_pack_states)."""
    B, C, N, _ = batch_states.shape
    packed = torch.empty((B, packed_words(N)), dtype=_I32, device=batch_states.device)
    _lib.call('gg_batch_pack_states', batch_states, packed, B, N, _lib.stream_ptr(batch_states.device))
    return packed


def batch_unpack(packed, board_size):
    """Inverse of batch_pack (gg_batch_unpack_states)."""
    B = packed.shape[0]
    if packed.shape[1] != packed_words(board_size):
        raise ValueError('packed rows must have %d words for a %dx%d board' % (packed_words(board_size), board_size, board_size))
    states = torch.empty((B, govars.NUM_CHNLS, board_size, board_size), dtype=_U8, device=packed.device)
    _lib.call('gg_batch_unpack_states', packed, states, B, board_size, _lib.stream_ptr(packed.device))
    return states


# ---------------------------------------------------------------- the step path on packed boards
# Same operations as above on [B, 3N+1] int32 packed boards (batch_pack): 232 B per 19x19 board instead of 2 166 B and no
# byte <-> bit conversion inside the kernels - for search trees / replay buffers that unpack only what a network reads.

def _packed_size(packed):
    W = packed.shape[-1]
    if packed.dtype != _I32 or (W - 1) % 3 or not 2 <= (W - 1) // 3 <= 19:
        raise ValueError('packed boards are int32 [..., 3N+1] (got %s %s)' % (packed.dtype, tuple(packed.shape)))
    return (W - 1) // 3


def batch_next_states_packed(packed, batch_action1d, canonical=False, check=True):
    """gogame.batch_next_states (gym_go/gogame.py:90-150) on packed boards -> (packed_out, status int32 [B])."""
    N = _packed_size(packed)
    B = packed.shape[0]
    actions = _actions_tensor(batch_action1d, B, packed.device)
    out = torch.empty_like(packed)
    status = torch.empty(B, dtype=_I32, device=packed.device)
    _lib.call('gg_batch_next_states_packed', packed, actions, out, status, B, N, int(bool(canonical)), _lib.stream_ptr(packed.device))
    if check and bool((status != 0).any()):
        raise AssertionError('invalid move in batch (gym_go/gogame.py:117)')
    return out, status


def batch_rollout_packed(packed, rng, plies, auto_reset=True, last_actions=None, steps_done=None):
    """IN PLACE batch_rollout on packed boards (gg_batch_rollout_packed)."""
    N = _packed_size(packed)
    B = packed.shape[0]
    _lib.call('gg_batch_rollout_packed', packed, rng, last_actions, steps_done, B, N, int(plies), int(bool(auto_reset)),
              _lib.stream_ptr(packed.device))
    return packed


def batch_env_step_packed(packed, actions=None, rng=None, komi=0.0, reward_method='real', auto_reset=True, out=None):
    """IN PLACE batch_env_step on packed boards -> (rewards, dones, status, taken)."""
    N = _packed_size(packed)
    B = packed.shape[0]
    dev = packed.device
    if actions is None and rng is None:
        raise ValueError('batch_env_step_packed needs actions or an rng state to draw them with')
    if out is None:
        out = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=_U8, device=dev),
               torch.empty(B, dtype=_I32, device=dev), torch.empty(B, dtype=_I32, device=dev))
    rewards, dones, status, taken = out
    _lib.call('gg_batch_env_step_packed', packed, actions, rng, rewards, dones, status, taken, B, N, float(komi),
              REWARD_METHODS[reward_method], int(bool(auto_reset)), _lib.stream_ptr(dev))
    return out


def batch_children_packed(packed, canonical=False):
    """gogame.children (gym_go/gogame.py:175-186) of every packed parent -> int32 [B, N*N+1, 3N+1], invalid slots zero."""
    N = _packed_size(packed)
    B = packed.shape[0]
    kids = torch.empty((B, N * N + 1, packed_words(N)), dtype=_I32, device=packed.device)
    _lib.call('gg_batch_children_packed', packed, kids, B, N, int(bool(canonical)), _lib.stream_ptr(packed.device))
    return kids


def batch_play_moves(batch_states, moves):
    """IN PLACE: state[b] = next_state(state[b], moves[b, t]) for t = 0 .. T-1 in one launch (gg_batch_play_moves; a loop
    of gym_go/gogame.py:34-87).  `batch_states`: uint8 [B,6,N,N] or packed int32 [B,3N+1]; moves: int [B, T].
    -> played int32 [B]: moves applied per game (a game stops at its first illegal move or when it has ended)."""
    packed = batch_states.dim() == 2
    N = _packed_size(batch_states) if packed else batch_states.shape[-1]
    B = batch_states.shape[0]
    moves = moves.to(device=batch_states.device, dtype=_I32).contiguous()
    if moves.dim() != 2 or moves.shape[0] != B:
        raise ValueError('moves must be [B, T]')
    played = torch.empty(B, dtype=_I32, device=batch_states.device)
    _lib.call('gg_batch_play_moves_packed' if packed else 'gg_batch_play_moves', batch_states, moves, played, B, N, moves.shape[1],
              _lib.stream_ptr(batch_states.device))
    return played


# ---------------------------------------------------------------- tracked boards: packed boards + their liberty classes
def tracked_words(board_size):
    """uint32 words per tracked board (5 N + 1): rows of black, white, invalid, multi_black, multi_white + flags."""
    return 5 * board_size + 1


def _tracked_size(tracked):
    W = tracked.shape[-1]
    if tracked.dtype != _I32 or (W - 1) % 5 or not 2 <= (W - 1) // 5 <= 19:
        raise ValueError('tracked boards are int32 [..., 5N+1] (got %s %s)' % (tracked.dtype, tuple(tracked.shape)))
    return (W - 1) // 5


def batch_track(batch_states):
    """uint8 [B,6,N,N] -> tracked int32 [B, 5N+1] (gg_batch_track_states): the packed board plus the stones of either
    colour whose group has >= 2 liberties.  Tracked boards step at the fused kernel's rate even one ply per launch."""
    B, C, N, _ = batch_states.shape
    tracked = torch.empty((B, tracked_words(N)), dtype=_I32, device=batch_states.device)
    _lib.call('gg_batch_track_states', batch_states, tracked, B, N, _lib.stream_ptr(batch_states.device))
    return tracked


def batch_untrack(tracked, out=None):
    """tracked int32 [B, 5N+1] -> uint8 [B,6,N,N] (gg_batch_untrack_states); out: the tensor to write into (optional)."""
    N = _tracked_size(tracked)
    B = tracked.shape[0]
    states = out if out is not None else torch.empty((B, govars.NUM_CHNLS, N, N), dtype=_U8, device=tracked.device)
    if tuple(states.shape) != (B, govars.NUM_CHNLS, N, N):
        raise ValueError('out must be uint8 [B, 6, N, N]')
    _lib.call('gg_batch_untrack_states', tracked, states, B, N, _lib.stream_ptr(tracked.device))
    return states


POLICIES = {'uniform': 0, 'no_eye_fill': 1}   # GG_POLICY_* of include/gymgo_amd.h
PLAYOUT_POLICIES = {'uniform': 0, 'no_eye_fill': 1, 'tactical': 2}   # ... and GG_POLICY_TACTICAL of include/gymgo_amd_tactics.h
# ... and the policies that answer the board's previous move, which the playouts therefore carry from launch to launch:
# GG_POLICY_PATTERN of include/gymgo_amd_pattern.h, reached through the _policy3 entry points only
LOCAL_PLAYOUT_POLICIES = {'pattern': 3}


def _policy_code(policy):
    """The playout policy's C code; ValueError for anything but the names of PLAYOUT_POLICIES and LOCAL_PLAYOUT_POLICIES
    (checked before a device is touched).  Codes 0 and 1 go through the entry points of include/gymgo_amd.h, code 2 through
    the _policy2 ones, code 3 through the _policy3 ones."""
    for table in (PLAYOUT_POLICIES, LOCAL_PLAYOUT_POLICIES):
        if any(policy is k or (type(policy) is type(k) and policy == k) for k in table):
            return table[policy]
    raise ValueError("policy must be 'uniform', 'no_eye_fill', 'tactical' or 'pattern' (got %r)" % (policy,))


def batch_rollout_tracked(tracked, rng, plies, auto_reset=True, last_actions=None, steps_done=None, *, policy='uniform'):
    """IN PLACE batch_rollout on tracked boards (gg_batch_rollout_tracked).  policy: 'uniform' (every legal point and the
    pass alike) or 'no_eye_fill' (the mover's eyes - batch_eye_mask - are never played, the pass only when nothing else is
    left; gg_batch_rollout_tracked_policy) or 'tactical' (take what can be taken, pull out what is about to be taken, three plies
    in four, else as 'no_eye_fill' - batch_tactics gives the three sets; gg_batch_rollout_tracked_policy2) or 'pattern' (as
    'tactical', and between escaping and the plain draw it answers the board's previous move where a 3x3 shape around one of
    that move's eight neighbours calls for it - batch_patterns gives the sets; gg_batch_rollout_tracked_policy3).
    last_actions (int32 [B], or None): receives every board's last action of the launch, -1 for a board that did not play.
    policy='pattern' also READS it, as the previous action of every board (any value that is no point of the board: no
    previous point), so a tensor carried from launch to launch makes launches of any lengths play what one launch of the total
    length plays; None: no board has a previous point (a tensor of -1 is made for the call)."""
    pol = _policy_code(policy)
    N = _tracked_size(tracked)
    B = tracked.shape[0]
    name = 'gg_batch_rollout_tracked' + ('', '_policy', '_policy2', '_policy3')[pol]
    extra = (pol,) if pol else ()
    if pol == LOCAL_PLAYOUT_POLICIES['pattern'] and last_actions is None:
        last_actions = torch.full((B,), -1, dtype=_I32, device=tracked.device)
    _lib.call(name, tracked, rng, last_actions, steps_done, B, N, int(plies), int(bool(auto_reset)), *extra,
              _lib.stream_ptr(tracked.device))
    return tracked


def batch_rollout_tracked_log(tracked, rng, plies, log, last_actions=None, steps_done=None, *, policy='uniform'):
    """IN PLACE batch_rollout_tracked(..., auto_reset=False, policy=policy) that also logs its moves
    (gg_batch_rollout_tracked_log): log is an int16 [B, plies] device tensor (the C side's uint16), entry [b, t] receives the
    action board b played at ply t of this launch - a point, or N*N for the pass; a board writes exactly the plies it played,
    every other entry keeps its bytes.  -> log."""
    pol = _policy_code(policy)
    if pol not in PLAYOUT_POLICIES.values():
        raise ValueError('batch_rollout_tracked_log has no policy=%r: the move log serves %s' % (policy, sorted(PLAYOUT_POLICIES)))
    N = _tracked_size(tracked)
    B = tracked.shape[0]
    if tuple(log.shape) != (B, int(plies)):
        raise ValueError('log must be int16 [B, plies] = %s (got %s)' % ((B, int(plies)), tuple(log.shape)))
    _lib.call('gg_batch_rollout_tracked_log', tracked, rng, last_actions, steps_done, B, N, int(plies), pol, log,
              _lib.stream_ptr(tracked.device))
    return log


def batch_eye_mask(batch_states):
    """The mover's eyes of every board -> uint8 [B, N, N] (gg_batch_eye_mask): an empty point whose orthogonal neighbours on the
    board are all the mover's stones and of whose diagonal neighbours on the board at most one is the opponent's - none when
    the point lies on the first / last row or column.  All zero once the game has ended.  These are the points the
    'no_eye_fill' playouts never play."""
    box = _Box(batch_states)
    st = box.t
    if st.dim() != 4 or st.shape[1] != govars.NUM_CHNLS or st.shape[2] != st.shape[3]:
        raise ValueError('batch_states must be [B, 6, N, N] (got %s)' % (tuple(st.shape),))
    B, N = st.shape[0], st.shape[2]
    mask = torch.empty((B, N, N), dtype=_U8, device=st.device)
    _lib.call('gg_batch_eye_mask', st, mask, B, N, _lib.stream_ptr(st.device))
    return _back(box, mask)


def eye_mask(state):
    """batch_eye_mask of one state [6, N, N] -> uint8 [N, N]."""
    box = _Box(state)
    return _back(box, batch_eye_mask(box.t[None]), row0=True)


# ---------------------------------------------------------------- network input planes with per-group liberty counts
FEATURE_PLANES = 16   # gg_feature_planes() of include/gymgo_amd.h
FEATURE_NAMES = ('own', 'opponent', 'own_libs_1', 'own_libs_2', 'own_libs_3', 'own_libs_4plus', 'opp_libs_1', 'opp_libs_2',
                 'opp_libs_3', 'opp_libs_4plus', 'legal', 'ko', 'capture', 'black_to_move', 'prev_pass', 'ones')
FEATURE_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.uint8: 3}   # GG_W_* / GG_FEAT_U8


def _feature_dtype(dtype):
    """The C code of a plane dtype; ValueError for anything but the four of FEATURE_DTYPES (before a device is touched)."""
    if not isinstance(dtype, torch.dtype) or dtype not in FEATURE_DTYPES:
        raise ValueError('dtype must be torch.uint8, float16, bfloat16 or float32 (got %r)' % (dtype,))
    return FEATURE_DTYPES[dtype]


def _planes_out(out, shape, dtype, align, device=None):
    """out=None, or a contiguous device tensor of exactly this shape and dtype whose address is a multiple of `align` bytes
    (on `device` when given)."""
    if out is None:
        return
    if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dtype or tuple(out.shape) != tuple(shape)
            or not out.is_contiguous() or out.data_ptr() % align or (device is not None and out.device != device)):
        raise ValueError('out must be a contiguous%s %s %s tensor on the states\' device (got %s)' % (
            ', %d-byte aligned' % align if align > 1 else '', dtype, list(shape),
            '%s %s on %s' % (out.dtype, list(out.shape), out.device) if isinstance(out, torch.Tensor) else type(out)))


def _states_shape(x, what='batch_states'):
    """(B, N) of a [B, 6, N, N] tensor or array; ValueError otherwise (before a device is touched)."""
    shape = tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)
    if len(shape) != 4 or shape[1] != govars.NUM_CHNLS or shape[2] != shape[3]:
        raise ValueError('%s must be [B, 6, N, N] (got %s)' % (what, shape))
    return shape[0], shape[2]


def batch_group_liberties(batch_states):
    """The liberties of the group of the stone at every point -> uint8 [B, N, N] (gg_batch_group_liberties): a group is a
    maximal orthogonally connected set of stones of one colour, its liberties are the distinct empty points next to any of
    its stones; the count is exact up to 255 (saturated there) and 0 at empty points.  The per-group counterpart of
    `liberties` / `num_liberties`, which dilate a whole colour.  One launch; device memory of the result: B * N^2 bytes."""
    B, N = _states_shape(batch_states)
    box = _Box(batch_states)
    st = box.t
    libs = torch.empty((B, N, N), dtype=_U8, device=st.device)
    _lib.call('gg_batch_group_liberties', st, libs, B, N, _lib.stream_ptr(st.device))
    return _back(box, libs)


def group_liberties(state):
    """batch_group_liberties of one state [6, N, N] -> uint8 [N, N]."""
    box = _Box(state)
    return _back(box, batch_group_liberties(box.t[None]), row0=True)


def _orient_arg(orient, B):
    """ValueError unless orient is B integers (a tensor or an array) - before a device is touched."""
    if isinstance(orient, torch.Tensor):
        n, integral = orient.numel(), not (orient.dtype.is_floating_point or orient.dtype.is_complex or orient.dtype == torch.bool)
    else:
        orient = np.asarray(orient)
        n, integral = orient.size, orient.dtype.kind in 'iu'
    if not integral or n != B:
        raise ValueError('orient must be %d integers in 0..7, one per row (got %d of %s)' % (B, n, orient.dtype))


def _last_arg(last, B):
    """ValueError unless last is B integers that fit an int32 (a tensor or an array) - before a device is touched."""
    if isinstance(last, torch.Tensor):
        n, integral = last.numel(), not (last.dtype.is_floating_point or last.dtype.is_complex or last.dtype == torch.bool)
    else:
        last = np.asarray(last)
        n, integral = last.size, last.dtype.kind in 'iu'
    if not integral or n != B:
        raise ValueError('last must be %d integers, the previous action of every row (got %d of %s)' % (B, n, last.dtype))


def _side_arg(side, B):
    """ValueError unless side is B integers or booleans (a tensor or an array) - before a device is touched."""
    if isinstance(side, torch.Tensor):
        n, integral = side.numel(), not (side.dtype.is_floating_point or side.dtype.is_complex)
    else:
        side = np.asarray(side)
        n, integral = side.size, side.dtype.kind in 'iub'
    if not integral or n != B:
        raise ValueError('side must be %d integers, 0 = black\'s view, non-zero = white\'s, one per row (got %d of %s)' % (B, n, side.dtype))


def _side_tensor(side, B, device):
    """side (checked by _side_arg) as uint8 [B] on `device`: 0 / 1."""
    s = side if isinstance(side, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(side) != 0))
    return (s.to(device=device) != 0).to(_U8).reshape(B).contiguous()


def _counts_arg(counts, B, width=2):
    """ValueError unless counts is a flag or a contiguous int32 [B, width] device tensor to write into - before a device is touched."""
    if isinstance(counts, torch.Tensor) and (not counts.is_cuda or counts.dtype != _I32 or tuple(counts.shape) != (B, width)
                                             or not counts.is_contiguous()):
        raise ValueError('counts must be a flag or a contiguous int32 [%d, %d] device tensor (got %s %s on %s)' % (
            B, width, counts.dtype, list(counts.shape), counts.device))


def _status_own_arg(own, boards, B, N):
    """ValueError unless own is the int32 [B, 2, N, N] ownership counts of the boards - a tensor on the boards' device when those
    are a device tensor, else a tensor or an array - before a device is touched."""
    tensor = isinstance(own, torch.Tensor)
    if not tensor and not isinstance(own, np.ndarray):
        raise ValueError('ownership must be an int32 [B, 2, N, N] tensor or array, or a Playouts that has one (got %s)' % (type(own),))
    if tuple(own.shape) != (B, 2, N, N) or own.dtype != (_I32 if tensor else np.int32):
        raise ValueError('ownership must be int32 %s (got %s %s)' % ([B, 2, N, N], own.dtype, list(own.shape)))
    if tensor and isinstance(boards, torch.Tensor) and own.device != boards.device:
        raise ValueError('ownership must live on the boards\' device (got %s, the boards are on %s)' % (own.device, boards.device))


def _plane_args(name, boards, orient, values):
    """(entry point, *its arguments) of a plane launch, bound BY NAME from the entry point's row of the binding table (_lib.PARAMS),
    the one place that knows the order: boards is the first parameter, every other one takes the value `values` (a dict) holds
    under its name - out, out_dtype, B, N, hip_stream and what the family adds (settled / aborted, side and counts, last, own with
    playouts, num and den, the ring's rows, count, H, T and moves) - and a pointer that is not given goes down as NULL.  An entry
    point whose row has no orient, called with one, is its _oriented form (the feature planes).  A name the row does not have is
    a TypeError."""
    names = _lib.PARAMS[name]
    if orient is not None and 'orient' not in names:
        name += '_oriented'
        names = _lib.PARAMS[name]
    if 'orient' in names:
        values['orient'] = orient
    if not values.keys() <= names.keys():
        raise TypeError('%s has no parameter %s' % (name, ', '.join(values.keys() - names.keys())))
    args = list(map(values.get, names))
    args[0] = boards
    return (name, *args)


def _plane_launch(name, boards, orient, values):
    """One launch of a plane entry point on tensors, its arguments by name (_plane_args)."""
    _lib.call(*_plane_args(name, boards, orient, values))


def _planes(name, count, align, boards, tracked, dtype, out, orient, per_board=None, **inputs):
    """The body of the batch plane calls: `count` planes per board from byte planes (a tensor or an array) or, `tracked`,
    from tracked boards (a device tensor), through the C entry point `name` (_plane_launch), into `out` (aligned to
    `align` bytes) or a new tensor.  inputs: what the family takes beside the boards, under the names of the entry point's
    parameters, each with its checker - last (None or B actions: _last_arg), side (None or B flags: _side_arg, _side_tensor), own
    (the ownership counts, a tensor or an array: _status_own_arg) with the scalars playouts, num and den, checked by the caller -
    and history (a StoneHistory: _past_arg; its planes are `count`, its ring five more arguments).  per_board: the one optional
    per-board output as (parameter name, wanted, shape behind B, dtype) - settled / aborted uint8 [B], counts int32 [B, 2] or
    [B, 4]; wanted: a flag or, for counts, the caller's buffer (_counts_arg) -> planes, or (planes, that output).  Every ValueError
    comes before a device is touched."""
    code = _feature_dtype(dtype)
    B, N = _hash_shape(boards, tracked)
    past = 'history' in inputs
    if past:
        history = inputs.pop('history')
        count = _past_arg(history, B, N).planes
    if not tracked:
        _planes_out(out, (B, count, N, N), dtype, align)
    if orient is not None:
        _orient_arg(orient, B)
    last, side = inputs.get('last'), inputs.get('side')
    if last is not None:
        _last_arg(last, B)
    if side is not None:
        _side_arg(side, B)
    pname, wanted, tail, pdtype = per_board or (None, False, (), None)
    if pname == 'counts':
        _counts_arg(wanted, B, *tail)
    if 'own' in inputs:
        _status_own_arg(inputs['own'], boards, B, N)
    if tracked:
        box, st = None, boards
        _planes_out(out, (B, count, N, N), dtype, align, st.device if st.is_cuda else None)
    else:
        if not isinstance(boards, torch.Tensor) and dtype == torch.bfloat16:
            raise ValueError('NumPy has no bfloat16: pass a device tensor, or another dtype')
        box = _Box(boards)
        st = box.t
        _planes_out(out, (B, count, N, N), dtype, align, st.device)
    dev = st.device
    if past:
        if history.rows.device != dev:
            raise ValueError('history must live on the boards\' device (%s)' % (dev,))
        inputs.update(rows=history.rows, count=history.count, H=history.capacity, T=history.positions, moves=int(history.moves))
    planes = out if out is not None else torch.empty((B, count, N, N), dtype=dtype, device=dev)
    if isinstance(wanted, torch.Tensor):   # (checked by _counts_arg: the caller's buffer)
        if wanted.device != dev:
            raise ValueError('counts must live on the states\' device (got %s)' % (wanted.device,))
        extra = wanted
    else:
        extra = torch.empty((B,) + tail, dtype=pdtype, device=dev) if wanted else None
    if pname is not None:
        inputs[pname] = extra
    o = None if orient is None else _actions_tensor(orient, B, dev)
    if side is not None:
        inputs['side'] = _side_tensor(side, B, dev)
    if 'own' in inputs:
        own = inputs['own'] if isinstance(inputs['own'], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(inputs['own']))
        inputs['own'] = own.to(dev).contiguous()
    if last is not None:
        inputs['last'] = _actions_tensor(last, B, dev)
    inputs.update(out=planes, out_dtype=code, B=B, N=N, hip_stream=_lib.stream_ptr(dev))
    _plane_launch(name, st, o, inputs)
    if box is not None:
        planes, extra = _back(box, planes), _back(box, extra)
    return planes if extra is None else (planes, extra)


def _plane_single(batch_fn, state, dtype, **kw):
    """The single-state form of a batch plane call: state [6, N, N] as a batch of one, row 0 of every result."""
    _feature_dtype(dtype)
    if not isinstance(state, torch.Tensor) and dtype == torch.bfloat16:
        raise ValueError('NumPy has no bfloat16: pass a device tensor, or another dtype')
    box = _Box(state)
    res = batch_fn(box.t[None], dtype, **kw)
    return tuple(_back(box, t, row0=True) for t in res) if isinstance(res, tuple) else _back(box, res, row0=True)


def batch_features(batch_states, dtype=torch.float16, out=None, orient=None):
    """Network input planes of every board -> [B, 16, N, N] of `dtype` (gg_batch_features), from the mover's point of view
    ("own" = the player to move).  Plane by plane (FEATURE_NAMES), each value exactly 0 or 1:
       0      own stone                      1      opponent stone
       2 - 5  own stone whose group has exactly 1 / exactly 2 / exactly 3 / >= 4 liberties (a hand-made group with none: no plane)
       6 - 9  the same for opponent stones
      10      legal point: empty, plane 3 (invalid) clear, game not over
      11      ko point: empty, plane 3 set, game not over, next to an opponent group with exactly one liberty (this point)
      12      capturing point: legal and next to an opponent group with exactly one liberty
      13      all ones iff the mover is black      14      all ones iff the previous move was a pass      15      all ones
    Groups and liberties as in batch_group_liberties.  Exact: every group is counted by a flood of its own on the device;
    plane 3 of the input is taken as given.  dtype: torch.uint8, float16, bfloat16 or float32 (ValueError otherwise; 0 and 1
    are exact in all four).  out: a contiguous, 16-byte aligned device tensor of that shape and dtype to write into.  NumPy in
    gives NumPy out (through the device; not for bfloat16, which NumPy lacks).  One launch; device memory of the result:
    16 * B * N^2 elements - 11.5 KB per 19x19 board in a 16-bit dtype.
    orient (None: the call above, launch for launch; or int [B], a tensor or an array, only orient & 7 is read): row b is
    view orient[b] of its planes, all sixteen turned alike (gg_batch_features_oriented; bit 0 flips the columns, then bit 1
    the rows, then bit 2 rotates: batch_symmetry's orientations).  That is also batch_features of the turned position,
    batch_symmetry(batch_states, orient).  Still one launch."""
    return _planes('gg_batch_features', FEATURE_PLANES, 16, batch_states, False, dtype, out, orient)


def features(state, dtype=torch.float16):
    """batch_features of one state [6, N, N] -> [16, N, N]."""
    return _plane_single(batch_features, state, dtype)


def batch_features_tracked(tracked, dtype=torch.float16, out=None, orient=None):
    """batch_features of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 16, N, N] of `dtype`
    (gg_batch_features_tracked): bit for bit what batch_features gives for batch_untrack(tracked) - the search's leaf
    boards go to the network without the byte planes in between.  dtype, out, exactness and device memory: batch_features.
    orient: as batch_features (gg_batch_features_tracked_oriented) - what batch_symmetry_rows followed by this call gives,
    in one launch and without the second board buffer."""
    return _planes('gg_batch_features_tracked', FEATURE_PLANES, 16, tracked, True, dtype, out, orient)


# ---------------------------------------------------------------- pass-alive (Benson) life planes
LIFE_PLANES = 4   # gg_life_planes() of include/gymgo_amd.h
LIFE_NAMES = ('own_alive', 'opp_alive', 'own_safe', 'opp_safe')


def batch_life(batch_states, dtype=torch.uint8, out=None, orient=None, settled=False):
    """Pass-alive (Benson) life planes of every board -> [B, 4, N, N] of `dtype` (gg_batch_life), from the mover's point of
    view, each value exactly 0 or 1 (LIFE_NAMES):
       0  own stones that can never be captured, whatever the opponent plays and even if the owner always passes
       1  the opponent's such stones
       2  the points (empty, or holding opponent stones) of the regions those own chains enclose and live by
       3  the same for the opponent
    For a colour, chains are the components of its stones and regions the components of everything else; a region is vital to a
    chain when it has an empty point and every empty point of it touches the chain; chains with fewer than two vital regions
    are dropped, then regions that border a dropped chain, until nothing changes (include/gymgo_amd.h).  Exact, no reading:
    only planes 0, 1 and 2 of the states are read, so an ended game gets its planes like any other.  dtype: torch.uint8,
    float16, bfloat16 or float32 (ValueError otherwise).  out: a contiguous device tensor of that shape and dtype to write
    into.  orient (None, or int [B], only orient & 7 is read): row b is view orient[b] of its planes - also the planes of the
    turned position.  settled=True: -> (planes, uint8 [B]): 1 iff every point of the board lies in some plane (nothing is
    left to play for; it does not depend on orient).  NumPy in gives NumPy out (through the device; not for bfloat16).
    One launch either way; device memory of the result: 4 * B * N^2 elements (+ B bytes)."""
    return _planes('gg_batch_life', LIFE_PLANES, 1, batch_states, False, dtype, out, orient, ('settled', bool(settled), (), _U8))


def life(state, dtype=torch.uint8, settled=False):
    """batch_life of one state [6, N, N] -> [4, N, N] (with settled=True: and a uint8 scalar)."""
    return _plane_single(batch_life, state, dtype, settled=settled)


def batch_life_tracked(tracked, dtype=torch.uint8, out=None, orient=None, settled=False):
    """batch_life of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 4, N, N] of `dtype` (gg_batch_life_tracked):
    bit for bit what batch_life gives for batch_untrack(tracked); only the two stone row sets and the turn flag are read."""
    return _planes('gg_batch_life_tracked', LIFE_PLANES, 1, tracked, True, dtype, out, orient, ('settled', bool(settled), (), _U8))


def batch_settled(batch_states):
    """uint8 [B]: 1 iff every point of the board is a pass-alive stone or lies in a region such stones live by (batch_life's
    settled byte): nothing is left to play for - the test a self-play driver ends a game on.  The empty board is not
    settled.  The launch of batch_life into a scratch buffer."""
    return batch_life(batch_states, torch.uint8, settled=True)[1]


# ---------------------------------------------------------------- ladder planes
LADDER_PLANES = 4   # GG_LADDER_PLANES of include/gymgo_amd.h
LADDER_NAMES = ('own_laddered', 'opp_laddered', 'ladder_capture', 'ladder_escape')


def batch_ladder(batch_states, dtype=torch.uint8, out=None, orient=None, aborted=False):
    """Ladder planes of every board -> [B, 4, N, N] of `dtype` (gg_batch_ladder), from the mover's point of view, each value
    exactly 0 or 1 (LADDER_NAMES):
       0  own stones of laddered chains          1  the opponent's
       2  ladder captures: the ataris on an opponent chain with two liberties that capture it in a ladder
       3  ladder escapes: the moves that get an own chain with one liberty out
    by a bounded search per board on the device: the prey extends or captures a chaser in atari, the attacker ataris on either
    of the two liberties, until the prey has three liberties (escaped) or none to play for (captured); a chain with two
    liberties is laddered when some atari works, a chain with one when no move escapes.  A root query gets
    GG_LADDER_DEPTH(N) = 4 N plies and GG_LADDER_NODES(N) = 16 N nodes; past either it is aborted and answers "not captured" /
    "escapes".  The definition with its evaluation order: include/gymgo_amd.h.  Exact, bit for bit.  A board whose game is
    over gets planes 2 and 3 clear.  dtype: torch.uint8, float16, bfloat16 or float32 (ValueError otherwise).  out: a
    contiguous device tensor of that shape and dtype to write into.  orient (None, or int [B], only orient & 7 is read): row b
    holds the planes of the turned position (turned first, then searched).  aborted=True: -> (planes, uint8 [B]): the
    aborted root queries of the board, saturated at 255.  NumPy in gives NumPy out (through the device; not for bfloat16).
    One launch either way; device memory of the result: 4 * B * N^2 elements (+ B bytes)."""
    return _planes('gg_batch_ladder', LADDER_PLANES, 1, batch_states, False, dtype, out, orient, ('aborted', bool(aborted), (), _U8))


def ladder(state, dtype=torch.uint8, aborted=False):
    """batch_ladder of one state [6, N, N] -> [4, N, N] (with aborted=True: and a uint8 scalar)."""
    return _plane_single(batch_ladder, state, dtype, aborted=aborted)


def batch_ladder_tracked(tracked, dtype=torch.uint8, out=None, orient=None, aborted=False):
    """batch_ladder of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 4, N, N] of `dtype` (gg_batch_ladder_tracked):
    bit for bit what batch_ladder gives for batch_untrack(tracked); the class rows are not read."""
    return _planes('gg_batch_ladder_tracked', LADDER_PLANES, 1, tracked, True, dtype, out, orient, ('aborted', bool(aborted), (), _U8))


# ---------------------------------------------------------------- move-outcome planes
MOVE_PLANES = 12   # GG_MOVE_PLANES of include/gymgo_amd.h
MOVE_COUNTS = 3    # GG_MOVE_COUNTS
MOVE_NAMES = ('libs_after_1', 'libs_after_2', 'libs_after_3', 'libs_after_4plus', 'captures_1', 'captures_2', 'captures_3',
              'captures_4plus', 'self_atari_1', 'self_atari_2', 'self_atari_3', 'self_atari_4plus')
MOVE_COUNT_NAMES = ('libs_after', 'captured', 'chain_size')


def batch_move_planes(batch_states, dtype=torch.uint8, out=None, orient=None):
    """Move-outcome planes of every board -> [B, 12, N, N] of `dtype` (gg_batch_move_planes), from the mover's point of view,
    each value exactly 0 or 1 (MOVE_NAMES).  For every candidate point - empty, plane 3 clear, game not over: the legal plane
    of batch_features - a stone of the mover is put there, the opponent chains left without a liberty are removed
    (captured = their stones), and the chain of the played stone has libs liberties and size stones:
       0 -  3  libs     exactly 1 / exactly 2 / exactly 3 / >= 4
       4 -  7  captured exactly 1 / exactly 2 / exactly 3 / >= 4
       8 - 11  a self-atari (libs exactly 1) of a chain of exactly 1 / exactly 2 / exactly 3 / >= 4 stones
    A candidate whose chain would have no liberty (a suicide: only with a plane 3 that is not the true mask) and every point
    that is no candidate is in no plane.  Exact, from the stones alone; the definition: include/gymgo_amd.h.  dtype:
    torch.uint8, float16, bfloat16 or float32 (ValueError otherwise).  out: a contiguous device tensor of that shape and
    dtype to write into.  orient (None, or int [B], only orient & 7 is read): row b is view orient[b] of its planes - also the
    planes of the turned position.  NumPy in gives NumPy out (through the device; not for bfloat16).  One launch; device
    memory of the result: 12 * B * N^2 elements - against the (N^2 + 1) * 6 * N^2 bytes per board of batch_children."""
    return _planes('gg_batch_move_planes', MOVE_PLANES, 1, batch_states, False, dtype, out, orient)


def move_planes(state, dtype=torch.uint8):
    """batch_move_planes of one state [6, N, N] -> [12, N, N]."""
    return _plane_single(batch_move_planes, state, dtype)


def batch_move_planes_tracked(tracked, dtype=torch.uint8, out=None, orient=None):
    """batch_move_planes of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 12, N, N] of `dtype`
    (gg_batch_move_planes_tracked): bit for bit what batch_move_planes gives for batch_untrack(tracked); the class rows
    are not read."""
    return _planes('gg_batch_move_planes_tracked', MOVE_PLANES, 1, tracked, True, dtype, out, orient)


def batch_move_counts(batch_states):
    """The numbers behind batch_move_planes -> uint8 [B, 3, N, N] (gg_batch_move_counts; MOVE_COUNT_NAMES): at every
    candidate point min(libs, 255), min(captured, 255), min(size, 255) of the move there, all three 0 for a suicide and at
    every point that is no candidate.  One launch; device memory of the result: 3 * B * N^2 bytes."""
    B, N = _states_shape(batch_states)
    box = _Box(batch_states)
    st = box.t
    counts = torch.empty((B, MOVE_COUNTS, N, N), dtype=_U8, device=st.device)
    _lib.call('gg_batch_move_counts', st, counts, B, N, _lib.stream_ptr(st.device))
    return _back(box, counts)


def move_counts(state):
    """batch_move_counts of one state [6, N, N] -> uint8 [3, N, N]."""
    box = _Box(state)
    return _back(box, batch_move_counts(box.t[None]), row0=True)


# ---------------------------------------------------------------- area ownership planes, ownership and score targets
AREA_PLANES = 3   # gg_area_planes() of include/gymgo_amd_area.h
AREA_NAMES = ('own_area', 'opp_area', 'neutral')


def batch_area_planes(batch_states, dtype=torch.uint8, out=None, orient=None, side=None, counts=False):
    """Area ownership planes of every board -> [B, 3, N, N] of `dtype` (gg_batch_area), each value exactly 0 or 1
    (AREA_NAMES): the points Tromp-Taylor scoring (`areas`) counts for each side, and those it counts for neither.  E = the
    empty points; a colour REACHES the empty points connected through E to an empty point next to one of its stones:
       0  own_area   own stones, and the empty points only the own colour reaches
       1  opp_area   the opponent's stones, and the empty points only the opponent reaches
       2  neutral    the other empty points: their region touches both colours, or neither (a board without stones)
    The three planes partition the board.  Exact; only planes 0, 1 and 2 of the states are read, so an ended game gets its
    planes like any other.  side (None: "own" = the player to move, as in every other plane family; or B flags, a tensor or
    an array): side[b] == 0 is black's view of board b, non-zero white's, whatever its turn plane says - what a training
    target needs, where a game's final position is seen by the mover of a sampled one.  counts=True: -> (planes, int32
    [B, 2]): the number of points in plane 0 and in plane 1; with side all 0 that is batch_areas.  (counts may also be a
    contiguous int32 [B, 2] device tensor to write into.)  dtype: torch.uint8, float16, bfloat16 or float32 (ValueError
    otherwise).  out: a contiguous device tensor of that shape and dtype to write into.  orient (None, or int [B], only
    orient & 7 is read): row b is view orient[b] of its planes - also the planes of the turned position; the counts do not
    turn.  NumPy in gives NumPy out (through the device; not for bfloat16).  One launch either way; device memory of the
    result: 3 * B * N^2 elements (+ 8 B bytes)."""
    return _planes('gg_batch_area', AREA_PLANES, 1, batch_states, False, dtype, out, orient, ('counts', counts, (2,), _I32), side=side)


def area_planes(state, dtype=torch.uint8, side=None, counts=False):
    """batch_area_planes of one state [6, N, N] -> [3, N, N] (with counts=True: and int32 [2]); side: None or one flag."""
    return _plane_single(batch_area_planes, state, dtype, side=None if side is None else [side], counts=bool(counts))


def batch_area_planes_tracked(tracked, dtype=torch.uint8, out=None, orient=None, side=None, counts=False):
    """batch_area_planes of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 3, N, N] of `dtype`
    (gg_batch_area_tracked): bit for bit what batch_area_planes gives for batch_untrack(tracked); only the two stone row
    sets and the turn flag are read."""
    return _planes('gg_batch_area_tracked', AREA_PLANES, 1, tracked, True, dtype, out, orient, ('counts', counts, (2,), _I32), side=side)


# ---------------------------------------------------------------- the sets of the tactical playout policy
TACTICS_PLANES = 3   # gg_tactics_planes() of include/gymgo_amd_tactics.h
TACTICS_NAMES = ('capture', 'escape', 'no_eye_fill')


def batch_tactics(batch_states, dtype=torch.uint8, out=None, orient=None):
    """The three sets a ply of the 'tactical' playout policy draws from -> [B, 3, N, N] of `dtype` (gg_batch_tactics), each
    value exactly 0 or 1 (TACTICS_NAMES), from the mover's view; all zero for a game that has ended.  low = the stones of
    either colour whose group has fewer than two liberties (batch_group_liberties), valid = the points whose invalid bit is clear:
       0  capture      C: valid points orthogonally next to an opponent stone in low - the move takes that group
       1  escape       E: valid points next to a mover's stone in low with at least two empty orthogonal neighbours
       2  no_eye_fill  F: valid points that are not eyes of the mover (batch_eye_mask): the candidates of 'no_eye_fill'
    The ply: with u the high 32 bits of its draw and the gate open when (u & 3) != 0, it draws from C if the gate is open and
    C is not empty, else from E if the gate is open and E is not empty, else from F; the pass when the set is empty (F only).
    dtype, out, orient and NumPy input: as batch_area_planes.  One launch; device memory of the result: 3 * B * N^2 elements."""
    return _planes('gg_batch_tactics', TACTICS_PLANES, 1, batch_states, False, dtype, out, orient)


def tactics(state, dtype=torch.uint8):
    """batch_tactics of one state [6, N, N] -> [3, N, N]."""
    return _plane_single(batch_tactics, state, dtype)


def batch_tactics_tracked(tracked, dtype=torch.uint8, out=None, orient=None):
    """batch_tactics of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 3, N, N] of `dtype`
    (gg_batch_tactics_tracked): bit for bit what batch_tactics gives for batch_untrack(tracked); every group is counted from
    the stones, the class rows are not read."""
    return _planes('gg_batch_tactics_tracked', TACTICS_PLANES, 1, tracked, True, dtype, out, orient)


# ---------------------------------------------------------------- the sets of the pattern playout policy
PATTERN_PLANES = 2   # gg_pattern_planes() of include/gymgo_amd_pattern.h
PATTERN_NAMES = ('pattern', 'local')


def batch_patterns(batch_states, last=None, dtype=torch.uint8, out=None, orient=None):
    """The two sets the 'pattern' playout policy adds to those of batch_tactics -> [B, 2, N, N] of `dtype` (gg_batch_patterns),
    each value exactly 0 or 1 (PATTERN_NAMES); all zero for a game that has ended:
       0  pattern  P: the empty points whose eight neighbours (empty, black, white, off the board) match one of the thirteen
                   3x3 patterns of include/gymgo_amd_pattern.h in some rotation or reflection, under either colouring
       1  local    L: the points of P among the up to eight neighbours of the previous move that are candidates of
                   'no_eye_fill' (batch_tactics' plane 2)
    last: the previous action of every board, B integers (a tensor or an array) that refer to the board as it is given, before
    orient turns it; a value outside [0, N*N) - -1, the pass, anything - means no previous point, as does last=None: plane 1 is
    then all zero.
    The ply: with the gate of 'tactical' open it draws from the first non-empty of C, E, L, F; with it closed, from F.
    dtype, out, orient and NumPy input: as batch_area_planes.  One launch; device memory of the result: 2 * B * N^2 elements."""
    return _planes('gg_batch_patterns', PATTERN_PLANES, 1, batch_states, False, dtype, out, orient, last=last)


def patterns(state, last=None, dtype=torch.uint8):
    """batch_patterns of one state [6, N, N] and its previous action (an integer or None) -> [2, N, N]."""
    return _plane_single(lambda st, dt: batch_patterns(st, None if last is None else [int(last)], dt), state, dtype)


def batch_patterns_tracked(tracked, last=None, dtype=torch.uint8, out=None, orient=None):
    """batch_patterns of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 2, N, N] of `dtype`
    (gg_batch_patterns_tracked): bit for bit what batch_patterns gives for batch_untrack(tracked)."""
    return _planes('gg_batch_patterns_tracked', PATTERN_PLANES, 1, tracked, True, dtype, out, orient, last=last)


# ---------------------------------------------------------------- move priors from the sets of both playout policies
UctPrior = collections.namedtuple('UctPrior', 'even capture escape pattern local eye_fill')
UctPrior.__doc__ = """A prior for the nodes of the RAVE search (batch_uct(prior=...), batch_move_priors; include/gymgo_amd_prior.h):
six pairs (visits, wins) of integers with 0 <= wins <= visits, virtual simulations that a legal point of a new node starts with -
`even` for every legal point, and on top of it `capture` for a point of C, `escape` for one of E (batch_tactics), `pattern` for one
of P, `local` for one of L (batch_patterns, the previous point being the action that led to the node) and `eye_fill` for a legal
point that is an eye of the mover (legal, and not in batch_tactics' plane 2)."""
# The default: every legal point starts as eight simulations at 0.5; a capture, an escape and a local answer count as eight won
# ones more, a pattern point as four, filling an own eye as sixteen lost ones.  UNTUNED: nobody has measured playing strength with
# these values - they are data, not part of the rule.
UCT_PRIOR = UctPrior(even=(8, 4), capture=(8, 8), escape=(8, 8), pattern=(4, 4), local=(8, 8), eye_fill=(16, 0))


def _prior_arg(prior):
    """prior=True -> UCT_PRIOR; else six (visits, wins) pairs of integers with 0 <= wins <= visits < 2^31 -> UctPrior of int pairs.
    ValueError otherwise - before a device is touched."""
    if prior is True:
        prior = UCT_PRIOR
    integral = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))
    try:
        pairs = [tuple(p) for p in prior]
    except TypeError:
        pairs = None
    if (pairs is None or len(pairs) != len(UctPrior._fields) or any(len(p) != 2 or not all(integral(x) for x in p) for p in pairs)
            or any(not 0 <= w <= v < 2 ** 31 for v, w in pairs)):
        raise ValueError('prior must be True or six (visits, wins) pairs of integers with 0 <= wins <= visits, %s (got %r)'
                         % (', '.join(UctPrior._fields), prior))
    return UctPrior(*[(int(v), int(w)) for v, w in pairs])


def _prior_weights(pr, device):
    """The weights of the C entry points: int32 [12] on `device`, the six pairs in UctPrior's order."""
    return torch.tensor([x for p in pr for x in p], dtype=_I32).to(device)


def _move_priors(name, boards, pr, last, B, N):
    out = torch.empty((B, N * N, 2), dtype=_I32, device=boards.device)
    la = None if last is None else _actions_tensor(last, B, boards.device)
    _lib.call(name, boards, la, _prior_weights(pr, boards.device), out, B, N, _lib.stream_ptr(boards.device))
    return out


def batch_move_priors(batch_states, prior=True, last=None):
    """The pairs a prior gives the points of every board -> int32 [B, N*N, 2] (gg_batch_move_priors): entry [b, p] = (visits,
    2 * wins) - the units of batch_uct's rave_visits / rave_score - of point p of board b: the sum of prior.even and of the pairs
    of the sets p lies in (UctPrior) when p is legal (its plane-3 bit is clear and the game has not ended), (0, 0) otherwise.
    prior: True (UCT_PRIOR) or a UctPrior; last: as in batch_patterns - the previous action of every board, anything that is no
    point of the board means none.  This is what batch_uct(prior=...) adds to a new node.  One launch; NumPy in, NumPy out."""
    pr = _prior_arg(prior)
    B, N = _states_shape(batch_states)
    if last is not None:
        _last_arg(last, B)
    box = _Box(batch_states)
    return _back(box, _move_priors('gg_batch_move_priors', box.t, pr, last, B, N))


def move_priors(state, prior=True, last=None):
    """batch_move_priors of one state [6, N, N] and its previous action (an integer or None) -> int32 [N*N, 2]."""
    pr = _prior_arg(prior)
    box = _Box(state)
    return _back(box, batch_move_priors(box.t[None], pr, None if last is None else [int(last)]), row0=True)


def batch_move_priors_tracked(tracked, prior=True, last=None):
    """batch_move_priors of tracked boards (int32 [B, 5N+1], a device tensor) -> int32 [B, N*N, 2] (gg_batch_move_priors_tracked):
    bit for bit what batch_move_priors gives for batch_untrack(tracked)."""
    pr = _prior_arg(prior)
    if not isinstance(tracked, torch.Tensor) or tracked.dim() != 2:
        raise ValueError('tracked boards are int32 [B, 5N+1] device tensors')
    N, B = _tracked_size(tracked), tracked.shape[0]
    if last is not None:
        _last_arg(last, B)
    return _move_priors('gg_batch_move_priors_tracked', tracked, pr, last, B, N)


def _prior_kw(kw, R, N, iterations, playouts):
    """The checks of batch_uct's prior= and last_actions= (kw: the keywords given) -> (UctPrior or None, int32 array [R] or None).
    Every ValueError before a device is touched."""
    prior, last = kw.get('prior'), kw.get('last_actions')
    if prior is None:
        if last is not None:
            raise ValueError('last_actions= goes with prior=: it is the previous point of the root\'s prior')
        return None, None
    if kw.get('rave_equiv') is None:
        raise ValueError('prior= needs rave_equiv=: the pairs it seeds are those of the RAVE search')
    pr = _prior_arg(prior)
    total = 2 * (int(iterations) * int(playouts) + sum(v for v, _ in pr))
    if total >= 2 ** 31:
        raise ValueError('a prior needs 2 * (iterations * playouts + the visits of its six pairs) < 2^31 (got %d)' % total)
    if last is None:
        return pr, None
    if isinstance(last, torch.Tensor):
        integral = not (last.dtype.is_floating_point or last.dtype.is_complex or last.dtype == torch.bool)
        la = last.detach().cpu().numpy() if integral else None
    else:
        la = np.asarray(last)
        integral = la.dtype.kind in 'iu'
    if not integral or la.size != R or (la.size and (int(la.min()) < -1 or int(la.max()) > N * N)):
        raise ValueError('last_actions must be %d integers in [-1, %d]: the previous action of every root, -1 or the pass for none'
                         % (R, N * N))
    return pr, la.astype(np.int32).reshape(R)


def batch_ownership(batch_states, side=None, orient=None):
    """Who owns every point under Tromp-Taylor scoring, and by how much that side leads -> (owner int8 [B, N, N], margin int32
    [B]): owner = +1 on the points of batch_area_planes' plane 0, -1 on those of plane 1, 0 on neutral points; margin = the
    number of +1 minus the number of -1 (no komi).  side, orient: as batch_area_planes - side=None is the view of the player
    to move, orient turns owner and leaves margin.  One launch (gg_batch_area, byte planes and counts) plus a subtraction
    each; NumPy in gives NumPy out."""
    B, _ = _states_shape(batch_states)   # (every ValueError before a device is touched)
    if orient is not None:
        _orient_arg(orient, B)
    if side is not None:
        _side_arg(side, B)
    box = _Box(batch_states)
    planes, counts = batch_area_planes(box.t, torch.uint8, orient=orient, side=side, counts=True)
    owner = planes[:, 0].to(torch.int8) - planes[:, 1].to(torch.int8)
    return _back(box, owner), _back(box, counts[:, 0] - counts[:, 1])


def ownership(state, side=None):
    """batch_ownership of one state [6, N, N] -> (owner int8 [N, N], margin: an int32 scalar); side: None or one flag."""
    box = _Box(state)
    owner, margin = batch_ownership(box.t[None], None if side is None else [side])
    return _back(box, owner, row0=True), _back(box, margin, row0=True)


# ---------------------------------------------------------------- stone status and the final score from playout ownership
STATUS_PLANES = 9   # gg_status_planes() of include/gymgo_amd_status.h
STATUS_NAMES = ('own_alive', 'own_dead', 'own_unsettled', 'opp_alive', 'opp_dead', 'opp_unsettled', 'own_area', 'opp_area', 'neutral')
STATUS_MAX_PLAYOUTS, STATUS_MAX_DEN = 1 << 20, 1024   # GG_STATUS_MAX_PLAYOUTS, GG_STATUS_MAX_DEN


def _status_inputs(ownership, playouts, threshold):
    """_planes' inputs of a status call - own, playouts, num, den -: ValueError for a Playouts without ownership, for playouts outside
    [1, STATUS_MAX_PLAYOUTS] and for a threshold that is not two integers 1 <= num <= den <= STATUS_MAX_DEN with 2 num > den -
    before a device is touched."""
    if isinstance(ownership, tuple) and hasattr(ownership, 'ownership'):
        ownership = ownership.ownership
        if ownership is None:
            raise ValueError('these Playouts carry no ownership: run batch_playouts(..., ownership=True)')
    integral = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))
    if not integral(playouts) or not 1 <= playouts <= STATUS_MAX_PLAYOUTS:
        raise ValueError('playouts must be an integer in [1, %d] (got %r)' % (STATUS_MAX_PLAYOUTS, playouts))
    try:
        num, den = threshold
    except (TypeError, ValueError):
        raise ValueError('threshold must be (num, den) (got %r)' % (threshold,)) from None
    if not integral(num) or not integral(den) or not (1 <= num <= den <= STATUS_MAX_DEN and 2 * num > den):
        raise ValueError('threshold (num, den) must be integers with 1 <= num <= den <= %d and 2 num > den (got %r)'
                         % (STATUS_MAX_DEN, threshold))
    return dict(own=ownership, playouts=int(playouts), num=int(num), den=int(den))


def batch_stone_status(batch_states, ownership, playouts, threshold=(2, 3), dtype=torch.uint8, out=None, orient=None, side=None,
                       counts=False):
    """Which chains the playouts of a position call alive, dead or unsettled, and the areas once the dead are gone ->
    [B, 9, N, N] of `dtype` (gg_batch_status), each value exactly 0 or 1 (STATUS_NAMES):
       0 / 1 / 2  own stones whose chain is alive / dead / unsettled
       3 / 4 / 5  the opponent's stones whose chain is alive / dead / unsettled
       6 / 7 / 8  own area / opponent's area / neutral points of the board with the dead chains of both colours taken off
                  (batch_area_planes' rule on what remains; unsettled chains stay, so the liberties a seki shares are neutral)
    ownership: int32 [B, 2, N, N], in how many of `playouts` playouts each point ended in black's / white's area, in the
    stored frame of the board - the `ownership` of batch_playouts(..., ownership=True), or those Playouts themselves
    (ValueError if they carry none).  threshold (num, den), integers with 1 <= num <= den <= 1024 and 2 num > den;
    1 <= playouts <= 2^20.  With K = playouts, a chain C (4-connected stones of one colour) of |C| stones, D = the sum over
    its stones of the other colour's count and A = that of its own colour's: C is dead iff D den >= num K |C|, else alive iff
    A den >= num K |C|, else unsettled - in 64-bit integers, so the result is bit-defined.  The counts are expected to obey
    0 <= count <= K and black + white <= K per point; other values give an unspecified status for their chain and nothing
    worse.  Counts on empty points are not read.
    Own = the player to move, or with side (B flags, a tensor or an array: 0 = black's view, non-zero = white's) the side
    named, whatever the turn plane says.  counts=True: also int32 [B, 4] = own area, opponent's area, own dead stones,
    opponent's dead stones (counts may also be a contiguous int32 [B, 4] device tensor to write into).  dtype, out (aligned to
    its element), orient (the planes turn, ownership is always in the stored frame, the counts do not turn) and NumPy input:
    as batch_area_planes.  Every bad argument is a ValueError before a device is touched.  One launch."""
    return _planes('gg_batch_status', STATUS_PLANES, 1, batch_states, False, dtype, out, orient, ('counts', counts, (4,), _I32),
                   side=side, **_status_inputs(ownership, playouts, threshold))


def stone_status(state, ownership, playouts, threshold=(2, 3), dtype=torch.uint8, side=None, counts=False):
    """batch_stone_status of one state [6, N, N] and its ownership [2, N, N] (or the Playouts of that state) -> [9, N, N] (with
    counts=True: and int32 [4]); side: None or one flag."""
    own = _status_inputs(ownership, playouts, threshold)['own']          # (every ValueError before a device is touched)
    shape = tuple(state.shape) if isinstance(state, torch.Tensor) else np.shape(state)
    if len(shape) != 3 or not isinstance(own, (torch.Tensor, np.ndarray)) or own.ndim != 3:
        raise ValueError('stone_status takes one state [6, N, N] and its ownership, int32 [2, N, N], or the Playouts that hold it')
    _status_own_arg(own[None], state if isinstance(state, torch.Tensor) else None, 1, shape[-1])
    batch_fn = lambda st, dt, **kw: batch_stone_status(st, own[None], playouts, threshold, dt, **kw)
    return _plane_single(batch_fn, state, dtype, side=None if side is None else [side], counts=bool(counts))


def batch_stone_status_tracked(tracked, ownership, playouts, threshold=(2, 3), dtype=torch.uint8, out=None, orient=None, side=None,
                               counts=False):
    """batch_stone_status of tracked boards (int32 [B, 5N+1], a device tensor) -> [B, 9, N, N] of `dtype`
    (gg_batch_status_tracked): bit for bit what batch_stone_status gives for batch_untrack(tracked); only the two stone row
    sets and the turn bit are read."""
    return _planes('gg_batch_status_tracked', STATUS_PLANES, 1, tracked, True, dtype, out, orient, ('counts', counts, (4,), _I32),
                   side=side, **_status_inputs(ownership, playouts, threshold))


# ---------------------------------------------------------------- position hashes and positional superko
HASH_SEED = 0x676F2D6861736821   # GG_HASH_SEED of include/gymgo_amd.h


# ---------------------------------------------------------------- history input planes: past positions and recent moves
PAST_MAX_POSITIONS = 8   # GG_PAST_MAX_POSITIONS of include/gymgo_amd_past.h


def _past_shape(positions, moves):
    """(T, moves as 0 / 1) of a plane request; ValueError outside gg_past_planes' domain (before a device is touched)."""
    if (isinstance(positions, bool) or not isinstance(positions, (int, np.integer))
            or not 1 <= int(positions) <= PAST_MAX_POSITIONS):
        raise ValueError('positions must be an integer in 1..%d (got %r)' % (PAST_MAX_POSITIONS, positions))
    if not isinstance(moves, (bool, np.bool_)) and not (isinstance(moves, (int, np.integer)) and moves in (0, 1)):
        raise ValueError('moves must be a flag (got %r)' % (moves,))
    return int(positions), int(bool(moves))


def past_plane_count(positions=8, moves=False):
    """The planes per board of a history request (gg_past_planes): 2 T, plus T - 1 with moves - 23 at the most."""
    T, mv = _past_shape(positions, moves)
    return 2 * T + (T - 1 if mv else 0)


class StoneHistory:
    """The earlier positions of a batch of games, on the device: what the history planes (batch_past_planes, PuctSearch(past=))
    read beside the current position.  positions = T (1 .. PAST_MAX_POSITIONS): position 0 is the current one, position t the
    one t plies ago; moves: whether the T - 1 "stone played t plies ago" planes are wanted too; planes = 2 T + (T - 1 if moves
    else 0).  rows: int32 [B, capacity, 2, N] - per entry the N black rows, then the N white rows, as bit masks, bit c = column
    c, as in tracked boards; count: int32 [B], the pushes per board.  A RING like PositionHistory: push writes at
    count % capacity, the position t >= 1 plies ago is entry (count - t) mod capacity and exists iff
    t <= min(max(count, 0), capacity).  capacity: default and minimum max(T - 1, 1).
    The ring holds the positions strictly BEFORE the current one: push a position before you play on it, one push per ply,
    passes included.  push / push_tracked are one launch each (gg_past_push[_tracked]), reset is plain torch; nothing reads
    back or synchronises.  device: None = the current ROCm device."""

    def __init__(self, batch_size, board_size, positions=8, moves=False, capacity=None, device=None):
        T, mv = _past_shape(positions, moves)
        batch_size, board_size = int(batch_size), int(board_size)
        if batch_size < 0 or not 2 <= board_size <= 19:
            raise ValueError('need batch_size >= 0 and 2 <= board_size <= 19 (got %d, %d)' % (batch_size, board_size))
        least = max(T - 1, 1)
        if capacity is None:
            capacity = least
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < least:
            raise ValueError('capacity must be an integer >= max(positions - 1, 1) = %d (got %r)' % (least, capacity))
        dev = _device() if device is None else device
        self.positions, self.moves, self.capacity, self.board_size = T, bool(mv), int(capacity), board_size
        self.planes = 2 * T + (T - 1 if mv else 0)
        self.rows = torch.zeros((batch_size, self.capacity, 2, board_size), dtype=_I32, device=dev)
        self.count = torch.zeros(batch_size, dtype=_I32, device=dev)

    def _mask(self, mask):
        """mask as uint8 / bool [B] on the ring's device, or None; ValueError first."""
        if mask is None:
            return None
        B = self.count.shape[0]
        if not isinstance(mask, torch.Tensor):
            mask = np.asarray(mask)
            ok = mask.dtype in (np.bool_, np.uint8)
        else:
            ok = mask.dtype in (torch.bool, _U8)
        if not ok or tuple(mask.shape) != (B,):
            raise ValueError('mask must be bool or uint8 [%d] (got %s %s)' % (B, mask.dtype, tuple(mask.shape)))
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask))
        return mask.to(self.count.device).contiguous()

    def _push(self, name, boards, mask):
        B, N = self.count.shape[0], self.board_size
        if B:
            _lib.call(name, boards, mask, self.rows, self.count, self.capacity, B, N, _lib.stream_ptr(self.count.device))
        return self

    def push(self, batch_states, mask=None):
        """The positions batch_states ([B, 6, N, N], a device tensor or an array: their stones) enter the rings of the
        boards where mask (None = all; bool or uint8 [B]) is set - written at count % capacity, count + 1; a masked-out
        board keeps every byte.  One launch (gg_past_push).  -> self."""
        if _states_shape(batch_states) != (self.count.shape[0], self.board_size):
            raise ValueError('batch_states must be [%d, 6, %d, %d] (got %s)' % (self.count.shape[0], self.board_size, self.board_size,
                                                                               tuple(np.shape(batch_states))))
        mask = self._mask(mask)
        st = _Box(batch_states).t
        if st.device != self.count.device:
            raise ValueError('batch_states must live on the history\'s device (%s)' % (self.count.device,))
        return self._push('gg_past_push', st, mask)

    def push_tracked(self, tracked, mask=None):
        """push of tracked boards (int32 [B, 5N+1], a device tensor): gg_past_push_tracked.  -> self."""
        if (not isinstance(tracked, torch.Tensor) or tracked.dim() != 2 or tracked.shape[0] != self.count.shape[0]
                or _tracked_size(tracked) != self.board_size):
            raise ValueError('tracked must be int32 [%d, %d]' % (self.count.shape[0], tracked_words(self.board_size)))
        mask = self._mask(mask)
        if tracked.device != self.count.device:
            raise ValueError('tracked must live on the history\'s device (%s)' % (self.count.device,))
        return self._push('gg_past_push_tracked', tracked, mask)

    def reset(self, mask=None):
        """Forget everything about the boards where mask (None = all) is set: entries and count zero.  -> self."""
        mask = self._mask(mask)
        if mask is None:
            self.rows.zero_()
            self.count.zero_()
        else:
            self.rows.masked_fill_(mask.bool()[:, None, None, None], 0)
            self.count.masked_fill_(mask.bool(), 0)
        return self


def _past_arg(history, B, N, what='history'):
    """ValueError unless history is a StoneHistory of B boards of size N (sizes None: not checked) whose tensors have the
    shapes its numbers say - before a device is touched."""
    if not isinstance(history, StoneHistory):
        raise ValueError('%s must be a StoneHistory (got %r)' % (what, type(history)))
    rows, count = history.rows, history.count
    _past_shape(history.positions, history.moves)
    if (not isinstance(rows, torch.Tensor) or not isinstance(count, torch.Tensor) or rows.dtype != _I32 or count.dtype != _I32
            or rows.dim() != 4 or tuple(rows.shape) != (count.shape[0], history.capacity, 2, history.board_size)
            or tuple(count.shape) != (rows.shape[0],) or not rows.is_contiguous() or not count.is_contiguous()
            or history.capacity < 1 or (B is not None and rows.shape[0] != B) or (N is not None and history.board_size != N)):
        raise ValueError('%s must be a StoneHistory of %s boards of size %s: rows int32 [B, H, 2, N], count int32 [B]' % (what, B, N))
    return history


def batch_past_planes(batch_states, history, dtype=torch.uint8, out=None, orient=None):
    """History input planes of every board -> [B, history.planes, N, N] of `dtype` (gg_batch_past), each value exactly 0 or 1.
    batch_states are the CURRENT positions, history (a StoneHistory of the B games) the positions before them; T and moves
    are the history's.  From the view of the player to move NOW:
       2 t      (t = 0 .. T-1)   own stones at position t (t plies ago; 0 = now)
       2 t + 1                   the opponent's stones at position t
       2 T + t  (t = 0 .. T-2)   with moves: the point of the move played t plies ago - the points occupied at position t and
                                 empty at position t + 1 -, nothing for a pass or where position t + 1 does not exist
    A position that does not exist (the game is younger, or the ring shorter) gives empty planes: AlphaGo Zero's convention.
    T = 8 without moves plus batch_features' plane 13 is AlphaGo Zero's input; the move planes are KataGo's recent moves.
    dtype, out (aligned to its element), orient (every position of a board is turned alike) and NumPy in / NumPy out: as
    batch_area_planes.  One launch; nothing synchronises."""
    return _planes('gg_batch_past', None, 1, batch_states, False, dtype, out, orient, history=history)


def batch_past_planes_tracked(tracked, history, dtype=torch.uint8, out=None, orient=None):
    """batch_past_planes of tracked boards (int32 [B, 5N+1], a device tensor): gg_batch_past_tracked, bit for bit what
    batch_past_planes gives for batch_untrack(tracked)."""
    return _planes('gg_batch_past_tracked', None, 1, tracked, True, dtype, out, orient, history=history)


def past_planes(states, positions=8, moves=False, dtype=torch.uint8):
    """The history planes of ONE game given as its positions [K, 6, N, N], oldest first (K >= 1) -> [planes, N, N] of the last
    position: a StoneHistory of one board filled with the T - 1 positions before it, then batch_past_planes."""
    T, mv = _past_shape(positions, moves)
    _feature_dtype(dtype)
    K, N = _states_shape(states, 'states')
    if K < 1:
        raise ValueError('states must hold at least one position')
    if not isinstance(states, torch.Tensor) and dtype == torch.bfloat16:
        raise ValueError('NumPy has no bfloat16: pass a device tensor, or another dtype')
    box = _Box(states)
    hist = StoneHistory(1, N, T, mv, device=box.t.device)
    for k in range(max(0, K - T), K - 1):
        hist.push(box.t[k:k + 1])
    return _back(box, batch_past_planes(box.t[K - 1:K], hist, dtype), row0=True)


def _puct_past_history(past, box):
    """past= of a move loop -> its StoneHistory (or None): an int T or a pair (T, moves) makes an empty one for the roots of
    box, made before the search that keeps it; a StoneHistory is used as given (PuctSearch checks it)."""
    if past is None or isinstance(past, StoneHistory):
        return past
    T, mv = _past_request(past)
    st = box.t
    if st.dim() != 4 or st.shape[2] != st.shape[3]:
        raise ValueError('batch_states must be [R, 6, N, N] (got %s)' % (tuple(st.shape),))
    return StoneHistory(st.shape[0], st.shape[2], T, mv, device=st.device)


def _past_request(past):
    """(T, moves) of past= given as an int T or a pair (T, moves); ValueError otherwise (before a device is touched)."""
    if isinstance(past, tuple) and len(past) == 2:
        return _past_shape(*past)
    if isinstance(past, bool) or not isinstance(past, (int, np.integer)):
        raise ValueError('past must be an integer T, a pair (T, moves) or a StoneHistory (got %r)' % (past,))
    return _past_shape(past, False)


def zobrist_keys():
    """The key table of the position hashes -> NumPy int64 [2, 19, 19]: keys[c, y, x] for a black (c = 0) / white (c = 1) stone
    at row y, column x - output number c * 361 + y * 19 + x + 1 of splitmix64 started at HASH_SEED, whatever the board size
    (include/gymgo_amd.h).  Computed here on the host, from Python integers, for users who hash elsewhere; the kernels hold the
    same numbers as a constant table."""
    M, x, keys = (1 << 64) - 1, HASH_SEED, []
    for _ in range(2 * 19 * 19):
        x = (x + 0x9E3779B97F4A7C15) & M
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        keys.append(z ^ (z >> 31))
    return np.array(keys, dtype=np.uint64).view(np.int64).reshape(2, 19, 19)


class PositionHistory:
    """The hashes of the positions a batch of games has been through, on the device: what the superko calls compare the move
    hashes against.  hashes: int64 [B, capacity], count: int32 [B] - the number of pushes per board; a board's valid entries
    are its first min(count, capacity).  A RING: push writes at count % capacity, so once a board has been pushed more than
    `capacity` times it holds its LAST `capacity` positions and older ones are forgotten - give it the length of the game
    (+ 1 for the starting position) to forget nothing.  device: None = the current ROCm device.  Plain torch ops on the
    current stream; nothing synchronises."""

    def __init__(self, batch_size, capacity, device=None):
        batch_size, capacity = int(batch_size), int(capacity)
        if batch_size < 0 or capacity < 1:
            raise ValueError('need batch_size >= 0 and capacity >= 1 (got %d, %d)' % (batch_size, capacity))
        dev = _device() if device is None else device
        self.capacity = capacity
        self.hashes = torch.zeros((batch_size, capacity), dtype=_I64, device=dev)
        self.count = torch.zeros(batch_size, dtype=_I32, device=dev)

    def _mask(self, mask):
        if mask is None:
            return None
        mask = torch.as_tensor(mask, device=self.count.device)
        if tuple(mask.shape) != tuple(self.count.shape) or mask.dtype not in (torch.bool, _U8):
            raise ValueError('mask must be bool or uint8 [%d] (got %s %s)' % (self.count.shape[0], mask.dtype, tuple(mask.shape)))
        return mask.bool()

    def push(self, hashes, mask=None):
        """Append hashes (int64 [B], batch_hash of the positions) to the boards where mask (None = all; bool or uint8 [B]) is
        set: written at count % capacity, count + 1.  -> self."""
        h = torch.as_tensor(hashes, device=self.count.device)
        if tuple(h.shape) != tuple(self.count.shape) or h.dtype != _I64:
            raise ValueError('hashes must be int64 [%d] (got %s %s)' % (self.count.shape[0], h.dtype, tuple(h.shape)))
        mask = self._mask(mask)
        at = (self.count.to(_I64) % self.capacity)[:, None]
        if mask is not None:
            h = torch.where(mask, h, self.hashes.gather(1, at)[:, 0])
        self.hashes.scatter_(1, at, h[:, None])
        self.count += 1 if mask is None else mask.to(_I32)
        return self

    def reset(self, mask=None):
        """Forget everything about the boards where mask (None = all) is set: entries and count zero.  -> self."""
        mask = self._mask(mask)
        if mask is None:
            self.hashes.zero_()
            self.count.zero_()
        else:
            self.hashes.masked_fill_(mask[:, None], 0)
            self.count.masked_fill_(mask, 0)
        return self


def _history_arg(history, B):
    """(hashes int64 [B, H], count int32 [B], H) of a PositionHistory (or a (hashes, count) pair); ValueError otherwise -
    before a device is touched."""
    hashes, count = history if isinstance(history, tuple) else (getattr(history, 'hashes', None), getattr(history, 'count', None))
    if (not isinstance(hashes, torch.Tensor) or not isinstance(count, torch.Tensor) or hashes.dtype != _I64 or count.dtype != _I32
            or hashes.dim() != 2 or hashes.shape[0] != B or tuple(count.shape) != (B,) or not hashes.is_contiguous()
            or not count.is_contiguous()):
        raise ValueError('history must be a PositionHistory of %d boards: hashes int64 [%d, H], count int32 [%d]' % (B, B, B))
    return hashes, count, hashes.shape[1]


def _hash_shape(boards, tracked):
    """(B, N) of byte planes (a tensor or an array) or tracked boards (a tensor); ValueError otherwise, before a device is touched."""
    if not tracked:
        return _states_shape(boards)
    if not isinstance(boards, torch.Tensor) or boards.dim() != 2:
        raise ValueError('tracked boards are int32 [B, 5N+1] device tensors')
    return boards.shape[0], _tracked_size(boards)


def _move_hashes(boards, tracked, history=None, out=None, hashes=False, repeat=False, rows=False):
    """One launch of gg_batch_move_hashes[_tracked] -> (box or None, hashes, repeat, rows): device tensors, None where not asked for."""
    B, N = _hash_shape(boards, tracked)
    A = N * N + 1
    hist = _history_arg(history, B) if repeat or rows else (None, None, 0)
    _planes_out(out, (B, A), _I64, 8)
    box = None if tracked else _Box(boards)
    st = boards if tracked else box.t
    dev = st.device
    _planes_out(out, (B, A), _I64, 8, dev if st.is_cuda else None)
    h = (out if out is not None else torch.empty((B, A), dtype=_I64, device=dev)) if hashes else None
    rp = torch.empty((B, A), dtype=_U8, device=dev) if repeat else None
    rw = torch.empty((B, N), dtype=_I32, device=dev) if rows else None
    _lib.call('gg_batch_move_hashes_tracked' if tracked else 'gg_batch_move_hashes', st, hist[0], hist[1], hist[2], h, rp, rw, B, N,
              _lib.stream_ptr(dev))
    return box, h, rp, rw


def _batch_hash(boards, tracked):
    B, N = _hash_shape(boards, tracked)
    box = None if tracked else _Box(boards)
    st = boards if tracked else box.t
    out = torch.empty(B, dtype=_I64, device=st.device)
    _lib.call('gg_batch_hash_tracked' if tracked else 'gg_batch_hash', st, out, B, N, _lib.stream_ptr(st.device))
    return out if box is None else _back(box, out)


def batch_hash(batch_states):
    """The 64-bit position hash of every board -> int64 [B] (gg_batch_hash): the XOR of zobrist_keys()[colour, y, x] over the
    stones.  Positional: turn, pass, ko and game-over planes do not enter; the empty board hashes to 0.  For transposition
    checks and the de-duplication of records without moving 6 N^2 bytes per board to the host.  One launch."""
    return _batch_hash(batch_states, False)


def batch_hash_tracked(tracked):
    """batch_hash of tracked boards (int32 [B, 5N+1], a device tensor) -> int64 [B] (gg_batch_hash_tracked)."""
    return _batch_hash(tracked, True)


def position_hash(state):
    """batch_hash of one state [6, N, N] -> an int64 scalar."""
    box = _Box(state)
    return _back(box, batch_hash(box.t[None]), row0=True)


def batch_move_hashes(batch_states, out=None):
    """The hash of the position after every move of the mover -> int64 [B, N*N + 1] (gg_batch_move_hashes), WITHOUT building the
    children: at a candidate point (empty, plane 3 clear, game not over - the legal plane of batch_features) the hash after
    the stone is put there and the opponent chains left without a liberty are removed; at the pass and at every other
    point the board's own hash.  Every slot is written.  out: a contiguous int64 device tensor of that shape to write into.
    One launch; device memory of the result: 8 * B * (N^2 + 1) bytes."""
    box, h, _, _ = _move_hashes(batch_states, False, out=out, hashes=True)
    return _back(box, h)


def batch_move_hashes_tracked(tracked, out=None):
    """batch_move_hashes of tracked boards (int32 [B, 5N+1], a device tensor; gg_batch_move_hashes_tracked).  The class rows
    are read - they say which opponent stones are in atari, so no group is counted - and must belong to the position."""
    return _move_hashes(tracked, True, out=out, hashes=True)[1]


def move_hashes(state):
    """batch_move_hashes of one state [6, N, N] -> int64 [N*N + 1]."""
    box = _Box(state)
    return _back(box, batch_move_hashes(box.t[None]), row0=True)


def batch_superko_moves(batch_states, history):
    """The moves positional superko forbids -> uint8 [B, N*N + 1] (the repeat mask of gg_batch_move_hashes): 1 at every
    candidate point whose move hash equals a valid entry of `history` (a PositionHistory of the B games, the current
    position included), 0 elsewhere; the pass is never a repeat.  Equal 64-bit hashes are taken as equal positions (a
    collision, about 2^-64 per comparison, forbids a legal move).  One launch."""
    box, _, rp, _ = _move_hashes(batch_states, False, history, repeat=True)
    return _back(box, rp)


def batch_superko_moves_tracked(tracked, history):
    """batch_superko_moves of tracked boards (gg_batch_move_hashes_tracked)."""
    return _move_hashes(tracked, True, history, repeat=True)[2]


def batch_forbid_repeats(batch_states, history):
    """OR the repeat points of batch_superko_moves into plane 3 of batch_states IN PLACE -> batch_states.  Plane 3 then means
    "ko, suicide, occupied or superko", and every consumer of it - sampling, batch_valid_moves, the legal plane of
    batch_features, the step kernels, the searches - treats those points as illegal with no change of its own.  The next
    step recomputes plane 3 for the next mover, so the call is made once per position, before its move is chosen."""
    B, N = _states_shape(batch_states)
    if isinstance(batch_states, torch.Tensor) and batch_states.dtype != _U8:
        raise ValueError('batch_states must be uint8 to be changed in place (got %s)' % batch_states.dtype)
    rep = batch_superko_moves(batch_states, history)
    if isinstance(batch_states, torch.Tensor):
        batch_states[:, govars.INVD_CHNL].bitwise_or_(rep[:, :N * N].view(B, N, N))
    else:
        inv = batch_states[:, govars.INVD_CHNL]
        np.maximum(inv, rep[:, :N * N].reshape(B, N, N).astype(inv.dtype), out=inv)
    return batch_states


def batch_forbid_repeats_tracked(tracked, history):
    """OR the repeat points into the invalid rows of tracked boards IN PLACE -> tracked (the `rows` output of
    gg_batch_move_hashes_tracked); gg_batch_play_moves_tracked, the tracked draws and gg_puct_legal then refuse them."""
    rows = _move_hashes(tracked, True, history, rows=True)[3]
    N = _tracked_size(tracked)
    tracked[:, 2 * N:3 * N].bitwise_or_(rows)
    return tracked


def batch_play_moves_tracked(tracked, moves, played=None):
    """IN PLACE batch_play_moves on tracked boards; moves [B, T] (T = 1: one GoEnv.step per game) -> played int32 [B]."""
    N = _tracked_size(tracked)
    B = tracked.shape[0]
    moves = moves.to(device=tracked.device, dtype=_I32).reshape(B, -1).contiguous()
    if played is None:
        played = torch.empty(B, dtype=_I32, device=tracked.device)
    _lib.call('gg_batch_play_moves_tracked', tracked, moves, played, B, N, moves.shape[1], _lib.stream_ptr(tracked.device))
    return played


def batch_env_step_tracked(tracked, actions=None, rng=None, komi=0.0, reward_method='real', auto_reset=True, out=None,
                           states_out=None, steps_done=None, weights=None):
    """IN PLACE GoEnv.step (gym_go/envs/go_env.py:49-76) of every game on TRACKED boards in ONE launch
    (gg_batch_env_step_tracked): no per-ply analysis.  -> (rewards, dones, status, taken) like batch_env_step;
    states_out: a uint8 [B,6,N,N] device tensor that receives the byte-plane observation of every game (optional);
    steps_done: an int64 [B] device tensor, += 1 for every game whose step was played (optional).
    weights: float32 [B, N*N+1] policy weights - the move of every game is then DRAWN from them by the same launch
    (gg_batch_env_step_tracked_weighted: gogame.random_weighted_action, gym_go/gogame.py:385-392, masked by the game's
    invalid moves, with `rng`); `taken` receives the drawn moves, a game without a positive playable weight is refused."""
    N = _tracked_size(tracked)
    B = tracked.shape[0]
    dev = tracked.device
    if weights is not None:
        if actions is not None:
            raise ValueError('give actions OR weights, not both')
        if rng is None:
            raise ValueError('drawing from weights needs the rng state')
        weights, wcode = _weights_tensor(weights, B, N, dev)
    if actions is None and rng is None:
        raise ValueError('batch_env_step_tracked needs actions or an rng state to draw them with')
    if out is None:
        out = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=_U8, device=dev),
               torch.empty(B, dtype=_I32, device=dev), torch.empty(B, dtype=_I32, device=dev))
    if states_out is not None and tuple(states_out.shape) != (B, govars.NUM_CHNLS, N, N):
        raise ValueError('states_out must be uint8 [B, 6, N, N]')
    rewards, dones, status, taken = out
    name, move = ('gg_batch_env_step_tracked', (actions,)) if weights is None else ('gg_batch_env_step_tracked_weighted', (weights, wcode))
    _lib.call(name, tracked, *move, rng, rewards, dones, status, taken, states_out, steps_done, B, N, float(komi),
              REWARD_METHODS[reward_method], int(bool(auto_reset)), _lib.stream_ptr(dev))
    return out


# ---------------------------------------------------------------- Monte Carlo playouts to the end of the game
# K uniform-random playouts of every root until the game ends (GoEnv.uniform_random_action + step, gym_go/envs/go_env.py:49-81),
# scored with Tromp-Taylor areas (gogame.areas / winning, gym_go/gogame.py:225-230, :275-300) and reduced per root on the
# device (gg_playouts_begin / gg_playouts_advance, include/gymgo_amd.h): the leaf values of a Monte Carlo search, value
# targets, ownership estimates.

Playouts = collections.namedtuple('Playouts', 'black_wins white_wins draws unfinished margin_sum plies_sum ownership')
PlayoutsAmaf = collections.namedtuple('PlayoutsAmaf', Playouts._fields + ('amaf',))
PlayoutsAmaf.__doc__ = """Playouts plus amaf (batch_playouts(..., amaf=True)): int32 [R, 2, 3, N, N] - per root and colour (0 black,
1 white), [0]: in how many playouts the colour was the first to play the point (all-moves-as-first), [1] / [2]: how many of
those were scored as a black / a white win."""
Playouts.__doc__ = """Per-root results of batch_playouts: black_wins / white_wins / draws / unfinished (int32: outcome
sign(black - white - komi); playouts cut off by max_plies), margin_sum (int64: sum of black - white area), plies_sum (int64:
plies played) and ownership (int32 [R, 2, N, N]: per point, in how many playouts it ended in black's / white's area; None
unless asked for)."""

# the seeding of rng_seed and of the playout jobs (k_rng_seed, csrc/gg_common.h; po_seed, csrc/gg_po.h): the multiplier of the
# game / job index and splitmix64's increment
_JOB_MUL, _GOLDEN_GAMMA, _M64 = 0xD1342543DE82EF95, 0x9E3779B97F4A7C15, 2 ** 64 - 1


def _drive_playouts(advance, counter, J, S, max_plies, chunk_plies, dev, what):
    """Host loop of batch_playouts / batch_move_playouts after the begin call: queues advance(n) (n chunks) until the
    counter's outstanding-job count reaches zero."""
    # Every playout is harvested within max_plies / chunk_plies chunks of its start and all S slots are busy while the queue
    # holds jobs, so this many chunks always suffice; more means the device did not do what it was asked: raise, never spin.
    M = int(max_plies) // int(chunk_plies)
    bound = (-(-J // S) + 1) * M + 2
    step = max(1, min(4, M))
    # Two batches of chunks in flight: the outstanding-job count of one is read (pinned copy + event wait) while the next runs.
    host = [torch.empty(2, dtype=_I64, pin_memory=True) for _ in range(2)]
    pending, queued, k = [], 0, 0
    with torch.cuda.device(dev):
        while True:
            if queued < bound:
                n = min(step, bound - queued)
                advance(n)
                queued += n
                host[k].copy_(counter, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending.append((ev, host[k]))
                k ^= 1
            if len(pending) == 2 or queued >= bound:
                ev, h = pending.pop(0)
                ev.synchronize()
                outstanding = int(h[1]) - int(h[0])
                if outstanding == 0:
                    break
                if not pending:
                    raise _lib.GymGoNativeError('%s: %d jobs still outstanding after %d chunks (the bound for %d '
                                                'jobs on %d slots)' % (what, outstanding, queued, J, S))
        for ev, _ in pending:   # (the pinned buffers stay alive until the copies still queued have landed)
            ev.synchronize()


def _run_queue(family, what, head, komi, bufs, counter, J, S, max_plies, chunk_plies, dev, policy=0, amaf=None):
    """gg_<family>_begin, then gg_<family>_advance_policy (_policy2 for a policy beyond no_eye_fill, _policy3 for one of
    LOCAL_PLAYOUT_POLICIES; _amaf with amaf) until the counter drains (_drive_playouts).  head: the arguments up to chunk_plies,
    bufs: those from slots on (_queue_args, and what the family adds); advance takes komi, the chunk count and the playout
    policy's code between the two, and behind bufs _policy3 the slots' previous actions (int32 [S], -1 after begin), _amaf the
    buffers of amaf (_amaf_buffers; all but the log zeroed here: only written log entries are read)."""
    begin = 'gg_%s_begin' % family
    advance = 'gg_%s_advance_%s' % (family, 'policy' + ('', '', '2', '3')[int(policy)] if amaf is None else 'amaf')
    stream = _lib.current_raw_stream(dev)   # torch's current stream: the counter copies of _drive_playouts go there too
    _lib.call(begin, *head, *bufs, stream)
    if amaf is not None:
        for t in amaf[1:]:
            t.zero_()
        bufs = tuple(bufs) + tuple(amaf)
    elif int(policy) in LOCAL_PLAYOUT_POLICIES.values():
        with torch.cuda.device(dev):
            bufs = tuple(bufs) + (torch.full((S,), -1, dtype=_I32, device=dev),)
    _drive_playouts(lambda n: _lib.call(advance, *head, float(komi), n, int(policy), *bufs, stream),
                    counter, J, S, max_plies, chunk_plies, dev, what)


def _slot_buffers(S, N, dev):
    """Working slots of the playout queue: (slots, rng, plies, job, counter) device tensors."""
    return (torch.empty((S, tracked_words(N)), dtype=_I32, device=dev), torch.empty(S, dtype=_I64, device=dev),
            torch.empty(S, dtype=_I64, device=dev), torch.empty(S, dtype=_I64, device=dev),
            torch.empty(2, dtype=_I64, device=dev))


def _playout_buffers(R, S, N, dev):
    """Everything _run_playouts writes for R roots on S slots: (slots, rng, plies, job, counter, counts, sums)."""
    return _slot_buffers(S, N, dev) + (torch.empty((R, 4), dtype=_I32, device=dev), torch.empty((R, 2), dtype=_I64, device=dev))


def _queue_args(slots, rng, plies, job, counter, counts, sums):
    """The queue's buffers as both families' C entry points take them: slots, rng, plies, job, S, counter, counts, sums."""
    return slots, rng, plies, job, slots.shape[0], counter, counts, sums


def _run_playouts(roots, R, N, K, max_plies, komi, seed, first_root, ownership, S, chunk_plies, dev, buffers=None, policy=0,
                  amaf=None):
    """Device work of batch_playouts on tracked roots: -> (counts int32 [R, 4], sums int64 [R, 2], own or None); no launch
    for R = 0.  buffers: _playout_buffers(R, S, N, dev) to reuse (a search evaluates its leaves with the same buffers every
    iteration).  amaf: _amaf_buffers(R, S, N, chunk_plies, dev) - the playouts then run through gg_playouts_advance_amaf and
    leave their first-play counts in amaf[3]."""
    buffers = buffers if buffers is not None else _playout_buffers(R, S, N, dev)
    counter, counts, sums = buffers[4:]
    own = torch.empty((R, 2, N, N), dtype=_I32, device=dev) if ownership else None
    if R > 0:
        head = (roots, R, N, K, int(first_root), int(seed) & _M64, int(max_plies), int(chunk_plies))
        # (amaf= only when given: tests/test_gpu_tactics.py and test_gpu_pattern.py stand in for _run_queue without that keyword)
        with_amaf = {} if amaf is None else {'amaf': amaf}
        _run_queue('playouts', 'batch_playouts', head, komi, _queue_args(*buffers) + (own,), counter, R * K, S, max_plies,
                   chunk_plies, dev, policy, **with_amaf)
    return counts, sums, own


def _amaf_buffers(R, S, N, chunk_plies, dev):
    """What gg_playouts_advance_amaf takes beyond the queue's buffers: (log int16 [S, chunk_plies], first int32 [S, 2, N],
    mark int64 [S], amaf int32 [R, 2, 3, N, N])."""
    return (torch.empty((S, chunk_plies), dtype=torch.int16, device=dev), torch.empty((S, 2, N), dtype=_I32, device=dev),
            torch.empty(S, dtype=_I64, device=dev), torch.empty((R, 2, 3, N, N), dtype=_I32, device=dev))


def _playout_args(st, playouts, max_plies, chunk_plies, first_root):
    """Argument checks and defaults shared by batch_playouts and batch_move_playouts -> (R, N, K, max_plies, chunk_plies)."""
    if st.dim() != 4 or st.shape[1] != govars.NUM_CHNLS or st.shape[2] != st.shape[3]:
        raise ValueError('batch_states must be [R, 6, N, N] (got %s)' % (tuple(st.shape),))
    R, N, K, chunk_plies = st.shape[0], st.shape[2], int(playouts), int(chunk_plies)
    if chunk_plies < 1:
        raise ValueError('chunk_plies must be >= 1')
    if max_plies is None:
        max_plies = -(-8 * N * N // chunk_plies) * chunk_plies
    max_plies = int(max_plies)
    if K < 1 or max_plies < 1 or max_plies % chunk_plies or int(first_root) < 0:
        raise ValueError('need playouts >= 1, max_plies >= 1 and a multiple of chunk_plies, first_root >= 0 (got %d, %d, %d, %d)'
                         % (K, max_plies, chunk_plies, int(first_root)))
    return R, N, K, max_plies, chunk_plies


def _default_slots(slots):
    return 256 * int(_lib.lib().gg_device_cus()) if slots is None else slots   # 19x19: k_rollout5 from 256 games per CU on


def _track_roots(st):
    """batch_track; an empty batch without a launch (the run helpers return their empty results before they touch it)."""
    return batch_track(st) if st.shape[0] else torch.empty((0, tracked_words(st.shape[2])), dtype=_I32, device=st.device)


def _back(box, res, row0=False):
    """Results in the caller's form: every tensor of `res` (a tensor, None, or a - nested - namedtuple of them) as it is or, for
    NumPy input, as a NumPy array; row0: its row 0 (the single-state forms)."""
    if res is None:
        return None
    if isinstance(res, tuple):
        return type(res)(*[_back(box, t, row0) for t in res])
    res = res[0] if row0 else res
    return res.cpu().numpy() if box.numpy else res


def _policy_kw(kw):
    """The checks of a forwarding call's policy= (_policy_code) and of what goes with it, before a device is touched: the move
    log behind amaf=True and rave_equiv= serves PLAYOUT_POLICIES only."""
    pol = _policy_code(kw.get('policy', 'uniform'))
    if pol not in PLAYOUT_POLICIES.values() and (kw.get('amaf') or kw.get('rave_equiv') is not None):
        raise ValueError('amaf=True / rave_equiv= have no policy=%r: the move log serves %s' % (kw['policy'], sorted(PLAYOUT_POLICIES)))
    return pol


def _single(batch_fn, state, *args, **kw):
    """The single-state form of a batch function: state [6, N, N] as a batch of one, row 0 of every result."""
    _policy_kw(kw)
    box = _Box(state)
    return _back(box, batch_fn(box.t[None], *args, **kw), row0=True)


def _best_legal(box, legal, score):
    """int64 [R]: per row of score (int64 [R, A], above -2^62) the legal action with the largest score, ties to the lowest
    action, -1 for a row without a legal action."""
    score = torch.where(legal, score, torch.full_like(score, -(2 ** 62)))
    idx = torch.arange(score.shape[1], dtype=_I64, device=score.device).expand_as(score)
    act = torch.where(score == score.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, score.shape[1])).min(dim=1).values
    return _back(box, torch.where(legal.any(dim=1), act, torch.full_like(act, -1)))


def batch_playouts(batch_states, playouts, max_plies=None, komi=0.0, seed=20260927, first_root=0, ownership=False, slots=None,
                   chunk_plies=32, *, policy='uniform', amaf=False):
    """`playouts` uniform-random playouts of every root of batch_states ([R, 6, N, N]) to the end of the game, scored and
    reduced per root on the device -> Playouts (device tensors for a device tensor, NumPy arrays for NumPy input).

    Playout j of root r is global job p = (first_root + r) * playouts + j: its generator is rng_seed(.., seed, first_game=p),
    it plays batch_rollout's sampler without auto-reset from root r until the game ends or max_plies plies have been played
    (then it also counts as unfinished) and is scored as it stands.  Results are integer sums: they do not depend on
    `slots` (working boards, default: enough to fill the device) or `chunk_plies` (plies per rollout launch between two
    harvests; max_plies must be a multiple of it), and shards by first_root concatenate to the whole.  Default max_plies:
    8 N^2 rounded up to a multiple of chunk_plies.  The roots are not modified.
    policy: what a playout ply draws from - 'uniform' (batch_rollout's sampler), 'no_eye_fill', 'tactical' or 'pattern'
    (batch_rollout_tracked; under 'pattern' a playout's first ply has no previous move, whatever led to the root).
    amaf=True: the same playouts, with their all-moves-as-first statistics -> PlayoutsAmaf (gg_playouts_advance_amaf: the
    rollouts log their moves, the harvest reduces per root which colour played each point first, and with what outcome)."""
    pol = _policy_kw({'policy': policy, 'amaf': amaf})
    box = _Box(batch_states)
    st = box.t
    R, N, K, max_plies, chunk_plies = _playout_args(st, playouts, max_plies, chunk_plies, first_root)
    if amaf and chunk_plies > 4096:
        raise ValueError('amaf=True needs chunk_plies <= 4096 (got %d)' % chunk_plies)
    S = max(1, min(int(_default_slots(slots)), R * K))
    abufs = _amaf_buffers(R, S, N, chunk_plies, st.device) if amaf else None
    if amaf and R == 0:
        abufs[3].zero_()
    counts, sums, own = _run_playouts(_track_roots(st), R, N, K, max_plies, komi, seed, first_root, ownership, S, chunk_plies,
                                      st.device, policy=pol, amaf=abufs)
    res = Playouts(counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3], sums[:, 0], sums[:, 1], own)
    return _back(box, PlayoutsAmaf(*res, abufs[3]) if amaf else res)


def playouts(state, n, **kw):
    """batch_playouts of one state [6, N, N] -> Playouts of scalars (and ownership [2, N, N])."""
    return _single(batch_playouts, state, n, **kw)


# ---------------------------------------------------------------- the final score: playouts, stone status, areas
FinalScore = collections.namedtuple('FinalScore', 'black_area white_area margin winner owner dead unsettled playouts')
FinalScore.__doc__ = """Per-board results of batch_final_score: black_area / white_area (int32: the areas with the dead stones
taken off), margin (int32: black - white, no komi), winner (float64: sign(margin - komi), as batch_winning), owner (int8
[R, N, N]: +1 black's point, -1 white's, 0 neutral), dead / unsettled (uint8 [R, N, N]: the stones of either colour whose chain is
dead / unsettled) and playouts (the Playouts that voted, ownership included)."""


def batch_final_score(batch_states, playouts=64, komi=0.0, threshold=(2, 3), policy='no_eye_fill', **playout_kw):
    """Who won: `playouts` playouts of every board (batch_playouts with ownership=True, policy and playout_kw - max_plies,
    seed, first_root, slots, chunk_plies - passed on), then one batch_stone_status launch from black's view with that
    ownership and `threshold` -> FinalScore.  The dead chains are taken off before the areas are counted, so a stone left
    inside the other side's territory no longer turns that territory neutral, as it does for batch_areas / batch_winning.
    NumPy in gives NumPy out; every ValueError of the two calls comes before a device is touched."""
    B, N = _states_shape(batch_states)
    if 'ownership' in playout_kw or 'amaf' in playout_kw:
        raise ValueError('batch_final_score runs its playouts with ownership=True and without amaf')
    _status_inputs(None, playouts, threshold)
    _policy_kw({'policy': policy})
    box = _Box(batch_states)
    st = box.t
    po = batch_playouts(st, playouts, komi=komi, ownership=True, policy=policy, **playout_kw)
    planes, counts = batch_stone_status(st, po.ownership, playouts, threshold, side=torch.zeros(B, dtype=_U8, device=st.device),
                                        counts=True)
    margin = counts[:, 0] - counts[:, 1]
    return _back(box, FinalScore(counts[:, 0], counts[:, 1], margin, torch.sign(margin.to(torch.float64) - komi),
                                 planes[:, 6].to(torch.int8) - planes[:, 7].to(torch.int8), planes[:, 1] | planes[:, 4],
                                 planes[:, 2] | planes[:, 5], po))


def final_score(state, playouts=64, **kw):
    """batch_final_score of one state [6, N, N] -> FinalScore of scalars and [N, N] planes (its Playouts: those of `playouts`)."""
    return _single(batch_final_score, state, playouts, **kw)


# ---------------------------------------------------------------- flat Monte Carlo: playouts per legal first move
# The statistics batch_playouts gives per root, per legal first move instead (gg_move_playouts_plan / _begin / _advance,
# include/gymgo_amd.h): the root's legal actions are listed on the device, and a refill of the playout queue plays the
# job's first move before its playout starts - no child is materialised, no playout runs for an illegal action.

MovePlayouts = collections.namedtuple('MovePlayouts', 'legal black_wins white_wins draws unfinished margin_sum plies_sum')
MovePlayouts.__doc__ = """Per (root, first move) results of batch_move_playouts, each [R, N*N + 1]: legal (bool), black_wins /
white_wins / draws / unfinished (int32), margin_sum / plies_sum (int64; plies_sum does not count the first move) - as in
Playouts, all zero where the move is not legal."""


def _run_move_playouts(roots, R, N, K, max_plies, komi, seed, first_root, slots, chunk_plies, dev, policy=0):
    """Device work of batch_move_playouts on tracked roots: -> (legal bool [R, A], counts int32 [R, A, 4], sums [R, A, 2]); no
    launch for R = 0."""
    A = N * N + 1
    counts = torch.zeros((R, A, 4), dtype=_I32, device=dev)
    sums = torch.zeros((R, A, 2), dtype=_I64, device=dev)
    legal = torch.zeros((R, A), dtype=torch.bool, device=dev)
    if R == 0:
        return legal, counts, sums
    offsets = torch.empty(R + 1, dtype=_I32, device=dev)
    plan = torch.empty(R * A, dtype=_I32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('gg_move_playouts_plan', roots, R, N, offsets, plan, _lib.current_raw_stream(dev))
        T = int(offsets[R])   # (a synchronising read, as the un-padded children do)
    if T == 0:
        return legal, counts, sums
    legal.view(-1)[plan[:T].long()] = True
    J = T * K
    S = max(1, min(int(slots), J))
    slot_bufs = _slot_buffers(S, N, dev)
    head = (roots, R, N, plan, T, K, int(first_root), int(seed) & _M64, int(max_plies), int(chunk_plies))
    _run_queue('move_playouts', 'batch_move_playouts', head, komi, _queue_args(*slot_bufs, counts, sums), slot_bufs[4], J, S,
               max_plies, chunk_plies, dev, policy)
    return legal, counts, sums


def batch_move_playouts(batch_states, playouts, max_plies=None, komi=0.0, seed=20260927, first_root=0, slots=None,
                        chunk_plies=32, *, policy='uniform'):
    """Flat Monte Carlo: `playouts` playouts after every legal first move of every root of batch_states ([R, 6, N, N]),
    reduced per (root, action) on the device -> MovePlayouts of [R, N*N + 1] (device tensors for a device tensor, NumPy
    arrays for NumPy input).

    Action a is legal at root r when the root's game has not ended and a is the pass or its plane-3 (invalid) bit is clear.
    A root whose game has ended has NO legal first move - its row is all False and zero (unlike children(), which keeps
    every slot of such a state).  Playout j of the legal pair (r, a) is global job ((first_root + r) * A + a) * playouts + j
    (A = N*N + 1): it starts from next_state(root_r, a) and is played and scored as batch_playouts plays its playouts,
    max_plies counting the plies after the first move.  So row (r, a) equals batch_playouts(next_state(root_r, a)[None],
    playouts, first_root=(first_root + r) * A + a, ...).  Defaults, validation and the invariance under slots, chunk_plies
    and sharding by first_root are those of batch_playouts.  The roots are not modified.
    policy: as in batch_playouts; it governs the playout plies only - every legal first move is tried."""
    pol = _policy_code(policy)
    box = _Box(batch_states)
    st = box.t
    R, N, K, max_plies, chunk_plies = _playout_args(st, playouts, max_plies, chunk_plies, first_root)
    legal, counts, sums = _run_move_playouts(_track_roots(st), R, N, K, max_plies, komi, seed, first_root, _default_slots(slots),
                                             chunk_plies, st.device, policy=pol)
    return _back(box, MovePlayouts(legal, counts[..., 0], counts[..., 1], counts[..., 2], counts[..., 3], sums[..., 0],
                                   sums[..., 1]))


def move_playouts(state, n, **kw):
    """batch_move_playouts of one state [6, N, N] -> MovePlayouts of [N*N + 1] vectors."""
    return _single(batch_move_playouts, state, n, **kw)


def flat_mc_actions(batch_states, playouts, **kw):
    """The flat Monte Carlo move of every root -> int64 [R]: the legal action with the most (mover's wins - mover's losses)
    over batch_move_playouts(batch_states, playouts, **kw), the mover being the root's turn (plane 2); ties go to the lowest
    action, a root without a legal move gives -1."""
    _policy_code(kw.get('policy', 'uniform'))
    box = _Box(batch_states)
    res = batch_move_playouts(box.t, playouts, **kw)
    bw, ww = res.black_wins.to(_I64), res.white_wins.to(_I64)
    white = box.t[:, govars.TURN_CHNL, 0, 0].to(torch.bool)[:, None]
    return _best_legal(box, res.legal, torch.where(white, ww - bw, bw - ww))


# ---------------------------------------------------------------- UCT tree search over the playouts
# R independent searches (gg_uct_begin / gg_uct_select / gg_uct_backup, include/gymgo_amd.h): the trees live on the device,
# each iteration selects and expands one leaf per root, evaluates the R leaves with batch_playouts' queue and backs the
# counts up - the host only queues launches and waits for the playout queue to drain.

Uct = collections.namedtuple('Uct', 'legal visits black_wins white_wins draws root_visits unfinished plies_sum nodes tree')
Uct.__doc__ = """Results of batch_uct per root: legal (bool [R, A], A = N*N + 1), visits / black_wins / white_wins / draws
(int32 [R, A]: the stats of the root's children, 0 where there is none), root_visits (int32 [R]), unfinished / plies_sum
(int64 [R]: over every playout of the search), nodes (int32 [R]: tree nodes in use) and tree (UctTree or None)."""
UctTree = collections.namedtuple('UctTree', 'parent action visits black_wins white_wins draws')
UctRave = collections.namedtuple('UctRave', Uct._fields + ('rave_visits', 'rave_score'))
UctRave.__doc__ = """Uct of a RAVE search (batch_uct(..., rave_equiv=k)), plus the root's AMAF pairs: rave_visits / rave_score (int32
[R, N*N]: per point, the simulations in which the root's mover played it first, and twice its wins plus the draws among them).
tree, when asked for, is a UctRaveTree."""
UctRaveTree = collections.namedtuple('UctRaveTree', UctTree._fields + ('node_amaf',))
UctRaveTree.__doc__ = """UctTree plus node_amaf (int32 [R, iterations + 1, N*N, 2]: the pairs of every node)."""
UctTree.__doc__ = """The whole tree of every root, each field int32 [R, iterations + 1] ([R, iterations * leaves + 1] with `leaves`) indexed by node (node 0 = the root;
parent / action -1 at the root and at unused nodes, whose stats are 0)."""


def _uct_seed(seed, i):
    """Base seed of iteration i's playouts, on the host (no device round trip per iteration): restates gg_rng_seed(base_seed=
    seed, first_game=i) (k_rng_seed), the generator of game i = (seed ^ i * _JOB_MUL) + _GOLDEN_GAMMA mod 2^64."""
    return (((int(seed) & _M64) ^ ((int(i) * _JOB_MUL) & _M64)) + _GOLDEN_GAMMA) & _M64


def _uct_args(iterations, playouts, c):
    I, K, c = int(iterations), int(playouts), float(c)
    if I < 1 or not math.isfinite(c) or c < 0 or I * K >= 2 ** 31:
        raise ValueError('need iterations >= 1, c >= 0 and finite, iterations * playouts < 2^31 (got %d, %r, %d)' % (I, c, I * K))
    return I, c


def _legal_roots(st):
    """bool [R, A]: the pass and every point whose plane-3 bit is clear, nothing for a root whose game has ended."""
    R, N = st.shape[0], st.shape[2]
    legal = torch.cat([st[:, govars.INVD_CHNL].reshape(R, N * N) == 0, torch.ones((R, 1), dtype=torch.bool, device=st.device)], 1)
    ended = st[:, govars.DONE_CHNL].reshape(R, N * N).any(dim=1).bool()   # (any() of uint8 is uint8)
    return legal & ~ended[:, None]


def _uct_leaves(leaves):
    """leaves=None -> None (the one-leaf path); else the validated int L >= 1."""
    if leaves is None:
        return None
    if not _int_arg(leaves) or int(leaves) < 1:
        raise ValueError('leaves must be None or an integer >= 1 (got %r)' % (leaves,))
    return int(leaves)


def _uct_prior_kw(kw, shape, iterations, playouts):
    """_prior_kw for batch_uct and the calls that forward to it (its ValueErrors before a device is touched), leaves= and its
    bounds checked first: with it every bound counts iterations * leaves leaves.  shape: a function -> (R, N), asked only when
    prior= or last_actions= is given."""
    L = _uct_leaves(kw.get('leaves'))
    # batch_uct states this bound again where the capacity is known; here it stands in front of the first use of a device (uct and
    # uct_actions box the state before batch_uct runs).  Counts that are no integers are _uct_args' and _playout_args' to refuse
    if L is not None and _int_arg(iterations) and _int_arg(playouts):
        jobs = int(iterations) * L * int(playouts) * (1 if kw.get('rave_equiv') is None else 2)
        if jobs >= 2 ** 31:
            raise ValueError('leaves=%d needs iterations * leaves * playouts < 2^31, with rave_equiv twice that (got %d)' % (L, jobs))
    if kw.get('prior') is None and kw.get('last_actions') is None:
        return None, None
    return _prior_kw(kw, *shape(), int(iterations) * (L or 1), playouts)


def _run_uct(roots, R, N, I, K, c, max_plies, komi, seed, first_root, S, chunk_plies, dev, policy=0, rave=None, prior=None,
             leaves=None):
    """Device work of batch_uct on tracked roots -> (child int32 [R, I+1, A], links [R, I+1, 2], stats [R, I+1, 4],
    nodes [R], totals int64 [R, 2]); no launch for R = 0.  rave: None (the plain search, through the plain entry points) or
    (rave_equiv, fpu) - then a sixth result, node_amaf int32 [R, I+1, N^2, 2].  prior (with rave only): None - not one launch
    more - or (weights int32 [12], last_actions int32 [R] or None) on the device: gg_uct_prior_begin seeds the roots,
    gg_uct_prior_expand every new node once its board has been played.
    leaves: None - everything above, not one launch different - or L >= 1: I rounds of L slots per root through the _leaves
    entry points of include/gymgo_amd_uct_leaves.h.  The same loop on R L rows: the trees have I L + 1 nodes where they had
    I + 1, leaf / move / leaf_id and the playout buffers have R L rows, virt int32 [R, I L + 1] is added."""
    L = 1 if leaves is None else leaves
    rounds, rows, I = I, R * L, I * L          # from here on I is the capacity of a tree, as the entry points take it
    W, A, NN = tracked_words(N), N * N + 1, I + 1
    boards = torch.empty((R, NN, W), dtype=_I32, device=dev)
    child = torch.empty((R, NN, A), dtype=_I32, device=dev)
    links = torch.empty((R, NN, 2), dtype=_I32, device=dev)
    stats = torch.empty((R, NN, 4), dtype=_I32, device=dev)
    nodes = torch.empty(R, dtype=_I32, device=dev)
    totals = torch.zeros((R, 2), dtype=_I64, device=dev)
    node_amaf = torch.zeros((R, NN, N * N, 2), dtype=_I32, device=dev) if rave is not None else None
    res = (child, links, stats, nodes, totals) + ((node_amaf,) if rave is not None else ())
    if R == 0:
        return res
    leaf = torch.empty((rows, W), dtype=_I32, device=dev)
    move = torch.empty(rows, dtype=_I32, device=dev)
    leaf_id = torch.empty(rows, dtype=_I32, device=dev)
    with np.errstate(divide='ignore'):   # (L[0] = -inf is never read: a node with children has n >= K)
        log_table = torch.from_numpy(np.log(np.arange(NN, dtype=np.float64) * K)).to(dev)
    pbufs = _playout_buffers(rows, S, N, dev)
    counts, sums = pbufs[5], pbufs[6]
    stream = _lib.current_raw_stream(dev)
    _lib.call('gg_uct_begin', roots, R, N, I, K, boards, child, links, stats, nodes, stream)
    # the RAVE entry points take the plain ones' arguments with their own spliced in: rave_equiv and fpu, node_amaf, the AMAF counts;
    # the _leaves entry points take either's with L behind I and virt behind the tree's buffers (one kernel body serves both:
    # gg_uct.h's, with its VL switch on behind the _leaves names)
    abufs, sfx, kf, na, am = None, '', (), (), ()
    if rave is not None:
        abufs = _amaf_buffers(rows, S, N, chunk_plies, dev)
        sfx, kf, na, am = '_rave', (float(rave[0]), float(rave[1])), (node_amaf,), (abufs[3],)
    lf, lv, vt = '', (), ()
    if leaves is not None:
        lf, lv, vt = '_leaves', (L,), (torch.zeros((R, NN), dtype=_I32, device=dev),)
    select = ('gg_uct_select' + lf + sfx, R, N, I, *lv, K, c, *kf, log_table, boards, child, links, stats, *na, nodes, *vt, leaf, move,
              leaf_id, stream)
    backup = ('gg_uct_backup' + lf + sfx, R, N, I, *lv, K, counts, sums, *am, totals, boards, links, stats, *na, *vt, leaf, move,
              leaf_id, stream)
    if prior is not None:
        _lib.call('gg_uct_prior_begin', roots, prior[1], R, N, I, prior[0], node_amaf, stream)
    for i in range(rounds):
        _lib.call(*select)
        _lib.call('gg_batch_play_moves_tracked', leaf, move, None, rows, N, 1, stream)
        if prior is not None:
            _lib.call('gg_uct_prior_expand' + lf, R, N, I, *lv, prior[0], leaf, move, leaf_id, node_amaf, stream)
        _run_playouts(leaf, rows, N, K, max_plies, komi, _uct_seed(seed, i), first_root * L, False, S, chunk_plies, dev, pbufs, policy,
                      amaf=abufs)
        _lib.call(*backup)
    return res


def batch_uct(batch_states, iterations, playouts, c=math.sqrt(2), max_plies=None, komi=0.0, seed=20260927, first_root=0,
              slots=None, chunk_plies=32, tree=False, *, policy='uniform', rave_equiv=None, fpu=1.0, prior=None, last_actions=None,
              leaves=None):
    """UCT search of `iterations` iterations from every root of batch_states ([R, 6, N, N]), the leaves evaluated with
    `playouts` playouts each -> Uct (device tensors for a device tensor, NumPy arrays for NumPy input).

    Each root has its own tree with room for iterations + 1 nodes.  Iteration i, per root: select from the root - at a node
    whose game has ended, that node is the leaf; else the lowest legal action (batch_move_playouts' rule: the pass and every
    point whose plane-3 bit is clear) without a child is expanded into a new node, the leaf; else descend to the child of the
    largest U = (2 w + d) / (2 n) + c * sqrt(log(n_parent) / n) (w: the wins of the colour to move at the parent; float64,
    in this order, no fused multiply-add; ties to the lowest action).  The R leaves are evaluated by exactly
    batch_playouts(leaves, playouts, max_plies, komi, seed=s_i, first_root=first_root), s_i = rng_seed(.., seed,
    first_game=i)[0]'s value, and n += playouts, the wins and draws are added on the path from the leaf to the root.
    So a root that has not ended gets root_visits = iterations * playouts; an ended root evaluates itself every iteration.
    Defaults and validation are those of batch_playouts, plus iterations >= 1, c >= 0 and finite, iterations * playouts
    < 2^31; results do not depend on `slots` or `chunk_plies`, and shards by first_root concatenate to the whole.
    tree=True also returns the whole tree (UctTree).  The roots are not modified.

    Device memory of the tree: R * (iterations + 1) * (4 (5N + 1) + 4 (N^2 + 1) + 24) bytes (boards, child tables, links and
    stats: 1 856 bytes per node at 19x19, 124 MB for 1 024 roots x 64 iterations), plus the playout slots of batch_playouts.
    policy: as in batch_playouts; it governs the playouts of the leaves only - the tree keeps every legal action.

    rave_equiv: None - the search above, through the same entry points - or a positive number k, which turns RAVE on
    (gg_uct_select_rave / gg_uct_backup_rave; the playouts then run with amaf=True) -> UctRave.  Every node keeps, per point p,
    (n~, s~): the simulations through it in which its mover played p first - in the tree below it or in the playout - and
    twice the mover's wins plus the draws among them.  At a node, every legal action a - expanded or not - gets the value
    (1 - beta) q + beta q~ with q = (2 w + d) / (2 n) of its child, q~ = s~ / (2 n~) and beta = n~ / (n + n~ + n n~ / k); q or
    q~ alone when only one of the counts is positive, `fpu` when neither is; U adds c * sqrt(log(n_parent) / n) when n > 0
    (float64, in this order, no fused multiply-add).  The largest U wins, ties to the lowest action; a winner without a child
    is expanded.  So a node descends as soon as one action stands out, where the plain search first expands every legal
    action in board order.  The search needs 2 * iterations * playouts < 2^31 and chunk_plies <= 4096, and 8 N^2 more bytes
    per node.

    prior (with rave_equiv only): None - not one launch changes - or True (UCT_PRIOR, whose values are untuned) or a UctPrior:
    heuristic prior knowledge in the tree.  Every node starts with batch_move_priors(its board, prior, last) ADDED to its
    (n~, s~) pairs - the root before the first iteration, a new node when it is expanded -, `last` being the action that led to
    the node, and for the roots last_actions: None, or R integers in [-1, N*N], -1 and the pass N*N meaning no previous point.
    So a capture, an escape, a local answer to the previous move and a pattern point are tried before the rest of a new node's
    points, and a move into the mover's own eye after them; no memory is added and the select and the backup are the same
    kernels.  The pass has no pair - there is no slot for it -, its value stays q or fpu: a caller who seeds every point at 0.5
    will usually want fpu at or below that.  rave_visits and rave_score of the result, and node_amaf of its tree, then include
    the prior.  The search needs 2 * (iterations * playouts + the visits of the six pairs) < 2^31.

    leaves: None - everything above, not one launch different - or an integer L >= 1 (1 included): `iterations` ROUNDS that hand
    out up to L leaves per root each (include/gymgo_amd_uct_leaves.h holds the rule; plain, RAVE and RAVE with priors).  The
    slots of a root are chosen one after the other under VIRTUAL LOSS: a node counts v more visits of `playouts` lost playouts
    each for the v leaves of this round that went through it - in the denominator of a child's U and in the argument of the
    parent's logarithm, never in the wins.  A walk that reaches a node made earlier in the same round - it has no board yet -
    is a collision: that slot and the later slots of the root stay empty.  The R * L rows are evaluated together by exactly
    batch_playouts(rows, playouts, max_plies, komi, seed=s_t, first_root=first_root * L) for round t (empty rows too: they are
    evaluated and ignored) and backed up in slot order.  So leaves=1 gives the trees of leaves=None bit for bit, root_visits is
    playouts times the non-empty slots, and the results keep their fields with iterations * L + 1 nodes per tree (the tree
    fields are [R, iterations * L + 1]).  The bounds above hold with iterations * L for iterations.  Device memory: the tree
    with iterations * L + 1 nodes per root plus 4 bytes a node for the virtual visits, the playout slots for R * L roots, and
    under RAVE the playouts' AMAF buffer of R * L rows (24 N^2 bytes each)."""
    pol = _policy_kw({'policy': policy, 'rave_equiv': rave_equiv})
    pr, la = _uct_prior_kw({'prior': prior, 'last_actions': last_actions, 'rave_equiv': rave_equiv, 'leaves': leaves},
                           lambda: _states_shape(batch_states), iterations, playouts)
    L = None if leaves is None else int(leaves)     # (_uct_prior_kw has validated it)
    box = _Box(batch_states)
    st = box.t
    R, N, K, max_plies, chunk_plies = _playout_args(st, playouts, max_plies, chunk_plies, first_root)
    I, c = _uct_args(iterations, K, c)
    C = I * (L or 1)     # the leaves a root can get: what the bounds count
    if C * K >= 2 ** 31:
        raise ValueError('need iterations * leaves * playouts < 2^31 (got %d)' % (C * K))
    rave = None
    if rave_equiv is not None:
        rave = (float(rave_equiv), float(fpu))
        if not (math.isfinite(rave[0]) and rave[0] > 0 and math.isfinite(rave[1])) or 2 * C * K >= 2 ** 31 or chunk_plies > 4096:
            raise ValueError('RAVE needs rave_equiv > 0 and finite, fpu finite, 2 * iterations * playouts < 2^31 (with leaves: '
                             'times leaves) and chunk_plies <= 4096 (got %r, %r, %d, %d)' % (rave_equiv, fpu, 2 * C * K, chunk_plies))
    S = max(1, min(int(_default_slots(slots)), R * (L or 1) * K))
    child, links, stats, nodes, totals, *more = _run_uct(_track_roots(st), R, N, I, K, c, max_plies, komi, seed, first_root, S,
                                                         chunk_plies, st.device, policy=pol, rave=rave,
                                                         prior=None if pr is None or R == 0 else (
                                                             _prior_weights(pr, st.device),
                                                             None if la is None else torch.from_numpy(la).to(st.device)),
                                                         **({} if L is None else {'leaves': L}))
    rc = child[:, 0, :]
    kid = torch.gather(stats, 1, rc.clamp(min=0).long()[..., None].expand(R, N * N + 1, 4))
    kid = torch.where((rc >= 0)[..., None], kid, torch.zeros_like(kid))
    whole = UctTree(links[..., 0], links[..., 1], stats[..., 0], stats[..., 1], stats[..., 2], stats[..., 3]) if tree else None
    res = Uct(_legal_roots(st), kid[..., 0], kid[..., 1], kid[..., 2], kid[..., 3], stats[:, 0, 0], totals[:, 0], totals[:, 1], nodes,
              whole)
    if rave is not None:
        node_amaf = more[0]
        res = UctRave(*res[:-1], UctRaveTree(*whole, node_amaf) if tree else None, node_amaf[:, 0, :, 0], node_amaf[:, 0, :, 1])
    return _back(box, res)


def uct(state, iterations, playouts, **kw):
    """batch_uct of one state [6, N, N] -> Uct of [N*N + 1] vectors and scalars (tree fields [iterations + 1])."""
    def shape():
        if len(np.shape(state)) != 3:
            raise ValueError('state must be [6, N, N] (got %s)' % (tuple(np.shape(state)),))
        return 1, np.shape(state)[-1]
    _uct_prior_kw(kw, shape, iterations, playouts)
    return _single(batch_uct, state, iterations, playouts, **kw)


def uct_actions(batch_states, iterations, playouts, **kw):
    """The UCT move of every root -> int64 [R]: the legal root child with the most visits after batch_uct(batch_states,
    iterations, playouts, **kw); ties go to the lowest action, a root without a legal move gives -1."""
    _policy_kw(kw)
    _uct_prior_kw(kw, lambda: _states_shape(batch_states), iterations, playouts)
    box = _Box(batch_states)
    res = batch_uct(box.t, iterations, playouts, **kw)
    return _best_legal(box, res.legal, res.visits.to(_I64))


# ---------------------------------------------------------------- PUCT tree search with priors and an outside evaluator
# R independent AlphaZero-style searches (gg_puct_begin / gg_puct_select / gg_puct_backup, include/gymgo_amd.h): the trees
# live on the device, each iteration selects one leaf per root by the PUCT score, hands the R leaves out as byte planes with
# their legality mask, and backs the caller's priors and values up.  The host only queues launches: nothing is read back.

Puct = collections.namedtuple('Puct', 'legal visits value_sum priors root_visits root_value_sum nodes tree')
Puct.__doc__ = """Results of batch_puct per root: legal (bool [R, A], A = N*N + 1), visits (int32 [R, A]) / value_sum (float64
[R, A]: the n / w of the root's children, w from black's point of view; 0 where there is none), priors (float32 [R, A]: the
root's, as stored - zero on illegal actions), root_visits (int32 [R]), root_value_sum (float64 [R]), nodes (int32 [R]: tree
nodes in use) and tree (PuctTree or None)."""
PuctTree = collections.namedtuple('PuctTree', 'parent action visits value_sum')
PuctTree.__doc__ = """The whole tree of every root, each field [R, iterations + 1] ([R, iterations * leaves + 1] with `leaves`;
[R, capacity] with `capacity`) indexed by node (node 0 = the root): parent / action / visits int32 (-1 / -1 / 0 at unused nodes; -1 / -1 at the root),
value_sum float64 (w, black's point of view)."""


def _puct_args(iterations, c, komi):
    I, c, komi = int(iterations), float(c), float(komi)
    if I < 1 or I >= 2 ** 31 - 1 or not math.isfinite(c) or c < 0 or not math.isfinite(komi):
        raise ValueError('need 1 <= iterations < 2^31 - 1, c >= 0 and finite, komi finite (got %d, %r, %r)' % (I, c, komi))
    return I, c, komi


def _puct_leaves(iterations, leaves):
    """leaves=None -> None (the one-leaf path); else the validated int L >= 1 with iterations * L < 2^31 - 1."""
    if leaves is None:
        return None
    if isinstance(leaves, bool) or not isinstance(leaves, (int, np.integer)):
        raise ValueError('leaves must be None or an integer >= 1 (got %r)' % (leaves,))
    L = int(leaves)
    if L < 1 or int(iterations) * L >= 2 ** 31 - 1:
        raise ValueError('need leaves >= 1 and iterations * leaves < 2^31 - 1 (got %d, %d)' % (L, int(iterations) * L))
    return L


def _puct_capacity(iterations, leaves, capacity):
    """-> nodes per root: capacity=None gives iterations + 1 (iterations * leaves + 1); an integer must be at least that and
    below 2^31."""
    least = int(iterations) * (leaves or 1) + 1
    if capacity is None:
        return least
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not least <= int(capacity) < 2 ** 31:
        raise ValueError('capacity must be None or an integer in [%d, 2^31) (got %r)' % (least, capacity))
    return int(capacity)


_ON_DEVICE = collections.namedtuple('_OnDevice', 'numpy')(False)   # a _Box stand-in: results stay device tensors


# ---------------------------------------------------------------- the Gumbel root rule (include/gymgo_amd_gumbel.h)
Gumbel = collections.namedtuple('Gumbel', 'considered simulations c_visit c_scale', defaults=(16, None, 50.0, 0.5))
Gumbel.__doc__ = """The Gumbel root rule of PuctSearch(gumbel=): considered (m, the actions drawn without replacement by the
Gumbel-top-k trick), simulations (n, the budget sequential halving spreads over them; None = max(1, (iterations - 1) * leaves),
what a fresh root gets, whose round 0 evaluates the root alone), c_visit and c_scale (sigma(q) = (c_visit + max visits) *
c_scale * q; the paper's c_scale = 1.0 is for q in [0, 1], values here are in [-1, 1], and a constant shift changes neither an
argmax nor a softmax)."""


def _int_arg(x):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def gumbel_sequence(considered, simulations):
    """The schedule of sequential halving -> int32 [simulations] (NumPy; gg_gumbel_sequence, host only): entry t is the number
    of this move's simulations the action that gets simulation t must have had.  gumbel_sequence(4, 8) = 0,0,0,0,1,1,2,2."""
    if not _int_arg(considered) or not _int_arg(simulations) or considered < 1 or simulations < 1 or max(considered, simulations) >= 2 ** 31:
        raise ValueError('need integers considered >= 1 and simulations >= 1 below 2^31 (got %r, %r)' % (considered, simulations))
    seq = np.empty(int(simulations), np.int32)
    _lib.call('gg_gumbel_sequence', int(considered), int(simulations), seq.ctypes.data)
    return seq


def _gumbel_arg(gumbel, iterations, leaves):
    """gumbel=None -> None; an int m or a Gumbel -> the validated Gumbel with its simulations filled in."""
    if gumbel is None:
        return None
    if _int_arg(gumbel):
        gumbel = Gumbel(int(gumbel))
    if not isinstance(gumbel, Gumbel):
        raise ValueError('gumbel must be None, an integer >= 1 (the actions considered) or a Gumbel (got %r)' % (gumbel,))
    m, n, cv, cs = gumbel
    if n is None:
        n = max(1, (int(iterations) - 1) * leaves)
    if not _int_arg(m) or not _int_arg(n) or m < 1 or n < 1 or max(m, n) >= 2 ** 31:
        raise ValueError('need integers considered >= 1 and simulations >= 1 below 2^31 (got %r, %r)' % (m, n))
    try:
        cv, cs = float(cv), float(cs)
    except (TypeError, ValueError):
        raise ValueError('c_visit and c_scale must be numbers (got %r, %r)' % (gumbel.c_visit, gumbel.c_scale)) from None
    if not (math.isfinite(cv) and cv >= 0 and math.isfinite(cs) and cs >= 0):
        raise ValueError('need c_visit >= 0 and c_scale >= 0, both finite (got %r, %r)' % (cv, cs))
    return Gumbel(int(m), int(n), cv, cs)


def gumbel_noise(generator=None):
    """The Gumbel(0, 1) draws of a Gumbel search -> a callable noise(move, legal) -> float32 [R, A] on legal's device:
    -log(-log(u)) of torch's uniform draws u (`generator`: a torch.Generator of that device, None = torch's default), one per
    action, legal or not (the search never reads the entries of illegal actions).  NOT bit-defined, like dirichlet_noise: the
    draws and the logarithms are torch's; everything the library does with the noise is exact."""
    def noise(move, legal):
        u = torch.rand(legal.shape, dtype=torch.float32, device=legal.device, generator=generator)
        return -torch.log(-torch.log(u.clamp(min=torch.finfo(torch.float32).tiny)))

    return noise


# THE table of the optional plane sets a leaf of the search (PuctSearch) or a sample of a record (selfplay_batch) can carry, in
# hand-out order: the option's keyword, the entry point on tracked boards, the planes per board, the public call on byte planes and
# the words of the error message.  The history planes (past=: always last, gg_puct_past reads the tree) and symmetry= are no rows:
# they are written out where they differ.
_LeafSet = collections.namedtuple('_LeafSet', 'key entry planes batch words')
_LEAF_SETS = (_LeafSet('life', 'gg_batch_life_tracked', LIFE_PLANES, batch_life, 'life'),
              _LeafSet('ladder', 'gg_batch_ladder_tracked', LADDER_PLANES, batch_ladder, 'ladder'),
              _LeafSet('outcome', 'gg_batch_move_planes_tracked', MOVE_PLANES, batch_move_planes, 'move-outcome'),
              _LeafSet('area', 'gg_batch_area_tracked', AREA_PLANES, batch_area_planes, 'area'))
_SEARCH_OPTIONS = ('leaves', 'capacity', 'features', 'symmetry', 'first_root') + tuple(s.key for s in _LEAF_SETS) + ('past', 'gumbel')


def _search_options(given):
    """The options of PuctSearch among the arguments of a public function (given: its locals() on entry, or its **kw) -> one dict,
    handed on as it is."""
    return {k: given[k] for k in _SEARCH_OPTIONS if k in given}


def _puct_planes_guard(opts):
    """ValueError for an option that hands out planes - symmetry=, a set of _LEAF_SETS, past= - without features= (opts: a dict
    of the options given) - before a device is touched."""
    if opts.get('features') is not None:
        return
    if opts.get('symmetry') is not None:
        raise ValueError('symmetry turns the planes and legal that features= hands out: give features= too')
    for s in _LEAF_SETS:
        if opts.get(s.key):
            raise ValueError('%s=True hands out the %s planes in the dtype of features=: give features= too' % (s.key, s.words))
    if opts.get('past') is not None:
        raise ValueError('past= hands out the history planes in the dtype of features=: give features= too')


class PuctSearch:
    """The step-wise form of batch_puct, for callers who batch their network calls their own way:

        search = PuctSearch(batch_states, iterations, c=1.25, komi=0.0)
        for _ in range(iterations):
            states, legal = search.select()          # uint8 [R, 6, N, N], bool [R, A]: device tensors owned by the search,
            priors, values = network(states, legal)  # valid until the next select()
            search.backup(priors, values)            # float32 [R, A], float32 [R]
        result = search.result()                     # Puct (NumPy arrays if batch_states was a NumPy array)

    select() and backup() alternate, at most `iterations` times; result() may be called whenever no leaf is outstanding.
    Anything else raises ValueError.  Every call queues its launches on torch's current stream of the states' device and
    returns without synchronising.  Semantics, sizes and device memory: batch_puct.

    leaves=L (an integer >= 1; None = the path above, untouched): every round hands out up to L leaves per root, chosen
    one after the other under virtual loss (batch_puct).  select() then returns states uint8 [R * L, 6, N, N] and legal
    bool [R * L, A] in row order r * L + j, backup() takes priors [R * L, A] and values [R * L]; rows of empty slots are
    evaluated like any other and ignored.  `search.live` (bool [R, L], a device tensor valid until the next select()) says
    which slots hold a leaf, for evaluators that want to skip the rest ([R, 1] and all true with leaves=None).  The tree
    has iterations * L + 1 nodes per root.  Either way a select() queues the select launch (gg_puct_select, or
    gg_puct_select_leaves with L), the one-move step on the leaf boards, their untrack and gg_puct_legal, which writes
    `legal` and `live` from the tracked leaves; only the entry points of select and backup differ.

    capacity (None = the sizes above, every allocation and launch as without it): the nodes per root, an integer >= that
    default and < 2^31; `iterations` stays the bound on rounds.  Room beyond the default is what advance() needs to go on
    growing a kept tree.

    advance(actions) plays one action per root between two rounds and keeps the subtree under it (gg_puct_advance); then
    `iterations` more rounds may follow.  A tree that is full falls under the no-room rule of batch_puct: the search goes
    on refining values and expands nothing.  No finite capacity excludes that over many moves; result().nodes shows how
    full the trees are.  A kept root is already evaluated and is not handed out again, so root noise that the evaluator
    adds would reach only fresh roots: add_root_noise() mixes noise into the stored priors of kept and fresh roots alike.

    add_root_noise(noise, eps, todo) and root_policy(sample, rng) are what a self-play loop needs on top (puct_selfplay is
    that loop): exploration noise in the root's priors, the move by the most visits or drawn in proportion to them, and
    the policy target and root value, all on the device.

    features (None = everything above, launch for launch; or a dtype of batch_features): select() returns (planes, legal)
    with planes [R, 16, N, N] ([R * L, ..] with leaves=L) of that dtype - batch_features of the leaves, made from the tracked
    leaf boards by gg_batch_features_tracked - instead of (states, legal).  That launch REPLACES the untrack of the leaf
    boards, with and without leaves=L: nothing is untracked.  Rows of empty slots hold the planes of whatever board their
    row holds.  Device memory: 16 N^2 elements per row handed out.

    symmetry (None = everything above, launch for launch; or an integer base seed; needs features=, ValueError otherwise):
    every evaluation sees its leaf in a random one of the eight orientations of batch_symmetry - AlphaGo Zero's random
    rotation or reflection per leaf.  The search keeps one generator per row it hands out, rng_seed(R * rows, symmetry,
    first_root * rows) with rows = L (1 without leaves): shards by root with first_root = the shard's first root
    concatenate to the whole.  Every select() draws one orientation per row (batch_draw_orient; `search.orient`, int32
    [R * rows], a device tensor valid until the next select()) and hands out planes AND legal in that view: the planes by
    the oriented feature launch, which replaces the plain one, legal through batch_symmetry_policy; backup() turns the
    priors back (inverse=True) before the backup launch it queues anyway.  The tree, the stored priors, root_policy,
    add_root_noise and advance stay in the board's own frame: the tree is bit for bit the tree of the same search
    without symmetry and with the evaluator E'(planes, legal) = inverse_o(E(view_o(planes), view_o(legal))), o the
    orientations drawn for that call (the values are not turned).  Two launches more per select(), one per backup().

    life (False = everything above, launch for launch; True needs features=, ValueError otherwise): select() returns
    (planes, legal, life) with life [R, 4, N, N] ([R * L, ..]) of the feature dtype - batch_life of the leaves, from the
    tracked leaf boards (gg_batch_life_tracked) - in the orientation of `search.orient` with symmetry=.  One launch more
    per select(); backup, advance, root_policy and the tree do not change.  Rows of empty slots hold the planes of whatever
    board their row holds.

    ladder (False = everything above, launch for launch; True needs features=, ValueError otherwise): select() returns the
    ladder planes [R, 4, N, N] ([R * L, ..]) of the feature dtype as its last element, after the life planes if both are on -
    batch_ladder of the leaves, from the tracked leaf boards (gg_batch_ladder_tracked), in the orientation of
    `search.orient` with symmetry= (the planes of the turned leaf).  One launch more per select(); nothing else changes.

    outcome (False = everything above, launch for launch; True needs features=, ValueError otherwise): select() returns the
    move-outcome planes [R, 12, N, N] ([R * L, ..]) of the feature dtype as its last element, after the life and ladder
    planes when those are on - batch_move_planes of the leaves, from the tracked leaf boards
    (gg_batch_move_planes_tracked), in the orientation of `search.orient` with symmetry=.  One launch more per select();
    nothing else changes.

    area (False = everything above, launch for launch; True needs features=, ValueError otherwise): select() returns the
    area ownership planes [R, 3, N, N] ([R * L, ..]) of the feature dtype as its LAST element, after the life, ladder and
    move-outcome planes when those are on - batch_area_planes of the leaves from the mover's view, from the tracked leaf boards
    (gg_batch_area_tracked), in the orientation of `search.orient` with symmetry=.  One launch more per select(); nothing
    else changes.

    past (None = everything above, launch for launch; or a StoneHistory of the R games holding the positions BEFORE the roots;
    needs features=, ValueError otherwise): select() returns the history planes [R, past.planes, N, N] ([R * L, ..]) of the
    feature dtype as its LAST element, after the life, ladder, move-outcome and area planes when those are on -
    batch_past_planes of the leaves with their true past (gg_puct_past): one ply back is the leaf's parent node, further back
    its ancestors' boards in the tree, beyond node 0 the history's ring - in the orientation of `search.orient` with
    symmetry=.  One launch more per select().  advance() pushes node 0's board into the history for every root whose action
    is not -1, before the tree is renumbered, so the history follows the game; the search keeps the object and reads its
    tensors at launch time.

    superko (None = everything above, every allocation and launch as without it; or a PositionHistory of the R games with
    the current roots included; anything else raises _history_arg's ValueError): positional superko AT EVERY NODE below the
    root (gg_puct_superko).  At node y a board move is illegal if it recreates - by its 64-bit hash - a valid entry of the
    history or the position of any node on y's parent chain up to node 0.  The tree is a tree, so a node's chain never
    changes and the rule is applied once, when the node is made: select() queues gg_puct_superko directly behind
    gg_batch_play_moves_tracked and in front of every hand-out launch, it ORs the forbidden points into the invalid rows of
    the new leaves, and the planes, `legal`, the stored priors and every later select follow from the board.  The search
    keeps the history object - its tensors are read at launch time, nothing synchronises - and `node_hash`, int64
    [R, capacity]: the hash of every evaluated node, refilled by one gg_batch_hash_tracked over the whole boards buffer
    (allocated zeroed: an unused node is an empty board, hash 0, above nodes[r] and never read) after gg_puct_begin and
    after every advance().  The caller still pushes the new roots' hashes after advance() and still calls forbid_repeats()
    for node 0 - with no argument it uses the search's history.  THE INVARIANT that keeps the marks right across advance():
    a kept node was marked against (old history + its old chain); the old root and the node under the action played leave
    the chain and enter the history, so that set IS (new history + its new chain) - provided the history has dropped no
    entry: give the PositionHistory the capacity of the whole game.  One launch more per select(), one per advance().

    gumbel (None = everything above, every allocation and launch as without it; or an int m, or a Gumbel): the Gumbel root
    rule by sequential halving (include/gymgo_amd_gumbel.h, which holds the normative text).  At node 0 the walk takes the
    action the schedule gumbel_sequence(m, n) asks for - among the legal actions with that many of this move's simulations,
    the one with the largest base + sigma(q), base = g + log(prior) - instead of the largest U'; below the root nothing
    changes.  leaves=None counts as leaves=1 (the same tree as the one-leaf path).  The schedule is uploaded once;
    gg_gumbel_begin (seen = the visits the root's children have now, done = 0) runs at construction and at the end of every
    advance().  g starts as zeros - noise-free sequential halving, for match play - and set_gumbel(g) replaces it (float32
    [R, A]; gumbel_noise() makes the draws), only before the first select() after construction or after an advance
    (ValueError otherwise).  select() refreshes `search.base` = g + log(prior[:, 0, :]) by torch, on the device, before the
    select launches of the first two rounds after a begin or an advance - after round 0 every live root is evaluated - and
    later rounds reuse the tensor; then it queues gg_gumbel_select_leaves in place of gg_puct_select_leaves.  gumbel_root() is
    the read-out: the move, the improved policy and the root value.  add_root_noise() raises ValueError on such a search: the
    exploration is g.  Rounds beyond the schedule (a kept root has iterations * leaves slots, a fresh one (iterations - 1) *
    leaves) go to the actions with the most simulations of this move."""

    def __init__(self, batch_states, iterations, c=1.25, komi=0.0, leaves=None, capacity=None, features=None, symmetry=None,
                 first_root=0, life=False, ladder=False, outcome=False, superko=None, area=False, past=None, gumbel=None):
        opts = _search_options(locals())
        self._feat = None if features is None else (features, _feature_dtype(features))
        _gumbel_arg(gumbel, 2, 1)   # (what it is, before a device is touched; its simulations further down)
        if superko is not None:   # (before a device is touched)
            shape = np.shape(batch_states.t if isinstance(batch_states, _Box) else batch_states)
            _history_arg(superko, shape[0] if shape else -1)
        _puct_planes_guard(opts)
        if past is not None:      # (before a device is touched)
            shape = np.shape(batch_states.t if isinstance(batch_states, _Box) else batch_states)
            _past_arg(past, shape[0] if shape else -1, shape[-1] if shape else -1, 'past')
        self._past = past
        self._sym = None if symmetry is None else int(symmetry)
        self._first_root = int(first_root)
        self.orient = None
        self._box = batch_states if isinstance(batch_states, _Box) else _Box(batch_states)   # (a _Box: puct_play's own states)
        st = self._box.t
        if st.dim() != 4 or st.shape[1] != govars.NUM_CHNLS or st.shape[2] != st.shape[3]:
            raise ValueError('batch_states must be [R, 6, N, N] (got %s)' % (tuple(st.shape),))
        self._I, self._c, self._komi = _puct_args(iterations, c, komi)
        self._I0 = self._I      # the rounds as constructed: advance()'s default, whatever an earlier advance was given
        self._L = _puct_leaves(self._I, 1 if gumbel is not None and leaves is None else leaves)
        self._gumbel = _gumbel_arg(gumbel, self._I, self._L or 1)
        NN = _puct_capacity(self._I, self._L, capacity)
        R, N, dev = st.shape[0], st.shape[2], st.device
        self._R, self._N, self._dev = R, N, dev
        self._history = superko
        if superko is not None:
            self._hist = _history_arg(superko, R)
            if self._hist[0].device != dev or self._hist[1].device != dev:
                raise ValueError('history must be a PositionHistory of %d boards on the device of batch_states (%s)' % (R, dev))
        self._C = NN - 1        # what the kernels get as I / C: only a capacity there
        self._scratch = None    # advance()'s buffers, allocated on its first call
        W, A, B = tracked_words(N), N * N + 1, R * (self._L or 1)   # B: the rows handed out per select()
        self._legal_roots = _legal_roots(st)
        self._boards = (torch.empty if superko is None else torch.zeros)((R, NN, W), dtype=_I32, device=dev)
        self.node_hash = None if superko is None else torch.zeros((R, NN), dtype=_I64, device=dev)
        self._child = torch.empty((R, NN, A), dtype=_I32, device=dev)
        self._prior = torch.empty((R, NN, A), dtype=torch.float32, device=dev)
        self._links = torch.empty((R, NN, 2), dtype=_I32, device=dev)
        self._stats = torch.empty((R, NN, 4), dtype=_I32, device=dev)   # gg_puct_stat: w float64 (words 0 - 1), n (word 2), v
        self._nodes = torch.empty(R, dtype=_I32, device=dev)
        self._leaf = torch.empty((B, W), dtype=_I32, device=dev)
        self._move = torch.empty(B, dtype=_I32, device=dev)
        self._leaf_id = torch.empty(B, dtype=_I32, device=dev)
        if self._feat is None:
            self._states = torch.empty((B, govars.NUM_CHNLS, N, N), dtype=_U8, device=dev)
        else:   # (the leaves go out as planes: no byte-plane buffer)
            self._states = torch.empty((B, FEATURE_PLANES, N, N), dtype=self._feat[0], device=dev)
        self._legal = torch.empty((B, A), dtype=torch.bool, device=dev)
        # the plane sets that are on, in hand-out order: (the set's row, its planes)
        self._sets = [(s, torch.empty((B, s.planes, N, N), dtype=self._feat[0], device=dev)) for s in _LEAF_SETS if opts[s.key]]
        self._set_launches = []
        if past is not None:
            if past.rows.device != dev or past.count.device != dev:
                raise ValueError('past must be a StoneHistory of %d boards on the device of batch_states (%s)' % (R, dev))
            self._past_planes = torch.empty((B, past.planes, N, N), dtype=self._feat[0], device=dev)
        self.live = torch.full((R, self._L or 1), self._L is None, dtype=torch.bool, device=dev)   # (one leaf: always live)
        self._done, self._pending = 0, False
        self._init_symmetry(B)
        if self._gumbel is not None:   # (g is zeros: noise-free sequential halving; base is written by select())
            self._g = torch.zeros((R, A), dtype=torch.float32, device=dev)
            self.base = torch.zeros((R, A), dtype=torch.float32, device=dev)
            self._seen = torch.zeros((R, A), dtype=_I32, device=dev)
            self._sims = torch.zeros(R, dtype=_I32, device=dev)
            self._g_open, self._since = True, 0   # set_gumbel() is allowed; rounds selected since the last begin
        if not R:   # no device work at all: select / backup only keep the call order
            return
        # the search's own buffers are checked once, through the table; every call below gets their pointers
        self._tree = _lib.ptrs('gg_puct_begin', boards=self._boards, child=self._child, prior=self._prior, links=self._links,
                               stats=self._stats, nodes=self._nodes)
        self._out = _lib.ptrs('gg_puct_select', leaf=self._leaf, move=self._move, leaf_id=self._leaf_id)
        self._hand = (_lib.ptrs('gg_batch_untrack_states', states=self._states) if self._feat is None else
                      _lib.ptrs('gg_batch_features_tracked', out=self._states)) + _lib.ptrs('gg_puct_legal', legal=self._legal, live=self.live)
        self._rows = [p for p in _lib.ABI['gg_puct_backup'] if p.name in ('priors', 'values')]
        if self._feat is not None:   # the hand-out launches are prepared once: the feature planes first, then the sets that are on
            self._op = None if self._sym is None else _lib.ptrs('gg_batch_draw_orient', orient=self.orient)[0]
            self._feature_launch = self._prepared('gg_batch_features_tracked', self._states)
            self._set_launches = [self._prepared(s.entry, planes) for s, planes in self._sets]
        _lib.call('gg_puct_begin', _track_roots(st), R, N, self._C, *self._tree, _lib.current_raw_stream(dev))
        if superko is not None:
            self._ko = _lib.ptrs('gg_puct_superko', links=self._links, node_hash=self.node_hash)
            self._fill_node_hash()
        if past is not None:   # (the history's tensors are written in place: their addresses hold)
            self._past_ptrs = _lib.ptrs('gg_puct_past', boards=self._boards, links=self._links, rows=past.rows, count=past.count,
                                        out=self._past_planes)
        if self._gumbel is not None:
            self._seq = torch.from_numpy(gumbel_sequence(self._gumbel.considered, self._gumbel.simulations)).to(dev)
            self._root = _lib.ptrs('gg_gumbel_select_leaves', base=self.base, seen=self._seen, done=self._sims, seq=self._seq)
            self._gumbel_begin()

    def _prepared(self, name, planes):
        """A plane launch on the leaf boards into `planes`, prepared: (entry point, *its arguments but the stream) with every
        pointer an address - the leaves, search.orient with symmetry= and the planes are the search's own buffers and never move."""
        out, = _lib.ptrs(name, out=planes)
        return _plane_args(name, self._out[0], self._op, dict(out=out, out_dtype=self._feat[1], B=planes.shape[0], N=self._N))[:-1]

    def _gumbel_begin(self):
        """seen = the visits of node 0's children as they stand, done = 0 (R > 0): the search of a move begins; one launch."""
        _, child, _, _, stats, nodes = self._tree
        _lib.call('gg_gumbel_begin', self._R, self._N, self._C, child, stats, nodes, self._seen, self._sims,
                  _lib.current_raw_stream(self._dev))

    def _refresh_base(self):
        """base = g + log(the root's stored priors), float32, by torch on the device (R > 0)."""
        with torch.cuda.device(self._dev):
            torch.add(self._g, torch.log(self._prior[:, 0, :]), out=self.base)

    def set_gumbel(self, g):
        """Replace g, the Gumbel draws of this move: floating point [R, A], a tensor or NumPy array (gumbel_noise() makes them;
        the entries of illegal actions are never read).  Only before the first select() after construction or after an
        advance(): ValueError otherwise, and on a search without gumbel=."""
        if self._gumbel is None:
            raise ValueError('PuctSearch.set_gumbel(): the search was made without gumbel=')
        if not self._g_open:
            raise ValueError('PuctSearch.set_gumbel(): only before the first select() after construction or after advance()')
        R, A = self._R, self._N * self._N + 1
        if not isinstance(g, torch.Tensor):
            g = torch.from_numpy(np.ascontiguousarray(g))
        if tuple(g.shape) != (R, A) or not g.dtype.is_floating_point:
            raise ValueError('g must be floating point [%d, %d] (got %s %s)' % (R, A, g.dtype, tuple(g.shape)))
        if R:
            with torch.cuda.device(self._dev):
                self._g.copy_(g.to(device=self._dev, dtype=torch.float32))

    def gumbel_root(self, pi=True):
        """The read-out of a Gumbel search (gg_gumbel_root) -> (actions int32 [R], pi float32 [R, A] or None with pi=False,
        value float32 [R]); device tensors, or NumPy arrays for NumPy input.  actions: among the legal actions with the most
        simulations of this move, the one with the largest base + sigma(q), ties to the lowest action; -1 for a root whose game
        has ended.  pi: the improved policy, softmax over the legal actions of log(prior[a]) + (c_visit + max visits) * c_scale
        * q[a], q the child's mean value for the player to move or, without visits, the root's - by torch on the device in
        float64, cast to float32, +0 on illegal actions, a zero row for an ended root (where the largest term is infinite the
        mass is shared by the actions that have it).  value: the root's mean value for the player to move.  May be called
        whenever no leaf is outstanding; queues one launch and a handful of torch ops, reads nothing back."""
        if self._gumbel is None:
            raise ValueError('PuctSearch.gumbel_root(): the search was made without gumbel=')
        if self._pending:
            raise ValueError('PuctSearch.gumbel_root(): the leaves of the last select() have not been backed up')
        return tuple(_back(self._box, t) for t in self._gumbel_root(pi))

    def _gumbel_root(self, pi=True):
        """gumbel_root() as new device tensors."""
        R, A, dev = self._R, self._N * self._N + 1, self._dev
        acts = torch.empty(R, dtype=_I32, device=dev)
        v = torch.empty(R, dtype=torch.float32, device=dev)
        q = torch.empty((R, A), dtype=torch.float32, device=dev) if pi else None
        n = torch.empty((R, A), dtype=_I32, device=dev) if pi else None
        if R:
            if self._since < 2:   # (fewer than two selects since the begin: base is not yet the one of the evaluated roots)
                self._refresh_base()
            boards, child, _, _, stats, nodes = self._tree
            _lib.call('gg_gumbel_root', R, self._N, self._C, boards, child, stats, nodes, self.base, self._seen, self._gumbel.c_visit,
                      self._gumbel.c_scale, acts, q, n, v, _lib.current_raw_stream(dev))
        if not pi:
            return acts, None, v
        if not R:
            return acts, torch.zeros((R, A), dtype=torch.float32, device=dev), v
        with torch.cuda.device(dev):
            legal, f64 = self._legal_roots, torch.float64
            scale = (self._gumbel.c_visit + n.max(dim=1, keepdim=True).values.to(f64)) * self._gumbel.c_scale
            x = torch.log(self._prior[:, 0, :].to(f64)) + scale * q.to(f64)
            x = torch.where(legal & (x == x), x, torch.full_like(x, -math.inf))
            top = x.max(dim=1, keepdim=True).values
            e = torch.where(legal, torch.where(x == top, torch.ones_like(x), torch.exp(x - top)), torch.zeros_like(x))
            p = torch.where(legal, e / e.sum(dim=1, keepdim=True), torch.zeros_like(x)).to(torch.float32)
        return acts, p, v

    def _fill_node_hash(self):
        """node_hash = the hash of every board of the boards buffer (R > 0): one launch."""
        R, NN = self._R, self._C + 1
        _lib.call('gg_batch_hash_tracked', self._boards.view(R * NN, -1), self.node_hash, R * NN, self._N,
                  _lib.current_raw_stream(self._dev))

    def _init_symmetry(self, B):
        """symmetry: the generators of the B rows handed out, their orientations, legal in the view, the priors turned back."""
        if self._sym is None:
            return
        A, dev = self._N * self._N + 1, self._dev
        self.orient = torch.zeros(B, dtype=_I32, device=dev)
        self._legal_view = torch.empty((B, A), dtype=torch.bool, device=dev)
        self._priors_back = torch.empty((B, A), dtype=torch.float32, device=dev)
        self._sym_rng = torch.empty(B, dtype=_I64, device=dev)
        if B:
            rows = B // self._R
            _lib.call('gg_rng_seed', self._sym_rng, self._sym & (2 ** 64 - 1), self._first_root * rows, B, _lib.current_raw_stream(dev))

    def _draw_orient(self, B, stream):
        """The orientations of this select()'s B rows -> the pointer of search.orient."""
        _lib.call('gg_batch_draw_orient', self._sym_rng, self._op, B, stream)
        return self._op

    def _turn_legal(self, op, B, stream):
        _lib.call('gg_batch_symmetry_policy', self._legal, op, self._legal_view, 1, 0, B, self._N, stream)

    def _turn_priors_back(self, priors, B):
        """priors [B, A] over the views -> over the boards (R > 0)."""
        _lib.call('gg_batch_symmetry_policy', priors, self.orient, self._priors_back, 4, 1, B, self._N,
                  _lib.current_raw_stream(self._dev))
        return self._priors_back

    @property
    def iterations_done(self):
        return self._done

    def select(self):
        """Step 1 and 2 of the next iteration -> (states uint8 [R, 6, N, N], legal bool [R, A]) of the R leaves ([R * L, ..]
        with leaves=L); with features=dtype (planes [R, 16, N, N] of that dtype, legal); with life=True (planes, legal, life
        [R, 4, N, N] of that dtype); with ladder=True the ladder planes [R, 4, N, N] of that dtype after those; with
        outcome=True the move-outcome planes [R, 12, N, N] of that dtype after those; with area=True the area planes
        [R, 3, N, N] of that dtype after those; with past= the history planes [R, past.planes, N, N] of that dtype as the last
        element."""
        if self._pending:
            raise ValueError('PuctSearch.select(): the leaves of the last select() have not been backed up')
        if self._done >= self._I:
            raise ValueError('PuctSearch.select(): all %d iterations are done' % self._I)
        R, N, B = self._R, self._N, self._R * (self._L or 1)
        if R:
            # every pointer below is a prepared one and host time per round is this path's cost: fn(...) plus check, in line
            lib, check, stream = _lib.lib(), _lib.check, _lib.current_raw_stream(self._dev)
            lp, mp, ip = self._out
            sp, gp, vp = self._hand
            if self._gumbel is None:
                name, slots = ('gg_puct_select', ()) if self._L is None else ('gg_puct_select_leaves', (self._L,))
                check(getattr(lib, name)(R, N, self._C, *slots, self._c, *self._tree, lp, mp, ip, stream), name)
            else:
                if self._since < 2:   # (round 0 evaluates the fresh roots: from round 1 on every live root has its priors)
                    self._refresh_base()
                check(lib.gg_gumbel_select_leaves(R, N, self._C, self._L, self._c, *self._tree, *self._root, self._seq.numel(),
                                                  self._gumbel.c_visit, self._gumbel.c_scale, lp, mp, ip, stream),
                      'gg_gumbel_select_leaves')
            check(lib.gg_batch_play_moves_tracked(lp, mp, None, B, N, 1, stream), 'gg_batch_play_moves_tracked')
            if self._history is not None:   # (the history's tensors as they are now: PositionHistory.push works in place)
                hp, cp = _lib.ptrs('gg_puct_superko', history=self._hist[0], count=self._hist[1])
                check(lib.gg_puct_superko(R, N, self._C, self._L or 1, *self._ko, hp, cp, self._hist[2], lp, mp, ip, stream),
                      'gg_puct_superko')
            if self._feat is None:
                check(lib.gg_batch_untrack_states(lp, sp, B, N, stream), 'gg_batch_untrack_states')
            else:   # (the feature planes, into sp)
                op = None if self._sym is None else self._draw_orient(B, stream)
                _lib.launch(*self._feature_launch, stream)
            check(lib.gg_puct_legal(lp, ip, B, N, gp, vp, stream), 'gg_puct_legal')
            if self._sym is not None:
                self._turn_legal(op, B, stream)
            for prepared in self._set_launches:   # (the sets that are on, in the table's order)
                _lib.launch(*prepared, stream)
            if self._past is not None:
                bp, kp, rp, cp, pp = self._past_ptrs
                past = self._past
                check(lib.gg_puct_past(R, N, self._C, self._L or 1, bp, kp, rp, cp, past.capacity, past.positions, int(past.moves),
                                       lp, ip, op, pp, self._feat[1], stream), 'gg_puct_past')
        self._pending = True
        if self._gumbel is not None:
            self._g_open, self._since = False, self._since + 1
        legal = self._legal if self._sym is None else self._legal_view
        res = (self._states, legal) + tuple(planes for _, planes in self._sets)
        return res + (self._past_planes,) if self._past is not None else res

    def backup(self, priors, values):
        """Step 4: priors float32 [R, A] and values float32 [R] (the value for the player to move at the leaf) of the leaves
        the last select() handed out ([R * L, A] and [R * L] with leaves=L); tensors on the search's device or NumPy arrays."""
        if not self._pending:
            raise ValueError('PuctSearch.backup(): no select() is outstanding')
        R, N, A, B = self._R, self._N, self._N * self._N + 1, self._R * (self._L or 1)
        f32 = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(
            device=self._dev, dtype=torch.float32).contiguous()
        priors, values = f32(priors), f32(values)
        if tuple(priors.shape) != (B, A) or values.numel() != B:
            raise ValueError('need priors [%d, %d] and values [%d] (got %s, %s)' % (B, A, B, tuple(priors.shape), tuple(values.shape)))
        if R:
            if self._sym is not None:
                priors = self._turn_priors_back(priors, B)
            boards, _, prior, links, stats, _ = self._tree
            name, slots = ('gg_puct_backup', ()) if self._L is None else ('gg_puct_backup_leaves', (self._L,))
            kp, kv = self._rows     # (the evaluator's two tensors are checked every round, against the table's entry)
            code = getattr(_lib.lib(), name)(R, N, self._C, *slots, self._komi, _lib.dev_ptr(priors, kp.kind, kp.name),
                                             _lib.dev_ptr(values.reshape(B), kv.kind, kv.name), boards, prior, links, stats,
                                             *self._out, _lib.current_raw_stream(self._dev))
            _lib.check(code, name)
        self._pending = False
        self._done += 1

    def result(self, tree=False):
        """-> Puct of the iterations done so far (tree=True: with the whole tree, PuctTree).  For device input some fields are
        views of the search's own buffers: clone what has to survive a later select()."""
        if self._pending:
            raise ValueError('PuctSearch.result(): the leaves of the last select() have not been backed up')
        return _back(self._box, self._result(tree))

    def _result(self, tree=False):
        """result() as device tensors, whatever batch_states was."""
        R, A = self._R, self._N * self._N + 1
        n, w = self._stats[..., 2], self._stats.view(torch.float64)[..., 0]
        rc = self._child[:, 0, :]
        has, idx = rc >= 0, rc.clamp(min=0).long()
        visits = torch.where(has, torch.gather(n, 1, idx), torch.zeros_like(rc))
        vsum = torch.where(has, torch.gather(w, 1, idx), torch.zeros((R, A), dtype=torch.float64, device=self._dev))
        whole = PuctTree(self._links[..., 0], self._links[..., 1], n, w) if tree else None
        return Puct(self._legal_roots, visits, vsum, self._prior[:, 0, :], n[:, 0], w[:, 0], self._nodes, whole)

    def root_states(self):
        """-> uint8 [R, 6, N, N]: the current roots, untracked from node 0 of every tree (a new tensor, or NumPy array for
        NumPy input), so that the caller need not step a second copy of the games."""
        if self._pending:
            raise ValueError('PuctSearch.root_states(): the leaves of the last select() have not been backed up')
        return self._box.back(self._root_states()) if self._box.numpy else self._root_states()

    def _root_states(self):
        R, N = self._R, self._N
        states = torch.empty((R, govars.NUM_CHNLS, N, N), dtype=_U8, device=self._dev)
        if R:
            _lib.call('gg_batch_untrack_states', self._root_boards(), states, R, N, _lib.current_raw_stream(self._dev))
        return states

    def _advance_buffers(self):
        """next [R, W], remap [R, capacity] and kept [R]: allocated once per search."""
        if self._scratch is None:
            R, dev = self._R, self._dev
            self._next = torch.empty((R, tracked_words(self._N)), dtype=_I32, device=dev)
            self._remap = torch.empty((R, self._C + 1), dtype=_I32, device=dev)
            self._kept = torch.empty(R, dtype=_I32, device=dev)
            self._scratch = _lib.ptrs('gg_puct_advance', next=self._next, remap=self._remap, kept=self._kept) if R else ()
        return self._scratch

    def _root_boards(self):
        """-> next [R, W], the search's scratch boards, as a copy of node 0's boards (R > 0): one copy."""
        self._advance_buffers()
        with torch.cuda.device(self._dev):
            self._next.copy_(self._boards[:, 0, :])
        return self._next

    def _play_on_roots(self, acts):
        """next = node 0's boards after acts (int64 [R] on the device; R > 0) -> the pointers of (actions as int32, next,
        remap, kept).  Whatever lies outside [-1, A) - below -1 too, which must not become the -1 that leaves a root
        alone - goes down as A: an illegal action in int32 range."""
        A = self._N * self._N + 1
        acts = torch.where((acts < -1) | (acts > A), torch.full_like(acts, A), acts).to(_I32).contiguous()
        np_, rp, kp = self._advance_buffers()
        ap, = _lib.ptrs('gg_puct_advance', actions=acts)
        self._root_boards()
        _lib.call('gg_batch_play_moves_tracked', np_, ap, None, self._R, self._N, 1, _lib.current_raw_stream(self._dev))
        return ap, np_, rp, kp

    def _push_past(self, acts):
        """past=: node 0's boards, from the tree's boards buffer, enter the history of every root whose action (acts: int64 [R]
        on the device; R > 0) is not -1 - the position the move is played on, pushed before it is played.  One copy, one
        compare, one launch; nothing is read back."""
        if self._past is None:
            return
        with torch.cuda.device(self._dev):
            self._past.push_tracked(self._root_boards(), acts != -1)

    def _played_states(self, acts):
        """-> uint8 [R, 6, N, N], a new device tensor: the roots after acts (int64 [R] on the device, -1 stays put), played on
        a copy of node 0's boards alone; the tree is not touched."""
        R, N = self._R, self._N
        states = torch.empty((R, govars.NUM_CHNLS, N, N), dtype=_U8, device=self._dev)
        if R:
            _, np_, _, _ = self._play_on_roots(acts)
            _lib.call('gg_batch_untrack_states', np_, states, R, N, _lib.current_raw_stream(self._dev))
        return states

    def advance(self, actions, iterations=None, check=True):
        """Play actions (int [R], a tensor or NumPy array; -1 = this root does not move) between two rounds and keep the
        subtree under each action -> kept, an int32 [R] device tensor owned by the search: the nodes kept per root, 0 where
        the tree starts afresh (the action had no child yet).  The next boards come from gg_batch_play_moves_tracked on a
        copy of the roots, the trees are renumbered in place by gg_puct_advance, result().legal follows the new roots and
        the round counter starts again: `iterations` (default: as constructed, whatever an earlier advance was given) more
        rounds may follow.  check=True verifies on
        the device that every action other than -1 is legal at its root - one synchronisation - and raises ValueError naming
        the first root where it is not; check=False does not synchronise: an illegal action then does what
        gg_batch_play_moves_tracked does with it, and its root gets a fresh tree (so does anything outside [-1, A): only -1
        itself leaves a root alone).  With past= the roots that move enter the history first (_push_past)."""
        if self._pending:
            raise ValueError('PuctSearch.advance(): the leaves of the last select() have not been backed up')
        R, N, A = self._R, self._N, self._N * self._N + 1
        if not isinstance(actions, torch.Tensor):
            actions = torch.from_numpy(np.ascontiguousarray(actions))
        if tuple(actions.shape) != (R,) or actions.dtype.is_floating_point or actions.dtype == torch.bool:
            raise ValueError('actions must be integers [%d] (got %s %s)' % (R, actions.dtype, tuple(actions.shape)))
        rounds = self._I0 if iterations is None else _puct_args(iterations, self._c, self._komi)[0]
        if self._gumbel is not None:
            self._g_open, self._since = True, 0
        if not R:
            self._done, self._I = 0, rounds
            return torch.empty(0, dtype=_I32, device=self._dev)
        acts = actions.to(device=self._dev, dtype=_I64)
        if check:
            inside = (acts >= 0) & (acts < A)
            ok = torch.gather(self._legal_roots, 1, acts.clamp(0, A - 1)[:, None])[:, 0] & inside
            bad = torch.nonzero((acts != -1) & ~ok)
            if bad.numel():   # (the synchronisation)
                r = int(bad[0, 0])
                raise ValueError('PuctSearch.advance(): action %d is not legal at root %d' % (int(acts[r]), r))
        self._push_past(acts)
        ap, np_, rp, kp = self._play_on_roots(acts)
        _lib.call('gg_puct_advance', ap, np_, R, N, self._C, *self._tree, rp, kp, _lib.current_raw_stream(self._dev))
        if self._history is not None:
            self._fill_node_hash()
        self._legal_roots = _legal_roots(self._root_states())
        self._done, self._I = 0, rounds
        if self._gumbel is not None:
            self._gumbel_begin()
        return self._kept

    def _root_hashes(self):
        """int64 [R], a new device tensor: batch_hash of the current roots (node 0 of every tree)."""
        R = self._R
        if not R:
            return torch.empty(0, dtype=_I64, device=self._dev)
        return batch_hash_tracked(self._root_boards())

    def forbid_repeats(self, history=None):
        """Positional superko AT THE ROOTS: the moves that would recreate a position of `history` (a PositionHistory of the R
        games, the current roots included) become illegal at node 0 of every tree - the repeat points of
        gg_batch_move_hashes_tracked, as row masks, are ORed into the invalid rows of the root boards, and result().legal
        follows.  Select, the prior mask of a root's first evaluation, add_root_noise and root_policy all read legality from
        the board, so a child kept under a forbidden action simply stops being chosen or counted.  Only the roots are
        marked here: the nodes below them are marked when they are made, and only by a search constructed with superko= (whose
        history is the default of `history`; without one the argument is required).  Call it before the rounds of a move (and before
        add_root_noise); advance() brings new root boards, whose invalid rows are their own.  Raises ValueError while leaves
        are outstanding.  One copy, one launch and two torch ops; nothing synchronises."""
        if self._pending:
            raise ValueError('PuctSearch.forbid_repeats(): the leaves of the last select() have not been backed up')
        R, N = self._R, self._N
        if history is None:
            history = self._history
        _history_arg(history, R)
        if not R:
            return
        with torch.cuda.device(self._dev):
            _, _, rep, rows = _move_hashes(self._root_boards(), True, history, repeat=True, rows=True)
            self._boards[:, 0, 2 * N:3 * N].bitwise_or_(rows)
            self._legal_roots = self._legal_roots & (rep == 0)

    def add_root_noise(self, noise, eps=0.25, todo=None):
        """Mix noise into the root's stored priors (gg_puct_root_noise) -> todo.  noise: float32 [R, A], a tensor or NumPy
        array, NOT normalised by the library (dirichlet_noise makes rows that sum to 1 over the legal actions); eps in
        [0, 1]; todo: a bool or uint8 [R] device tensor, updated in place (None: a fresh all-ones buffer, which is returned).
        A root with todo set that is evaluated and whose game has not ended gets prior = (1 - eps) * prior + eps * noise on
        its legal actions (float32, NaN / negative noise as 0) and its todo cleared; every other root keeps its bytes.  So
        one call before round 0 reaches the kept roots, a second call with the same noise and todo after round 0 the fresh
        roots that round has just evaluated, and no root is changed twice.  May be called whenever no leaf is outstanding;
        queues one launch, reads nothing back."""
        if self._gumbel is not None:
            raise ValueError('PuctSearch.add_root_noise(): a Gumbel search explores through g (set_gumbel), not through the priors')
        if self._pending:
            raise ValueError('PuctSearch.add_root_noise(): the leaves of the last select() have not been backed up')
        R, A = self._R, self._N * self._N + 1
        eps = float(eps)
        if not 0.0 <= eps <= 1.0:
            raise ValueError('need 0 <= eps <= 1 (got %r)' % eps)
        if not isinstance(noise, torch.Tensor):
            noise = torch.from_numpy(np.ascontiguousarray(noise))
        if tuple(noise.shape) != (R, A):
            raise ValueError('noise must be [%d, %d] (got %s)' % (R, A, tuple(noise.shape)))
        if todo is None:
            todo = torch.ones(R, dtype=_U8, device=self._dev)
        elif (not isinstance(todo, torch.Tensor) or todo.dtype not in (torch.bool, _U8) or tuple(todo.shape) != (R,)
              or not todo.is_contiguous()):
            raise ValueError('todo must be a contiguous bool or uint8 [%d] device tensor' % R)
        if R:
            noise = noise.to(device=self._dev, dtype=torch.float32).contiguous()
            boards, _, prior, _, stats, nodes = self._tree
            _lib.call('gg_puct_root_noise', R, self._N, self._C, eps, noise, todo, boards, prior, stats, nodes,
                      _lib.current_raw_stream(self._dev))
        return todo

    def root_policy(self, sample=None, rng=None, pi=True):
        """The move, the policy target and the value of every root (gg_puct_root_policy) -> (actions int64 [R], pi float32
        [R, A] or None with pi=False, value float32 [R]); device tensors, or NumPy arrays for NumPy input.  sample: None (no
        root draws) or bool / uint8 [R]; where it is set and the root's children have visits, the action is drawn in
        proportion to the visit counts with rng - the caller's gogame.rng_seed(..) tensor, int64 [R] on the device,
        advanced in place once per root that draws -, elsewhere it is the legal child with the most visits, ties to the
        lowest action: puct_actions' move.  pi = visits / their sum (all zero without visits), value = the root's mean
        value for the player to move.  A root whose game has ended gives -1, a zero row and 0.  May be called whenever no
        leaf is outstanding; queues one launch, reads nothing back."""
        if self._pending:
            raise ValueError('PuctSearch.root_policy(): the leaves of the last select() have not been backed up')
        R = self._R
        if sample is not None:
            if rng is None:
                raise ValueError('PuctSearch.root_policy(): sample needs rng (gogame.rng_seed)')
            if not isinstance(sample, torch.Tensor):
                sample = torch.from_numpy(np.ascontiguousarray(sample))
            if tuple(sample.shape) != (R,) or sample.dtype not in (torch.bool, _U8):
                raise ValueError('sample must be bool or uint8 [%d] (got %s %s)' % (R, sample.dtype, tuple(sample.shape)))
            if (not isinstance(rng, torch.Tensor) or rng.dtype != _I64 or tuple(rng.shape) != (R,) or not rng.is_contiguous()):
                raise ValueError('rng must be a contiguous int64 [%d] device tensor (gogame.rng_seed)' % R)
            sample = sample.to(self._dev).contiguous()
        acts, p, v = self._root_policy(sample, rng, pi)
        return tuple(_back(self._box, t) for t in (acts.to(_I64), p, v))

    def _root_policy(self, sample, rng, pi=True):
        """root_policy() on checked device tensors -> (actions int32 [R], pi or None, value), new device tensors."""
        R, A, dev = self._R, self._N * self._N + 1, self._dev
        acts = torch.empty(R, dtype=_I32, device=dev)
        p = torch.empty((R, A), dtype=torch.float32, device=dev) if pi else None
        v = torch.empty(R, dtype=torch.float32, device=dev)
        if R:
            boards, child, _, _, stats, nodes = self._tree
            _lib.call('gg_puct_root_policy', R, self._N, self._C, sample, rng if sample is not None else None, boards, child, stats,
                      nodes, acts, p, v, _lib.current_raw_stream(dev))
        return acts, p, v


def batch_puct(batch_states, iterations, evaluator, c=1.25, komi=0.0, tree=False, leaves=None, capacity=None, features=None,
               symmetry=None, first_root=0, life=False, ladder=False, outcome=False, superko=None, area=False, past=None,
               gumbel=None):
    """PUCT search (the AlphaZero search) of `iterations` iterations from every root of batch_states ([R, 6, N, N]) with the
    caller's evaluator -> Puct (device tensors for a device tensor, NumPy arrays for NumPy input).  The loop over PuctSearch.

    evaluator(states, legal) -> (priors, values): states uint8 [R, 6, N, N] and legal bool [R, A] (A = N*N + 1) are device
    tensors whatever batch_states was; priors float32 [R, A], values float32 [R] - the value in [-1, 1] for the player to move
    at the leaf.  Priors are NOT renormalised by the library (a float sum would depend on the kernel's order): normalising
    over `legal` is the evaluator's job.  Root Dirichlet noise can be its business too - iteration 0 always hands out the roots -
    but only for a search from fresh roots: a root kept by PuctSearch.advance is not handed out again, and
    PuctSearch.add_root_noise reaches both kinds.

    Each root has its own tree with room for iterations + 1 nodes; a node keeps n (visits), w (float64 sum of the backed-up
    values from BLACK's point of view), its priors and a child table.  Iteration i, per root: select from the root - a node
    whose game has ended, or that has not been evaluated (the root at i = 0), is the leaf; else take the legal action
    (batch_uct's rule) of the largest U = q + c * prior[a] * sqrt(n_x) / (1 + n_c), q = +-w_c / n_c for the player to move at
    x (0 without visits; float64, in this order, no fused multiply-add; ties to the lowest action): without a child under
    it, the child is created and is the leaf, else the walk goes on there.  n_x counts the node's own evaluation
    (n_x = 1 + sum of n_c): with the children's sum alone the first selection below a fresh node would see sqrt(0) and
    ignore the priors.  The leaves are evaluated; a node's first evaluation stores max(prior, 0) on its legal actions and 0
    elsewhere (NaN -> 0); the value is clamped to [-1, 1] (NaN -> 0) and turned to black's point of view - at a leaf whose
    game has ended it is sign(black area - white area - komi) instead and the evaluator's row is ignored - and n += 1,
    w += value on the path from the leaf to the root.  So root_visits = iterations, a live root's visits sum to
    iterations - 1, an ended root evaluates itself every iteration.  No random numbers; the result of a root depends on
    that root and the evaluator's answers alone, so shards by root concatenate to the whole.  Needs 1 <= iterations < 2^31 - 1,
    c >= 0 and finite, komi finite.  tree=True also returns the whole tree (PuctTree).  The roots are not modified.

    Device memory of the tree: R * (iterations + 1) * (4 (5N + 1) + 8 (N^2 + 1) + 24) bytes (boards, child tables, priors,
    links and stats: 3 304 bytes, about 3.3 KB, per node at 19x19; 220 MB for 1 024 roots x 64 iterations).

    leaves=L (an integer >= 1; the default None is the search above, launch for launch): `iterations` ROUNDS of up to L leaves
    per root.  A node also has v, its virtual visits (0 outside a round).  The L slots of a root are selected one after the
    other; each walks from the root: a node with n = 0 and v > 0 was handed out earlier in this round - a collision: this
    slot and the root's later ones stay empty (evaluated as a copy of the root and ignored) -; else an ended or unevaluated
    node is the leaf; else the walk follows the largest U' = q + c * prior[a] * sqrt(n_x + v_x) / (1 + n_c + v_c),
    q = (+-w_c - v_c) / (n_c + v_c) - one virtual visit is one loss for the side that chose the child - and expands as
    above.  The slot's path from the leaf to the root then gets v += 1.  The evaluator sees states [R * L, 6, N, N] and legal
    [R * L, A] (row r * L + j = slot j of root r) and returns priors [R * L, A], values [R * L]; the backup runs the slots in
    order (n += 1, w += value, v -= 1 on the path).  root_visits = the non-empty slots (round 0 evaluates the root alone);
    leaves=1 gives the tree of leaves=None exactly; no random numbers, shards by root still concatenate.  Needs
    iterations * L < 2^31 - 1.  Device memory of the tree: R * (iterations * L + 1) * (4 (5N + 1) + 8 (N^2 + 1) + 24)
    bytes - the formula above with iterations * L + 1 nodes - and PuctTree fields are [R, iterations * L + 1].

    capacity (None: the sizes above): the nodes per root, an integer >= the default and < 2^31; the tree, its device memory
    and the PuctTree fields are then [R, capacity].  It changes no result of this call (the extra nodes stay unused): it is
    PuctSearch.advance and puct_play that need the room.

    features (None: the search above, launch for launch; or torch.uint8 / float16 / bfloat16 / float32): the evaluator is
    called as evaluator(planes, legal) with planes [R, 16, N, N] ([R * L, ..]) of that dtype - batch_features of the leaves,
    written by one launch from the tracked leaf boards (PuctSearch) - instead of the byte-plane states.  An evaluator that
    needs states (playout_evaluator: its attribute needs_states) is refused with ValueError.

    symmetry (None: the search above, launch for launch; or an integer base seed, with features=): the evaluator sees every
    leaf - planes and legal - in a random orientation and its priors are turned back (PuctSearch); first_root: the global
    index of root 0, so that shards by root draw what the whole draws.

    life (False: the search above, launch for launch; True, with features=): the evaluator is called as
    evaluator(planes, legal, life) with life [R, 4, N, N] ([R * L, ..]) of the feature dtype - batch_life of the leaves, in
    the leaf's orientation with symmetry= (PuctSearch).  The tree does not depend on it but through the evaluator.

    ladder (False: the search above, launch for launch; True, with features=): the evaluator is called as
    evaluator(planes, legal, [life,] ladder) with ladder [R, 4, N, N] ([R * L, ..]) of the feature dtype - batch_ladder of the
    leaves, in the leaf's orientation with symmetry= (PuctSearch).

    outcome (False: the search above, launch for launch; True, with features=): the evaluator gets as its last argument,
    after life and ladder when those are on, the move-outcome planes [R, 12, N, N] ([R * L, ..]) of the feature dtype -
    batch_move_planes of the leaves, in the leaf's orientation with symmetry= (PuctSearch).

    superko (None: the search above, launch for launch; or a PositionHistory of the R games, batch_states' own positions
    included): the search of one position of a recorded game under positional superko - PuctSearch.forbid_repeats once before
    round 0 for the roots, and gg_puct_superko in every round for the nodes below them (PuctSearch): no node of the tree
    reached by a board move has the position of one of its ancestors or of the history.  result().legal is the reduced set.

    area (False: the search above, launch for launch; True, with features=): the evaluator gets as its LAST argument, after
    life, ladder and outcome when those are on, the area ownership planes [R, 3, N, N] ([R * L, ..]) of the feature dtype -
    batch_area_planes of the leaves, in the leaf's orientation with symmetry= (PuctSearch).

    past (None: the search above, launch for launch; or a StoneHistory of the R games holding the positions before the roots,
    with features=): the evaluator gets as its LAST argument, after life, ladder, outcome and area when those are on, the
    history planes [R, past.planes, N, N] ([R * L, ..]) of the feature dtype - the leaf, its ancestors in the tree and, beyond
    node 0, the history (PuctSearch) - in the leaf's orientation with symmetry=.

    gumbel (None: the search above, launch for launch; or an int m, or a Gumbel): the Gumbel root rule by sequential halving
    (PuctSearch): the root's simulations follow the schedule instead of U'.  The result type does not change - the visits
    are those the schedule handed out -; puct_actions(gumbel=) gives the Gumbel move, PuctSearch.gumbel_root the improved
    policy."""
    return _puct_searched(batch_states, iterations, evaluator, c, komi, superko, **_search_options(locals())).result(tree=tree)


def _puct_searched(batch_states, iterations, evaluator, c=1.25, komi=0.0, superko=None, **opts):
    """batch_puct's loop -> the PuctSearch after its last backup.  opts: the options of PuctSearch (_SEARCH_OPTIONS)."""
    _puct_komi_guard(evaluator, komi)
    _puct_features_guard(evaluator, opts.get('features'))
    _puct_planes_guard(opts)
    search = PuctSearch(batch_states, iterations, c, komi, superko=superko, **opts)
    if superko is not None:
        search.forbid_repeats()
    for _ in range(search._I):
        priors, values = evaluator(*search.select())
        search.backup(priors, values)
    return search


def _puct_komi_guard(evaluator, komi):
    ek = getattr(evaluator, 'komi', None)   # (playout_evaluator says what komi it scores with)
    if ek is not None and float(ek) != float(komi):
        raise ValueError('the evaluator scores its playouts with komi %r, the search its ended leaves with %r' % (ek, komi))


def _puct_superko_guard(superko):
    if superko is not False and superko is not True and not (type(superko) is type('') and superko == 'tree'):   # (before a device is touched)
        raise ValueError("superko must be False, True (the roots) or 'tree' (every node) (got %r)" % (superko,))


def _puct_superko_history(superko, box, moves):
    """The PositionHistory of a move loop with superko='tree' (else None), made BEFORE the search that keeps it: it is seeded
    once the search stands, and the search reads it no earlier than its first select()."""
    st = box.t
    if superko is True or not superko or st.dim() != 4 or not st.shape[0]:
        return None
    return PositionHistory(st.shape[0], moves + 1, st.device)


def _puct_features_guard(evaluator, features):
    if features is not None:
        _feature_dtype(features)
        if getattr(evaluator, 'needs_states', False):   # (playout_evaluator plays on from the byte planes)
            raise ValueError('the evaluator needs states (needs_states), the search hands out feature planes (features=%r)' % (features,))


def puct_play(batch_states, moves, iterations, evaluator, c=1.25, komi=0.0, leaves=None, capacity=None, reuse=True, features=None,
              symmetry=None, first_root=0, life=False, ladder=False, outcome=False, superko=False, area=False, past=None,
              gumbel=None, gumbel_noise=None):
    """Play `moves` moves from every root of batch_states ([R, 6, N, N]) with a PUCT search per move -> (actions int64
    [R, moves], the final states uint8 [R, 6, N, N]); device tensors for a device tensor, NumPy arrays for NumPy input.
    Per move: `iterations` rounds of PuctSearch (batch_puct's loop, with `leaves` and `capacity` as there), the move of
    every root is its legal child with the most visits (ties to the lowest action; -1 for a root without a legal move,
    which stays where it is), then PuctSearch.advance: with reuse=True the subtree under the move played is the next
    move's tree, so its visits are not paid for again and the roots get deeper for the same evaluator work.  reuse=False
    is the same loop with a new PuctSearch on the next states (the move played on node 0's boards alone, no advance over a
    tree that is dropped) after every move: what a caller could do before advance
    existed, kept as the comparison.  The evaluator is called moves * iterations times and must score with the search's
    komi (batch_puct's guard).

    A kept tree keeps its nodes, so with the default capacity it is full after the first move or soon after: a full tree
    falls under the no-room rule - it goes on refining the values of the nodes it has and expands nothing.  Give `capacity`
    room for the moves to come; no finite capacity excludes a full tree over many moves, and PuctSearch.result().nodes
    shows how full the trees are.  A kept root is already evaluated and is not handed out again, so root noise that the
    evaluator adds would reach only fresh roots: PuctSearch.add_root_noise reaches kept roots too, and puct_selfplay is this
    loop with it, with moves drawn from the visit counts and with the training records.  features: as batch_puct - the
    evaluator gets (planes, legal).  symmetry, first_root: as batch_puct; with reuse=False the search of move mv draws from
    the base seed symmetry + mv (a new search would repeat the first one's draws otherwise).  life: as batch_puct - the
    evaluator gets (planes, legal, life).  ladder: as batch_puct - the ladder planes as the evaluator's next argument.
    outcome: as batch_puct - the move-outcome planes as the evaluator's last argument.
    superko (False = everything above, launch for launch): positional superko at the roots - a PositionHistory of capacity
    moves + 1 is seeded with the roots' hashes, PuctSearch.forbid_repeats runs before each move's rounds, and the new roots'
    hashes are pushed after each move, so no move played recreates an earlier position of its game.  With True the
    repetitions inside the tree below the root are not checked: the search still plans with them.  superko='tree': the loop of
    True with the history also handed to the search (PuctSearch(superko=)), with reuse=False to the new search of every move
    too: the rule holds at every node.  Any other value raises ValueError.  area: as batch_puct - the area ownership planes as
    the evaluator's last argument.  past (None = everything above, launch for launch; with features=): the history planes
    as the evaluator's last argument (PuctSearch(past=)).  An int T or a pair (T, moves) makes an empty StoneHistory for games
    that start here; the loop keeps it - every move the roots that move are pushed before they are played on, by advance or,
    with reuse=False, before the new search gets the same object; a StoneHistory is used as given, for games that do not
    start here (it holds the positions before batch_states).  gumbel (None = everything above, launch for launch; or an int
    m, or a Gumbel): every move's search runs under the Gumbel root rule (PuctSearch(gumbel=)) and the move played is the
    Gumbel action (PuctSearch.gumbel_root; -1 for a root whose game has ended); gumbel_noise (None, or a callable
    noise(mv, legal) -> float [R, A] as gumbel_noise() returns; needs gumbel=): g of move mv, set before its first round;
    None leaves g at zeros - noise-free sequential halving, for match play."""
    opts = _search_options(locals())
    _gumbel_noise_guard(gumbel, gumbel_noise)
    _puct_superko_guard(superko)
    _puct_komi_guard(evaluator, komi)
    _puct_features_guard(evaluator, features)
    _puct_planes_guard(opts)
    if past is not None and not isinstance(past, StoneHistory):
        _past_request(past)
    moves = int(moves)
    if moves < 0:
        raise ValueError('need moves >= 0 (got %d)' % moves)
    deep = None
    if past is not None:
        batch_states = batch_states if isinstance(batch_states, _Box) else _Box(batch_states)
        opts['past'] = _puct_past_history(past, batch_states)
    if superko is not True and superko:   # ('tree': the search keeps the history, which therefore stands before the search)
        batch_states = batch_states if isinstance(batch_states, _Box) else _Box(batch_states)
        deep = _puct_superko_history(superko, batch_states, moves)
    search = PuctSearch(batch_states, iterations, c, komi, superko=deep, **opts)
    box = search._box
    played = torch.empty((search._R, moves), dtype=_I64, device=box.t.device)
    seen = None
    if superko and search._R:
        seen = (deep or PositionHistory(search._R, moves + 1, box.t.device)).push(search._root_hashes())
    for mv in range(moves):
        if seen is not None:
            search.forbid_repeats(seen)
        if gumbel_noise is not None:
            search.set_gumbel(gumbel_noise(mv, search._legal_roots))
        for _ in range(search._I):
            priors, values = evaluator(*search.select())
            search.backup(priors, values)
        if gumbel is None:
            res = search._result()
            played[:, mv] = _best_legal(_ON_DEVICE, res.legal, res.visits.to(_I64))
        else:
            played[:, mv] = search._gumbel_root(pi=False)[0]
        if reuse:
            search.advance(played[:, mv], check=False)
        else:   # only node 0's boards are played on: the tree goes, so no advance over it; the states stay on the device
            if search._R:
                search._push_past(played[:, mv])
            box.t = search._played_states(played[:, mv])
            if symmetry is not None:   # (a new search would repeat the first one's draws otherwise)
                opts['symmetry'] = int(symmetry) + mv + 1
            search = PuctSearch(box, iterations, c, komi, superko=deep, **opts)
        if seen is not None:
            seen.push(search._root_hashes())
    return _back(box, played), box.back(search._root_states())


def _gumbel_noise_guard(gumbel, noise, default=None):
    if noise is not None and noise != default and not callable(noise):   # (before a device is touched)
        raise ValueError('gumbel_noise must be None or a callable noise(move, legal) -> float [R, A]')
    if gumbel is None and callable(noise):
        raise ValueError('gumbel_noise makes the draws of a Gumbel search: give gumbel= too')


def dirichlet_noise(alpha, generator=None):
    """Root exploration noise for puct_selfplay -> a callable noise(move, legal) -> float32 [R, A] on legal's device: per
    root a Dirichlet(alpha) sample over its legal actions (legal: bool [R, A]) - Gamma(alpha) draws by torch (`generator`:
    a torch.Generator of that device, None = torch's default), zero on illegal actions, divided by the row sum; a row
    whose draws all underflowed is uniform over the legal actions, a root without legal actions gets zeros.  NOT
    bit-defined: the draws are torch's and the row sum is a float sum in torch's order, so a game played with this noise
    is reproducible only as far as torch's generator is; everything the library does with the noise is exact."""
    alpha = float(alpha)
    if not (alpha > 0 and math.isfinite(alpha)):
        raise ValueError('need alpha > 0 and finite (got %r)' % alpha)

    def noise(move, legal):
        conc = torch.full(legal.shape, alpha, dtype=torch.float32, device=legal.device)
        g = torch.where(legal, torch._standard_gamma(conc, generator=generator), torch.zeros_like(conc))
        total = g.sum(dim=1, keepdim=True)
        count = legal.sum(dim=1, keepdim=True).to(torch.float32)
        uniform = torch.where(legal, 1.0 / count.clamp(min=1.0), torch.zeros_like(conc))
        return torch.where(total > 0, g / total.clamp(min=torch.finfo(torch.float32).tiny), uniform)

    return noise


SelfPlay = collections.namedtuple('SelfPlay', 'actions pi value outcome lengths final_states states')
SelfPlay.__doc__ = """Records of puct_selfplay per root: actions (int64 [R, moves], -1 once the game has ended), pi (float32
[R, moves, A]: the root's visit counts over their sum before each move, zero rows once the game has ended), value (float32
[R, moves]: the root's mean value for the player to move), outcome (int8 [R]: sign(black area - white area - komi) of a game
that ended, 0 for one still running), lengths (int32 [R]: moves played), final_states (uint8 [R, 6, N, N]) and states (uint8
[R, moves, 6, N, N], the roots before each move, or None)."""


def puct_selfplay(batch_states, moves, iterations, evaluator, c=1.25, komi=0.0, leaves=None, capacity=None, noise=None,
                  eps=0.25, sample_moves=0, seed=20260927, first_game=0, record_states=False, features=None, symmetry=None,
                  life=False, ladder=False, outcome=False, superko=False, area=False, past=None, gumbel=None, gumbel_noise='default'):
    """Self-play games for training: `moves` moves from every root of batch_states ([R, 6, N, N]) with a PUCT search per move
    on the kept tree -> SelfPlay (device tensors for a device tensor, NumPy arrays for NumPy input).  puct_play's
    reuse=True loop (`iterations` rounds per move with `leaves` and `capacity` as there, then PuctSearch.advance) with
    four changes, per move mv:
      - noise (None, or a callable noise(mv, legal) -> float32 [R, A] as dirichlet_noise returns; legal: the roots' bool
        [R, A]): z = noise(mv, legal) is mixed into the roots' priors with weight eps by PuctSearch.add_root_noise, once
        before round 0 - which reaches the roots kept from the move before - and once after it with the same z and todo -
        which reaches the fresh roots round 0 has just evaluated; no root gets it twice, ended roots never.
      - after the last round PuctSearch.root_policy gives the move, the policy target and the root value: while
        mv < sample_moves the move is drawn in proportion to the visit counts, afterwards it is the child with the most
        visits (puct_play's move).  The generators are rng_seed(R, seed, first_game), made once per call, so shards by root
        with first_game = the shard's first root concatenate to the whole.
      - the records are kept: see SelfPlay.  A game that has ended stays where it is: action -1, a zero pi row, value 0.
      - outcome: for a game that ended, sign(black area - white area - komi) by the rule of the search's ended leaves (komi
        and the difference in float32); 0 for a game still running after `moves`.
    Nothing synchronises: every step queues launches on torch's current stream.  The evaluator is called moves * iterations
    times and must score with the search's komi (batch_puct's guard).  Without record_states a trainer replays the
    positions from the roots with batch_play_moves(states, actions).  Device memory of the records: pi takes
    4 * R * moves * A bytes (189 MB for 1 024 roots x 128 moves at 19x19), states 6 N^2 * R * moves.  moves = 0 or R = 0:
    no device call, empty records of these shapes.  features: as batch_puct - the evaluator gets (planes, legal); the records
    (states included) are unchanged.  symmetry (None, or an integer base seed, with features=): every leaf evaluation in a
    random orientation, as batch_puct; the search gets first_root=first_game, so shards concatenate here too.  The records stay
    in the boards' own frame.  A trainer takes its samples from the records with selfplay_batch: the planes of the recorded
    positions and the policy targets, in any of the eight orientations.  life: as batch_puct - the evaluator gets (planes,
    legal, life); the records do not change, and there is no stopping rule here: a driver that wants to stop settled games
    early asks batch_settled(search.root_states()) in a loop of its own.  ladder: as batch_puct - the ladder planes as the
    evaluator's next argument; the records do not change.  outcome: as batch_puct - the move-outcome planes as the evaluator's
    last argument; the records do not change.  superko (False = everything above, launch for launch): positional superko at
    the roots, as puct_play - PuctSearch.forbid_repeats before each move's rounds and before the root noise, so
    noise(mv, legal) sees the reduced legal set, and the new roots' hashes pushed after each advance: no recorded game
    recreates an earlier position of its own, so games that would cycle until `moves` cuts them off with outcome 0 come to
    an end.  With True the repetitions inside the tree below the root are not checked, and the visit counts recorded as pi
    include plans through them; superko='tree' is the loop of True with the history also handed to the search
    (PuctSearch(superko=)): the rule holds at every node.  Any other value raises ValueError.  area: as batch_puct - the area
    ownership planes as the evaluator's last argument; the records do not change (selfplay_batch makes the ownership and
    score targets from them).  past: as puct_play - the history planes as the evaluator's last argument, an int T or a pair
    (T, moves) for games that start here, or a StoneHistory of the positions before batch_states; the records do not change
    (selfplay_batch(past=) makes the planes of the sampled positions from record.states).  gumbel (None = everything above,
    launch for launch; or an int m, or a Gumbel): self-play under the Gumbel root rule (PuctSearch(gumbel=)).  Per move
    g = gumbel_noise(mv, legal) is set before the first round (gumbel_noise: 'default' = gumbel_noise(), torch's default
    generator; None = zeros; or a callable as gumbel_noise() returns), the move is the Gumbel action - already a draw from the
    improved policy, so sample_moves > 0 raises ValueError, as does noise other than None: the exploration is g -, the
    recorded pi is the improved policy and value the root's mean value (PuctSearch.gumbel_root).  selfplay_batch takes the
    records as they are."""
    opts = dict(_search_options(locals()), first_root=first_game)
    _gumbel_noise_guard(gumbel, gumbel_noise, 'default')
    _gumbel_arg(gumbel, 2, 1)
    _puct_planes_guard(opts)
    if past is not None and not isinstance(past, StoneHistory):
        _past_request(past)
    _puct_superko_guard(superko)
    _puct_komi_guard(evaluator, komi)
    _puct_features_guard(evaluator, features)
    moves, sample_moves, eps = int(moves), int(sample_moves), float(eps)
    if moves < 0:
        raise ValueError('need moves >= 0 (got %d)' % moves)
    if sample_moves < 0:
        raise ValueError('need sample_moves >= 0 (got %d)' % sample_moves)
    if not 0.0 <= eps <= 1.0:
        raise ValueError('need 0 <= eps <= 1 (got %r)' % eps)
    if noise is not None and not callable(noise):
        raise ValueError('noise must be None or a callable noise(move, legal) -> float32 [R, A]')
    if gumbel is not None and noise is not None:
        raise ValueError('a Gumbel search explores through gumbel_noise, not through noise in the priors: noise must be None')
    if gumbel is not None and sample_moves > 0:
        raise ValueError('the Gumbel action is already a draw from the improved policy: sample_moves must be 0 with gumbel=')
    box = batch_states if isinstance(batch_states, _Box) else _Box(batch_states)
    st = box.t
    if st.dim() != 4 or st.shape[1] != govars.NUM_CHNLS or st.shape[2] != st.shape[3]:
        raise ValueError('batch_states must be [R, 6, N, N] (got %s)' % (tuple(st.shape),))
    I, c, komi = _puct_args(iterations, c, komi)
    _puct_capacity(I, _puct_leaves(I, leaves), capacity)
    _gumbel_arg(gumbel, I, _puct_leaves(I, leaves) or 1)
    draws = None if gumbel is None else (globals()['gumbel_noise']() if gumbel_noise == 'default' else gumbel_noise)
    R, N, dev = st.shape[0], st.shape[2], st.device
    A = N * N + 1
    played = torch.full((R, moves), -1, dtype=_I64, device=dev)
    pis = torch.zeros((R, moves, A), dtype=torch.float32, device=dev)
    vals = torch.zeros((R, moves), dtype=torch.float32, device=dev)
    lengths = torch.zeros(R, dtype=_I32, device=dev)
    won = torch.zeros(R, dtype=torch.int8, device=dev)   # (who won, for the record: the field's own name is an option's here)
    before = torch.empty((R, moves, govars.NUM_CHNLS, N, N), dtype=_U8, device=dev) if record_states else None
    if not R or not moves:
        return _back(box, SelfPlay(played, pis, vals, won, lengths, st, before))
    deep = _puct_superko_history(superko, box, moves)
    opts['past'] = _puct_past_history(past, box)
    search = PuctSearch(box, I, c, komi, superko=deep, **opts)
    rng = rng_seed(R, seed, first_game, device=dev)
    ones, todo = torch.ones(R, dtype=_U8, device=dev), torch.empty(R, dtype=_U8, device=dev)
    seen = (deep or PositionHistory(R, moves + 1, dev)).push(search._root_hashes()) if superko else None
    for mv in range(moves):
        if record_states:
            before[:, mv] = search._root_states()
        if seen is not None:
            search.forbid_repeats(seen)
        if noise is not None:
            z = noise(mv, search._legal_roots)
            todo.fill_(1)
            search.add_root_noise(z, eps, todo)     # the roots kept from the move before
        if draws is not None:
            search.set_gumbel(draws(mv, search._legal_roots))
        for t in range(search._I):
            priors, values = evaluator(*search.select())
            search.backup(priors, values)
            if t == 0 and noise is not None:
                search.add_root_noise(z, eps, todo)   # the fresh roots round 0 has just evaluated
        acts, p, v = search._root_policy(ones if mv < sample_moves else None, rng) if gumbel is None else search._gumbel_root()
        played[:, mv], pis[:, mv], vals[:, mv] = acts, p, v
        lengths += (acts >= 0).to(_I32)
        search.advance(played[:, mv], check=False)
        if seen is not None:
            seen.push(search._root_hashes())
    final = search._root_states()
    black, white = _areas_dev(final)
    x = (black - white).to(torch.float32) - torch.full((), komi, dtype=torch.float32, device=dev)   # gg_puct_backup's terminal rule
    ended = final[:, govars.DONE_CHNL, 0, 0] != 0
    won = torch.where(ended, torch.sign(x), torch.zeros_like(x)).to(torch.int8)
    return _back(box, SelfPlay(played, pis, vals, won, lengths, final, before))


def puct(state, iterations, evaluator, **kw):
    """batch_puct of one state [6, N, N] -> Puct of [N*N + 1] vectors and scalars (tree fields [iterations + 1]); the evaluator
    still sees a batch of one."""
    _puct_planes_guard(kw)
    return _single(batch_puct, state, iterations, evaluator, **kw)


def puct_actions(batch_states, iterations, evaluator, **kw):
    """The PUCT move of every root -> int64 [R]: the legal root child with the most visits after batch_puct(batch_states,
    iterations, evaluator, **kw); ties go to the lowest action, a root without a legal move gives -1.  With gumbel= it is the
    Gumbel move (PuctSearch.gumbel_root): among the actions with the most simulations the largest g + logit + sigma(q), g = 0."""
    _puct_planes_guard(kw)
    box = _Box(batch_states)
    if kw.get('gumbel') is not None:
        kw.pop('tree', None)
        search = _puct_searched(box.t, iterations, evaluator, **kw)
        return _back(box, search._gumbel_root(pi=False)[0].to(_I64))
    res = batch_puct(box.t, iterations, evaluator, **kw)
    return _best_legal(box, res.legal, res.visits.to(_I64))


def playout_evaluator(playouts, max_plies=None, seed=20260927, first_root=0, policy='uniform', slots=None, chunk_plies=32, *,
                      komi):
    """A ready-made evaluator for batch_puct / PuctSearch that needs no network: uniform priors and Monte Carlo values.
    priors = float32(1) / float32(number of legal actions) on the legal actions, 0 elsewhere; values = float32(wins of the
    side to move - its losses) / float32(playouts) over exactly batch_playouts(leaves, playouts, max_plies, komi,
    seed=s_j, first_root, slots=slots, chunk_plies=chunk_plies, policy=policy) in its j-th call (j = 0, 1, ...), s_j the
    generator of game j under `seed` as in batch_uct.  komi (required, keyword only): the komi of the search - the playouts
    and the search's ended leaves must be scored alike, so there is no default to forget; batch_puct refuses an evaluator
    whose komi (its attribute `komi`) differs from its own.  The object counts its calls: make a new one per search.  Its attribute plies_sum is an int64 device scalar: the plies all its playouts have played
    (None before the first call)."""
    pol_name, K = policy, int(playouts)
    _policy_code(policy)
    komi = float(komi)
    if K < 1 or not math.isfinite(komi):
        raise ValueError('need playouts >= 1 and a finite komi')
    calls = [0]

    def evaluate(states, legal):
        j = calls[0]
        calls[0] += 1
        res = batch_playouts(states, K, max_plies, komi, seed=_uct_seed(seed, j), first_root=first_root, slots=slots,
                             chunk_plies=chunk_plies, policy=pol_name)
        # (tensor / tensor: a true float32 division - by a Python number torch multiplies with the rounded reciprocal)
        one, kf = (torch.full((), v, dtype=torch.float32, device=legal.device) for v in (1.0, float(K)))
        count = legal.sum(dim=1, keepdim=True).to(torch.float32)
        priors = torch.where(legal, one / count, torch.zeros_like(one))
        white = states[:, govars.TURN_CHNL, 0, 0].to(torch.bool)
        diff = res.black_wins - res.white_wins
        values = torch.where(white, -diff, diff).to(torch.float32) / kf
        plies = res.plies_sum.sum()
        evaluate.plies_sum = plies if evaluate.plies_sum is None else evaluate.plies_sum + plies
        return priors, values

    evaluate.plies_sum = None
    evaluate.komi = komi
    evaluate.needs_states = True   # (it plays on from the byte planes: batch_puct refuses it together with features=)
    return evaluate


# ---------------------------------------------------------------- policy-weighted sampling on the device
# gogame.random_weighted_action / random_action (gym_go/gogame.py:385-404) for every game of a batch: what a self-play loop
# with a policy network calls after the forward pass.  The draw is defined in integers (include/gymgo_amd.h,
# gg_batch_sample_weighted) so that device and CPU restatement agree bit for bit; P(a) = w[a] / sum(w) over the playable
# actions up to 22-bit fixed point relative to the largest weight.

WEIGHT_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}   # GG_W_* of include/gymgo_amd.h


def _weights_tensor(weights, B, N, device):
    """-> (contiguous device tensor in its own dtype if that is float32 / bfloat16 / float16 - anything else becomes
    float32 - and the GG_W_* code).  The 16-bit forms are widened exactly by the kernels: half the bytes, the same draw."""
    if not isinstance(weights, torch.Tensor):
        weights = torch.as_tensor(np.asarray(weights, dtype=np.float32))
    if weights.dtype not in WEIGHT_DTYPES:
        weights = weights.to(torch.float32)
    w = weights.to(device=device).contiguous()
    if tuple(w.shape) != (B, N * N + 1):
        raise ValueError('weights must be [B, N*N+1] = [%d, %d] (got %s)' % (B, N * N + 1, tuple(w.shape)))
    return w, WEIGHT_DTYPES[w.dtype]


def _check_drawn(actions, check):
    if check and bool((actions < 0).any()):
        raise ValueError('no positive weight on a playable action for some game (np.random.choice raises here too)')
    return actions


def batch_sample_weighted(batch_states, weights, rng, check=False):
    """actions[b] ~ weights[b] / sum(weights[b]) over the actions plane 3 of batch_states[b] allows (the pass always;
    a finished game allows everything) - gogame.random_weighted_action (gym_go/gogame.py:385-392) per game, on the device,
    with the per-game generator `rng` (advanced once).  batch_states=None: nothing is masked (the reference "assumes all
    invalid moves have weight 0").  A game without a positive playable weight gets -1 (check=True: ValueError)."""
    if batch_states is not None:
        B, C, N, _ = batch_states.shape
        dev = batch_states.device
    else:
        if not isinstance(weights, torch.Tensor):
            raise ValueError('without states the weights must be a device tensor')
        B, dev = weights.shape[0], weights.device
        N = int(round((weights.shape[1] - 1) ** 0.5))
    w, wcode = _weights_tensor(weights, B, N, dev)
    actions = torch.empty(B, dtype=_I32, device=dev)
    _lib.call('gg_batch_sample_weighted', batch_states, w, wcode, rng, actions, B, N, _lib.stream_ptr(dev))
    return _check_drawn(actions, check)


def batch_sample_weighted_rows(boards, board_size, weights, rng, check=False):
    """The same draw for packed (int32 [B, 3N+1]) or tracked (int32 [B, 5N+1]) boards."""
    B, W = boards.shape
    N = int(board_size)
    planes = (W - 1) // N if N > 0 else 0
    if boards.dtype != _I32 or planes * N + 1 != W or planes not in (3, 5):
        raise ValueError('boards must be packed [B, 3N+1] or tracked [B, 5N+1] int32 for N = %d (got %s)' % (N, tuple(boards.shape)))
    w, wcode = _weights_tensor(weights, B, N, boards.device)
    actions = torch.empty(B, dtype=_I32, device=boards.device)
    _lib.call('gg_batch_sample_weighted_rows', boards, planes, w, wcode, rng, actions, B, N, _lib.stream_ptr(boards.device))
    return _check_drawn(actions, check)


def batch_random_action(batch_states, rng):
    """gogame.random_action (gym_go/gogame.py:395-404) per game: weights 1 - invalid_moves, i.e. uniform over the playable
    actions, through the weighted sampler (batch_sample_actions draws the same distribution with a cheaper kernel)."""
    B, C, N, _ = batch_states.shape
    ones = torch.ones((B, N * N + 1), dtype=torch.float32, device=batch_states.device)
    return batch_sample_weighted(batch_states, ones, rng)


# ---------------------------------------------------------------- batched symmetries on the device
# gogame.all_symmetries / random_symmetry (gym_go/gogame.py:340-382) for whole batches: one orientation per game or all
# eight, on byte planes (any channel count) and on packed / tracked boards.

def batch_symmetry(batch_images, orient=None, out=None):
    """uint8 [B, C, N, N] device tensor -> the view `orient[b]` (int32 [B], 0..7, composed as the reference does: bit 0
    flip the columns, bit 1 flip the rows, bit 2 rot90) of every image: [B, C, N, N]; orient=None: all eight views,
    [B, 8, C, N, N] in the order of all_symmetries (gg_batch_symmetry)."""
    B, C, N, N2 = batch_images.shape
    if N != N2:
        raise ValueError('images must be [B, C, N, N]')
    dev = batch_images.device
    shape = (B, C, N, N) if orient is not None else (B, 8, C, N, N)
    if out is None:
        out = torch.empty(shape, dtype=_U8, device=dev)
    elif tuple(out.shape) != shape:
        raise ValueError('out must be uint8 %s' % (shape,))
    if orient is not None:
        orient = _actions_tensor(orient, B, dev)
    _lib.call('gg_batch_symmetry', batch_images, orient, out, B, C, N, _lib.stream_ptr(dev))
    return out


def batch_symmetry_rows(boards, board_size, orient=None):
    """The same on packed (int32 [B, 3N+1]) / tracked (int32 [B, 5N+1]) boards: -> [B, W], or [B, 8, W] for all eight
    views (gg_batch_symmetry_rows).  A transformed tracked board is a valid tracked board."""
    B, W = boards.shape
    N = int(board_size)
    planes = (W - 1) // N if N > 0 else 0
    if boards.dtype != _I32 or planes * N + 1 != W or planes not in (3, 5):
        raise ValueError('boards must be packed [B, 3N+1] or tracked [B, 5N+1] int32 for N = %d (got %s)' % (N, tuple(boards.shape)))
    out = torch.empty((B, W) if orient is not None else (B, 8, W), dtype=_I32, device=boards.device)
    if orient is not None:
        orient = _actions_tensor(orient, B, boards.device)
    _lib.call('gg_batch_symmetry_rows', boards, planes, orient, out, B, N, _lib.stream_ptr(boards.device))
    return out


def batch_random_symmetry(batch_images, generator=None):
    """gogame.random_symmetry (gym_go/gogame.py:340-359) per game: -> (views [B, C, N, N], orient int32 [B]); the
    orientations come from torch's device generator (pass `generator` for reproducibility)."""
    B = batch_images.shape[0]
    orient = torch.randint(0, 8, (B,), dtype=_I32, device=batch_images.device, generator=generator)
    return batch_symmetry(batch_images, orient), orient


def symmetry_actions(actions, orient, board_size):
    """Where a move lands under the views above: action a of the ORIGINAL board -> the action that marks the same point
    on the view `orient` (the pass stays the pass).  int tensors / arrays [B] -> int32 tensor [B] on actions' device."""
    N = int(board_size)
    a = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions))
    o = orient if isinstance(orient, torch.Tensor) else torch.as_tensor(np.asarray(orient))
    a = a.to(torch.int64)
    o = o.to(device=a.device, dtype=torch.int64)
    sr, sc = torch.div(a, N, rounding_mode='floor'), a % N
    r1 = torch.where((o & 2) != 0, N - 1 - sr, sr)
    c1 = torch.where((o & 1) != 0, N - 1 - sc, sc)
    r = torch.where((o & 4) != 0, N - 1 - c1, r1)
    c = torch.where((o & 4) != 0, r1, c1)
    return torch.where(a >= N * N, a, r * N + c).to(_I32)


POLICY_DTYPES = {torch.bool: 1, torch.uint8: 1, torch.float16: 2, torch.bfloat16: 2, torch.float32: 4, torch.int32: 4}   # element bytes


def _policy_size(A):
    """N of a row of A = N*N + 1 elements with N in [2, 19]; ValueError otherwise."""
    N = int(round(math.sqrt(max(int(A) - 1, 0))))
    if N * N + 1 != A or not 2 <= N <= 19:
        raise ValueError('rows over the actions hold N*N + 1 elements with N in [2, 19] (got %d)' % A)
    return N


def batch_symmetry_policy(policy, orient, inverse=False, out=None):
    """Turn vectors over the actions - priors, legal masks, visit-count targets - with the board (gg_batch_symmetry_policy).
    policy: [B, A] of bool / uint8 / float16 / bfloat16 / float32 / int32, A = N*N + 1 with N in [2, 19]; orient: int [B], a
    tensor or an array (batch_symmetry's orientations, only orient & 7 is read).  With T = symmetry_actions(., orient[b], N):
    inverse=False gives out[b, T(a)] = policy[b, a] - the first N*N elements turned as batch_symmetry turns a one-plane image,
    the pass kept: a vector over the board becomes the vector over the view; inverse=True gives out[b, a] = policy[b, T(a)]:
    a vector over the view (what a network answers on oriented planes) comes back to the board.  Elements move as bit
    patterns.  out: a contiguous device tensor of policy's shape and dtype that does not overlap it; slices of larger
    tensors are fine on both sides, no alignment is needed.  Anything else raises ValueError before a device is touched.
    NumPy in gives NumPy out (not bfloat16).  One launch, no synchronisation."""
    is_np = not isinstance(policy, torch.Tensor)
    if is_np:
        policy = np.asarray(policy)
        if policy.dtype not in (np.bool_, np.uint8, np.float16, np.float32, np.int32):
            raise ValueError('policy must be bool, uint8, float16, float32 or int32 (got %s)' % policy.dtype)
    elif policy.dtype not in POLICY_DTYPES:
        raise ValueError('policy must be bool, uint8, float16, bfloat16, float32 or int32 (got %s)' % policy.dtype)
    if policy.ndim != 2:
        raise ValueError('policy must be [B, N*N + 1] (got %s)' % (tuple(policy.shape),))
    B, A = policy.shape
    N = _policy_size(A)
    _orient_arg(orient, B)
    if is_np:
        if out is not None:
            raise ValueError('out needs a device tensor as policy')
        policy = torch.from_numpy(np.ascontiguousarray(policy)).to(_device())
    elif not policy.is_cuda:
        raise ValueError('policy must be a device tensor or a NumPy array')
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != policy.dtype or tuple(out.shape) != (B, A)
                            or out.device != policy.device or not out.is_contiguous()):
        raise ValueError('out must be a contiguous %s [%d, %d] tensor on policy\'s device' % (policy.dtype, B, A))
    policy = policy.contiguous()
    es = POLICY_DTYPES[policy.dtype]
    if out is None:
        out = torch.empty((B, A), dtype=policy.dtype, device=policy.device)
    elif B and out.data_ptr() < policy.data_ptr() + B * A * es and policy.data_ptr() < out.data_ptr() + B * A * es:
        raise ValueError('out overlaps policy')
    o = _actions_tensor(orient, B, policy.device)
    _lib.call('gg_batch_symmetry_policy', policy, o, out, es, 1 if inverse else 0, B, N, _lib.stream_ptr(policy.device))
    return out.cpu().numpy() if is_np else out


def batch_draw_orient(rng):
    """One orientation per generator -> int32 [B] on rng's device (gg_batch_draw_orient): rng is rng_seed's int64 [B] device
    tensor, advanced in place by one step per row; orient[b] = the top three bits of the generator's output.  One launch."""
    if not isinstance(rng, torch.Tensor) or rng.dtype != _I64 or rng.dim() != 1 or not rng.is_contiguous():
        raise ValueError('rng must be a contiguous int64 [B] device tensor (gogame.rng_seed)')
    B = rng.shape[0]
    orient = torch.empty(B, dtype=_I32, device=rng.device)
    _lib.call('gg_batch_draw_orient', rng, orient, B, _lib.stream_ptr(rng.device))
    return orient


def selfplay_targets(record, games, moves):
    """The value target and the validity of recorded positions -> (z float32 [B], valid bool [B]), plain torch on the
    record's device.  record: a SelfPlay made with record_states=True (ValueError if record.states is None); games, moves:
    int [B], position i is move moves[i] of game games[i].  z = the outcome from the point of view of the player to move at
    that position: +outcome if black moves (plane 2 of the recorded state is clear), else -outcome; valid = moves <
    lengths[games]: the game had not ended there."""
    if record.states is None:
        raise ValueError('the record has no states: run puct_selfplay with record_states=True')
    t = lambda x, dev=None: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev)
    states = t(record.states)
    dev = states.device
    g, m = t(games, dev).to(_I64), t(moves, dev).to(_I64)
    if g.dim() != 1 or g.shape != m.shape:
        raise ValueError('games and moves must be int [B] (got %s, %s)' % (tuple(g.shape), tuple(m.shape)))
    white = states[g, m, govars.TURN_CHNL, 0, 0] != 0
    outcome = t(record.outcome, dev)[g].to(torch.float32)
    return torch.where(white, -outcome, outcome), m < t(record.lengths, dev)[g].to(_I64)


def selfplay_batch(record, games, moves, orient, dtype=torch.float16, life=False, ladder=False, outcome=False, area=False,
                   ownership=False, past=None):
    """Training samples from a self-play record, in one of the eight orientations each -> (planes [B, 16, N, N] of `dtype`,
    pi [B, A] float32, z float32 [B], valid bool [B]).  record: a SelfPlay of puct_selfplay(.., record_states=True)
    (ValueError if record.states is None); games, moves, orient: int [B] - sample i is the position before move moves[i] of
    game games[i], seen in view orient[i].  planes = batch_features of the recorded position with orient (one launch), pi =
    the recorded visit-count target turned with batch_symmetry_policy - both in the view; z, valid: selfplay_targets.  The
    eightfold augmentation of a sample is this call with orient = 0 .. 7.  Nothing synchronises; device tensors, or NumPy
    arrays for a NumPy record (through the device).  life=True: a fifth element, the life planes [B, 4, N, N] of the
    recorded positions in view orient and dtype `dtype` (batch_life, one launch more).  ladder=True: as the last element the
    ladder planes [B, 4, N, N] of the recorded positions in view orient and dtype `dtype` (batch_ladder, one launch more).
    outcome=True: as the last element, after those, the move-outcome planes [B, 12, N, N] of the recorded positions in view
    orient and dtype `dtype` (batch_move_planes, one launch more).  area=True: as the last element, after those, the area
    ownership planes [B, 3, N, N] of the recorded positions in view orient and dtype `dtype`, from the mover's view
    (batch_area_planes, one launch more).  ownership=True: two more elements after everything else, the KataGo-style
    targets owner int8 [B, N, N] and margin float32 [B] - batch_ownership of record.final_states[games] in view orient with
    side = the turn of the SAMPLED position (plane 2 of record.states[games, moves]): +1 = "ends up mine" for the player to
    move in the sample, margin = that player's area minus the other's at the end of the game (one launch more).  Komi is not
    in the record: subtract it from margin on black's samples and add it on white's.  For a game that had not ended after
    the recorded moves the final position is just the last one: `valid` and record.outcome == 0 tell.  past (None; an int T
    or a pair (T, moves)): after the area planes and before the ownership targets, the history planes [B, planes, N, N] of
    the sampled positions in view orient and dtype `dtype` - a StoneHistory of the B samples filled from
    record.states[games, moves - t] for t = T - 1 .. 1, oldest first, where moves - t >= 0 (T - 1 pushes), then one
    batch_past_planes launch with orient."""
    given = locals()   # (the sets that are on are read from it by the table's keywords)
    _feature_dtype(dtype)
    if past is not None:
        past = _past_request(past)
    z, valid = selfplay_targets(record, games, moves)
    is_np = not isinstance(record.states, torch.Tensor)
    B = z.shape[0]
    _orient_arg(orient, B)
    if is_np and dtype == torch.bfloat16:
        raise ValueError('NumPy has no bfloat16: pass a device record, or another dtype')
    dev = _device() if is_np else record.states.device
    t = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev)
    g, m = t(games).to(_I64), t(moves).to(_I64)
    positions = t(record.states)[g, m]
    planes = batch_features(positions, dtype, orient=orient)
    pi = batch_symmetry_policy(t(record.pi)[g, m].to(torch.float32), orient)
    res = (planes, pi, z.to(dev), valid.to(dev))
    for s in _LEAF_SETS:
        if given[s.key]:
            res += (s.batch(positions, dtype, orient=orient),)
    if past is not None:
        hist = StoneHistory(B, positions.shape[2], past[0], past[1], device=dev)
        all_states = t(record.states)
        for back in range(past[0] - 1, 0, -1):
            hist.push(all_states[g, (m - back).clamp(min=0)], m - back >= 0)
        res += (batch_past_planes(positions, hist, dtype, orient=orient),)
    if ownership:
        owner, margin = batch_ownership(t(record.final_states)[g], side=positions[:, govars.TURN_CHNL, 0, 0] != 0, orient=orient)
        res += (owner, margin.to(torch.float32))
    return tuple(x.cpu().numpy() for x in res) if is_np else res
