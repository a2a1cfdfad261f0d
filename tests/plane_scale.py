"""Thousands of game positions per board size for the plane kernels, and what is expected of them from the CHILDREN the pinned
C oracle builds - test infrastructure, CPU only: NumPy, SciPy, oracle.c_oracle.

The definitional expect modules (features_expect, outcome_expect, hash_expect) play every candidate in Python and have seen
some 42 positions per size.  What the move kernels claim is a statement about children - the stones a move captures, the
liberties and the size of its chain, the child's hash - and c_oracle.batch_children builds those children under the pinned
rules at thousands of parents per second.  reference() reads the claims off them in whole-array NumPy: one
scipy.ndimage.label call over all children of a chunk (its 3-D structure connects inside a board only), liberties as the
distinct (label, empty neighbour) pairs, hashes as an XOR reduction over a key table built here from the splitmix64 definition
of include/gymgo_amd.h.  The feature planes and group liberties of the parents come from the same labelling.
tests/test_plane_scale_host.py pins all of it against the definitional modules, so the reference does not define itself.

positions(N): oracle rollouts from the empty board at eight depths, plus the children that carry a ko point.
games(N): oracle games ply by ply with their histories, for the repeat mask - expected stone by stone, never by hash."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy import ndimage

from oracle import c_oracle

SIZES = tuple(range(2, 20))
CHUNK_BYTES = 96 << 20          # of oracle children held at a time (19x19: 784 KB per parent)
KO_CHILDREN = 64
_CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
_INSIDE = np.stack([np.zeros((3, 3), int), _CROSS, np.zeros((3, 3), int)])      # no link from board to board
_SHIFTS = ((np.s_[:, 1:, :], np.s_[:, :-1, :]), (np.s_[:, :-1, :], np.s_[:, 1:, :]),
           (np.s_[:, :, 1:], np.s_[:, :, :-1]), (np.s_[:, :, :-1], np.s_[:, :, 1:]))   # (a point, its neighbour) slices


def batch_of(N):
    """the first-generation boards per size"""
    return 2048 if N <= 9 else 1024 if N <= 13 else 512


def key_table():
    """uint64 [2, 19, 19]: key(c, y, x) = output number c * 361 + y * 19 + x + 1 of splitmix64 started at GG_HASH_SEED
    (include/gymgo_amd.h), whatever the board size."""
    with np.errstate(over='ignore'):
        z = np.uint64(0x676F2D6861736821) + np.uint64(0x9E3779B97F4A7C15) * np.arange(1, 2 * 361 + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return (z ^ (z >> np.uint64(31))).reshape(2, 19, 19)


KEYS = key_table()


def hash_planes(stones):
    """int64 [M] of stones [M, 2, N, N]: the XOR of the keys over the stones"""
    M, _, N, _ = stones.shape
    out = np.empty(M, np.uint64)
    keys = KEYS[:, :N, :N].reshape(-1)
    step = max(1, (32 << 20) // (16 * N * N))
    for lo in range(0, M, step):
        s = stones[lo:lo + step].reshape(min(step, M - lo), -1) != 0
        out[lo:lo + step] = np.bitwise_xor.reduce(np.where(s, keys, np.uint64(0)), axis=1)
    return out.view(np.int64)


def chains(stones, empty):
    """stones, empty bool [M, N, N] (stones of ONE colour per board) -> lab int32 [M, N, N]: the chain of the stone at each point,
    0 elsewhere, numbered through all boards; libs, size int64 [chains + 1]: per chain its liberties - the distinct (chain, empty
    neighbour) pairs - and its stones."""
    M, N, _ = stones.shape
    P = N * N
    lab, n = ndimage.label(stones, structure=_INSIDE)
    size = np.bincount(lab.reshape(-1), minlength=n + 1)
    size[0] = 0
    point = np.broadcast_to(np.arange(P).reshape(1, N, N), lab.shape)
    pairs = []
    for here, there in _SHIFTS:
        sel = (lab[here] > 0) & empty[there]
        pairs.append(lab[here][sel].astype(np.int64) * P + point[there][sel])
    pairs = np.unique(np.concatenate(pairs))
    return lab, np.bincount(pairs // P, minlength=n + 1), size


def dilate(x):
    """bool [M, N, N]: the points next to a point of x"""
    out = np.zeros_like(x)
    for here, there in _SHIFTS:
        out[here] |= x[there]
    return out


def flags(states):
    """(white to move, previous move was a pass, game over), bool [B] each"""
    return states[:, 2, 0, 0] != 0, states[:, 4, 0, 0] != 0, states[:, 5, 0, 0] != 0


def candidates(states):
    """bool [B, N, N]: empty, plane 3 clear, game not over"""
    over = flags(states)[2]
    return (states[:, 0] == 0) & (states[:, 1] == 0) & (states[:, 3] == 0) & ~over[:, None, None]


def parent_planes(states):
    """-> (features uint8 [B, 16, N, N], group liberties uint8 [B, N, N]) by the table of include/gymgo_amd.h"""
    B, _, N, _ = states.shape
    white, passed, over = flags(states)
    black, whites = states[:, 0] != 0, states[:, 1] != 0
    empty = ~(black | whites)
    lab, libs, _ = chains(np.concatenate([black, whites]), np.concatenate([empty, empty]))
    n = libs[lab[:B]] + libs[lab[B:]]                  # at a stone: the liberties of its chain; a point holds one colour at most
    w = white[:, None, None]
    own, opp = np.where(w, whites, black), np.where(w, black, whites)
    inv, live = states[:, 3] != 0, ~over[:, None, None]
    atari = empty & dilate(opp & (n == 1))
    f = np.zeros((B, 16, N, N), np.uint8)
    f[:, 0], f[:, 1] = own, opp
    for k in (1, 2, 3, 4):
        hit = (n == k) if k < 4 else (n >= 4)
        f[:, 1 + k], f[:, 5 + k] = own & hit, opp & hit
    f[:, 10] = empty & ~inv & live
    f[:, 11] = empty & inv & live & atari
    f[:, 12] = empty & ~inv & live & atari
    f[:, 13], f[:, 14], f[:, 15] = ~w, passed[:, None, None], 1
    return f, np.where(black | whites, np.minimum(n, 255), 0).astype(np.uint8)


def move_planes_of(raw):
    """uint8 [B, 12, N, N] from the counts int [B, 3, N, N] (not saturated): libs == 1, 2, 3, >= 4; captured == 1, 2, 3, >= 4;
    libs == 1 and size == 1, 2, 3, >= 4"""
    libs, cap, size = raw[:, 0], raw[:, 1], raw[:, 2]
    rows = []
    for v, gate in ((libs, True), (cap, True), (size, libs == 1)):
        rows += [(v == 1) & gate, (v == 2) & gate, (v == 3) & gate, (v >= 4) & gate]
    return np.stack(rows, axis=1).astype(np.uint8)


def reference(states, zero_suicides=True):
    """The expectation of the parents `states` uint8 [B, 6, N, N] from the oracle's children -> .cand bool [B, N, N], .raw int32
    [B, 3, N, N] (libs, captured, size of every candidate's move, not saturated), .counts uint8 [B, 3, N, N], .planes uint8
    [B, 12, N, N], .hashes int64 [B], .moves int64 [B, N*N + 1], .features uint8 [B, 16, N, N], .libs uint8 [B, N, N].
    zero_suicides: rule 4 of the header (a candidate whose chain has no liberty counts 0, 0, 0)."""
    states = np.ascontiguousarray(states, dtype=np.uint8)
    B, _, N, _ = states.shape
    P = N * N
    white = flags(states)[0]
    cand = candidates(states)
    raw = np.zeros((B, 3, P), np.int32)
    hashes = hash_planes(states[:, :2])
    moves = np.repeat(hashes[:, None], P + 1, axis=1)
    step = max(1, CHUNK_BYTES // ((P + 1) * 6 * P))
    for lo in range(0, B, step):
        par = states[lo:lo + step]
        kids = c_oracle.batch_children_mt(par)
        bi, ai = np.nonzero(cand[lo:lo + step].reshape(len(par), P))
        if not len(bi):
            continue
        ch = kids[bi, ai]                                         # [M, 6, N, N]: the child of every candidate
        del kids
        w = white[lo + bi][:, None, None]
        own, opp = np.where(w, ch[:, 1], ch[:, 0]) != 0, np.where(w, ch[:, 0], ch[:, 1]) != 0
        opp_before = np.where(white[lo:lo + step][:, None, None], par[:, 0], par[:, 1]).reshape(len(par), P).sum(axis=1)
        captured = opp_before[bi] - opp.reshape(len(bi), P).sum(axis=1)
        lab, libs, size = chains(own, ~(own | opp))
        mine = lab.reshape(len(bi), P)[np.arange(len(bi)), ai]   # the chain of the played stone
        assert (mine > 0).all()
        out = np.stack([libs[mine], captured, size[mine]], axis=1)
        if zero_suicides:
            out[libs[mine] == 0] = 0
        raw[lo + bi, :, ai] = out
        moves[lo + bi, ai] = hash_planes(ch[:, :2])
    raw = raw.reshape(B, 3, N, N)
    features, glibs = parent_planes(states)
    return SimpleNamespace(cand=cand, raw=raw, counts=np.minimum(raw, 255).astype(np.uint8), planes=move_planes_of(raw),
                           hashes=hashes, moves=moves, features=features, libs=glibs)


def stones_only(states):
    """a copy whose plane 3 holds only the stones: ko and suicide points become candidates"""
    out = np.array(states, dtype=np.uint8, copy=True)
    out[:, 3] = out[:, 0] | out[:, 1]
    return out


def capture_identity(ref):
    """What the capture plane must ALSO equal, from the children: plane 12 = a candidate whose move captures."""
    assert np.array_equal(ref.features[:, 12] != 0, ref.cand & (ref.raw[:, 1] > 0))


def ko_identity(states, ref, ref_open):
    """What the ko plane must ALSO equal on positions whose plane 3 is the rules' mask: plane 11 = a refused empty point of a
    live game that is no suicide (no suicide: libs > 0 on the copy whose plane 3 is the stones).  Its move takes one stone,
    and a board has one at most."""
    over = flags(states)[2][:, None, None]
    refused = (states[:, 0] == 0) & (states[:, 1] == 0) & (states[:, 3] != 0) & ~over
    ko = ref.features[:, 11] != 0
    assert np.array_equal(ko, refused & (ref_open.raw[:, 0] > 0))
    assert (ref_open.raw[:, 1][ko] == 1).all() and ko.reshape(len(states), -1).sum(axis=1).max(initial=0) <= 1


def rollouts(N, B, seed):
    """uint8 [B, 6, N, N]: uniform oracle play from the empty board (auto_reset off), an eighth of the boards each after
    (i + 1) * max(1, N^2 // 5) plies, i = 0 .. 7"""
    cur, rng = np.zeros((B, 6, N, N), np.uint8), c_oracle.rng_seed(seed, B)
    out = np.zeros_like(cur)
    for i in range(8):
        cur, rng, _ = c_oracle.batch_rollout_mt(cur, rng, max(1, N * N // 5), auto_reset=False)
        out[i * B // 8:(i + 1) * B // 8] = cur[i * B // 8:(i + 1) * B // 8]
    return out


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def _joined(a, b):
    return SimpleNamespace(**{k: np.concatenate([v, getattr(b, k)]) for k, v in vars(a).items()})


@functools.lru_cache(maxsize=None)
def positions(N, B=None, seed=None):
    """The positions of size N with their expectation, computed once -> .states uint8 [B', 6, N, N]: the rollouts (seed
    1000 + N; 2048 boards for N <= 9, 1024 for N <= 13, 512 above) and a second generation - up to KO_CHILDREN oracle children
    of candidates that capture one stone with one stone left on one liberty, the only positions that carry a ko point;
    .ref = reference(states); .open = stones_only(states), .ref_open = its reference; .first: the number of rollouts.
    capture_identity and ko_identity hold.  Read only."""
    B = batch_of(N) if B is None else B
    first = rollouts(N, B, 1000 + N if seed is None else seed)
    ref1 = reference(first)
    b, y, x = np.nonzero((ref1.raw[:, 0] == 1) & (ref1.raw[:, 1] == 1) & (ref1.raw[:, 2] == 1))
    pick = np.linspace(0, len(b) - 1, min(len(b), KO_CHILDREN)).astype(int) if len(b) else np.zeros(0, int)
    second, status = c_oracle.batch_next_states(first[b[pick]], (y[pick] * N + x[pick]).astype(np.int32))
    assert not status.any()
    states = np.concatenate([first, second])
    ref = _joined(ref1, reference(second)) if len(second) else ref1
    opened = stones_only(states)
    ref_open = reference(opened)
    capture_identity(ref)
    ko_identity(states, ref, ref_open)
    return _freeze(SimpleNamespace(N=N, first=B, states=states, ref=_freeze(ref), open=opened, ref_open=_freeze(ref_open)))


# ---------------------------------------------------------------- games for the repeat mask
GAME_SIZES = (4, 5, 6, 7, 9)
GAME_PLIES = {4: 64, 5: 100, 6: 120, 7: 150, 9: 200}
GAMES = 256
PLANT_EVERY = 4
# Uniform games repeat a position 3 to 12 times per size without the planted entries; at 9x9 all three such rows have index 4
# mod 5, where the cycle of counts_of would give them count -1 and the mask no hit of that kind: the cycle starts one later there.
COUNT_PHASE = {9: 1}


def _position_keys(stones):
    """a list of bytes, one per row of stones [M, 2, N, N]: the position stone by stone"""
    M = len(stones)
    packed = np.packbits(np.ascontiguousarray(stones != 0).reshape(M, -1), axis=1)
    return packed.view('V%d' % packed.shape[1]).reshape(M).tolist() if M else []


def counts_of(length, H, phase=0):
    """count[b]: the exact length, the length minus one, 0, H + 5, -1 by the row's index + phase (test_gpu_hash.COUNTS on real
    lengths)"""
    k = (np.arange(len(length)) + phase) % 5
    return np.select([k == 0, k == 1, k == 2, k == 3], [length, length - 1, 0, H + 5], -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def games(N, G=GAMES, T=None):
    """G oracle games of T plies from the empty board, one ply per call (uniform draws, auto_reset off, seed 300 + N); every
    (game, ply) board whose game is live is a row -> .states uint8 [M, 6, N, N].  A row's history: the earlier positions of its
    game and the row's own, and for every fourth row (.planted bool [M]) the position after the move the game played next - a
    repeat point whenever that was a board move, captures included; .history int64 [M, H] holds their hashes (hash_planes; zero
    beyond), H = T + 2; .count int32 [M] = counts_of(lengths); .game, .ply int [M]; .stones uint8 [G, T + 2, 2, N, N];
    .mask uint8 [M, N*N + 1]: candidates whose child, stone by stone, is among the first
    min(max(count, 0), H) entries (entries beyond a row's length are the empty board, which no child is); .mask_plain: the same
    with the planted entries left out.  Read only."""
    T = GAME_PLIES[N] if T is None else T
    P, H = N * N, T + 2
    cur, rng = np.zeros((G, 6, N, N), np.uint8), c_oracle.rng_seed(300 + N, G)
    seq = [cur]
    for _ in range(T + 1):
        cur, rng, _ = c_oracle.batch_rollout_mt(cur, rng, 1, auto_reset=False)
        seq.append(cur)
    seq = np.stack(seq, axis=1)                                    # [G, T + 2, 6, N, N]
    live = seq[:, :T, 5, 0, 0] == 0
    g, t = np.nonzero(live)
    M = len(g)
    states = seq[g, t]
    planted = (np.arange(M) % PLANT_EVERY == 0)
    length = (t + 1 + planted).astype(np.int32)
    game_hash = hash_planes(seq[:, :, :2].reshape(-1, 2, N, N)).reshape(G, T + 2)
    history = np.zeros((M, H), np.int64)
    keep = np.arange(H)[None, :] < length[:, None]
    history[keep] = game_hash[g][:, :H][keep]                      # row (g, t): the game's positions 0 .. t (and t + 1)
    count = counts_of(length, H, COUNT_PHASE.get(N, 0))
    valid = np.minimum(np.maximum(count, 0), H)
    # the expected masks, stone by stone: per game the first ply each position occurred at
    game_keys = _position_keys(seq[:, :, :2].reshape(-1, 2, N, N))
    first_seen = []
    for i in range(G):
        d = {}
        for ply, k in enumerate(game_keys[i * (T + 2):(i + 1) * (T + 2)]):
            d.setdefault(k, ply)
        first_seen.append(d)
    mask, plain = np.zeros((M, P + 1), np.uint8), np.zeros((M, P + 1), np.uint8)
    cand = candidates(states).reshape(M, P)
    step = max(1, CHUNK_BYTES // ((P + 1) * 6 * P))
    for lo in range(0, M, step):
        kids = c_oracle.batch_children_mt(states[lo:lo + step])
        bi, ai = np.nonzero(cand[lo:lo + step])
        keys = _position_keys(kids[bi, ai][:, :2])
        del kids
        for r, a, k in zip((lo + bi).tolist(), ai.tolist(), keys):
            ply = first_seen[g[r]].get(k)
            if ply is None:
                continue
            own = min(int(valid[r]), int(t[r]) + 1)                # the valid entries among the game's positions 0 .. t
            if ply < own:
                mask[r, a] = plain[r, a] = 1
            elif planted[r] and valid[r] >= t[r] + 2 and k == game_keys[g[r] * (T + 2) + t[r] + 1]:
                mask[r, a] = 1
    return _freeze(SimpleNamespace(N=N, T=T, H=H, states=states, game=g, ply=t, planted=planted, history=history, count=count,
                                   mask=mask, mask_plain=plain, stones=seq[:, :, :2]))
