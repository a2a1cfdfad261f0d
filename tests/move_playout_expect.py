"""Expected results of gogame.batch_move_playouts (flat Monte Carlo), built from the C restatement under oracle/ (test
infrastructure, CPU only): every legal first move is played by the restatement's next_state, every playout from the child
is replayed whole with its job's generator (auto_reset off), scored with the restatement's areas and reduced per
(root, action) on the host."""
import numpy as np

from oracle import c_oracle
import playout_expect as px

GOLDEN_GAMMA = 0x9E3779B97F4A7C15   # splitmix64 increment
JOB_MUL = 0xD1342543DE82EF95        # job id multiplier of the seeding
KEYS = ('black_wins', 'white_wins', 'draws', 'unfinished', 'margin_sum', 'plies_sum')


def po_seed(base_seed, p):
    """Generator of global job p (po_seed of gg_po.h, gg_rng_seed(base_seed, first_game = p)): splitmix64's state after one
    step from base_seed ^ p * JOB_MUL, mod 2^64.  p: int or integer array -> uint64 array."""
    p = np.asarray(p, dtype=np.int64).astype(np.uint64)
    with np.errstate(over='ignore'):
        return (np.uint64(base_seed & (2 ** 64 - 1)) ^ (p * np.uint64(JOB_MUL))) + np.uint64(GOLDEN_GAMMA)


def legal_mask(roots):
    """bool [R, N*N + 1]: valid_moves (plane 3 clear, pass always) of every root, all False for a root whose game has ended."""
    roots = np.asarray(roots)
    R, _, N, _ = roots.shape
    valid = np.concatenate([roots[:, 3].reshape(R, N * N) == 0, np.ones((R, 1), bool)], axis=1)
    ended = roots[:, 5].reshape(R, -1).any(axis=1)
    valid[ended] = False
    return valid


def children_of(roots, legal):
    """The children of the legal pairs in row-major (root, action) order -> (r, a, children uint8 [T, 6, N, N])."""
    r, a = np.nonzero(legal)
    kids, status = c_oracle.batch_next_states(np.ascontiguousarray(roots, np.uint8)[r], a.astype(np.int32))
    assert not status.any()
    return r, a, kids


def expected(roots, K, max_plies, komi=0.0, base_seed=20260927, first_root=0):
    """-> dict of the outputs of batch_move_playouts ([R, A] NumPy arrays, legal included), every playout replayed."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    legal = legal_mask(roots)
    out = {'legal': legal}
    for k in KEYS:
        out[k] = np.zeros((R, A), np.int32 if k not in ('margin_sum', 'plies_sum') else np.int64)
    if not legal.any():
        return out
    r, a, kids = children_of(roots, legal)
    T = r.size
    st = np.repeat(kids, K, axis=0)
    jobs = (((first_root + r) * A + a)[:, None] * K + np.arange(K)[None, :]).reshape(-1)
    rng0 = po_seed(base_seed, jobs)
    fin, rng1, _ = c_oracle.batch_rollout_mt(st, rng0.copy(), max_plies, auto_reset=False)
    b, w = c_oracle.batch_areas_mt(fin)
    d = np.asarray(b, np.int64) - np.asarray(w, np.int64)
    x = d - komi
    ended = fin[:, 5, 0, 0] != 0
    per = lambda v: np.asarray(v, np.int64).reshape(T, K).sum(axis=1)
    vals = {'black_wins': per(x > 0), 'white_wins': per(x < 0), 'draws': per(x == 0), 'unfinished': per(~ended),
            'margin_sum': per(d), 'plies_sum': per(px.plies_from_rng(rng0, rng1))}
    for k in KEYS:
        out[k][r, a] = vals[k]
    return out


def flat_mc_choice(roots, res):
    """NumPy restatement of flat_mc_actions over results `res` (dict or MovePlayouts of NumPy arrays)."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    legal = np.asarray(get('legal'), bool)
    bw, ww = np.asarray(get('black_wins'), np.int64), np.asarray(get('white_wins'), np.int64)
    white = np.asarray(roots)[:, 2, 0, 0] != 0
    score = np.where(white[:, None], ww - bw, bw - ww)
    out = np.full(legal.shape[0], -1, np.int64)
    for i in range(legal.shape[0]):
        if legal[i].any():
            s = np.where(legal[i], score[i], np.iinfo(np.int64).min)
            out[i] = int(np.flatnonzero(s == s.max())[0])
    return out


KO_POINT = (1, 1)


def crafted_roots(N):
    """Hand-made roots of size N >= 5: [the empty board, a root whose last move was a pass (its pass child is terminal), a
    root with an active ko point at KO_POINT (white to move may not retake), a finished game]."""
    empty = np.zeros((6, N, N), np.uint8)
    passed = c_oracle.next_state(c_oracle.next_state(empty, (N // 2) * N + N // 2), N * N)   # black plays, white passes
    # black surrounds (1, 1) on three sides, white surrounds (1, 2); white plays into (1, 1), black captures it from (1, 2)
    ko = empty
    for y, x in [(0, 1), (0, 2), (1, 0), (1, 3), (2, 1), (2, 2), (N - 1, N - 1), (1, 1), (1, 2)]:
        ko = c_oracle.next_state(ko, y * N + x)
    assert ko[1, 1, 1] == 0 and ko[0, 1, 2] == 1 and ko[3, 1, 1] == 1 and ko[2].all()
    end = c_oracle.next_state(c_oracle.next_state(empty, N * N), N * N)
    assert passed[4].all() and not passed[5].any() and end[5].all()
    return np.stack([empty, passed, ko, end])


CAPTURE_ROWS = ('WWWWWW.',   # the white group on top has one liberty, (0, 6); black's row below it one too, (1, 6)
                'BBBBBB.',
                'WWWWWWW',
                '.......',
                'BBBBBBB',
                '.......',
                '.......')
CAPTURE_MOVE = 6             # black to move: (0, 6) captures the top group and wins the race


def capture_root():
    """A 7x7 root, black to move, where one move (CAPTURE_MOVE) captures a large group and decides the game."""
    N = len(CAPTURE_ROWS)
    st = np.zeros((6, N, N), np.uint8)
    for y, row in enumerate(CAPTURE_ROWS):
        for x, c in enumerate(row):
            st[0 if c == 'B' else 1, y, x] = c != '.'
    st[3] = c_oracle.compute_invalid_moves(st, 0)
    return st
