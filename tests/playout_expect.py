"""Expected results of gogame.batch_playouts, built from the C restatement under oracle/ (test infrastructure, CPU only):
every playout is replayed whole (roots repeated K times, the job's generator, auto_reset off), scored with the restatement's
areas and reduced per root on the host."""
import numpy as np
from scipy import ndimage

from oracle import c_oracle

C = 0x9E3779B97F4A7C15
C_INV = pow(C, -1, 2 ** 64)


def plies_from_rng(rng_before, rng_after):
    """Plies a playout played: the sampler adds C to the generator once per ply, so (after - before) / C mod 2^64."""
    d = np.asarray(rng_after, np.uint64) - np.asarray(rng_before, np.uint64)
    return (d * np.uint64(C_INV)).astype(np.int64)


def ownership(states):
    """Per point of each board [B, 6, N, N] -> uint8 [B, 2, N, N]: in black's / white's Tromp-Taylor area (a stone of that
    colour, or an empty region - 4-connected - that touches only that colour)."""
    B, _, N, _ = states.shape
    out = np.zeros((B, 2, N, N), np.uint8)
    for i in range(B):
        bl, wh = states[i, 0] != 0, states[i, 1] != 0
        empty = ~(bl | wh)
        lab, n = ndimage.label(empty)
        touch = []
        for col in (bl, wh):
            adj = np.zeros_like(col)
            adj[1:] |= col[:-1]
            adj[:-1] |= col[1:]
            adj[:, 1:] |= col[:, :-1]
            adj[:, :-1] |= col[:, 1:]
            t = np.zeros(n + 1, bool)
            t[lab[adj & empty]] = True
            t[0] = False
            touch.append(t[lab])
        out[i, 0] = bl | (touch[0] & ~touch[1])
        out[i, 1] = wh | (touch[1] & ~touch[0])
    return out


def job_seeds(base_seed, first_root, R, K):
    return c_oracle.rng_seed(base_seed, (first_root + R) * K)[first_root * K:]


def expected(roots, K, max_plies, komi=0.0, base_seed=20260927, first_root=0, with_ownership=False):
    """-> dict of the per-root outputs of batch_playouts (NumPy), every playout replayed by the restatement."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    st = np.repeat(roots, K, axis=0)
    rng0 = job_seeds(base_seed, first_root, R, K)
    fin, rng1, _ = c_oracle.batch_rollout_mt(st, rng0.copy(), max_plies, auto_reset=False)
    b, w = c_oracle.batch_areas_mt(fin)
    b, w = np.asarray(b, np.int64), np.asarray(w, np.int64)
    d = b - w
    x = d - komi
    ended = fin[:, 5, 0, 0] != 0
    per = lambda v: np.asarray(v, np.int64).reshape(R, K).sum(axis=1)
    out = {
        'black_wins': per(x > 0).astype(np.int32), 'white_wins': per(x < 0).astype(np.int32),
        'draws': per(x == 0).astype(np.int32), 'unfinished': per(~ended).astype(np.int32),
        'margin_sum': per(d), 'plies_sum': per(plies_from_rng(rng0, rng1)),
        'ownership': None,
    }
    if with_ownership:
        out['ownership'] = ownership(fin).astype(np.int32).reshape(R, K, 2, N, N).sum(axis=1).astype(np.int32)
    return out


def make_roots(N, R, seed, max_ply=200, step=8):
    """R positions of random play from the empty board, root r after (r * step) % (max_ply + step) plies (r = 0: the empty
    board), plus - as the last root - a game played to its end."""
    roots = np.zeros((R, 6, N, N), np.uint8)
    target = (np.arange(R) * step) % (max_ply + step)
    rng = c_oracle.rng_seed(seed, R)
    for t in range(0, int(target.max()), step):
        m = target > t
        roots[m], rng[m], _ = c_oracle.batch_rollout(roots[m], rng[m], step, auto_reset=False)
    end, _, _ = c_oracle.batch_rollout(np.zeros((1, 6, N, N), np.uint8), c_oracle.rng_seed(seed + 1, 1), 8 * N * N + 64,
                                       auto_reset=False)
    assert end[0, 5, 0, 0] == 1
    roots[-1] = end[0]
    return roots
