"""Expected results of the symmetry-aware network I/O (gogame.batch_features(orient=), batch_symmetry_policy,
batch_draw_orient, PuctSearch(symmetry=), selfplay_batch) - test infrastructure, CPU only, NumPy only.  Written from the text
of include/gymgo_amd.h: orientation o flips the columns (bit 0), then the rows (bit 1), then rotates by 90 degrees (bit 2)."""
import numpy as np

import mc_expect as mc
from mc_puct_selfplay_expect import splitmix_step


def orient_image(x, o):
    """View o of an image whose last two axes are the board."""
    x = np.flip(x, -1) if o & 1 else x
    x = np.flip(x, -2) if o & 2 else x
    return np.rot90(x, axes=(-2, -1)) if o & 4 else x


def orient_images(x, orient):
    """Row b of x ([B, ..., N, N]) in view orient[b]."""
    return np.stack([orient_image(x[b], int(orient[b]) & 7) for b in range(len(x))]) if len(x) else x.copy()


def action_tables(N):
    """-> (forward, inverse) int64 [8, A]: forward[o, a] = T(a), the action that marks on view o the point action a marks on
    the board; inverse[o, T(a)] = a.  From the orientation of an image of point indices: the view holds at q the index it took
    from the board."""
    P = N * N
    fwd, inv = np.zeros((8, P + 1), np.int64), np.zeros((8, P + 1), np.int64)
    for o in range(8):
        src = orient_image(np.arange(P).reshape(N, N), o).reshape(P)    # view point q <- board point src[q]
        inv[o, :P] = src
        fwd[o, src] = np.arange(P)
        fwd[o, P] = inv[o, P] = P
    return fwd, inv


def turn_policy(p, orient, inverse=False):
    """gg_batch_symmetry_policy: p [B, A] -> out[b, T(a)] = p[b, a], or out[b, a] = p[b, T(a)] with inverse."""
    B, A = p.shape
    N = int(round((A - 1) ** 0.5))
    fwd, inv = action_tables(N)
    out = np.empty_like(p)
    for b in range(B):
        o = int(orient[b]) & 7
        out[b] = p[b, fwd[o]] if inverse else p[b, inv[o]]
    return out


def seeds(B, seed, first=0):
    """gogame.rng_seed(B, seed, first) as Python integers."""
    return [int(v) for v in mc.po_seed(seed, first + np.arange(B, dtype=np.int64))]


def draw_orient(rng):
    """gg_batch_draw_orient on a list of generator states -> (orient int32 [B], the generators afterwards)."""
    out, nxt = [], []
    for x in rng:
        x, u = splitmix_step(x)
        out.append(u >> 61)
        nxt.append(x)
    return np.array(out, np.int32), nxt


def wrapped(E, seed, first_row=0):
    """E'(planes, legal) = inverse_o(E(view_o(planes), view_o(legal))) with the orientations PuctSearch(symmetry=seed) draws:
    one generator per row handed out (global row first_row + b), one draw per call.  E and E' work on NumPy arrays:
    (planes [B, 16, N, N], legal bool [B, A]) -> (priors float32 [B, A], values float32 [B]).  E'.orients: the draws so far."""
    state = {}

    def evaluate(planes, legal):
        B = len(planes)
        if 'rng' not in state:
            state['rng'] = seeds(B, seed, first_row)
        o, state['rng'] = draw_orient(state['rng'])
        evaluate.orients.append(o)
        priors, values = E(orient_images(planes, o), turn_policy(legal, o))
        return turn_policy(np.asarray(priors, np.float32), o, inverse=True), np.asarray(values, np.float32)

    evaluate.orients = []
    return evaluate
