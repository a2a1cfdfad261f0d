"""-m gpu: the history input planes (gogame.StoneHistory, batch_past_planes[_tracked], past_planes, PuctSearch(past=) and its
loops, selfplay_batch(past=)) bit-exact against the definition tests/past_expect.py, whose premises tests/test_past_host.py
checks on the CPU.  Everything the kernels write is 0 / 1 or integer ring words: every comparison is exact.

The boards sit at different plies of the games of past_expect.games(N) (played by the oracle, passes and captures included);
a board's ring is filled by the pushes themselves, one position per launch, under a mask."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mc_expect as mc
import past_expect as pe
import plane_cases as pc

B11 = 11            # a ragged last wave at four boards per wave (2 x 4 + 3) and at two (5 x 2 + 1)
SENTINEL = 0xA5
COUNTS = (0, 1, 3, 99)      # per board, cut to the plies its game has behind it: none, some, and all of them (past H: the ring wraps)


def same(got, want, tag=''):
    got = mc.to_np(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
    assert len(bad) == 0, (tag, len(bad), 'rows', bad[:12].tolist())


def mixed(n):
    return ((np.arange(n) * 3 + 1) % 8).astype(np.int32)


def boards(N, B, lead=0):
    """B boards at different plies of different games -> [(the game's positions up to the board's own, oldest first)]."""
    gs = pe.games(N)
    return [gs[g].states[:k + 1] for g, k in pe.samples(N, B, lead)]


def pushes_of(seqs, counts):
    """How many of its earlier positions board b pushes: counts[b % len] cut to what it has."""
    return [min(counts[b % len(counts)], len(s) - 1) for b, s in enumerate(seqs)]


def fill(gogame, hist, seqs, npush, tracked=False, turn=None, check_masked=False):
    """Board b pushes its last npush[b] earlier positions, oldest first, one launch per step under the mask `step < npush[b]`;
    turn: orientations the pushed positions are turned by first (gogame.batch_symmetry).  check_masked: at every step the
    boards the mask leaves out keep every byte of ring and count."""
    import torch
    B = len(seqs)
    for step in range(max(npush) if npush else 0):
        on = np.array([step < n for n in npush])
        st = np.stack([s[len(s) - 1 - n + step] if step < n else s[-1] for s, n in zip(seqs, npush)])
        st = mc.to_dev(st)
        if turn is not None:
            st = gogame.batch_symmetry(st, turn)
        before = (hist.rows.clone(), hist.count.clone()) if check_masked else None
        mask = None if on.all() and step % 2 else (mc.to_dev(on) if step % 3 else on.astype(np.uint8))
        res = hist.push_tracked(gogame.batch_track(st), mask) if tracked else hist.push(st, mask)
        assert res is hist
        if check_masked and not on.all():
            off = mc.to_dev(~on)
            assert torch.equal(hist.rows[off], before[0][off]) and torch.equal(hist.count[off], before[1][off]), step
            assert bool((hist.count[~off] == before[1][~off] + 1).all()), step
    return hist


def want_ring(seqs, npush, H, N):
    rings = [pe.ring(s[len(s) - 1 - n:len(s) - 1], H, N) for s, n in zip(seqs, npush)]
    return np.stack([r[0] for r in rings]), np.array([r[1] for r in rings], np.int32)


def want_planes(seqs, npush, H, T, moves):
    return np.stack([pe.planes(pe.with_ring(s, n, H), T, moves) for s, n in zip(seqs, npush)])


# ---------------------------------------------------------------- push and planes at every size
@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_push_and_planes_byte_planes_and_tracked(N):
    import torch
    from gymgo_amd import gogame
    seqs = boards(N, B11)
    assert len({len(s) for s in seqs}) > 2
    cur = mc.to_dev(np.stack([s[-1] for s in seqs]))
    tr = gogame.batch_track(cur)
    npush = pushes_of(seqs, COUNTS)
    if N >= 3:
        assert 0 in npush and 1 in npush and max(npush) > pe.LARGEST_RING
    for i, T in enumerate((1, 2, 8)):
        for H in sorted({max(T - 1, 1), T + 2}):
            hist = fill(gogame, gogame.StoneHistory(B11, N, T, True, capacity=H), seqs, npush, tracked=bool((i + H) % 2),
                        check_masked=(T, H) in ((8, 7), (2, 4)))
            rows, count = want_ring(seqs, npush, H, N)
            same(hist.rows, rows, (N, T, H, 'ring'))
            same(hist.count, count, (N, T, H, 'count'))
            if T == 8 and H == 7:      # the other push form leaves the same ring
                other = fill(gogame, gogame.StoneHistory(B11, N, T, True, capacity=H), seqs, npush, tracked=not bool((i + H) % 2))
                assert torch.equal(other.rows, hist.rows) and torch.equal(other.count, hist.count)
            for moves in (True, False):
                h = hist
                if not moves:
                    h = gogame.StoneHistory(B11, N, T, False, capacity=H)
                    h.rows.copy_(hist.rows)
                    h.count.copy_(hist.count)
                assert h.planes == pe.plane_count(T, moves)
                want = want_planes(seqs, npush, H, T, moves)
                same(gogame.batch_past_planes(cur, h), want, (N, T, H, moves, 'bytes'))
                same(gogame.batch_past_planes_tracked(tr, h), want, (N, T, H, moves, 'tracked'))
            if T == 8 and H == 10:
                # reset under a mask: those boards forget, the others keep every byte
                m = np.arange(B11) % 3 == 1
                keep = (hist.rows.clone(), hist.count.clone())
                assert hist.reset(mc.to_dev(m)) is hist
                assert not bool(hist.rows[mc.to_dev(m)].any()) and not bool(hist.count[mc.to_dev(m)].any())
                assert torch.equal(hist.rows[mc.to_dev(~m)], keep[0][mc.to_dev(~m)]) and torch.equal(hist.count[mc.to_dev(~m)], keep[1][mc.to_dev(~m)])
                after = [0 if m[b] else n for b, n in enumerate(npush)]
                same(gogame.batch_past_planes(cur, hist), want_planes(seqs, after, H, T, True), (N, 'after reset'))
                hist.reset()
                same(gogame.batch_past_planes(cur, hist), want_planes(seqs, [0] * B11, H, T, True), (N, 'after reset of all'))
    # NumPy in gives NumPy out; one game given as its positions
    s = seqs[3]
    hist = fill(gogame, gogame.StoneHistory(1, N, 4, True), [s], [min(3, len(s) - 1)])
    got = gogame.batch_past_planes(s[-1:].copy(), hist)
    assert isinstance(got, np.ndarray) and np.array_equal(got[0], pe.planes(s, 4, True))
    for T, moves in ((8, True), (3, False)):
        got = gogame.past_planes(s.copy(), T, moves)
        assert isinstance(got, np.ndarray) and got.dtype == s.dtype and np.array_equal(got, pe.planes(s, T, moves)), (N, T, moves)
    same(gogame.past_planes(mc.to_dev(s), 8, True, dtype=torch.float16).to(torch.uint8)[None], pe.planes(s, 8, True)[None])


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_oriented_calls_and_turned_inputs(N):
    """The turned expectation with a different orient per board, and the plain call on inputs turned by batch_symmetry."""
    import torch
    from gymgo_amd import gogame
    seqs = boards(N, B11, lead=5)
    cur = mc.to_dev(np.stack([s[-1] for s in seqs]))
    orient = mixed(B11)
    assert set(orient & 7) == set(range(8))
    o = mc.to_dev(orient)
    for T, H, moves in ((8, 7, True), (2, 4, False), (5, 6, True)):
        npush = pushes_of(seqs, (99, 3, 1, 0, 6))
        hist = fill(gogame, gogame.StoneHistory(B11, N, T, moves, capacity=H), seqs, npush)
        plain = want_planes(seqs, npush, H, T, moves)
        want = pc.turned(plain, orient)
        same(gogame.batch_past_planes(cur, hist, orient=o), want, (N, T, 'oriented'))
        same(gogame.batch_past_planes_tracked(gogame.batch_track(cur), hist, orient=orient), want, (N, T, 'oriented, tracked'))
        same(gogame.batch_past_planes(cur, hist, orient=np.zeros(B11, np.int64)), plain, (N, T, 'orient 0'))
        # the plain call on the turned game
        turned_hist = fill(gogame, gogame.StoneHistory(B11, N, T, moves, capacity=H), seqs, npush, turn=o)
        same(gogame.batch_past_planes(gogame.batch_symmetry(cur, o), turned_hist), want, (N, T, 'turned inputs'))
    if N >= 3:
        assert (want != plain).any()


# ---------------------------------------------------------------- output forms
def room(n, dt, lead):
    """a buffer of sentinels and the `n` elements of dtype dt that start `lead` elements into it"""
    import torch
    size = torch.empty(0, dtype=dt).element_size()
    raw = torch.full(((lead + n) * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    return raw[lead * size:(lead + n) * size].view(dt), lambda: bool((raw[:lead * size] == SENTINEL).all()) and bool(
        (raw[(lead + n) * size:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_dtypes_sub_batches_between_sentinels_and_a_ring_of_garbage(N):
    import torch
    from gymgo_amd import gogame
    seqs = boards(N, B11, lead=9)
    cur = mc.to_dev(np.stack([s[-1] for s in seqs]))
    tr = gogame.batch_track(cur)
    T, H = 8, 7
    npush = pushes_of(seqs, (99, 2, 7, 0))
    hist = fill(gogame, gogame.StoneHistory(B11, N, T, True), seqs, npush)
    want = want_planes(seqs, npush, H, T, True)
    for dt in (torch.uint8, torch.float16, torch.bfloat16, torch.float32):
        got = gogame.batch_past_planes(cur, hist, dtype=dt)
        assert got.dtype == dt and tuple(got.shape) == (B11, 23, N, N)
        same(got.to(torch.float32), want.astype(np.float32), (N, dt))
        for first, nb, lead in ((0, 1, 1), (4, 3, 7), (8, 3, 20), (10, 1, 7)):
            sub = gogame.StoneHistory(nb, N, T, True)
            sub.rows.copy_(hist.rows[first:first + nb])
            sub.count.copy_(hist.count[first:first + nb])
            for x, fn in ((cur, gogame.batch_past_planes), (tr, gogame.batch_past_planes_tracked)):
                flat, untouched = room(nb * 23 * N * N, dt, lead)
                out = flat.view(nb, 23, N, N)
                assert fn(x[first:first + nb], sub, dtype=dt, out=out) is out
                same(out.to(torch.float32), want[first:first + nb].astype(np.float32), (N, dt, first, nb, lead))
                assert untouched(), (N, dt, first, nb, lead)
    # a ring of all-ones words: full planes at the positions that exist, nothing outside the board, nothing where none exists
    hist.rows.fill_(-1)
    got = mc.to_np(gogame.batch_past_planes(cur, hist))
    for b in range(B11):
        have = min(npush[b], H)
        assert (got[b, 2:2 + 2 * have] == 1).all() and not got[b, 2 + 2 * have:16].any(), (N, b)
    same(got[:, :2], want[:, :2], (N, 'position 0 is the board given'))
    flat, untouched = room(B11 * 23 * N * N, torch.uint8, 3)
    gogame.batch_past_planes_tracked(tr, hist, out=flat.view(B11, 23, N, N))
    assert untouched() and np.array_equal(mc.to_np(flat.view(B11, 23, N, N)), got)


# ---------------------------------------------------------------- later trips of the grid-stride loop
B_TRIPS = 533
TRIP_SIZES = (9, 13, 19)


def _trips_child(N):
    import torch
    from gymgo_amd import gogame, _lib
    assert _lib.lib().gg_device_cus() == 1
    seqs = boards(N, B_TRIPS, lead=2)
    cur = mc.to_dev(np.stack([s[-1] for s in seqs]))
    tr = gogame.batch_track(cur)
    T, H = 8, 7
    npush = pushes_of(seqs, (99, 0, 5, 1, 12, 3, 7))
    orient = mixed(B_TRIPS)
    for tracked in (False, True):
        hist = fill(gogame, gogame.StoneHistory(B_TRIPS, N, T, True), seqs, npush, tracked=tracked)
        rows, count = want_ring(seqs, npush, H, N)
        same(hist.rows, rows, (N, tracked, 'ring'))
        same(hist.count, count, (N, tracked, 'count'))
    want = want_planes(seqs, npush, H, T, True)
    turned = pc.turned(want, orient)
    for x, fn in ((cur, gogame.batch_past_planes), (tr, gogame.batch_past_planes_tracked)):
        for w, o, lead in ((want, None, 5), (turned, orient, 11)):
            flat, untouched = room(want.size, torch.uint8, lead)
            out = flat.view(want.shape)
            fn(x, hist, out=out, orient=o)
            same(out, w, (N, fn.__name__, lead))
            assert untouched()
    sl = slice(3, 3 + 257)
    sub = gogame.StoneHistory(257, N, T, False)
    sub.rows.copy_(hist.rows[sl])
    sub.count.copy_(hist.count[sl])
    same(gogame.batch_past_planes(cur[sl], sub, dtype=torch.float32).to(torch.uint8), want[sl, :16], (N, 'sub-batch'))
    torch.cuda.synchronize()
    print('TRIPS ' + json.dumps({'N': N, 'ok': True}))


@pytest.mark.gpu
@pytest.mark.parametrize('N', TRIP_SIZES)
def test_later_trips_of_the_grid_stride_loop(N):
    """533 boards with the library sized for ONE compute unit (GYMGO_AMD_CUS=1, a grid of 64 workgroups) in a child process:
    the mechanism of tests/test_gpu_plane_trips.py - pushes and planes on second and later trips, a ragged last group."""
    nbw = 4 if N <= 13 else 2
    assert (B_TRIPS + nbw - 1) // nbw > 2 * 64 and B_TRIPS % nbw == 1
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(N)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('TRIPS ')][-1]
    assert json.loads(line[len('TRIPS '):]) == {'N': N, 'ok': True}


# ---------------------------------------------------------------- the tree
R5 = 5
TREE_COUNTS = (0, 1, 3, 11, 10)     # pushes behind the roots: none, some, and more than the ring holds (H = 7)


def tree_roots(N):
    """R5 roots that have not ended, with their games up to them -> (seqs, npush)."""
    gs = pe.games(N)
    seqs = []
    for r in range(R5):
        game = gs[r % pe.GAMES]
        k = min(TREE_COUNTS[r] + 2 * (r % 2), len(game.actions) - 1)
        while game.states[k][5, 0, 0]:
            k -= 1
        seqs.append(game.states[:k + 1])
    return seqs, [min(c, len(s) - 1) for c, s in zip(TREE_COUNTS, seqs)]


def expect_leaves(gogame, search, pushed, H, T, moves):
    """The definition applied to (ring oldest -> newest, node 0 and the nodes on the leaf's path read back from links and
    boards, the leaf) for every row of the last select(): -> (want [rows, planes, N, N], live [rows])."""
    R, N, L = search._R, search._N, search._L or 1
    W = 5 * N + 1
    links = mc.to_np(search._links)[..., 0]
    leaf_id = mc.to_np(search._leaf_id)
    leaf = mc.to_np(gogame.batch_untrack(search._leaf))
    live = mc.to_np(search.live).reshape(-1)
    words = mc.to_np(search._boards).view(np.uint32)         # [R, capacity, W]: only the stone rows of path nodes are read

    def node(r, x):
        s = np.zeros((6, N, N), np.uint8)
        for c in range(2):
            s[c] = (words[r, x, c * N:(c + 1) * N, None] >> np.arange(N, dtype=np.uint32)[None, :]) & 1
        return s
    want = np.zeros((R * L, pe.plane_count(T, moves), N, N), np.uint8)
    depth = 0
    for i in range(R * L):
        if not live[i]:
            continue
        r, x, chain = i // L, int(leaf_id[i]), []
        assert 0 <= x <= search._C
        while x != 0:
            p = int(links[r, x])
            assert 0 <= p < x
            chain.append(p)
            x = p
        depth = max(depth, len(chain))
        ringed = pushed[r][max(0, len(pushed[r]) - H):]
        seq = list(ringed) + [node(r, p) for p in reversed(chain)] + [leaf[i]]
        want[i] = pe.planes(np.stack(seq), T, moves)
    return want, live, depth


@pytest.mark.gpu
@pytest.mark.parametrize('N', (5, 11, 19))
@pytest.mark.parametrize('leaves', (None, 3))
@pytest.mark.parametrize('more', (False, True))
def test_search_hands_out_the_true_past_of_its_leaves(N, leaves, more):
    """PuctSearch(past=) alone and after life, ladder, outcome and area with symmetry=: a dozen rounds, an advance in the
    middle, against the reconstruction from the tree."""
    import torch
    from gymgo_amd import gogame
    import test_gpu_symmetry_io as tsio
    T, H, moves = 8, 7, True
    seqs, npush = tree_roots(N)
    assert npush[0] == 0 and max(npush) > H
    roots = mc.to_dev(np.stack([s[-1] for s in seqs]))
    hist = fill(gogame, gogame.StoneHistory(R5, N, T, moves), seqs, npush)
    pushed = [list(s[len(s) - 1 - n:len(s) - 1]) for s, n in zip(seqs, npush)]
    E = tsio.on_device(tsio.point_evaluator)
    kw = dict(life=True, ladder=True, outcome=True, area=True, symmetry=31 + N) if more else {}
    rounds = 6
    search = gogame.PuctSearch(roots, rounds, komi=0.5, leaves=leaves, capacity=2 * rounds * (leaves or 1) + 2, features=torch.float16,
                               past=hist, **kw)
    deepest = 0
    for part in range(2):
        for t in range(rounds):
            res = search.select()
            assert len(res) == (7 if more else 3)
            past = res[-1]
            assert past.dtype == torch.float16 and tuple(past.shape) == (R5 * (leaves or 1), 23, N, N)
            want, live, depth = expect_leaves(gogame, search, pushed, H, T, moves)
            deepest = max(deepest, depth)
            if more:
                want = pc.turned(want, mc.to_np(search.orient))
                assert tuple(res[5].shape)[1] == 3 and tuple(res[4].shape)[1] == 12
            got = mc.to_np(past.to(torch.uint8))
            assert live.any() and np.array_equal(got[live], want[live]), (N, leaves, more, part, t, np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1) & live))
            search.backup(*E(res[0], res[1]))
        if part == 0:
            result = search._result()
            acts = gogame._best_legal(gogame._ON_DEVICE, result.legal, result.visits.to(torch.int64)).clone()
            acts[1] = -1                                 # one root stays where it is: nothing is pushed for it
            before = mc.to_np(search.root_states())
            count0 = mc.to_np(hist.count).copy()
            search.advance(acts, check=False)
            moved = mc.to_np(acts) != -1
            assert moved.any() and not moved.all()
            assert np.array_equal(mc.to_np(hist.count), count0 + moved)
            for r in range(R5):
                if moved[r]:
                    pushed[r].append(before[r])
            assert np.array_equal(mc.to_np(hist.count), [len(p) for p in pushed])
    assert deepest >= 2


def play_line(line, actions):
    """the oracle's next position of every root whose action is not -1, appended to its line"""
    from oracle import c_oracle
    cur = np.stack([l[-1] for l in line])
    acts = np.asarray(actions).astype(np.int64)
    nxt, status = c_oracle.batch_next_states(cur, np.where(acts < 0, cur.shape[-1] ** 2, acts))
    for r, a in enumerate(acts):
        if a >= 0:
            assert status[r] == 0
            line[r].append(nxt[r])


PLAY = dict(N=5, R=6, moves=40, iterations=4, komi=0.5)


class _Spy:
    """Every PuctSearch the loops make, and what their evaluator got: (past planes, leaf_id) per call."""

    def __init__(self, gogame, E):
        self.gogame, self.E, self.made, self.calls = gogame, E, [], []
        spy = self

        class Search(gogame.PuctSearch):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                spy.made.append(self)
        self.cls, self.orig = Search, gogame.PuctSearch

    def __enter__(self):
        self.gogame.PuctSearch = self.cls
        return self

    def __exit__(self, *exc):
        self.gogame.PuctSearch = self.orig

    def __call__(self, planes, legal, past):
        import torch
        self.calls.append((mc.to_np(past.to(torch.uint8)), mc.to_np(self.made[-1]._leaf_id).copy()))
        return self.E(planes, legal)


def check_root_rows(spy, roots, actions, iterations, tag):
    """Every row the evaluator got with leaf_id == 0 equals the definition over the game up to that move."""
    R, M = actions.shape
    line = [[roots[r]] for r in range(R)]
    assert len(spy.calls) == M * iterations
    seen = longest = 0
    for mv in range(M):
        for t in range(iterations):
            past, leaf_id = spy.calls[mv * iterations + t]
            for r in np.flatnonzero(leaf_id == 0):
                want = pe.planes(np.stack(line[r]), 8, True)
                assert np.array_equal(past[r], want), (tag, mv, t, r)
                seen += 1
                longest = max(longest, len(line[r]))
        play_line(line, actions[:, mv])
    assert seen >= M and longest > 8, (tag, seen, longest)
    return line


@pytest.mark.gpu
@pytest.mark.parametrize('reuse', (True, False))
def test_puct_play_keeps_the_history_across_moves(reuse):
    import torch
    from gymgo_amd import gogame
    import test_gpu_symmetry_io as tsio
    N, R, M, I, komi = (PLAY[k] for k in ('N', 'R', 'moves', 'iterations', 'komi'))
    roots = tsio.roots7(N)[:R]
    E = tsio.on_device(tsio.point_evaluator)
    kw = dict(c=0.6, komi=komi, capacity=64, features=torch.float16, reuse=reuse)
    with _Spy(gogame, E) as spy:
        actions, final = gogame.puct_play(mc.to_dev(roots), M, I, spy, past=(8, True), **kw)
    assert len(spy.made) == (1 if reuse else M + 1)
    assert len({id(s._past) for s in spy.made}) == 1 and spy.made[0]._past.capacity == 7
    line = check_root_rows(spy, roots, mc.to_np(actions), I, ('puct_play', reuse))
    same(final, np.stack([l[-1] for l in line]), 'the final states are the lines\' ends')
    assert np.array_equal(mc.to_np(spy.made[0]._past.count), [len(l) - 1 for l in line])
    # defaults: the same games without past=, an evaluator of two arguments
    plain = gogame.puct_play(mc.to_dev(roots), M, I, E, **kw)
    assert len(plain) == 2 and torch.equal(plain[0], actions) and torch.equal(plain[1], final)
    # a game that does not start here: the history as given
    K = 12
    given = gogame.StoneHistory(R, N, 8, True)
    for k in range(K):
        given.push(np.stack([l[min(k, len(l) - 1)] for l in line]), np.array([k < len(l) - 1 for l in line]))
    later = np.stack([l[min(K, len(l) - 1)] for l in line])
    with _Spy(gogame, E) as spy2:
        gogame.puct_play(mc.to_dev(later), 1, I, spy2, past=given, **kw)
    assert spy2.made[0]._past is given
    past, leaf_id = spy2.calls[0]
    for r in np.flatnonzero(leaf_id == 0):
        assert np.array_equal(past[r], pe.planes(np.stack(line[r][:K + 1]), 8, True)), r


@pytest.mark.gpu
def test_puct_selfplay_and_selfplay_batch():
    import torch
    from gymgo_amd import gogame
    import test_gpu_symmetry_io as tsio
    N, R, M, I, komi = (PLAY[k] for k in ('N', 'R', 'moves', 'iterations', 'komi'))
    roots = tsio.roots7(N)[:R]
    E = tsio.on_device(tsio.point_evaluator)
    kw = dict(c=0.6, komi=komi, capacity=64, sample_moves=4, seed=7, features=torch.float16, record_states=True)
    with _Spy(gogame, E) as spy:
        rec = gogame.puct_selfplay(mc.to_dev(roots), M, I, spy, past=(8, True), **kw)
    actions, states = mc.to_np(rec.actions), mc.to_np(rec.states)
    line = check_root_rows(spy, roots, actions, I, 'puct_selfplay')
    for r in range(R):       # the lines are the recorded game
        n = int(mc.to_np(rec.lengths)[r])
        assert len(line[r]) == n + 1 and np.array_equal(np.stack(line[r]), states[r, :n + 1] if n < M else
                                                        np.concatenate([states[r], mc.to_np(rec.final_states)[r][None]]))
    plain = gogame.puct_selfplay(mc.to_dev(roots), M, I, E, **kw)
    assert all(torch.equal(getattr(plain, k), getattr(rec, k)) for k in rec._fields)
    # selfplay_batch(past=): every recorded position once, and a second time in another view
    games, moves = np.tile(np.repeat(np.arange(R), M), 2), np.tile(np.arange(M), 2 * R)
    orient = mixed(2 * R * M)
    orient[R * M:] += 3
    assert len(games) == 480 and set(orient & 7) == set(range(8))
    old = gogame.selfplay_batch(rec, games, moves, orient)
    off = gogame.selfplay_batch(rec, games, moves, orient, past=None)
    full = gogame.selfplay_batch(rec, games, moves, orient, past=(8, True))
    assert len(old) == len(off) == 4 and len(full) == 5
    assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(off, old))
    assert all(torch.equal(x, y) for x, y in zip(full[:4], old))
    want = np.stack([pe.planes(states[g, max(0, m - 7):m + 1], 8, True) for g, m in zip(games, moves)])
    assert full[4].dtype == torch.float16
    same(full[4].to(torch.uint8), pc.turned(want, orient), 'the past planes of the sampled positions')
    short = gogame.selfplay_batch(rec, games, moves, orient, dtype=torch.uint8, past=3)
    want3 = np.stack([pe.planes(states[g, max(0, m - 2):m + 1], 3, False) for g, m in zip(games, moves)])
    same(short[4], pc.turned(want3, orient), 'T = 3 without moves')
    # after the area planes, before the ownership targets
    seven = gogame.selfplay_batch(rec, games, moves, orient, area=True, ownership=True, past=(8, True))
    assert len(seven) == 8 and tuple(seven[4].shape) == (480, 3, N, N) and torch.equal(seven[5], full[4])
    assert seven[6].dtype == torch.int8 and seven[7].dtype == torch.float32
    # a NumPy record gives NumPy samples
    rec_np = type(rec)(*[mc.to_np(x) for x in rec])
    np_full = gogame.selfplay_batch(rec_np, games[:9], moves[:9], orient[:9], past=(8, True))
    assert all(isinstance(x, np.ndarray) for x in np_full) and np.array_equal(np_full[4], mc.to_np(full[4])[:9].astype(np_full[4].dtype))


@pytest.mark.gpu
def test_defaults_leave_the_search_as_it_was():
    """past=None: tuples of the old lengths with the old bytes, and the same tree with and without the history planes."""
    import torch
    from gymgo_amd import gogame
    import test_gpu_symmetry_io as tsio
    N = 9
    seqs, npush = tree_roots(N)
    roots = mc.to_dev(np.stack([s[-1] for s in seqs]))
    hist = fill(gogame, gogame.StoneHistory(R5, N, 8, False), seqs, npush)
    E = tsio.on_device(tsio.point_evaluator)
    a = gogame.PuctSearch(roots, 5, komi=0.5, leaves=2, features=torch.float16)
    b = gogame.PuctSearch(roots, 5, komi=0.5, leaves=2, features=torch.float16, past=hist)
    for t in range(5):
        ra, rb = a.select(), b.select()
        assert len(ra) == 2 and len(rb) == 3 and torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
        assert tuple(rb[2].shape) == (R5 * 2, 16, N, N)
        a.backup(*E(*ra))
        b.backup(*E(*rb[:2]))
    ta, tb = a.result(tree=True), b.result(tree=True)
    assert torch.equal(ta.visits, tb.visits) and torch.equal(ta.tree.parent, tb.tree.parent) and torch.equal(ta.tree.visits, tb.tree.visits)
    res = gogame.batch_puct(roots, 4, lambda p, l, h: E(p, l), komi=0.5, features=torch.float16, past=hist)
    ref = gogame.batch_puct(roots, 4, E, komi=0.5, features=torch.float16)
    assert torch.equal(res.visits, ref.visits)
    acts = gogame.puct_actions(roots, 4, lambda p, l, h: E(p, l), komi=0.5, features=torch.float16, past=hist)
    assert torch.equal(acts, gogame.puct_actions(roots, 4, E, komi=0.5, features=torch.float16))
    one = gogame.puct(roots[0], 4, lambda p, l, h: E(p, l), komi=0.5, features=torch.float16,
                      past=fill(gogame, gogame.StoneHistory(1, N, 8, False), seqs[:1], npush[:1]))
    assert torch.equal(one.visits, ref.visits[0])


if __name__ == '__main__':
    _trips_child(int(sys.argv[1]))
