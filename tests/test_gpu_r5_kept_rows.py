"""-m gpu: what round 35 keeps from one use to the next in k_rollout5's 19x19 ply (gymgo_amd/csrc/gg_v5_kernel.h; gg_v5.h: GG_AB_EMPTY1,
GG_AB_MINPLACE1, GG_AB_DESC1, GG_AB_DRAWC1): the empty rows of a job's board are formed once per flood batch and every liberties pass
takes them as they are, the atari-join leaves M alone and the mask rule ORs its fill in, a job descriptor carries its board's row
offset, and the running draw counter starts one increment further on.  Crafted batches, every launch checked against the pinned C
oracle: boards with their invalid plane, generator states, last actions and played counters.

X is the mover's colour, Y the opponent's; q is the point the first ply is forced onto (the invalid plane leaves only q and the pass).
The library is sized for four compute units (GYMGO_AMD_CUS=4): 1 024 games put 32 boards into a wave, 545 put 18.  A COMB is a chain of
vertical bars joined alternately at the bottom and at the top, seeded at the top of its first bar (its foot): a down sweep of the flood
fills one bar and the joint below, the up sweep the next bar and the joint above, and so on - a comb of k bars keeps its flood batch
running k - 2 trips past the first closure test, which comes after down + up (sweeps(), a model of flood_jobs' schedule, says so).

Kinds of board:
  G3 / G4 / G5   X comb of 3 / 4 / 5 bars walled in by Y, one liberty at its far end; q at its foot has no empty neighbour: the mover's
                 group G is in atari behind the move and its lane runs on 1 / 2 / 3 trips.  On the top, the middle (across the seam of
                 the lane pair, rows 9 and 10) and the bottom rows.  The Y wall next to q is a large group with many liberties in rows
                 the later sweeps still grow into: its lane is settled by two liberties while G's runs on.
  OC3 / OC4 / OC5  Y comb walled in by X whose last liberty is q: captured whole (the stones of the board change for the next ply).
  OL4            Y comb with two liberties, q and its far end: it keeps one and leaves M.
  JSEAM          a Y stone on row 10 in atari, three X stones around it in atari (one on row 9, across the seam): q captures the
                 stone and every one of the three groups gets its second liberty - several groups joined in one ply.
  JLONG          the same with one X chain of six stones in a row: the join needs four or more trips (one step sideways per trip).
  CAP            q captures a Y stone and no X group is in atari: a capture with nothing to join.
  ONLY           an empty board with one valid point: no capture, no job.
  JOBS           the position of tests/test_gpu_r5.py that posts three jobs per board, forced onto its three-job points: 96 jobs in a wave
                 of 32 boards, the second job batch - board 31's jobs are all in it, job lane 63 holds an opponent job.
  PASS1 / PASS2  a board that passes on ply 1 and plays on / whose two players pass on plies 1 and 2 (odd and even).
  MOVE           a mid-game board that simply plays.
Waves cycle through six layouts: a mix with combs on boards 0, 1, 30 and 31 (17 in a wave of 18), G in job lane 0; one board that joins
among boards that only capture; boards that only capture; boards without a capture; JOBS on every board; 21 JOBS boards (63 jobs) in
front of a G comb, whose G job is job lane 63.
Cases: '1024-8', '545-8' (black and white to move, auto_reset on and off, byte planes without a workspace, with one that misses, with
one that hits, tracked boards), '1024-9', '1024-11', '545-11' and '1024-9+9' (two launches of 9, checked after each against 9 and 18
oracle plies; without a workspace and tracked), 'deep' (one launch of 200 plies on 1 056 mid-game boards).
The self-checks run on the CPU before the GPU is touched: by the oracle's own plies every kind does what its name says.
Reference loop: gym_go/envs/go_env.py:49-81 over gym_go/gogame.py:34-87.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import sys
sys.path.insert(0, '@ROOT@')
sys.path.insert(0, '@ROOT@/tests')
import numpy as np
from oracle import c_oracle
CASE = sys.argv[1]
N = 19
P = N * N
GAMMA = 0x9E3779B97F4A7C15
NBR = ((-1, 0), (1, 0), (0, -1), (0, 1))
on = lambda p: 0 <= p[0] < N and 0 <= p[1] < N

def group(stones, p):
    """the group of colour plane `stones` at p, and its liberties given the occupied points `occ`"""
    seen, todo = {p}, [p]
    while todo:
        a = todo.pop()
        for d in NBR:
            b = (a[0] + d[0], a[1] + d[1])
            if on(b) and stones[b] and b not in seen:
                seen.add(b); todo.append(b)
    return seen

def libs(s, g):
    occ = s[0] | s[1]
    return {(a[0] + d[0], a[1] + d[1]) for a in g for d in NBR if on((a[0] + d[0], a[1] + d[1])) and not occ[a[0] + d[0], a[1] + d[1]]}

def all_alive(s):
    for c in (0, 1):
        done = set()
        for p in zip(*np.nonzero(s[c])):
            if p not in done:
                g = group(s[c], p)
                done |= g
                assert libs(s, g), ('a group without a liberty', p)

def sweeps(m, seed):
    """flood_jobs' schedule on the colour plane m from `seed`: sweeps alternately down and up, each row run-filled from itself and the
    row before it; -> the sweeps up to the fixed point (the first closure test comes after two)"""
    f = np.zeros((N, N), bool); f[seed] = True
    whole = group(m, seed)
    def visit(r, prev):
        src = f[r] | ((f[prev] & m[r].astype(bool)) if 0 <= prev < N else False)
        row, c = np.zeros(N, bool), 0
        while c < N:
            if m[r, c]:
                e = c
                while e < N and m[r, e]: e += 1
                if src[c:e].any(): row[c:e] = True
                c = e
            else:
                c += 1
        f[r] = row
    n = 0
    while int(f.sum()) < len(whole):
        for r in (range(N) if n % 2 == 0 else range(N - 1, -1, -1)):
            visit(r, r - 1 if n % 2 == 0 else r + 1)
        n += 1
        assert n < 40
    return n

def comb(top, bot, c0, bars):
    """-> the points of the comb (foot first), the point at its far end's open side"""
    pts = []
    for i in range(bars):
        col = c0 + 2 * i
        rows = range(top, bot + 1) if i % 2 == 0 else range(bot, top - 1, -1)
        pts += [(r, col) for r in rows]
        if i + 1 < bars:
            pts.append((bot if i % 2 == 0 else top, col + 1))
    end = pts[-1]
    far = (end[0] + (1 if (bars - 1) % 2 == 0 else -1), end[1])     # beyond the last bar, in its direction
    return pts, far

def forced(s, mover, qs):
    s[2] = mover
    s[3] = 1
    for q in qs:
        s[3][q] = 0
    return s

def walled(path, keep_empty, colour, s):
    """every neighbour of `path` that is neither in it nor in keep_empty becomes a stone of `colour`"""
    inside = set(path) | set(keep_empty)
    for a in path:
        for d in NBR:
            b = (a[0] + d[0], a[1] + d[1])
            if on(b) and b not in inside:
                s[colour][b] = 1

BANDS = {'top': (1, 6), 'mid': (7, 12), 'bot': (12, 17)}

def comb_board(kind, band, mover):
    """kind 'G' / 'OC' / 'OL' + bars"""
    bars = int(kind[-1]); what = kind[:-1]
    top, bot = BANDS[band]
    pts, far = comb(top, bot, 3, bars)
    q = (top, 2)
    s = np.zeros((6, N, N), np.uint8)
    own = mover if what == 'G' else 1 - mover
    for p in pts: s[own][p] = 1
    if what == 'G':
        walled(pts + [q], [far], 1 - own, s)        # q has no empty neighbour: G's one liberty is the far end
    else:
        walled(pts, [q] + ([far] if what == 'OL' else []), 1 - own, s)
    assert not (s[0] & s[1]).any() and not s[0][q] and not s[1][q] and (what == 'OC' or (not s[0][far] and not s[1][far]))
    return forced(s, mover, [q]), q, pts, far

def join_board(kind, mover):
    X, Y = mover, 1 - mover
    s = np.zeros((6, N, N), np.uint8)
    r, c = 10, 9
    s[Y][r, c] = 1
    q = (r, c + 1)
    if kind == 'JSEAM':
        for a in ((r - 1, c), (r + 1, c), (r, c - 1)): s[X][a] = 1
        for b in ((r - 2, c), (r - 1, c - 1), (r + 1, c - 1), (r + 2, c)): s[Y][b] = 1
        atari = [(r - 1, c), (r + 1, c), (r, c - 1)]
    else:
        chain = [(r, c - 1 - i) for i in range(6)]
        for a in chain: s[X][a] = 1
        for a in chain:
            s[Y][a[0] - 1, a[1]] = 1; s[Y][a[0] + 1, a[1]] = 1
        s[X][r - 1, c] = s[X][r + 1, c] = 1
        atari = [chain[0]]
    return forced(s, mover, [q]), q, (r, c), atari

def cap_board(mover):
    X, Y = mover, 1 - mover
    s = np.zeros((6, N, N), np.uint8)
    r, c = 5, 12
    s[Y][r, c] = 1
    for a in ((r - 1, c), (r + 1, c), (r, c - 1)): s[X][a] = 1
    return forced(s, mover, [(r, c + 1)]), (r, c + 1), (r, c)

def dense(mover, plies, seed):
    s = np.zeros((1, 6, N, N), np.uint8)
    rng = c_oracle.rng_seed(seed, 1)
    s, rng, _ = c_oracle.batch_rollout(s, rng, plies, False)
    while s[0, 2, 0, 0] != mover or s[0, 5, 0, 0] or s[0, 4, 0, 0] or not (s[0, 3] == 0).any():
        s, rng, _ = c_oracle.batch_rollout(s, rng, 1, False)
    return s[0]

def jobs_boards(mover):
    """the three-job position of tests/test_gpu_r5.py with `mover` to move, forced onto its three-job points"""
    X, Y = mover, 1 - mover
    s0 = np.zeros((6, N, N), np.uint8)
    for r in range(N):
        for c in range(N):
            if (r + c) % 2 == 0 and not (r % 4 == 2 and c % 4 == 2):
                s0[Y, r, c] = 1
    inv = c_oracle.compute_invalid_moves(s0, Y)
    legal = (inv == 0) & (s0[Y] == 0)
    wn = np.zeros((N, N), np.int64)
    wn[1:] += s0[Y, :-1]; wn[:-1] += s0[Y, 1:]; wn[:, 1:] += s0[Y, :, :-1]; wn[:, :-1] += s0[Y, :, 1:]
    pts = [tuple(p) for p in np.argwhere(legal & (wn == 3))]
    assert len(pts) >= 32
    return forced(s0.copy(), mover, pts)        # (every three-job point stays valid: the draw takes the pass once in sixty)

def legal_for(s, mover, q):
    return c_oracle.compute_invalid_moves(s, 1 - mover)[q] == 0

def boards_per_wave(B):
    """gg_kernels.hip at four compute units (boards_per_wave5, use_rollout5)"""
    waves = (B + 31) // 32
    rounds = (waves + 31) // 32
    nb = min(32, ((B + rounds * 32 - 1) // (rounds * 32) + 1) // 2 * 2)
    assert B > 4 * 128, B
    return nb

def pool_of(mover):
    """-> boards by name, after the CPU self-checks of every crafted kind"""
    pool = {}
    for band in BANDS:
        for kind, trips in (('G3', 1), ('G4', 2), ('G5', 3), ('OC3', 1), ('OC4', 2), ('OC5', 3), ('OL4', 2)):
            s, q, pts, far = comb_board(kind, band, mover)
            all_alive(s)
            assert legal_for(s, mover, q), (kind, band)
            own = mover if kind[0] == 'G' else 1 - mover
            t = c_oracle.next_state(s, q[0] * N + q[1])
            if kind[0] == 'G':
                m = s[own].copy(); m[q] = 1
                g = group(t[own], q)
                assert g == set(pts) | {q} and libs(t, g) == {far}, (kind, band)       # G: the comb and q, in atari
                assert sweeps(m, q) - 2 >= trips, (kind, band, sweeps(m, q))
                wall = group(s[1 - own], (q[0] + 1, q[1]))                             # the Y group below q: large, many liberties
                assert len(libs(s, wall)) >= 4 and len({p[0] for p in wall}) >= 3
            else:
                assert sweeps(s[own], pts[0]) - 2 >= trips, (kind, band, sweeps(s[own], pts[0]))
                g = group(s[own], pts[0])
                assert g == set(pts)
                if kind[:2] == 'OC':
                    assert libs(s, g) == {q} and not t[own].any(), (kind, band)        # captured whole
                else:
                    assert libs(s, g) == {q, far} and libs(t, group(t[own], pts[0])) == {far}   # it keeps one: leaves M
            pool[kind + band] = s
    for kind in ('JSEAM', 'JLONG'):
        s, q, b, atari = join_board(kind, mover)
        all_alive(s)
        assert legal_for(s, mover, q)
        assert libs(s, group(s[1 - mover], b)) == {q}
        for a in atari:
            assert len(libs(s, group(s[mover], a))) == 1, (kind, a)                    # in atari before the capture
        t = c_oracle.next_state(s, q[0] * N + q[1])
        assert not t[1 - mover][b] and int(t[1 - mover].sum()) == int(s[1 - mover].sum()) - 1
        for a in atari:
            assert len(libs(t, group(t[mover], a))) >= 2 and q not in group(t[mover], a), (kind, a)   # joined, and not through G
        if kind == 'JSEAM':
            assert {a[0] for a in atari} >= {9, 10} and b[0] == 10                     # across the seam of the lane pair
        else:
            assert len(group(s[mover], atari[0])) >= 6
        pool[kind] = s
    s, q, b = cap_board(mover)
    all_alive(s)
    t = c_oracle.next_state(s, q[0] * N + q[1])
    assert not t[1 - mover][b] and legal_for(s, mover, q)
    for p in zip(*np.nonzero(s[mover])):
        assert len(libs(s, group(s[mover], p))) >= 2                                  # nothing to join
    pool['CAP'] = s
    pool['ONLY'] = forced(np.zeros((6, N, N), np.uint8), mover, [(9, 7)])
    pool['MOVE'] = dense(mover, P // 3, 81 + mover)
    pool['PASS1'] = forced(dense(mover, P // 4, 91 + mover).copy(), mover, [])
    two = np.zeros((6, N, N), np.uint8)
    two[mover] = 1
    two[mover][0, 0] = two[mover][N - 1, N - 1] = 0
    pool['PASS2'] = forced(two, mover, [])
    pool['JOBS'] = jobs_boards(mover)
    return pool

MIX = ['G3top', 'OC4mid', 'JSEAM', 'JLONG', 'G5bot', 'OL4top', 'MOVE', 'CAP', 'PASS1', 'PASS2', 'OC3top', 'G4mid', 'OC5bot', 'OL4mid',
       'G3mid', 'OC3bot', 'ONLY', 'G4top', 'OC4top', 'G5mid', 'OL4bot', 'OC5mid', 'G4bot', 'MOVE', 'JSEAM', 'G3bot', 'OC3mid', 'CAP',
       'OC5top', 'G5top']

def wave(w, nb):
    t = w % 6
    if t == 0:       # the mix: combs on boards 0, 1, nb - 2 and nb - 1; board 0's G job is job lane 0
        body = (MIX * 2)[2:nb - 2]
        return ['G4mid', 'OC4mid'] + body + ['OC5bot', 'G5mid' if nb == 32 else 'OC4top']
    if t == 1:       # one board joins, the others only capture
        return ['CAP'] * 7 + ['JSEAM'] + ['CAP'] * (nb - 8)
    if t == 2:       # captures, nothing to join
        return ['CAP'] * nb
    if t == 3:       # no capture anywhere in the wave
        return ['ONLY'] * nb
    if t == 4:       # three jobs a board: the second job batch
        return ['JOBS'] * nb
    return (['JOBS'] * 21)[:nb - 1] + ['G4top'] + ['MOVE'] * max(0, nb - 22)   # 63 jobs, then a G job: job lane 63

def batch(mover, B):
    pool = pool_of(mover)
    nb = boards_per_wave(B)
    kind = []
    for w in range((B + nb - 1) // nb):
        ks = wave(w, nb)
        assert len(ks) == nb, (w, len(ks))
        kind += ks
    kind = kind[:B]
    return np.stack([pool[k] for k in kind]), np.array(kind), nb

def check_batch(states, kind, rng0, mover, nb):
    """ply 1 by the oracle: the crafted boards play their q (or pass: the draw may pick the pass), and the waves are what they are named"""
    s1, _, l1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
    s2, _, l2 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 2, True)
    B = len(kind)
    capt = np.array([int(states[b, 1 - mover].sum()) > int(s1[b, 1 - mover].sum()) for b in range(B)])
    played = l1 < P
    for name in ('G', 'OC', 'OL', 'JSEAM', 'JLONG', 'CAP', 'JOBS'):
        idx = np.flatnonzero(np.char.startswith(kind, name))
        assert played[idx].sum() >= len(idx) // 4, (name, int(played[idx].sum()), len(idx))       # (half the draws take the pass)
    for name in ('OC', 'JSEAM', 'JLONG', 'CAP', 'JOBS'):
        idx = np.flatnonzero(np.char.startswith(kind, name) & played)
        assert capt[idx].all() or name == 'JOBS', name
    assert (l1[kind == 'PASS1'] == P).all() and (l2[kind == 'PASS1'] >= 0).all() and not s1[kind == 'PASS1', 5].any()
    assert (l1[kind == 'PASS2'] == P).all() and (l2[kind == 'PASS2'] == P).all()
    nw = B // nb
    for w in range(nw):
        sl = slice(w * nb, (w + 1) * nb)
        t = w % 6
        if t == 1 and played[w * nb + 7]:
            assert capt[sl].sum() == played[sl].sum()            # one joins, the others only capture
        if t == 2:
            assert capt[sl].sum() == played[sl].sum() and not np.char.startswith(kind[sl], 'J').any()
        if t == 3:
            assert not capt[sl].any()
    seen = {t: sum(1 for w in range(nw) if w % 6 == t and played[w * nb:(w + 1) * nb].any()) for t in range(6)}
    assert all(v >= 1 for v in seen.values()), seen
    # job lanes on ply 1: three jobs per JOBS board that plays; a wave of 32 with more than 64 has board 31's jobs in its second batch
    if nb == 32:
        full = [w for w in range(nw) if w % 6 == 4 and played[w * nb:w * nb + 32].sum() >= 23 and played[w * nb + 31]]
        lane63 = [w for w in range(nw) if w % 6 == 5 and played[w * nb:w * nb + 22].all()]
        print('self-check', CASE, mover, 'waves with a second job batch that holds board 31:', len(full), 'with G in job lane 63:', len(lane63))
        assert len(full) >= 2 and len(lane63) >= 1, (len(full), len(lane63))
    print('self-check', CASE, mover, len(kind), 'boards that capture on ply 1:', int(capt.sum()))

def steps_of(rng0, want_rng, most):
    with np.errstate(over='ignore'):
        steps = np.full(len(rng0), -1, np.int64)
        for k in range(most + 1):
            steps[(rng0 + np.uint64(k) * np.uint64(GAMMA)) == want_rng] = k
    assert (steps >= 0).all()
    return steps

if CASE == 'deep':
    B, LAUNCHES = 1056, (200,)
else:
    B = int(CASE.split('-')[0])
    LAUNCHES = tuple(int(x) for x in CASE.split('-')[1].split('+'))
FULL = CASE in ('1024-8', '545-8')
batches = {}
for mover in (0, 1):
    rng0 = c_oracle.rng_seed(3500 + mover, B)
    if CASE == 'deep':
        if mover:
            continue
        states, rng0, _ = c_oracle.batch_rollout_mt(np.zeros((B, 6, N, N), np.uint8), rng0.copy(), 150, True)
    else:
        states, kind, nb = batch(mover, B)
        check_batch(states, kind, rng0, mover, nb)
    batches[mover] = (states, rng0)
if len(sys.argv) > 2 and sys.argv[2] == 'selfcheck':
    print('R5 KEPT ROWS SELF-CHECK OK', CASE)
    sys.exit(0)

import torch
from gymgo_amd import gogame, _lib
assert _lib.lib().gg_device_cus() == 4
MODES = ('none', 'miss', 'hit', 'tracked') if FULL else ('none', 'tracked')
for mover, (states, rng0) in batches.items():
    for auto_reset in ((True,) if CASE == 'deep' else (True, False)):
        refs, s, r, total = [], states.copy(), rng0.copy(), 0
        for plies in LAUNCHES:
            s, r, last = c_oracle.batch_rollout_mt(s.copy(), r.copy(), plies, auto_reset)
            total += plies
            refs.append((s, r, last, steps_of(rng0, r, total)))
        for mode in MODES:
            st = torch.from_numpy(states).cuda()
            rng = torch.from_numpy(rng0.view(np.int64).copy()).cuda()
            tr = gogame.batch_track(st) if mode in ('tracked', 'hit') else None
            sd = torch.zeros((B,), dtype=torch.int64, device='cuda')
            # a zero workspace misses on every board with stones; a tracked copy of the batch holds every board stone for stone, with its M
            ws = None if mode in ('none', 'tracked') else (torch.zeros((B, 5 * N + 1), dtype=torch.int32, device='cuda') if mode == 'miss' else tr.clone())
            for plies, (want, want_rng, want_last, want_steps) in zip(LAUNCHES, refs):
                la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
                if mode == 'tracked':
                    gogame.batch_rollout_tracked(tr, rng, plies, auto_reset, la, sd)
                else:
                    gogame.batch_rollout(st, rng, plies, auto_reset, la, sd, workspace=ws)
                got = gogame.batch_untrack(tr).cpu().numpy() if mode == 'tracked' else st.cpu().numpy()
                tag = (CASE, mover, auto_reset, mode, plies)
                bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
                assert len(bad) == 0, (tag, len(bad), bad[:6].tolist())
                assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), tag
                assert np.array_equal(la.cpu().numpy(), want_last), tag
                assert np.array_equal(sd.cpu().numpy(), want_steps), tag
print('R5 KEPT ROWS OK', CASE)
'''.replace('@ROOT@', ROOT)


@pytest.mark.parametrize('case', ['1024-8', '545-8', '1024-9', '1024-11', '545-11', '1024-9+9', 'deep'])
def test_r5_kept_rows_crafted_batches(case):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT, case], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 KEPT ROWS OK %s' % case in p.stdout
