"""Every launch reaches the instantiation its board size and flags ask for (gymgo_amd/csrc/gg_host.h: by_rows, by_size, by_flag).

The failure this file is about: a launch sent to the wrong instantiation for some N or some runtime flag - a row capacity too
small for the board, FULL claimed for a board that does not fill its rows, the auto-reset or the given-moves form swapped.  Such
a launch computes something else on real positions, so every board size from 2 to 19 runs a table of (boards, plies) cells that
between them reach every kernel family of the rollout dispatch, and the other entry points at the batch sizes on either side
of their take-overs.

The library is sized for ONE compute unit (GYMGO_AMD_CUS=1, read once per process: a child process per board size), so that
every take-over is reached with a few hundred boards and the C oracle can replay everything.  What the oracle has no call for
(the env steps, the tracked and packed layouts, the policy draw) is compared bit for bit with the same calls in a second
child at the device's own CU count, where these batch sizes take the small-batch kernels test_gpu_parity.py pins; that
child runs once for all sizes.  The host part needs no GPU: it holds the table against bench.rollout_kernel_name, the mirror
of the dispatch, so that the table cannot silently stop covering a branch.
Reference loop: gym_go/envs/go_env.py:49-81 over gym_go/gogame.py:34-87.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = list(range(2, 20))
FULL_SIZES = (9, 13, 19)          # boards that fill their row capacity: the sixteen- and thirty-two-board kernels serve only these


def rollout_cells(n):
    """(boards, plies) of the byte-plane rollouts at ONE compute unit (gg_kernels.hip: use_lat, use_rollout5, use_multi_ply,
    use_ns16, small_launch), and the kernel family each is there for."""
    cells = [(24, 9),       # k_rollout_lat: up to 128 / 80 / 31 boards, from 3 / 3 - 4 / 8 plies
             (200, 5),      # k_rollout4: from 32 boards and two plies on, too many boards for k_rollout_lat, too few plies for k_rollout5
             (200, 9),      # k_rollout5 at 9 / 13 / 19 (more than 159 / 159 / 128 boards, from 8 plies), k_rollout4 elsewhere
             (12, 1),       # k_rollout2_w4: one or two plies on up to 16 (N <= 9) / 8 pairs
             (40, 1),       # k_rollout2, the one- and two-ply form: 20 pairs, fewer than the four groups of k_env_step16
             (30, 2),       # ... two plies below 32 boards (N <= 9: 15 pairs are k_rollout2_w4's)
             (256, 1)]      # k_env_step16 at 9 / 13 / 19: sixteen groups of sixteen boards
    # k_rollout2, the multi-ply form: three plies or more on fewer than 32 boards where k_rollout_lat does not take them - from 8
    # plies at N > 13, from 4 plies below 16 boards at N in 10 .. 13, never at N <= 9
    if n > 13:
        cells.append((30, 5))
    elif n > 9:
        cells.append((12, 3))
    return cells


def families_wanted(n):
    rcap = 9 if n <= 9 else 13 if n <= 13 else 19
    full = 'true' if n == rcap else 'false'
    want = {'k_rollout_lat<%d, %s, true, 0>' % (rcap, full), 'k_rollout4<%d, 0, false, %s, false, false>' % (rcap, full),
            'k_rollout2_w4<%d, %s>' % (rcap, full), 'k_rollout2<%d, true, false, %s>' % (rcap, full)}
    if n in FULL_SIZES:
        want |= {'k_rollout5<%d, 0>' % n, 'k_env_step16<%d, false>' % n}
    if n > 9:
        want.add('k_rollout2<%d, false, false, %s>' % (rcap, full))
    return want


@pytest.mark.parametrize('size', SIZES)
def test_the_table_names_every_kernel_family_reachable_at_this_size(size):
    import bench
    named = {bench.rollout_kernel_name(size, B, plies, 1) for B, plies in rollout_cells(size)}
    assert families_wanted(size) <= named, sorted(families_wanted(size) - named)
    if size <= 9:      # use_lat and use_multi_ply cover every launch of three plies or more: no cell can name the multi-ply k_rollout2
        for B in range(1, 300):
            for plies in range(3, 12):
                assert not bench.rollout_kernel_name(size, B, plies, 1).startswith('k_rollout2<9, false'), (B, plies)


SCRIPT = r'''
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import gogame, _lib
from oracle import c_oracle
ORACLE = sys.argv[1] == 'oracle'
CELLS = {int(n): [tuple(c) for c in cells] for n, cells in json.loads(sys.argv[2]).items()}     # rollout_cells(n), from the parent
SIZES = sorted(CELLS)
if ORACLE:
    assert _lib.lib().gg_device_cus() == 1
out = {}


def dig(*ts):
    h = hashlib.sha1()
    for t in ts:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def positions(N):
    """256 positions the oracle makes: three in four from the middle of a game, every fourth from games played on until most have
    ended (frozen boards: what auto_reset decides about)."""
    B0 = 256
    z = np.zeros((B0, 6, N, N), np.uint8)
    mid, _, _ = c_oracle.batch_rollout_mt(z, c_oracle.rng_seed(100 + N, B0), N * N // 2 + 3, True, 16)
    late, _, _ = c_oracle.batch_rollout_mt(z[:B0 // 4], c_oracle.rng_seed(200 + N, B0 // 4), 3 * N * N, False, 16)
    mid[3::4] = late
    return mid


def same(a, b, what):
    assert np.array_equal(a, b), what


def rollout(N, start, B, plies, auto, tracked, seed):
    st = torch.from_numpy(start[:B]).cuda()
    rng = gogame.rng_seed(B, seed, 0, 'cuda')
    rng0 = rng.cpu().numpy().view(np.uint64).copy()
    la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
    sd = torch.zeros(B, dtype=torch.int64, device='cuda')
    if tracked:
        tr = gogame.batch_track(st)
        gogame.batch_rollout_tracked(tr, rng, plies, auto, la, sd)
        got = gogame.batch_untrack(tr)
    else:
        gogame.batch_rollout(st, rng, plies, auto, la, sd)
        got = st
    if ORACLE:
        want, want_rng, want_last = c_oracle.batch_rollout(start[:B], rng0, plies, auto)
        what = (N, B, plies, auto, tracked)
        same(got.cpu().numpy(), want, ('boards',) + what)
        same(rng.cpu().numpy().view(np.uint64), want_rng, ('generators',) + what)
        same(la.cpu().numpy(), want_last, ('last actions',) + what)
    return dig(got, rng, la, sd)


for N in SIZES:
    start = positions(N)
    dev = torch.from_numpy(start).cuda()
    A = N * N + 1
    rs = np.random.default_rng(N)
    d = []
    # ---- the rollouts on byte planes and on tracked boards, both values of auto_reset
    for B, plies in CELLS[N]:
        for auto in (True, False):
            d.append(rollout(N, start, B, plies, auto, False, 7 * B + plies))
    for B, plies in ((24, 1), (24, 3), (24, 9), (16, 1), (16, 3), (200, 1), (200, 3), (200, 9)):
        for auto in (True, False):
            d.append(rollout(N, start, B, plies, auto, True, 9 * B + plies))
    # ---- next states: straight (6 pairs), pipelined (100 pairs), sixteen boards per wave (9 / 13 / 19 x 256), through a workspace
    acts = rs.integers(0, A, size=256).astype(np.int32)      # many of them illegal
    for B in (12, 200, 256):
        for canonical in (False, True):
            nxt, stat = gogame.batch_next_states(dev[:B], torch.from_numpy(acts[:B]).cuda(), canonical=canonical, check=False)
            outw, statw = torch.empty_like(dev[:B]), torch.empty(B, dtype=torch.int32, device='cuda')
            gogame.batch_next_states(dev[:B], torch.from_numpy(acts[:B]).cuda(), canonical=canonical, check=False, out=outw, status=statw,
                                     workspace=gogame.next_states_workspace(B, N, 'cuda'))
            if ORACLE:
                want, ws = c_oracle.batch_next_states(start[:B], acts[:B], canonical)
                same(nxt.cpu().numpy(), want, ('next states', N, B, canonical))
                same(stat.cpu().numpy(), ws, ('status', N, B, canonical))
                same(outw.cpu().numpy(), want, ('next states through a workspace', N, B, canonical))
                same(statw.cpu().numpy(), ws, ('status through a workspace', N, B, canonical))
            d.append(dig(nxt, stat, outw, statw))
    # ---- the invalid mask (pairs: 200 boards, sixteen per wave: 256) and the areas
    playable = start[:, 5, 0, 0] == 0
    for B in (200, 256):
        mask = gogame._invalid_mask_dev(dev[:B])
        if ORACLE:
            # plane 3 carries the ko point of the last move, which planes 0 - 2 cannot tell: the recomputed mask may lack
            # exactly that one point and nothing else
            m, p = mask.cpu().numpy(), playable[:B]
            assert not ((m[p] == 1) & (start[:B][p, 3] == 0)).any(), ('mask: extra points', N, B)
            assert not (((m[p] == 0) & (start[:B][p, 3] == 1)).sum(axis=(1, 2)) > 1).any(), ('mask: missing points', N, B)
        d.append(dig(mask))
    gb, gw = gogame.batch_areas(dev)
    if ORACLE:
        wb, ww = c_oracle.batch_areas(start)
        same(gb.cpu().numpy(), wb, ('black areas', N))
        same(gw.cpu().numpy(), ww, ('white areas', N))
    d.append(dig(gb, gw))
    # ---- children: padded, un-padded, packed
    k = 24
    kids = gogame.batch_children(dev[:k])
    ckids, coffs = gogame.batch_children(dev[:k], padded=False)
    pkids = gogame.batch_children_packed(gogame.batch_pack(dev[:k]))
    ukids = gogame.batch_unpack(pkids.reshape(k * A, -1), N).reshape(k, A, 6, N, N)
    if ORACLE:
        want = c_oracle.batch_children(start[:k])
        same(kids.cpu().numpy(), want, ('children', N))
        keep = np.concatenate([start[:k, 3].reshape(k, -1) == 0, np.ones((k, 1), bool)], axis=1)
        keep[start[:k, 5, 0, 0] == 1] = True
        same(coffs.cpu().numpy(), np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32), ('children offsets', N))
        same(ckids.cpu().numpy(), want[keep], ('un-padded children', N))
    assert torch.equal(ukids, kids), ('packed children', N)
    d.append(dig(kids, ckids, coffs, pkids))
    out['oracle%%d' %% N] = d
    # ---- what the oracle has no call for: the same calls at the device's own CU count take the small-batch kernels
    e = []
    for B in (12, 200, 256):
        given = gogame.batch_sample_actions(dev[:B], gogame.rng_seed(B, 5, 0, 'cuda'))
        for method in ('real', 'heuristic'):
            for moves in (given, None):
                st, rng = dev[:B].clone(), gogame.rng_seed(B, 6, 0, 'cuda')
                e.append(dig(*gogame.batch_env_step(st, moves, rng, 0.5, method, True), st, rng))
                pk = gogame.batch_pack(dev[:B])
                e.append(dig(*gogame.batch_env_step_packed(pk, moves, rng, 0.5, method, True), pk, rng))
    w = torch.rand((200, A), generator=torch.Generator().manual_seed(N)).cuda()
    for B in (24, 200):
        given = gogame.batch_sample_actions(dev[:B], gogame.rng_seed(B, 5, 0, 'cuda'))
        for method in ('real', 'heuristic'):
            for moves in (given, None):
                for observe in (True, False):
                    tr, rng = gogame.batch_track(dev[:B]), gogame.rng_seed(B, 8, 0, 'cuda')
                    obs = torch.zeros_like(dev[:B]) if observe else None
                    sd = torch.zeros(B, dtype=torch.int64, device='cuda')
                    e.append(dig(*gogame.batch_env_step_tracked(tr, moves, rng, 0.5, method, True, states_out=obs, steps_done=sd), tr, rng,
                                 sd, *([obs] if observe else [])))
        tr, rng = gogame.batch_track(dev[:B]), gogame.rng_seed(B, 9, 0, 'cuda')
        e.append(dig(*gogame.batch_env_step_tracked(tr, None, rng, 0.5, 'real', True, weights=w[:B]), tr, rng))
        e.append(dig(gogame.batch_sample_weighted(dev[:B], w[:B], gogame.rng_seed(B, 10, 0, 'cuda'))))
    for B in (200, 256):       # (256 boards of 9x9 / 13x13 / 19x19: sixteen per wave)
        tr = gogame.batch_track(dev[:B])
        pk = gogame.batch_pack(dev[:B])
        assert torch.equal(gogame.batch_untrack(tr), dev[:B]) and torch.equal(gogame.batch_unpack(pk, N), dev[:B]), (N, B)
        e.append(dig(tr, pk))
    for B, T in ((24, 3), (200, 3)):     # the replay per pair of boards, and (from 32 boards and two moves on) sixteen boards per wave
        moves = torch.from_numpy(rs.integers(0, A, size=(B, T)).astype(np.int32)).cuda()
        st, pk, tr = dev[:B].clone(), gogame.batch_pack(dev[:B]), gogame.batch_track(dev[:B])
        p1, p2, p3 = gogame.batch_play_moves(st, moves), gogame.batch_play_moves(pk, moves), gogame.batch_play_moves_tracked(tr, moves)
        assert torch.equal(p1, p2) and torch.equal(p1, p3), (N, B)
        assert torch.equal(gogame.batch_unpack(pk, N), st) and torch.equal(gogame.batch_untrack(tr), st), (N, B)
        e.append(dig(st, p1))
        nxt, stat = gogame.batch_next_states_packed(gogame.batch_pack(dev[:B]), moves[:, 0].contiguous(), check=False)
        e.append(dig(nxt, stat))
    for B, plies in ((200, 5), (30, 5), (30, 2)):
        for auto in (True, False):
            pk, rng = gogame.batch_pack(dev[:B]), gogame.rng_seed(B, 11, 0, 'cuda')
            gogame.batch_rollout_packed(pk, rng, plies, auto)
            e.append(dig(pk, rng))
    for B, plies in ((24, 9), (200, 9), (200, 3)):     # the policy draw: k_rollout_lat_pol, and k_rollout5_pol at 9 / 13 / 19 x 200 x 9
        for auto in (True, False):
            tr, rng = gogame.batch_track(dev[:B]), gogame.rng_seed(B, 12, 0, 'cuda')
            gogame.batch_rollout_tracked(tr, rng, plies, auto, policy='no_eye_fill')
            e.append(dig(tr, rng))
    out['same%%d' %% N] = e
torch.cuda.synchronize()
print('DIGESTS ' + json.dumps(out))
''' % ROOT


def _child(mode, sizes, cus):
    env = dict(os.environ)
    env.pop('GYMGO_AMD_CUS', None)
    if cus:
        env['GYMGO_AMD_CUS'] = str(cus)
    p = subprocess.run([sys.executable, '-c', SCRIPT, mode, json.dumps({n: rollout_cells(n) for n in sizes})], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('DIGESTS ')][-1]
    return json.loads(line[len('DIGESTS '):])


@pytest.fixture(scope='module')
def own_cu_count():
    """every size once at the device's own CU count: the small-batch kernels"""
    return _child('digests', SIZES, None)


@pytest.mark.gpu
@pytest.mark.parametrize('size', SIZES)
def test_every_launch_reaches_the_instantiation_of_its_size_and_flags(size, own_cu_count):
    got = _child('oracle', [size], 1)
    for key in ('oracle%d' % size, 'same%d' % size):
        want = own_cu_count[key]
        assert len(got[key]) == len(want)
        bad = [i for i, (a, b) in enumerate(zip(got[key], want)) if a != b]
        assert not bad, (key, bad)
