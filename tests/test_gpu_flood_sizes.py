"""Positions that make a flood work as hard as the board allows (tests/flood_cases.py: board-filling snakes captured, put in
atari, joined, refused as suicide, and the corridor a capture leaves; spirals, serpentines, combs) through every step and rollout
kernel at EVERY board size from 2 to 19, bit for bit against the pinned C oracle.

The failure this file is about: a flood that is right on the groups random play makes - none deeper than 23 vertical steps at
19x19 - and wrong on a group 144 steps deep: a sweep too few, a run fill whose carry leaves the board in an instantiation whose
rows are wider than the board (N = 2 .. 8 in 9 rows, 10 .. 12 in 13, 14 .. 18 in 19), a closure test that is wrong for the rows
below the board, a class patch that is wrong for a capture of a hundred stones.

As in tests/test_gpu_dispatch_sizes.py the library is sized for ONE compute unit (GYMGO_AMD_CUS=1, a child process per board
size), so that the cells of its rollout_cells(N) reach every kernel family with a few hundred boards.  Every launch starts from
the first B boards of flood_cases.batch(N) - three crafted boards, then a random one of the dispatch test, so a wave holds lanes
that sweep many times next to lanes that are done at once - and board b always draws from generator (flood_cases.SEED, b):
tests/test_flood_cases_host.py asserts on the CPU that every launch plays the forced points.  Only the eye-aware draw, for which
the oracle has no call, is compared with the same launch at the device's own CU count.
Reference loop: gym_go/envs/go_env.py:49-81 over gym_go/gogame.py:34-87.
"""
import hashlib
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

import flood_cases as fc
from test_gpu_dispatch_sizes import rollout_cells

SIZES = list(fc.SIZES)
KOMI = 0.5


def _dig(*ts):
    h = hashlib.sha1()
    for t in ts:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def _policy_digests(N):
    """the eye-aware draw (a snake's teeth are one-point eyes): k_rollout_lat_pol, and k_rollout5_pol at 9 / 13 / 19 x 200 x 9"""
    import torch
    from gymgo_amd import gogame
    dev = torch.from_numpy(fc.batch(N).states).cuda()
    d = []
    for B, plies in fc.POLICY_CELLS:
        for auto in (True, False):
            tr, rng = gogame.batch_track(dev[:B]), gogame.rng_seed(B, fc.SEED, 0, 'cuda')
            la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
            gogame.batch_rollout_tracked(tr, rng, plies, auto, la, policy='no_eye_fill')
            d.append(_dig(tr, rng, la))
    return d


def _replay(start, moves):
    """gg_batch_play_moves by the oracle's next_state: a game stops at its first move that is out of range, on an invalid point
    or made after the game has ended, and keeps the state before that move -> (states, played)"""
    from oracle import c_oracle
    B, _, N, _ = start.shape
    cur, played, live = start.copy(), np.zeros(B, np.int32), np.ones(B, bool)
    for t in range(moves.shape[1]):
        a = moves[:, t]
        live &= (cur[:, 5, 0, 0] == 0) & (a >= 0) & (a <= N * N)
        nxt, status = c_oracle.batch_next_states(cur, np.where(live, a, N * N))
        live &= status == 0
        cur[live] = nxt[live]
        played += live
    return cur, played


def _oracle_child(N):
    import torch
    from gymgo_amd import gogame, _lib
    from oracle import c_oracle
    from test_gpu_env import _ref_reward
    assert _lib.lib().gg_device_cus() == 1
    b = fc.batch(N)
    start, kinds = b.states, b.kind
    dev = torch.from_numpy(start).cuda()
    A, B0 = N * N + 1, fc.BATCH
    forced = b.q >= 0
    rng_all = c_oracle.rng_seed(fc.SEED, B0)

    def same(got, want, *what, rows=None):
        """rows: the boards of the batch the rows of `got` belong to (default: the first ones), to name their kinds"""
        if torch.is_tensor(got):
            got = got.cpu().numpy()
        if got.dtype == np.int64 and want.dtype == np.uint64:
            got = got.view(np.uint64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        where = bad[:8] if rows is None else np.asarray(rows)[bad[:8]]
        assert len(bad) == 0, (N,) + what + (len(bad), where.tolist(), [kinds[i] for i in where])

    # ---- rollouts: byte planes (every cell of the dispatch table), tracked boards, packed boards; both values of auto_reset
    def rollout(B, plies, auto, layout):
        st, rng = dev[:B].clone(), gogame.rng_seed(B, fc.SEED, 0, 'cuda')
        same(rng, rng_all[:B], 'generators before', layout, B)
        la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
        want, want_rng, want_last = c_oracle.batch_rollout(start[:B], rng_all[:B], plies, auto)
        what = (layout, B, plies, auto)
        if layout == 'tracked':
            tr = gogame.batch_track(st)
            gogame.batch_rollout_tracked(tr, rng, plies, auto, la)
            got = gogame.batch_untrack(tr)
            # liberty classes are a function of the position: a snake left in atari is in the one-liberty class
            same(tr, gogame.batch_track(torch.from_numpy(want).cuda()).cpu().numpy(), 'tracked words', *what)
        elif layout == 'packed':
            pk = gogame.batch_pack(st)
            gogame.batch_rollout_packed(pk, rng, plies, auto, la)
            got = gogame.batch_unpack(pk, N)
        else:
            gogame.batch_rollout(st, rng, plies, auto, la)
            got = st
        same(got, want, 'boards', *what)
        same(rng, want_rng, 'generators', *what)
        same(la, want_last, 'last actions', *what)

    for auto in (True, False):
        for B, plies in rollout_cells(N):
            rollout(B, plies, auto, 'bytes')
        for B, plies in fc.TRACKED_CELLS:
            rollout(B, plies, auto, 'tracked')
        for B, plies in fc.PACKED_CELLS:
            rollout(B, plies, auto, 'packed')

    # ---- given moves: q on every forced board, elsewhere what the oracle draws (on a finished board: drawn after its reset)
    want1, rng1, last1 = c_oracle.batch_rollout(start, rng_all, 1, True)
    acts = np.where(forced, b.q, last1).astype(np.int32)
    acts_dev = torch.from_numpy(acts).cuda()
    for B in (12, 200, 256):       # straight (6 pairs), pipelined (100 pairs), sixteen boards per wave (9 / 13 / 19 x 256)
        for canonical in (False, True):
            nxt, stat = gogame.batch_next_states(dev[:B], acts_dev[:B], canonical=canonical, check=False)
            outw, statw = torch.empty_like(dev[:B]), torch.empty(B, dtype=torch.int32, device='cuda')
            gogame.batch_next_states(dev[:B], acts_dev[:B], canonical=canonical, check=False, out=outw, status=statw,
                                     workspace=gogame.next_states_workspace(B, N, 'cuda'))
            want, ws = c_oracle.batch_next_states(start[:B], acts[:B], canonical)
            assert (ws[forced[:B]] == 0).all()
            same(nxt, want, 'next states', B, canonical)
            same(stat, ws, 'status', B, canonical)
            same(outw, want, 'next states through a workspace', B, canonical)
            same(statw, ws, 'status through a workspace', B, canonical)
    post, post_status = c_oracle.batch_next_states(start, acts, False)
    post[post_status != 0] = start[post_status != 0]
    for B in (24, 200):            # per pair of boards, and (from 32 boards on) sixteen boards per wave
        nxt, stat = gogame.batch_next_states_packed(gogame.batch_pack(dev[:B]), acts_dev[:B], check=False)
        same(stat, post_status[:B], 'packed status', B)
        ok = post_status[:B] == 0
        same(gogame.batch_unpack(nxt, N).cpu().numpy()[ok], post[:B][ok], 'packed next states', B, rows=np.flatnonzero(ok))
        moves = np.concatenate([acts[:B, None], np.random.default_rng(N + B).integers(0, A, size=(B, 2)).astype(np.int32)], axis=1)
        want, want_played = _replay(start[:B], moves)
        assert (want_played[forced[:B]] >= 1).all()
        mv = torch.from_numpy(moves).cuda()
        st, pk, tr = dev[:B].clone(), gogame.batch_pack(dev[:B]), gogame.batch_track(dev[:B])
        same(gogame.batch_play_moves(st, mv), want_played, 'moves played', B)
        same(gogame.batch_play_moves(pk, mv), want_played, 'moves played, packed', B)
        same(gogame.batch_play_moves_tracked(tr, mv), want_played, 'moves played, tracked', B)
        same(st, want, 'replay', B)
        same(gogame.batch_unpack(pk, N), want, 'replay, packed', B)
        same(gogame.batch_untrack(tr), want, 'replay, tracked', B)

    # ---- the mask on the boards after the move (no ko: planes 0 - 2 cannot tell one), the areas before and after it
    post_dev = torch.from_numpy(post).cuda()
    fresh = np.stack([fc.invalid_moves(s) for s in post])
    playable = post[:, 5, 0, 0] == 0
    for B in (200, 256):           # pairs, and sixteen boards per wave
        mask = gogame._invalid_mask_dev(post_dev[:B]).cpu().numpy()
        p = playable[:B]
        same(mask[p], fresh[:B][p], 'invalid mask', B, rows=np.flatnonzero(p))
    for what, boards, boards_dev in (('before', start, dev), ('after', post, post_dev)):
        gb, gw = gogame.batch_areas(boards_dev)
        wb, ww = c_oracle.batch_areas(boards)
        same(gb, wb, 'black areas', what)
        same(gw, ww, 'white areas', what)

    # ---- children of the 24 deepest boards: eight crafted ones as they are (forced masks: q and the pass), sixteen after the move
    deep = [i for i in range(B0) if kinds[i] in fc.TURNED]       # (none at 2x2: the first boards of the batch then)
    sel, origin = np.concatenate([start[deep[:8]], post[deep[:16]], start]), np.array(deep[:8] + deep[:16] + list(range(B0)))
    live = np.flatnonzero(sel[:, 5, 0, 0] == 0)[:24]             # (the children of a finished game are undefined in the reference)
    sel, origin, k = sel[live], origin[live], len(live)
    sel_dev = torch.from_numpy(sel).cuda()
    for canonical in (False, True):
        same(gogame.batch_children(sel_dev, canonical=canonical), c_oracle.batch_children(sel, canonical), 'children', canonical, rows=origin)
    want = c_oracle.batch_children(sel)
    ckids, coffs = gogame.batch_children(sel_dev, padded=False)
    keep = np.concatenate([sel[:, 3].reshape(k, -1) == 0, np.ones((k, 1), bool)], axis=1)
    same(coffs, np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32), 'children offsets', rows=[0] * (k + 1))
    same(ckids, want[keep], 'un-padded children', rows=np.repeat(origin, keep.sum(axis=1)))
    pkids = gogame.batch_children_packed(gogame.batch_pack(sel_dev))
    same(gogame.batch_unpack(pkids.reshape(k * A, -1), N).reshape(k, A, 6, N, N), want, 'packed children', rows=origin)

    # ---- env steps, auto_reset on: q given on the forced boards (the oracle's draw elsewhere), and drawn moves
    want_given = want1.copy()
    want_given[forced] = post[forced]

    def env(step, B, method, given, unwrap, **kw):
        holder, rng = step['make'](dev[:B]), gogame.rng_seed(B, fc.SEED, 0, 'cuda')
        rewards, dones, status, taken = step['call'](holder, acts_dev[:B] if given else None, None if given else rng, KOMI, method, True, **kw)
        want = (want_given if given else want1)[:B]
        what = (step['name'], B, method, given)
        same(unwrap(holder), want, 'env boards', *what)
        if 'states_out' in kw:
            same(kw['states_out'], want, 'env observation', *what)
        if 'steps_done' in kw:
            assert int(kw['steps_done'].min()) == int(kw['steps_done'].max()) == 1, what
        same(status, np.zeros(B, np.int32), 'env status', *what)
        same(taken, (acts if given else last1)[:B], 'env actions', *what)
        same(dones, want[:, 5, 0, 0], 'env dones', *what)
        same(rewards.cpu().numpy().astype(np.float64), _ref_reward(want, KOMI, method, N), 'env rewards', *what)
        if not given:
            same(rng, rng1[:B], 'env generators', *what)

    plain = {'name': 'bytes', 'make': lambda s: s.clone(), 'call': gogame.batch_env_step}
    packed = {'name': 'packed', 'make': gogame.batch_pack, 'call': gogame.batch_env_step_packed}
    tracked = {'name': 'tracked', 'make': gogame.batch_track, 'call': gogame.batch_env_step_tracked}
    for method in ('real', 'heuristic'):       # (the rewards of the corridor boards: the area floods inside the step)
        for given in (True, False):
            for B in (12, 200, 256):
                env(plain, B, method, given, lambda s: s)
                env(packed, B, method, given, lambda pk: gogame.batch_unpack(pk, N))
            for B in (24, 200):
                env(tracked, B, method, given, gogame.batch_untrack)
                env(tracked, B, method, given, gogame.batch_untrack, states_out=torch.zeros_like(dev[:B]),
                    steps_done=torch.zeros(B, dtype=torch.int64, device='cuda'))
    torch.cuda.synchronize()


def _main(mode, sizes):
    import torch
    out = {}
    for N in sizes:
        if mode == 'oracle':
            _oracle_child(N)
        out['policy%d' % N] = _policy_digests(N)
    torch.cuda.synchronize()
    print('DIGESTS ' + json.dumps(out))


def _child(mode, sizes, cus):
    env = dict(os.environ)
    env.pop('GYMGO_AMD_CUS', None)
    if cus:
        env['GYMGO_AMD_CUS'] = str(cus)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), mode, json.dumps(sizes)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('DIGESTS ')][-1]
    return json.loads(line[len('DIGESTS '):])


@pytest.fixture(scope='module')
def own_cu_count():
    """the eye-aware rollouts of every size once at the device's own CU count: the small-batch kernels"""
    return _child('digests', SIZES, None)


@pytest.mark.gpu
@pytest.mark.parametrize('size', SIZES)
def test_flood_stressing_positions_through_every_step_kernel(size, own_cu_count):
    got = _child('oracle', [size], 1)
    key = 'policy%d' % size
    assert got[key] == own_cu_count[key], key


if __name__ == '__main__':
    _main(sys.argv[1], json.loads(sys.argv[2]))
