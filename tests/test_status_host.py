"""CPU: stone status and the final score from playout ownership without a device - the binding table of the family
(_lib.ABI_STATUS) against its header (include/gymgo_amd_status.h), the argument checks of the C entry points and every
ValueError of the Python API (before a device is touched), the rule of tests/status_expect.py on hand-made positions under the
committed CPU replay of the playouts, and the premises of every case tests/test_gpu_status.py runs."""
import ctypes
import os

import numpy as np
import pytest
from scipy import ndimage

import area_expect as ae
import mc_policy_expect as mp
import plane_cases as pc
import status_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['gg_status_planes', 'gg_batch_status', 'gg_batch_status_tracked']


# ---------------------------------------------------------------- the family's header against its binding table
def test_status_binding_table_matches_its_header(native_built):
    """ABI_STATUS against include/gymgo_amd_status.h parameter by parameter (test_area_host's comparison), the library exports
    the three symbols, INTEGRATION.md and the README name them, and no other table holds them."""
    import test_host_abi as tha
    from gymgo_amd import _lib
    decls = tha.header_declarations('gymgo_amd_status.h')
    assert list(decls) == NAMES
    assert tha._abi_mismatches(decls, _lib.ABI_STATUS) == []
    assert _lib.EXPORTS_STATUS == tuple(decls)
    others = (_lib.EXPORTS, _lib.EXPORTS_AREA, _lib.EXPORTS_PAST, _lib.EXPORTS_GUMBEL, _lib.EXPORTS_TACTICS, _lib.EXPORTS_AMAF,
              _lib.EXPORTS_PATTERN, _lib.EXPORTS_PRIOR)
    assert not set(decls) & {f for t in others for f in t}
    dropped = dict(_lib.ABI_STATUS, gg_batch_status=_lib.ABI_STATUS['gg_batch_status'][:2] + _lib.ABI_STATUS['gg_batch_status'][3:])
    assert any('13 parameters in the header, 12 in the table' in b for b in tha._abi_mismatches(decls, dropped))   # the comparison can fail
    for f, (argtypes, restype) in _lib._SIGNATURES_STATUS.items():
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_STATUS[f]]
        assert _lib._POINTERS[f][0] == len(_lib.ABI_STATUS[f])
    # const: every pointer but the two outputs
    for f, ps in tha.header_declarations('gymgo_amd_status.h', const=True).items():
        for ctype, pointer, name, const in ps:
            if pointer and name != 'hip_stream':
                assert const == (name not in ('out', 'counts')), (f, name)
    L = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'gymgo_amd_status.h')).read()
    for phrase in ('D den >= num K |C|', 'A den >= num K |C|', '64-bit', '4-byte aligned', 'aligned to its element', 'in this order'):
        assert phrase in hdr, phrase
    for doc in ('INTEGRATION.md', 'README.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NAMES + ['gymgo_amd_status.h']:
            assert name in text, (doc, name)
    for name in decls:
        assert hasattr(L, name), name
    assert native_built.gg_status_planes() == 9 == se.PLANES and native_built.gg_version() == _lib.ABI_VERSION == 5


def test_entry_points_check_arguments_in_order(native_built):
    """Pointers that are never followed: every call below returns from its checks, in the order the header gives."""
    from gymgo_amd import _lib
    L = _lib.lib()
    p = 0x1000          # "a pointer": aligned, never followed
    for fn in (L.gg_batch_status, L.gg_batch_status_tracked):
        call = lambda own=p, K=64, num=2, den=3, out=p, counts=None, dtype=3, B=2, N=9, states=p: fn(
            states, None, None, own, K, num, den, out, counts, dtype, B, N, None)
        # the sizes first, whatever the scalars are
        assert call(N=1, K=0) == -1 and call(N=20, num=0) == -1 and call(B=-1, den=0) == -1 and call(dtype=4, K=0) == -1
        assert call(dtype=-1) == -1
        # the scalars, also for an empty batch
        for bad in (dict(K=0), dict(K=(1 << 20) + 1), dict(K=-5), dict(num=0), dict(num=4, den=3), dict(num=1, den=2), dict(num=512, den=1024),
                    dict(num=1025, den=1025), dict(num=2, den=3000), dict(num=-2, den=-3)):
            assert call(**bad) == -3 and call(B=0, **bad) == -3, bad
        for good in (dict(K=1), dict(K=1 << 20), dict(num=1, den=1), dict(num=1024, den=1024), dict(num=513, den=1024), dict(num=2, den=2)):
            assert call(B=0, states=None, own=None, out=None, **good) == 0, good          # B = 0: no work, no pointer looked at
        # the 4-byte alignments before the NULL pointers
        assert call(own=p + 2) == -3 and call(counts=p + 1) == -3 and call(own=p + 2, out=None) == -3
        assert call(states=None) == -2 and call(own=None) == -2 and call(out=None) == -2
        # out aligned to its element
        assert call(out=p + 1, dtype=2) == -3 and call(out=p + 2, dtype=0) == -3 and call(out=p + 1, dtype=1) == -3


def test_constants_and_value_errors(native_built):
    """Everything here comes before a device is touched: the tensors are CPU tensors or arrays, and nothing but ValueError
    is accepted."""
    import torch
    from gymgo_amd import gogame
    assert gogame.STATUS_PLANES == 9 and gogame.STATUS_NAMES == se.NAMES
    assert gogame.FinalScore._fields == ('black_area', 'white_area', 'margin', 'winner', 'owner', 'dead', 'unsettled', 'playouts')
    st = np.zeros((2, 6, 5, 5), np.uint8)
    own = np.zeros((2, 2, 5, 5), np.int32)
    tracked = torch.zeros((2, 26), dtype=torch.int32)
    none = gogame.Playouts(*[None] * 7)
    for fn, boards in ((gogame.batch_stone_status, st), (gogame.batch_stone_status_tracked, tracked)):
        for bad in (dict(threshold=(1, 2)), dict(threshold=(3, 2)), dict(threshold=(0, 1)), dict(threshold=(1025, 1025)),
                    dict(threshold=(2.0, 3)), dict(threshold=2), dict(threshold=(2, 3, 4)), dict(threshold=(True, 1)),
                    dict(playouts=0), dict(playouts=(1 << 20) + 1), dict(playouts=16.0), dict(playouts=None),
                    dict(ownership=own[:1]), dict(ownership=own[:, :1]), dict(ownership=own[..., :4]), dict(ownership=own.astype(np.int64)),
                    dict(ownership=torch.zeros((2, 2, 5, 5), dtype=torch.int64)), dict(ownership=torch.zeros((2, 2, 5, 4), dtype=torch.int32)),
                    dict(ownership=own.tolist()), dict(ownership=none), dict(ownership=None),
                    dict(dtype=torch.float64), dict(orient=[0]), dict(side=[0]), dict(side=[0.0, 1.0]),
                    dict(counts=torch.zeros((2, 4), dtype=torch.int32)), dict(out=torch.zeros((2, 9, 5, 5), dtype=torch.uint8))):
            kw = dict(ownership=own, playouts=16)
            kw.update(bad)
            with pytest.raises(ValueError):
                fn(boards, kw.pop('ownership'), kw.pop('playouts'), **kw)
    with pytest.raises(ValueError):
        gogame.batch_stone_status(st[:, :5], own, 16)
    with pytest.raises(ValueError):
        gogame.batch_stone_status(st, own, 16, dtype=torch.bfloat16)          # NumPy has no bfloat16
    for bad in (dict(ownership=own), dict(ownership=own[0, 0]), dict(ownership=none), dict(threshold=(1, 2)), dict(playouts=0)):
        kw = dict(ownership=own[0], playouts=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            gogame.stone_status(st[0], kw.pop('ownership'), kw.pop('playouts'), **kw)
    for bad in (dict(playouts=0), dict(threshold=(1, 2)), dict(policy='no such policy'), dict(ownership=True), dict(amaf=True)):
        with pytest.raises(ValueError):
            gogame.batch_final_score(st, **bad)
    with pytest.raises(ValueError):
        gogame.batch_final_score(st[:, :5])


def test_the_ownership_device_is_checked_before_a_launch(native_built):
    """A device tensor's device is compared with the ownership's without touching either: meta tensors have a device and no memory."""
    import torch
    from gymgo_amd import gogame
    tracked = torch.zeros((2, 26), dtype=torch.int32, device='meta')
    with pytest.raises(ValueError, match='device'):
        gogame.batch_stone_status_tracked(tracked, torch.zeros((2, 2, 5, 5), dtype=torch.int32), 16)


# ---------------------------------------------------------------- the rule on hand-made positions
def test_the_rule_by_hand():
    s = mp.board(['BB.', '...', '.WW'])
    K = 12
    own = np.zeros((2, 3, 3), np.int32)
    own[1, 0, :2] = (9, 7)          # black's chain: D = 16 = 2/3 * 12 * 2 exactly
    own[1, 2, 1:] = (8, 7)          # white's chain: A = 15, one below
    own[0, 2, 1:] = (4, 5)          #                D = 9
    own[:, 1] = 6                   # empty points: never read
    dead, alive = se.vote(s, own, K, 2, 3)
    assert dead[0, 0, :2].all() and dead.sum() == 2 and not alive.any()
    planes, counts = se.status_planes(s, own, K, 2, 3, side=0)
    assert planes[1].sum() == 2 and planes[5].sum() == 2 and planes[[0, 2, 3, 4]].sum() == 0
    assert planes[7].all() and list(counts) == [0, 9, 2, 0]          # black gone: the board is white's
    assert (planes[:6].sum(axis=0) == ((s[0] | s[1]) != 0)).all() and (planes[6:].sum(axis=0) == 1).all()
    w, cw = se.status_planes(s, own, K, 2, 3, side=1)
    assert np.array_equal(w, se.white_view(planes, counts)[0]) and np.array_equal(cw, se.white_view(planes, counts)[1])
    own[1, 2, 1] = 9                # A = 16: alive
    assert se.vote(s, own, K, 2, 3)[1][1, 2, 1:].all()
    own[1, 0, 0] = 8                # D = 15: black is no longer dead - and with A = 0 unsettled
    dead, alive = se.vote(s, own, K, 2, 3)
    assert not dead.any() and not alive[0].any()
    # the verdicts at the edges of the contract
    assert se.verdict(0, 0, 1, 1, 1, 1) == 'unsettled' and se.verdict(1, 0, 1, 1, 1, 1) == 'dead' and se.verdict(0, 1, 1, 1, 1, 1) == 'alive'
    assert se.verdict(513, 511, 1, 1024, 513, 1024) == 'dead' and se.verdict(512, 512, 1, 1024, 513, 1024) == 'unsettled'


@pytest.fixture(scope='module')
def crafted_votes():
    """The committed CPU replay of K = 64 no_eye_fill playouts (komi 0, default seed, max_plies 392) from the two hand-made roots."""
    r7, r5 = se.crafted_roots()
    o7 = mp.expected_playouts_policy(r7[None], 64, 392, with_ownership=True)['ownership']
    o5 = mp.expected_playouts_policy(r5[None], 64, 392, with_ownership=True)['ownership']
    return (r7, o7[0]), (r5, o5[0])


def test_crafted_7x7_two_dead_stones_and_the_areas_after_removal(crafted_votes):
    """Exactly the two intruders are dead, nothing is unsettled, and each side gets its three columns: 21 points each by hand.
    Column 3 holds black's stone at (6, 3), which is alive, so black's area is 22 and the six empty points of that column are
    the neutral ones (a hand count of this position that leaves that stone out says 21 / 21 / 7)."""
    (s, own), _ = crafted_votes
    K = 64
    assert own.dtype == np.int32 and own.min() >= 0 and (own.sum(axis=0) <= K).all()
    planes, counts = se.status_planes(s, own, K, 2, 3, side=0)
    dead = planes[1] | planes[4]
    want = np.zeros((7, 7), np.uint8)
    want[2, 1] = want[2, 5] = 1
    assert np.array_equal(dead, want) and planes[4, 2, 1] and planes[1, 2, 5]
    assert not planes[2].any() and not planes[5].any()                         # no unsettled chain
    assert planes[6][:, :3].all() and planes[6][:, :3].sum() == 21 and planes[7][:, 4:].all() and planes[7].sum() == 21
    assert planes[6, 6, 3] and s[0, 6, 3] and planes[8][:6, 3].all() and planes[8].sum() == 6
    assert list(counts) == [22, 21, 1, 1]
    # the own-colour counts of the walls and the opponent counts of the intruders, as measured
    black, white = s[0] != 0, s[1] != 0
    wall_b, wall_w = black & (dead == 0), white & (dead == 0)
    assert 56 <= own[0][wall_b].min() and 56 <= own[1][wall_w].min()
    assert own[0][2, 1] == 62 and own[1][2, 5] == 59
    # Tromp-Taylor on the board as it stands: beyond its stones a side gets only the corner below its own wall (four points for
    # black, three for white); the intruder turns the rest of the side - the eight points above the wall - neutral
    plain = ae.area_planes(s, 0)
    assert plain[0].sum() == black.sum() + 4 and plain[1].sum() == white.sum() + 3
    assert plain[2][:4, :2].sum() == 7 and plain[2][:4, 5:].sum() == 7 and planes[6][:4, :2].all() and planes[7][:4, 5:].all()
    f = se.final_score(s[None], own[None], K)
    assert f['margin'][0] == 1 and f['winner'][0] == 1 and f['owner'].sum() == 1 and np.array_equal(f['dead'][0], want)
    assert se.final_score(s[None], own[None], K, komi=1.5)['winner'][0] == -1


def test_lone_stones_on_5x5_are_unsettled(crafted_votes):
    _, (s, own) = crafted_votes
    planes, counts = se.status_planes(s, own, 64, 2, 3, side=0)
    assert planes[2].sum() == 1 and planes[5].sum() == 1 and planes[[0, 1, 3, 4]].sum() == 0
    assert list(counts[2:]) == [0, 0] and np.array_equal(planes[6:], ae.area_planes(s, 0))      # nothing leaves the board


# ---------------------------------------------------------------- the premises of the GPU cases
@pytest.mark.parametrize('N', [n for n in pc.SIZES if n >= 3])
@pytest.mark.parametrize('threshold', se.THRESHOLDS)
def test_generated_cases_hold_what_the_gpu_test_relies_on(N, threshold):
    num, den = threshold
    K = se.PLAYOUTS[threshold]
    assert K % den == 0
    seen = {c: set() for c in (0, 1)}
    uneven = {0: False, 1: False}
    tall = {0: False, 1: False}
    for kind in pc.SETS:
        c = se.case(N, kind, threshold)
        assert len(c.states) == 21 and c.own.dtype == np.int32 and c.own.shape == (21, 2, N, N)
        assert c.own.min() >= 0 and (c.own.sum(axis=1) <= K).all()
        empty = (c.states[:, 0] | c.states[:, 1]) == 0
        assert (c.own[:, 0][empty] >= 1).all() and (c.own[:, 1][empty] >= 1).all()
        for b, col, m, what, D, A in c.info:
            n = int(m.sum())
            eq = num * K * n // den
            assert eq * den == num * K * n
            d, a = c.own[b, 1 - col][m], c.own[b, col][m]
            assert int(d.sum()) == D and int(a.sum()) == A and D + A <= K * n
            v = se.verdict(D, A, n, K, num, den)
            if what == 'dead_eq':
                assert D == eq and v == 'dead' and se.verdict(D - 1, A, n, K, num, den) != 'dead'
            elif what == 'dead_below':
                assert D == eq - 1 and v != 'dead' and se.verdict(D + 1, A, n, K, num, den) == 'dead'
            elif what == 'alive_eq':
                assert A == eq and v == 'alive' and se.verdict(D, A - 1, n, K, num, den) == 'unsettled'
            elif what == 'alive_below':
                assert A == eq - 1 and v == 'unsettled' and se.verdict(D, A + 1, n, K, num, den) == 'alive'
            else:
                assert v == what
            seen[col].add(what)
            seen[col].add('is ' + v)
            uneven[col] |= len(set(d.tolist())) > 1 and len(set(a.tolist())) > 1
            tall[col] |= 2 * int(m.any(axis=1).sum()) >= N
            if what in ('dead_below', 'alive_below'):
                # what lies next to the chain would lift it over if it were summed in: empty points hold both counts, and a
                # neighbouring stone of the other colour - where there is one - holds the count in question too
                r = ndimage.binary_dilation(m) & ~m
                plane = (1 - col) if what == 'dead_below' else col
                assert r.any() and (c.own[b, plane][r & empty[b]] >= 1).all()
        st = se.batch_status(c.states[:3], c.own[:3], K, num, den, side=1)
        assert np.array_equal(st[0], c.white[:3]) and np.array_equal(st[1], c.counts_white[:3])
        assert (c.black[:, :6].sum(axis=1) == ((c.states[:, 0] | c.states[:, 1]) != 0)).all() and (c.black[:, 6:].sum(axis=1) == 1).all()
    for col in (0, 1):
        assert set(se.KINDS) <= seen[col] and {'is dead', 'is alive', 'is unsettled'} <= seen[col], (N, col, seen[col])
        assert uneven[col] and tall[col], (N, col, uneven, tall)
    # some stone next to a chain one count below carries a count that would flip it
    flips = 0
    for kind in pc.SETS:
        c = se.case(N, kind, threshold)
        for b, col, m, what, D, A in c.info:
            if what in ('dead_below', 'alive_below'):
                r = ndimage.binary_dilation(m) & (c.states[b, 1 - col] != 0)
                plane = (1 - col) if what == 'dead_below' else col
                flips += int((c.own[b, plane][r] >= 1).sum())
    assert flips > 0, N


def test_planes_turn_with_the_board():
    """pc.turned(status planes, o) == the status planes of the turned board with the turned counts: the oriented GPU test may
    use pc.turned."""
    for N in (3, 8, 19):
        c = se.case(N, 'random')
        for o in range(8):
            orient = np.full(21, o)
            planes, counts = se.batch_status(pc.turned(c.states, orient), pc.turned(c.own, orient), c.K, c.num, c.den)
            assert np.array_equal(planes, pc.turned(c.planes, orient)) and np.array_equal(counts, c.counts), (N, o)


def test_large_value_case_needs_64_bit_products_and_whole_word_sums():
    N, K, den, n = (se.LARGE[k] for k in ('N', 'K', 'den', 'stones'))
    M32 = (1 << 32) - 1
    for num in (1024, 1000):
        c = se.large_case(num)
        assert c.own.min() >= 0 and (c.own.sum(axis=1) <= K).all() and c.own.max() <= K
        for i, (D, A) in enumerate(c.sums):
            col = i // 2
            m = c.states[i, col] != 0
            assert m.sum() == n and int(c.own[i, 1 - col][m].astype(np.int64).sum()) == D
            eq = num * K * n // den
            assert D == eq - (i % 2) and D > 1 << 28 and D * den > 1 << 32 and num * K * n > 1 << 32
            want = 'dead' if i % 2 == 0 else ('alive' if A * den >= num * K * n else 'unsettled')
            assert se.verdict(D, A, n, K, num, den) == want
            me = 1 if col == 0 else 4          # black's view: plane 1 black dead, plane 4 white dead
            assert c.black[i, me].sum() == (n if i % 2 == 0 else 0), (num, i)
            # the dead chain leaves an empty board: all neutral; the other stays and owns everything
            assert list(c.counts_black[i]) == ([0, 0, n, 0] if (i % 2 == 0 and col == 0) else [0, 0, 0, n] if i % 2 == 0
                                                else [N * N, 0, 0, 0] if col == 0 else [0, N * N, 0, 0])
            # a sum packed into a 16-bit field gets it wrong
            if i % 2 == 0:
                assert ((D & 0xFFFF) * den >= num * K * n) != (D * den >= num * K * n)
        if num == 1024:
            # num K n is a multiple of 2^32: in 32-bit products the chain one count below is dead too
            D = c.sums[1][0]
            assert (num * K * n) & M32 == 0 and D * den < num * K * n and ((D * den) & M32) >= ((num * K * n) & M32)
            assert not (c.own[1, 1][c.states[1, 0] != 0] == K).all()
        else:
            d = c.own[0, 1][c.states[0, 0] != 0]
            assert len(set(d.tolist())) > 16                                   # the per-stone values differ
            # the sum truncated to 28 bits is on the other side of the inequality
            D = c.sums[0][0]
            assert ((D & ((1 << 28) - 1)) * den >= num * K * n) != (D * den >= num * K * n)
