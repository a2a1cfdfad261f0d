"""CPU: what tests/test_gpu_area.py relies on, without a device - the definitional module tests/area_expect.py is pinned to
the oracle's batch_areas at every board size, its planes partition the board, follow `side` and the turn plane and turn with
the board; hand-made boards say what the three planes are; the sets are not vacuous; and the corridor boards are what their
name says: a snake-shaped region as long as the flood depth flood_cases documents, all own_area, and all neutral once one
opponent stone sits on its far end.  And the binding table of the area family (_lib.ABI_AREA) against its header
(include/gymgo_amd_area.h), as tests/test_host_abi.py holds _lib.ABI against include/gymgo_amd.h."""
import numpy as np
import pytest

import area_expect as ae
import features_expect as fe
import flood_cases as fc
import plane_cases as pc


@pytest.mark.parametrize('N', pc.SIZES)
def test_counts_are_the_oracles_areas(N):
    from oracle import c_oracle
    for kind in pc.SETS:
        c = ae.case(N, kind)
        black, white = c_oracle.batch_areas(c.states)
        assert len(c.states) == 21
        assert np.array_equal(c.counts_black[:, 0], black) and np.array_equal(c.counts_black[:, 1], white), (N, kind)
        for b in range(3):
            assert np.array_equal(ae.counts(ae.area_planes(c.states[b], side=0)), [black[b], white[b]]), (N, kind, b)


@pytest.mark.parametrize('N', pc.SIZES)
def test_partition_side_and_turn(N):
    for kind in pc.SETS + ('corridor',):
        c = ae.case(N, kind)
        if not len(c.states):
            continue
        for planes in (c.planes, c.black, c.white):
            assert planes.dtype == np.uint8 and planes.max() <= 1 and (planes.sum(axis=1) == 1).all(), (N, kind)
        assert np.array_equal(c.white, c.black[:, [1, 0, 2]]), (N, kind)
        white = c.states[:, 2, 0, 0] != 0
        assert np.array_equal(c.planes, np.where(white[:, None, None, None], c.white, c.black)), (N, kind)
        stones = (c.states[:, 0] | c.states[:, 1]) != 0
        assert not (c.black[:, 2].astype(bool) & stones).any()                       # neutral points are empty
        assert np.array_equal(c.black[:, 0].astype(bool) & stones, c.states[:, 0] != 0)
        assert np.array_equal(c.black[:, 1].astype(bool) & stones, c.states[:, 1] != 0)
        mixed = ae.mixed_side(len(c.states))
        assert np.array_equal(ae.batch_area_planes(c.states, mixed), np.where(mixed[:, None, None, None] != 0, c.white, c.black))
        own, margin = ae.owner(c.planes)
        assert own.dtype == np.int8 and margin.dtype == np.int32
        assert np.array_equal(own.astype(np.int32).sum(axis=(1, 2)), margin) and np.array_equal(own == 0, c.planes[:, 2] == 1)
    if len(pc.case(N, 'random').states):
        r = pc.case(N, 'random').states
        m = ae.mixed_side(21)
        assert (m != r[:, 2, 0, 0]).any() and (m == r[:, 2, 0, 0]).any() and m.any() and not m.all()


@pytest.mark.parametrize('N', pc.SIZES)
def test_planes_turn_with_the_board(N):
    """pc.turned(area_planes(s), o) == area_planes(turned s): the oriented GPU test may use pc.turned."""
    for kind in pc.SETS:
        c = ae.case(N, kind)
        for o in range(8):
            orient = np.full(len(c.states), o)
            turned = pc.turned(c.states, orient)
            assert np.array_equal(pc.turned(c.planes, orient), ae.batch_area_planes(turned)), (N, kind, o)
            assert np.array_equal(ae.counts(ae.batch_area_planes(turned)), c.counts), (N, kind, o)
    cb = ae.case(N, 'corridor')
    if len(cb.states):
        orient = (np.arange(len(cb.states)) * 3 + 1) % 8
        assert np.array_equal(pc.turned(cb.planes, orient), ae.batch_area_planes(pc.turned(cb.states, orient))), N


def planes_of(rows, side=0, **kw):
    return ae.area_planes(fe.board(rows, **kw), side)


def grid(plane):
    return [''.join('#' if v else '.' for v in r) for r in plane]


def test_hand_made_boards():
    # the empty board: all neutral
    for N in (2, 5, 19):
        p = ae.area_planes(np.zeros((6, N, N), np.uint8))
        assert not p[0].any() and not p[1].any() and p[2].all() and list(ae.counts(p)) == [0, 0]
    # one stone: the whole board for its colour, from either side
    for N in (2, 3, 9, 19):
        s = np.zeros((6, N, N), np.uint8)
        s[1, N // 2, 0] = 1
        p = ae.area_planes(s, side=0)
        assert not p[0].any() and p[1].all() and not p[2].any() and list(ae.counts(p)) == [0, N * N]
        assert list(ae.counts(ae.area_planes(s, side=1))) == [N * N, 0]
        s[2] = 1
        assert np.array_equal(ae.area_planes(s), ae.area_planes(s, side=1))
    # a region that touches both colours is neutral, all of it
    p = planes_of(['X...O', '.....', '.....', '.....', '.....'])
    assert grid(p[0]) == ['#....', '.....', '.....', '.....', '.....'] and grid(p[1]) == ['....#', '.....', '.....', '.....', '.....']
    assert p[2].sum() == 23 and list(ae.counts(p)) == [1, 1]
    # an enclosed one-colour region next to a two-colour one: black's eye in the corner, a shared region, a white corner
    rows = ['.X..O',
            'XX..O',
            '....O',
            '.OOO.',
            '.O...']
    p = planes_of(rows)
    assert grid(p[0]) == ['##...', '##...', '.....', '.....', '.....']
    assert grid(p[1]) == ['....#', '....#', '....#', '.####', '.####']
    assert grid(p[2]) == ['..##.', '..##.', '####.', '#....', '#....']
    assert list(ae.counts(p)) == [4, 11]
    q = planes_of(rows, side=1)
    assert np.array_equal(q[0], p[1]) and np.array_equal(q[1], p[0]) and np.array_equal(q[2], p[2])
    # the turn plane decides without `side`; plane 3, pass and done do not matter
    s = fe.board(rows, white_to_move=True)
    assert np.array_equal(ae.area_planes(s), q)
    t = s.copy()
    t[3:] = 1
    assert np.array_equal(ae.area_planes(t), q)
    # a full board: nothing is neutral
    p = planes_of(['XO', 'OX'])
    assert not p[2].any() and list(ae.counts(p)) == [2, 2]


@pytest.mark.parametrize('N', [n for n in pc.SIZES if n >= 3])
def test_every_plane_occurs_in_the_sets(N):
    seen = np.zeros(3, bool)
    for kind in pc.SETS:
        seen |= ae.case(N, kind).planes.any(axis=(0, 2, 3))
    assert seen.all(), (N, seen)
    assert any((ae.case(N, kind).black[:, 0].any() and ae.case(N, kind).black[:, 1].any()) for kind in pc.SETS), N


@pytest.mark.parametrize('N', pc.SIZES)
def test_corridor_boards(N):
    cb = ae.corridor_boards(N)
    c = ae.case(N, 'corridor')
    if N >= 5:
        assert cb.plain.sum() == 16 and (~cb.plain).sum() == 16, N                    # eight orientations x the ring's colour
        assert set(cb.ring[cb.plain]) == {0, 1}
    for i in range(len(cb.states)):
        s, ring = cb.states[i], int(cb.ring[i])
        assert s.max() <= 1 and not (s[0] & s[1]).any()
        region, seed = cb.corridor[i], tuple(cb.seed[i])
        assert not (region & ((s[0] | s[1]) != 0)).any() and region.any()
        black = c.black[i]
        if cb.plain[i]:
            # the whole snake-shaped region is the ring colour's area
            assert (black[ring][region] == 1).all(), (N, i)
            assert fc.every_group_has_a_liberty(s), (N, i)
        else:
            far = tuple(cb.far[i])
            assert s[1 - ring][far] and (s[1 - ring].sum() == 1 if N >= 5 else True), (N, i)
            stones, libs = fc.group(s, far)
            assert stones == {far} and len(libs) >= 1, (N, i)                           # the extra stone has a liberty
            assert (black[2][region] == 1).all() and black[1 - ring][far] == 1, (N, i)   # every corridor point turns neutral
        if N >= 5:
            # the length of the corridor is the flood depth flood_cases documents: (legs) x (N - 3) vertical steps from the
            # seed, in the unturned frame; a quarter turn makes them horizontal runs
            pts = {tuple(p) for p in np.argwhere(region)} | ({tuple(cb.far[i])} if not cb.plain[i] else set())
            legs = len(fc.snake(N)[1])
            depth_v = fc.vertical_depth(pts, seed)
            depth_h = fc.vertical_depth({(c_, r_) for r_, c_ in pts}, (seed[1], seed[0]))
            assert max(depth_v, depth_h) == legs * (N - 3), (N, i, depth_v, depth_h)
            if not cb.plain[i]:
                # the lone stone sits at the far end: as many corridor steps from the seed as the corridor has other points
                assert ae.corridor_of(cb.states[i - 1], seed)[tuple(cb.far[i])] == len(pts) - 1, (N, i)
    if N == 19:
        assert len(fc.snake(19)[1]) * (19 - 3) == 144


# ---------------------------------------------------------------- the area family's header against its binding table
def area_declarations():
    """{function: [(C type without const, is pointer, parameter name)]} of every `int32_t gg_*(...);` of include/gymgo_amd_area.h,
    in header order - tests/test_host_abi.py's reading of include/gymgo_amd.h, of this header."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'gymgo_amd_area.h')).read()
    decls = {}
    for m in re.finditer(r'^\s*(?:int32_t|int)\s+(gg_\w+)\s*\((.*?)\);', hdr, flags=re.M | re.S):
        params = []
        for text in m.group(2).split(','):
            text = ' '.join(text.split())
            if text == 'void':
                continue
            pm = re.fullmatch(r'(?:const )?(\w+) ?(\*?) ?(\w+)', text)
            assert pm, (m.group(1), text)
            params.append((pm.group(1), pm.group(2) == '*', pm.group(3)))
        decls[m.group(1)] = params
    return root, decls


def test_area_binding_table_matches_its_header(native_built):
    """ABI_AREA against include/gymgo_amd_area.h parameter by parameter (test_host_abi's comparison), the library exports the
    three symbols, INTEGRATION.md names them, and the table of include/gymgo_amd.h does not hold them."""
    import ctypes
    import os
    import test_host_abi as tha
    from gymgo_amd import _lib
    root, decls = area_declarations()
    assert list(decls) == ['gg_area_planes', 'gg_batch_area', 'gg_batch_area_tracked']
    assert tha._abi_mismatches(decls, _lib.ABI_AREA) == []
    assert _lib.EXPORTS_AREA == tuple(decls) and not set(decls) & set(_lib.EXPORTS)
    dropped = dict(_lib.ABI_AREA, gg_batch_area=_lib.ABI_AREA['gg_batch_area'][:2] + _lib.ABI_AREA['gg_batch_area'][3:])
    assert any('9 parameters in the header, 8 in the table' in b for b in tha._abi_mismatches(decls, dropped))      # the comparison can fail
    for f, (argtypes, restype) in _lib._SIGNATURES_AREA.items():
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_AREA[f]]
    L = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    for name in decls:
        assert hasattr(L, name) and name in doc, name
    assert native_built.gg_area_planes() == 3 and native_built.gg_version() == _lib.ABI_VERSION == 5
