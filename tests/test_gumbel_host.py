"""CPU: what tests/test_gpu_gumbel.py relies on, without a device.  The schedule of sequential halving (gg_gumbel_sequence is
host code) against its restatement in Python integers and the five worked sequences; the binding table of the Gumbel family
(_lib.ABI_GUMBEL) against its header (include/gymgo_amd_gumbel.h), as tests/test_host_abi.py holds _lib.ABI against
include/gymgo_amd.h; the codes of the entry points' checks and their order, with pointers that are never followed; every new
ValueError, raised before a device is touched; and the premises of the expectation (tests/mc_gumbel_expect.py): on a fresh
root with c_scale = 0 the root rule is plain sequential halving over the top m of base, with fewer legal actions than m the
fallback fires and every slot still finds a leaf, and the cases of the device test contain a collision round, a fallback, a
-inf base, a tie and a kept root with non-zero seen."""
import collections
import math

import numpy as np
import pytest

import mc_cases as cs
import mc_expect as mc
import mc_gumbel_expect as ge
import mc_puct_expect as pe


# ---------------------------------------------------------------- the schedule and the binding
def test_sequence_equals_its_restatement_and_the_worked_examples(native_built):
    from gymgo_amd import gogame
    for (m, n), want in ge.WORKED.items():
        got = gogame.gumbel_sequence(m, n)
        assert got.dtype == np.int32 and got.tolist() == want == ge.seq(m, n), (m, n)
    for m in range(1, 41):
        for n in range(1, 201):
            assert gogame.gumbel_sequence(m, n).tolist() == ge.seq(m, n), (m, n)
    assert gogame.gumbel_sequence(1, 5).tolist() == [0, 1, 2, 3, 4]
    # every action considered gets a simulation before any gets a second one, and an entry never exceeds its index
    for m, n in ((16, 32), (362, 64), (7, 300)):
        s = ge.seq(m, n)
        assert s[:min(m, n)] == [0] * min(m, n) and all(0 <= v <= t for t, v in enumerate(s)) and s == sorted(s)
    for bad in ((0, 4), (4, 0), (-1, 4), (2.0, 4), (True, 4), (4, None), (2 ** 31, 4)):
        with pytest.raises(ValueError):
            gogame.gumbel_sequence(*bad)


def gumbel_declarations():
    """{function: [(C type without const, is pointer, parameter name)]} of every `int32_t gg_*(...);` of
    include/gymgo_amd_gumbel.h, in header order - tests/test_host_abi.py's reading of include/gymgo_amd.h, of this header."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'gymgo_amd_gumbel.h')).read()
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


GUMBEL_ENTRY_POINTS = ['gg_gumbel_sequence', 'gg_gumbel_begin', 'gg_gumbel_select_leaves', 'gg_gumbel_root']


def test_gumbel_binding_table_matches_its_header(native_built):
    import ctypes
    import os
    import test_host_abi as tha
    from gymgo_amd import _lib
    root, decls = gumbel_declarations()
    assert list(decls) == GUMBEL_ENTRY_POINTS
    assert tha._abi_mismatches(decls, _lib.ABI_GUMBEL) == []
    assert _lib.EXPORTS_GUMBEL == tuple(decls)
    assert not set(decls) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_AREA) | set(_lib.EXPORTS_PAST))
    dropped = dict(_lib.ABI_GUMBEL, gg_gumbel_root=_lib.ABI_GUMBEL['gg_gumbel_root'][:3] + _lib.ABI_GUMBEL['gg_gumbel_root'][4:])
    assert any('16 parameters in the header, 15 in the table' in b for b in tha._abi_mismatches(decls, dropped))   # the comparison can fail
    for f, (argtypes, restype) in _lib._SIGNATURES_GUMBEL.items():
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_GUMBEL[f]]
    L = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    for name in decls:
        assert hasattr(L, name) and name in doc, name
    assert native_built.gg_version() == _lib.ABI_VERSION == 5 and len(_lib.EXPORTS) == 79
    assert 'gymgo_amd_gumbel.h' in open(os.path.join(root, 'gymgo_amd', '_lib.py')).read()   # the rebuild list


def test_entry_point_checks_come_before_any_device_work(native_built):
    """The codes and their order, with pointers that are never followed: sizes, then arguments, then the zero-work return,
    then NULL pointers, then the alignment of stats."""
    import os
    import re
    L = native_built
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gymgo_amd.h')).read()
    codes = {n: int(v) for n, v in re.findall(r'#define\s+(GG_E_\w+)\s+\(?(-?\d+)\)?', hdr)}
    BADSIZE, BADARG, NULLPTR = codes['GG_E_BADSIZE'], codes['GG_E_BADARG'], codes['GG_E_NULLPTR']
    p, odd, inf, nan = 4096, 4104, math.inf, math.nan
    # gg_gumbel_sequence(m, n, seq)
    assert L.gg_gumbel_sequence(0, 4, None) == BADARG and L.gg_gumbel_sequence(4, 0, None) == BADARG
    assert L.gg_gumbel_sequence(4, 8, None) == NULLPTR
    # gg_gumbel_begin(R, N, C, child, stats, nodes, seen, done, stream)
    f = L.gg_gumbel_begin
    assert f(1, 1, 0, None, None, None, None, None, None) == BADSIZE                    # N first, whatever C is
    assert f(1, 20, 4, p, p, p, p, p, None) == BADSIZE and f(-1, 9, 4, p, p, p, p, p, None) == BADSIZE
    assert f(0, 9, 0, None, None, None, None, None, None) == BADARG                     # C before the zero-work return
    assert f(1, 9, 2 ** 31 - 1, None, p, p, p, p, None) == BADARG
    assert f(0, 9, 4, None, None, None, None, None, None) == 0                          # R == 0 before NULL
    for hole in range(3, 8):
        args = [1, 9, 4, p, p, p, p, p, None]
        args[hole] = None
        assert f(*args) == NULLPTR, hole
    assert f(1, 9, 4, None, odd, p, p, p, None) == NULLPTR                              # NULL before alignment
    assert f(1, 9, 4, p, odd, p, p, p, None) == BADARG
    # gg_gumbel_select_leaves(R, N, C, L, c, boards, child, prior, links, stats, nodes, base, seen, done, seq, S, c_visit,
    #                         c_scale, leaf, move, leaf_id, stream)
    f = L.gg_gumbel_select_leaves
    good = [1, 9, 8, 2, 1.25, p, p, p, p, p, p, p, p, p, p, 4, 50.0, 0.5, p, p, p, None]
    def call(**kw):
        names = ('R', 'N', 'C', 'L', 'c', 'boards', 'child', 'prior', 'links', 'stats', 'nodes', 'base', 'seen', 'done', 'seq', 'S',
                 'c_visit', 'c_scale', 'leaf', 'move', 'leaf_id', 'stream')
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    assert call(N=1, C=0) == BADSIZE and call(N=20) == BADSIZE and call(R=-1, L=0) == BADSIZE
    for kw in (dict(C=0), dict(C=2 ** 31 - 1), dict(L=0), dict(L=9), dict(c=-1.0), dict(c=inf), dict(c=nan), dict(S=0), dict(S=-3),
               dict(c_visit=-1.0), dict(c_visit=inf), dict(c_visit=nan), dict(c_scale=-0.5), dict(c_scale=inf), dict(c_scale=nan)):
        assert call(boards=None, **kw) == BADARG, kw                                    # arguments before NULL
        assert call(R=0, **kw) == BADARG, kw                                            # ... and before the zero-work return
    assert call(R=0, boards=None, seq=None, stats=odd) == 0
    assert call(c_visit=0.0, c_scale=0.0, c=0.0, boards=None) == NULLPTR                # zero is allowed
    for name in ('boards', 'child', 'prior', 'links', 'stats', 'nodes', 'base', 'seen', 'done', 'seq', 'leaf', 'move', 'leaf_id'):
        assert call(**{name: None}) == NULLPTR, name
    assert call(stats=odd, leaf=None) == NULLPTR and call(stats=odd) == BADARG          # alignment last
    # gg_gumbel_root(R, N, C, boards, child, stats, nodes, base, seen, c_visit, c_scale, actions, q, visits, value, stream)
    f = L.gg_gumbel_root
    good_root = [1, 9, 8, p, p, p, p, p, p, 50.0, 0.5, p, None, None, None, None]       # q, visits, value may be NULL
    def root(**kw):
        names = ('R', 'N', 'C', 'boards', 'child', 'stats', 'nodes', 'base', 'seen', 'c_visit', 'c_scale', 'actions', 'q', 'visits',
                 'value', 'stream')
        args = list(good_root)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    assert root(N=1, C=0) == BADSIZE and root(R=-1) == BADSIZE
    for kw in (dict(C=0), dict(C=2 ** 31 - 1), dict(c_visit=-1.0), dict(c_visit=nan), dict(c_scale=inf), dict(c_scale=-1.0)):
        assert root(boards=None, **kw) == BADARG and root(R=0, **kw) == BADARG, kw
    assert root(R=0, boards=None, actions=None) == 0
    for name in ('boards', 'child', 'stats', 'nodes', 'base', 'seen', 'actions'):
        assert root(**{name: None}) == NULLPTR, name
    assert root(stats=odd, actions=None) == NULLPTR and root(stats=odd) == BADARG


def test_value_errors_before_a_device_is_touched(native_built):
    """Every new ValueError, on a box without a device: none of these calls gets as far as one."""
    import torch
    from gymgo_amd import gogame
    G = gogame.Gumbel
    assert G() == (16, None, 50.0, 0.5) and G(4).considered == 4 and G._fields == ('considered', 'simulations', 'c_visit', 'c_scale')
    states = np.zeros((3, 6, 5, 5), np.uint8)
    ev = lambda *a: None
    for bad in (0, -4, 2.0, True, 'four', (4, 8), G(0), G(4, 0), G(4, -1), G(4, 2.5), G(4, 8, -1.0), G(4, 8, math.inf), G(4, 8, 50.0, math.nan),
                G(4, 8, 50.0, -0.5), G(4, 8, 'x'), G(2 ** 31)):
        with pytest.raises(ValueError):
            gogame.PuctSearch(states, 4, gumbel=bad)
        with pytest.raises(ValueError):
            gogame.puct_selfplay(states, 2, 4, ev, gumbel=bad)
    assert gogame._gumbel_arg(4, 9, 3) == G(4, 24, 50.0, 0.5) and gogame._gumbel_arg(G(2, None, 0, 0), 1, 8) == G(2, 1, 0.0, 0.0)
    assert gogame._gumbel_arg(None, 9, 3) is None and gogame._gumbel_arg(G(16, 5), 9, 3).simulations == 5
    # the move loops
    with pytest.raises(ValueError, match='gumbel='):
        gogame.puct_play(states, 2, 4, ev, gumbel_noise=gogame.gumbel_noise())        # draws without a Gumbel search
    with pytest.raises(ValueError):
        gogame.puct_play(states, 2, 4, ev, gumbel=4, gumbel_noise='default')          # not a callable
    with pytest.raises(ValueError, match='gumbel='):
        gogame.puct_selfplay(states, 2, 4, ev, gumbel_noise=gogame.gumbel_noise())
    with pytest.raises(ValueError):
        gogame.puct_selfplay(states, 2, 4, ev, gumbel=4, gumbel_noise=3)
    with pytest.raises(ValueError, match='noise must be None'):
        gogame.puct_selfplay(states, 2, 4, ev, gumbel=4, noise=gogame.dirichlet_noise(0.3))
    with pytest.raises(ValueError, match='sample_moves'):
        gogame.puct_selfplay(states, 2, 4, ev, gumbel=4, sample_moves=1)
    # the draws: a callable, one value per action, legal or not
    noise = gogame.gumbel_noise(torch.Generator().manual_seed(5))
    z = noise(0, torch.zeros((3, 26), dtype=torch.bool))
    assert z.dtype == torch.float32 and tuple(z.shape) == (3, 26) and bool(torch.isfinite(z).all()) and float(z.std()) > 0.5


# ---------------------------------------------------------------- premises on the expectation
def _fresh_root(N=5):
    root = cs.size_roots(N)['empty']
    assert mc.legal_actions(root).size == N * N + 1
    return root[None]


@pytest.mark.parametrize('m,n', [(4, 8), (16, 32), (3, 7), (2, 4), (1, 5)])
def test_c_scale_zero_is_sequential_halving_over_the_top_m_of_base(m, n):
    """A fresh root with at least m legal actions, L = 1, c_scale = 0, n = len(seq): the multiset of k_a is what the schedule
    implies, the visited set is the top m of base by an independent argsort, the action the top 1."""
    roots = _fresh_root()
    A = 26
    T = n + 1                                                       # round 0 evaluates the root alone
    s = ge.Search(roots, T, 1, m, n=n, c_scale=0.0, c_visit=50.0)
    s.set_g(ge.dyadic_g(1, A, salt=m))
    for _ in range(T):
        s.round(pe.hash_evaluator_np)
    t = s.trees[0]
    assert t.done == n and s.events()['fallback'] == 0 and s.events()['collision'] == 0
    base = t.base.astype(np.float64)
    legal = np.zeros(A, bool)
    legal[t.legal[0]] = True
    assert np.isfinite(base[legal]).sum() >= m                       # the premise: at least m actions that can be drawn
    order = np.argsort(-np.where(legal, base, -np.inf), kind='stable')
    acts, ka, ncs, _, _, _ = t.root_terms(False)
    visited = sorted(a for a, k in zip(acts, ka) if k > 0)
    assert visited == sorted(int(a) for a in order[:m]), (visited, order[:m])
    # what the schedule implies: action of rank i is simulated once for every entry of its column
    sched = ge.seq(m, n)
    want = collections.Counter()
    if m == 1:
        want[n] = 1
    else:
        width, pos = m, 0
        counts = [0] * m
        lg = max(1, math.ceil(math.log2(m)))
        while pos < n:
            e = max(1, n // (lg * width))
            for _ in range(e):
                for i in range(width):
                    if pos < n:
                        counts[i] += 1
                        pos += 1
            width = max(2, width // 2)
        want = collections.Counter(counts)
    assert collections.Counter(k for k in ka if k > 0) == want, (ka, want)
    if (m, n) == (4, 8):
        assert sorted((k for k in ka if k > 0), reverse=True) == [3, 3, 1, 1]
    assert ka == ncs and len(sched) == n                             # a fresh root: this move's simulations are the visits
    assert s.readout()[0][0] == order[0]                             # the action: the top 1 of base


def test_fewer_legal_actions_than_considered_falls_back_and_every_slot_finds_a_leaf():
    N, T, L, m = 5, 12, 1, 16
    roots = cs.stack(N, ('late0', 'late1', 'late2'))
    assert max(mc.legal_actions(r).size for r in roots) < min(m, T - 1)   # the first pass of the schedule is longer than that
    s = ge.expected_gumbel(roots, T, L, pe.hash_evaluator_np, m, c_scale=0.0)
    assert s.schedule == [0] * (T - 1)
    assert s.events()['fallback'] > 0 and s.events()['collision'] == 0
    for ids, _ in s.rounds:
        assert (ids >= 0).all()
    assert [t.done for t in s.trees] == [T - 1] * 3 and all(int(t.n[0]) == T for t in s.trees)


def test_the_device_cases_contain_every_kind_of_event():
    """A collision round, a fallback, a -inf base, a tie and a kept root with non-zero seen among the cases of
    tests/test_gpu_gumbel.py (the events are those of the expectation with NumPy's base)."""
    total = collections.Counter()
    for N in (2, 5, 9):
        for L in (1, 3):
            roots, name = ge.size_case(N, L)
            s = ge.expected_gumbel(roots, ge.SIZE_ROUNDS, L, ge.EVALUATORS[name][0], ge.SIZE_M, c=1.25, komi=0.5)
            total.update(s.events())
            assert not s.state()['v'].any()
    for k in ('collision', 'fallback', 'neg_inf', 'tie'):
        assert total[k] > 0, (k, total)
    # across moves: kept roots whose children carry visits when the next move's search begins, and a run past the schedule
    roots = cs.stack(5, ('mid0', 'late0', 'empty', 'ended'))
    s = ge.Search(roots, 5, 3, 4, c=1.25, komi=0.5)
    past = 0
    for mv in range(3):
        for _ in range(5):
            s.round(pe.hash_evaluator_np)
        kept = s.advance(s.readout()[0])
        past += s.events()['past']
        if mv == 0:
            assert any(k > 0 for k in kept) and any(t.seen.any() for t in s.trees)
    assert past > 0
