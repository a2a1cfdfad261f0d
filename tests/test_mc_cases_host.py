"""CPU: what tests/test_gpu_mc_sizes.py relies on, without a device - at every board size from 2 to 19 the roots of
tests/mc_cases.py are valid positions of every kind the device test names, and the expectations on them are not vacuous:
eyes to avoid, searches that walk below the root's children, every kind of advance, playouts that are cut off and playouts that
all end.  A generator that drifts turns this file red instead of letting a device case pass on nothing."""
import numpy as np
import pytest

import mc_cases as cs
import mc_expect as mc
import mc_policy_expect as mp
import mc_puct_advance_expect as pa
import mc_puct_expect as pe
import mc_puct_leaves_expect as pl
import test_gpu_puct_advance as tpa
from oracle import c_oracle


def test_the_sizes_cover_every_row_alignment():
    """The arithmetic the all-sizes case rests on (k_puct_advance moves rows of A = N^2 + 1 and W = 5 N + 1 words as dwordx4
    plus a tail of words % 4): even sizes put A on the odd alignment no odd size reaches, the sizes between them reach
    every alignment of W, and the lane-stride edges A = 5, 65 and 257 are among the sizes."""
    for N in cs.SIZES:
        assert (N * N + 1) % 4 == (1 if N % 2 == 0 else 2), N
    assert {(5 * N + 1) % 4 for N in cs.SIZES} == {0, 1, 2, 3}
    assert {(5 * N + 1) % 4 for N in cs.SIZES if N % 2 == 0} == {1, 3} and {(5 * N + 1) % 4 for N in cs.SIZES if N % 2} == {0, 2}
    assert {5, 65, 257} <= {N * N + 1 for N in cs.SIZES}
    assert tuple(cs.SIZES) == tuple(range(2, 20))


@pytest.mark.parametrize('N', cs.SIZES)
def test_roots_are_valid_positions_of_every_kind(N):
    roots = cs.size_roots(N)
    S = cs.stack(N)
    assert S.dtype == np.uint8 and S.shape[1:] == (6, N, N) and len(roots) == S.shape[0] <= 12
    assert len(roots) == (12 if N >= 4 else 11) and ('ko' in roots) == (N >= 4)        # 2 and 3 have no ko root
    assert S.max() <= 1 and not (S[:, 0] & S[:, 1]).any()
    for p in (2, 4, 5):
        assert (S[:, p] == S[:, p, :1, :1]).all(), p
    for name, r in roots.items():
        # plane 3 is the invalid mask of planes 0 - 2 (the restatement's `player`: who moved last), but for an active ko point
        inv = c_oracle.compute_invalid_moves(r, 1 - int(r[2, 0, 0]))
        extra = np.argwhere(r[3] != inv)
        assert len(extra) <= 1, (name, extra[:4])                       # (random play meets a ko now and then)
        for y, x in extra:
            assert r[3, y, x] == 1 and not r[:2, y, x].any() and not r[5].any(), (name, y, x)
        if name == 'ko':
            assert extra.tolist() == [list(mc.KO_POINT)]
    assert np.array_equal(S, np.stack([r for _, r in cs._size_roots.__wrapped__(N)]))                       # deterministic
    ended = S[:, 5, 0, 0] != 0
    assert ended[list(roots).index('ended')] and ended[list(roots).index('played_out')] and not ended.all()
    # a root whose pass child is terminal, a white-to-move root, roots where the mover has no candidate, eyes to avoid
    passed = roots['passed']
    assert passed[4].all() and not passed[5].any() and c_oracle.next_state(passed, N * N)[5].all()
    assert (S[~ended, 2, 0, 0] != 0).any() and roots['forced_white'][2].all()
    assert mp.eyes(S).sum() > 0 and mp.eyes(S[list(roots).index('forced_black')][None]).sum() == 2
    assert not mp.candidates(cs.stack(N, ('forced_black', 'forced_white'))).any()
    # the late roots: live, one to six legal points
    for k in ('late0', 'late1', 'late2'):
        assert not roots[k][5].any() and 1 <= int((roots[k][3] == 0).sum()) <= cs.LATE_POINTS, k
    assert not S[[list(roots).index(k) for k in cs.search_names(N)], 5].any()
    mv = cs.stack(N, cs.move_names(N))[:, 5, 0, 0]
    assert mv.tolist() == [0, 0, 1]


@pytest.mark.parametrize('N', cs.SIZES)
def test_searches_walk_below_the_children_of_the_late_roots(N):
    """UCT descends by its argmax only where every legal action of a node has a child: under the iteration count of the
    device test every late root's tree has nodes whose parent is not the root, and so have the PUCT trees."""
    names = cs.search_names(N)
    u = mc.expected_uct(cs.stack(N, names), cs.UCT_I, cs.UCT_K, komi=0.5)
    for i, k in enumerate(names):
        if k.startswith('late'):
            assert cs.deep_nodes(u['tree']['parent'][i]) >= 5, (k, u['tree']['parent'][i])
    roots = cs.size_roots(N)
    late = [i for i, k in enumerate(roots) if k.startswith('late')]
    I = cs.puct_iterations(N)
    for name in ('hash', 'hostile'):
        p = pe.expected_puct(cs.stack(N), I, tpa.EVALUATORS[name][0], komi=0.5)
        for i in late:
            assert cs.deep_nodes(p['tree']['parent'][i]) > 0, (name, i)
    for L, T in ((4, 6), (64, 2)):
        p = pl.expected_puct_leaves(cs.stack(N), T, L, pe.hash_evaluator_np, komi=0.5)
        live = np.stack(p['live'])
        assert live.any() and (L < 64 or not live.all()), (L, T)          # 64 slots: more than some root can fill
        if L == 4:
            assert sum(cs.deep_nodes(p['tree']['parent'][i]) for i in late) > 0
    # the finished and the full boards are scored by the device: the value depends on the komi
    sc = cs.stack(N, cs.scored_names(N))
    a, b = (pe.expected_puct(sc, I, pe.hash_evaluator_np, komi=k) for k in (0.0, -0.5))
    assert not np.array_equal(pe.bits(a['root_value_sum']), pe.bits(b['root_value_sum']))
    assert (a['nodes'][:2] == 1).all() and (a['nodes'][2:] > 1).all()


@pytest.mark.parametrize('N', cs.SIZES)
def test_the_advance_cases_mix_every_kind_of_move(N):
    """all five kinds at every N >= 3; at N = 2 too with one leaf a round, with four leaves a round every legal action has a
    child there: no 'unvisited', no fresh tree (mc_cases.advance_kinds / noise_kinds say so)."""
    S = cs.stack(N)
    T = cs.ADVANCE_T
    for L, name in cs.TREE_CASES:
        trees = pa.make_trees(S, 2 * T * (L or 1) + 7, L)
        pa.search_rounds(trees, T, L, tpa.EVALUATORS[name][0], 1.25, 0.5)
        acts, kinds = tpa._mixed_actions(trees)
        assert set(kinds) == cs.advance_kinds(N, L), (L, kinds)
        if N >= 3 or L is None:
            assert cs.advance_kinds(N, L) == cs.ALL_KINDS
        kept = [pa.advance(t, int(a), pa.next_root(t, int(a))) for t, a in zip(trees, acts)]
        assert any(k > 1 for k in kept) and (0 in kept) == ('unvisited' in kinds), (L, kept)
        # the move of the noise-and-policy case
        trees = pa.make_trees(S, 3 * T * (L or 1) + 5, L)
        pa.search_rounds(trees, T, L, tpa.EVALUATORS[name][0], 1.25, 0.5)
        for r, t in enumerate(trees):
            free = [int(a) for a in t.legal[0] if t.child[0, a] < 0]
            a = free[-1] if r % 3 == 1 and free else pa.most_visited_root(t)
            pa.advance(t, a, pa.next_root(t, a))
        kinds = {'ended' if t.legal[0].size == 0 else ('kept' if t.n[0] > 0 else 'fresh') for t in trees}
        assert kinds == cs.noise_kinds(N, L), (L, kinds)


@pytest.mark.parametrize('N', cs.SIZES)
def test_playouts_are_cut_off_under_one_chunk_and_end_under_the_full_cap(N):
    """One chunk of 8 plies cuts playouts off at every size and under both policies; one chunk of 32 plies does from N = 4
    on.  Under the full cap every uniform playout ends; so does every no_eye_fill playout from N = 3 on - at 2x2 that policy
    passes only when no point is left to play, and some games go round in captures for ever."""
    roots = cs.playout_roots(N)
    K = cs.PLAYOUT_K
    assert roots.shape[0] * K > max(cs.SLOTS)
    assert cs.full_cap(N) % 8 == 0 and cs.full_cap(N) % 32 == 0 and cs.full_cap(N) >= 8 * N * N
    for expected, policy in ((mc.expected_playouts, False), (mp.expected_playouts_policy, True)):
        for cut in cs.CHUNKS:
            e = expected(roots, K, cut, komi=0.5)
            if cut == 8 or N >= 4:
                assert e['unfinished'].sum() > 0, (policy, cut)
        e = expected(roots, K, cs.full_cap(N), komi=0.5)
        if N >= 3 or not policy:
            assert e['unfinished'].sum() == 0, policy
        assert e['plies_sum'].sum() > 0
