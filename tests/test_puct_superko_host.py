"""CPU: the premises of tests/test_gpu_puct_superko.py, asserted on the expectation alone (tests/mc_puct_superko_expect.py).
The plain search walks cycles below the root on small boards - the counts below - and the ruled search has none; the marks a
node gets when it is made are the marks it would get after an advance, against the longer history; the planted cases of the
launch test contain what they claim; and the argument errors that need no device."""
import numpy as np
import pytest

import mc_expect as mc
import mc_puct_expect as pe
import mc_puct_superko_expect as se

C_PUCT, KOMI = 0.6, 0.5
# (N, evaluator, iterations) -> nodes per root that a board move reaches and that have the stones of one of their own ancestors
COUNTS = {(2, 'hash', 64): (0, 1, 6, 0, 9, 0, 0), (3, 'pass', 200): (0, 0, 0, 4, 0, 2, 0)}
EVAL = {'hash': pe.hash_evaluator_np, 'pass': pe.pass_evaluator_np}


def roots7(N):
    return mc.make_roots(N, 7, 60 + N, max_ply=N * N, step=1)


@pytest.mark.parametrize('case', sorted(COUNTS))
def test_the_plain_search_repeats_positions_below_the_root_and_the_ruled_search_does_not(case):
    N, name, I = case
    roots = roots7(N)
    plain = se.expected_puct(roots, None, I, EVAL[name], c=C_PUCT, komi=KOMI, rule=False)
    ruled = se.expected_puct(roots, None, I, EVAL[name], c=C_PUCT, komi=KOMI)
    want = pe.expected_puct(roots, I, EVAL[name], c=C_PUCT, komi=KOMI)
    for k in pe.TREE_KEYS:                                      # rule=False is the plain expectation
        assert np.array_equal(pe.bits(plain['tree'][k]), pe.bits(want['tree'][k])), k
    assert tuple(len(se.repeats(t)) for t in plain['trees']) == COUNTS[case]
    assert all(not se.repeats(t, t.history) for t in ruled['trees'])
    for r, n in enumerate(COUNTS[case]):
        same = all(np.array_equal(pe.bits(plain['tree'][k][r]), pe.bits(ruled['tree'][k][r])) for k in pe.TREE_KEYS)
        assert same == (n == 0), (case, r, n)                   # the rule changes exactly the trees that repeated


@pytest.mark.parametrize('leaves', (None, 2))
def test_marks_made_at_creation_are_the_marks_after_an_advance(leaves):
    """Every kept node, re-marked from scratch against (the longer history + its new chain), gets the points it already has."""
    N, T, M = 2, 16, 4
    roots = roots7(N)
    checked = [0]

    def on_move(mv, trees, acts, kept):
        for t in trees:
            for y in range(1, len(t.boards)):
                if t.boards[y] is None or t.action[y] == N * N:
                    continue
                bare = t.boards[y].copy()
                bare[3] = mc_plain_invalid(t, y)
                again = se.recreating(bare, t.history | t.chain_keys(int(t.parent[y])))
                have = [a for a in np.flatnonzero(t.boards[y][3].reshape(-1)) if bare[3].reshape(-1)[a] == 0]
                assert sorted(again) == sorted(int(a) for a in have), (mv, y)
                checked[0] += len(again)

    def mc_plain_invalid(t, y):
        from oracle import c_oracle
        parent = t.boards[int(t.parent[y])].copy()
        return c_oracle.next_state(parent, int(t.action[y]))[3]          # plane 3 as the game's own rules leave it

    se.expected_puct_play(roots, M, T, pe.hash_evaluator_np, c=C_PUCT, komi=KOMI, leaves=leaves, capacity=256, on_move=on_move)
    assert checked[0] > 0


def test_play_and_selfplay_expectations_never_recreate_a_position():
    N, M, T = 2, 10, 6
    roots = roots7(N)
    for reuse in (True, False):
        acts, final, trees = se.expected_puct_play(roots, M, T, pe.hash_evaluator_np, c=C_PUCT, komi=KOMI, leaves=2, capacity=128,
                                                   reuse=reuse)
        from oracle import c_oracle
        for r in range(len(roots)):
            cur, keys = roots[r].copy(), {se.key_of(roots[r])}
            for a in acts[r]:
                if a < 0:
                    continue
                cur[3] = 0
                cur = c_oracle.next_state(cur, int(a))
                assert a == N * N or se.key_of(cur) not in keys, (reuse, r)
                keys.add(se.key_of(cur))
            assert np.array_equal(cur[:2], final[r][:2])


@pytest.mark.parametrize('N', range(2, 20))
def test_planted_cases_contain_what_they_claim(N):
    c = se.planted(N)
    flagged = lambda i, a: bool((int(c.rows[i, a // N]) >> (a % N)) & 1)
    assert c.C == 2 * se.CHUNK + 2 and c.states.shape[0] == 24
    assert c.hits and all(flagged(i, a) for i, a, _ in c.hits)
    assert c.decoys and not any(flagged(i, a) for i, a, _ in c.decoys)
    assert {w[0] for _, _, w in c.decoys} == {'off-chain', 'beyond count', 'other root'}
    on_chain = {w[1] for _, _, w in c.hits if w[0] == 'chain'}
    assert {0, se.CHUNK - 1, se.CHUNK, 2 * se.CHUNK - 1, 2 * se.CHUNK, c.C - 1} <= on_chain      # first, boundaries, node 0 at depth C
    assert {w[1] for _, _, w in c.hits if w[0] == 'history'} == {0, se.CHUNK - 1, se.CHUNK, c.H - 1}
    assert any(c.caps[i, a] for i, a, _ in c.hits)                                                # a capturing candidate is hit
    assert {int(v) for v in c.count} == set(se.COUNTS)
    for i, why in c.untouched.items():                                                            # skipped rows: nothing
        assert not c.rows[i].any(), why
    changed = np.argwhere(c.node_hash_after != c.node_hash)
    assert {(int(r), int(y)) for r, y in changed} <= {(i // c.L, int(c.leaf_id[i])) for i in c.marked}
    for i in c.marked:
        assert c.node_hash_after[i // c.L, c.leaf_id[i]] == c.hashes[i]
        assert se.chain_of(c.links, i // c.L, c.leaf_id[i], c.C) == c.chains[i] and c.chains[i][-1] == 0
        others = {int(c.leaf_id[k]) for k in c.marked if k != i and k // c.L == i // c.L}
        assert not others & set(c.chains[i])                     # no chain passes a node made in the same round
    # without the history fewer points are flagged, never others
    bare, _ = se.launch(c.states, c.hashes, c.moves, c.move, c.leaf_id, c.links, c.node_hash, None, None, c.C, c.L)
    only = {(i, a) for i, a, w in c.hits if w[0] == 'history'} - {(i, a) for i, a, w in c.hits if w[0] == 'chain'}
    assert not (bare & ~c.rows).any() and (N == 2 or only)        # (2x2: a board has at most two such candidates)
    assert all(not (int(bare[i, a // N]) >> (a % N)) & 1 for i, a in only)


def test_the_sizes_together_cover_every_chain_depth():
    depths = set()
    for N in range(2, 20):
        depths |= set(se.depth_plan(N)[:20])
    got = set()
    for N in (2, 9, 19):
        got |= set(se.planted(N).depths.values())
    assert depths >= set(range(1, se.C_CASE + 1)) and {1, se.C_CASE} <= got


def test_corrupt_links_cannot_loop_or_leave_the_slice():
    links = np.full((1, 6, 2), -1, np.int32)
    links[0, 5, 0], links[0, 4, 0], links[0, 3, 0] = 4, 4, 7          # a self-loop at 4; 3 points outside
    assert se.chain_of(links, 0, 5, 5) == [4] and se.chain_of(links, 0, 3, 5) == []
    links[0, 1:, 0] = np.arange(5)
    assert se.chain_of(links, 0, 5, 5) == [4, 3, 2, 1, 0] and se.chain_of(links, 0, 5, 3) == [4, 3, 2]


def test_argument_errors_that_need_no_device():
    import torch
    from gymgo_amd import gogame
    st = np.zeros((2, 6, 3, 3), np.uint8)
    E = lambda s, l: (None, None)
    for bad in ('roots', 1, None, 'Tree', 2.0):
        with pytest.raises(ValueError, match='superko'):
            gogame.puct_play(st, 1, 2, E, superko=bad)
        with pytest.raises(ValueError, match='superko'):
            gogame.puct_selfplay(st, 1, 2, E, superko=bad)
    hist = gogame.PositionHistory(2, 4, device='cpu')
    for bad in (gogame.PositionHistory(3, 4, device='cpu'), (hist.hashes.to(torch.int32), hist.count), 'history', 7):
        with pytest.raises(ValueError, match='history'):
            gogame.PuctSearch(torch.zeros((2, 6, 3, 3), dtype=torch.uint8), 4, superko=bad)
        with pytest.raises(ValueError, match='history'):
            gogame.batch_puct(torch.zeros((2, 6, 3, 3), dtype=torch.uint8), 4, E, superko=bad)
    # the table holds the entry point as the header spells it
    from gymgo_amd import _lib
    assert [p.name for p in _lib.ABI['gg_puct_superko']] == ['R', 'N', 'C', 'L', 'links', 'node_hash', 'history', 'count', 'H', 'leaf',
                                                             'move', 'leaf_id', 'hip_stream']
    assert len(_lib.EXPORTS) == 79
