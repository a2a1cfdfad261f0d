"""CPU: the composed restatement of the PUCT options (tests/mc_puct_combo_expect.py) and the premises of
tests/test_gpu_puct_combo.py.  With the other options off the composed move loops ARE the five restatements they are composed of
(ps / se / ge expected_selfplay, se.expected_puct_play, ge.expected_play), bit for bit, on those modules' own test inputs; the
move-loop cases cover every allowed pair of option values; and every input a device test uses shows the interaction it was
written for - a root whose forbidden move has a visited child under it wherever superko=True meets reuse, a node the rule marked
below the root wherever superko='tree' runs, a fallback, a run past the schedule and a collision among the Gumbel cases, games
that end - so that no device test passes on games where nothing interacted.  The figures are printed (pytest -s)."""
import collections
import itertools

import numpy as np
import pytest

import mc_cases as cs
import mc_expect as mc
import mc_gumbel_expect as ge
import mc_puct_combo_expect as ce
import mc_puct_expect as pe
import mc_puct_selfplay_expect as ps
import mc_puct_superko_expect as se
import test_puct_superko_host as tsh

FIELDS = ('actions', 'pi', 'value', 'lengths', 'states', 'final_states', 'outcome')


def same(got, want, fields, tag):
    for k in fields:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, g.dtype, w.shape, w.dtype)
        assert np.array_equal(pe.bits(g), pe.bits(w)), (tag, k, np.argwhere(pe.bits(g) != pe.bits(w))[:8])


def shown(tag, events, extra=''):
    print('%-52s %s %s' % (tag, ' '.join('%s=%d' % (k, events[k]) for k in ce.EVENTS), extra))


# ---------------------------------------------------------------- 1. the reductions
@pytest.mark.parametrize('L,sample_moves', [(None, 0), (None, 3), (4, 2)])
def test_without_rule_and_gumbel_it_is_the_selfplay_restatement(L, sample_moves):
    """tests/test_puct_selfplay_host.py's records case."""
    N, T, M = 5, 16, 5
    roots = np.concatenate([mc.crafted_roots(N), mc.make_roots(N, 3, 9, max_ply=20, step=10)[1:2]])
    z = lambda mv, legal: np.where(legal, np.float32(1) / np.float32(8), np.float32(0)).astype(np.float32)
    for noise in (z, None):
        kw = dict(c=0.6, komi=0.5, leaves=L, noise=noise, sample_moves=sample_moves, seed=7, first_game=2)
        want = ps.expected_selfplay(roots, M, T, pe.hash_evaluator_np, **kw)
        got = ce.expected_selfplay(roots, M, T, pe.hash_evaluator_np, **kw)
        same(got, want, FIELDS, (L, sample_moves, noise is not None))
        assert got['rng'] == want['rng'] and not any(got['events'][k] for k in ce.EVENTS if k != 'collision')


@pytest.mark.parametrize('N', (2, 3))
@pytest.mark.parametrize('L', (None, 2))
def test_with_the_rule_alone_it_is_the_superko_restatement(N, L):
    """tests/test_puct_superko_host.py's roots and parameters: self-play, and play with and without reuse."""
    M, T = 10, 6
    roots = tsh.roots7(N)
    kw = dict(c=tsh.C_PUCT, komi=tsh.KOMI, leaves=L, capacity=128)
    want = se.expected_selfplay(roots, M, T, pe.hash_evaluator_np, sample_moves=2, seed=7, first_game=1, **kw)
    got = ce.expected_selfplay(roots, M, T, pe.hash_evaluator_np, superko='tree', sample_moves=2, seed=7, first_game=1, **kw)
    same(got, want, FIELDS, (N, L, 'selfplay'))
    assert N == 3 or got['events']['deep_marks'] > 0
    for reuse in (True, False):
        acts, final, _ = se.expected_puct_play(roots, M, T, pe.hash_evaluator_np, reuse=reuse, **kw)
        g_acts, g_final, _, _ = ce.expected_play(roots, M, T, pe.hash_evaluator_np, superko='tree', reuse=reuse, **kw)
        assert np.array_equal(g_acts, acts) and np.array_equal(g_final, final), (N, L, reuse)


def test_the_rule_at_the_roots_only_is_the_rule_of_forbid_root_on_the_plain_walk():
    """superko=True has no restatement of its own to reduce to: it must be the plain loop wherever forbid_root takes nothing,
    and must never play a move that recreates a position of its game."""
    from oracle import c_oracle
    N, M, T = 2, 12, 6
    roots = tsh.roots7(N)
    kw = dict(c=tsh.C_PUCT, komi=tsh.KOMI, leaves=2, capacity=256)
    ruled = ce.expected_selfplay(roots, M, T, pe.hash_evaluator_np, superko=True, **kw)
    plain = ce.expected_selfplay(roots, M, T, pe.hash_evaluator_np, superko=False, **kw)
    assert ruled['events']['root_forbid'] > 0 and ruled['events']['deep_marks'] == 0
    differ = 0
    for r in range(len(roots)):
        cur, keys = roots[r].copy(), {se.key_of(roots[r])}
        for a in ruled['actions'][r]:
            if a < 0:
                continue
            cur[3] = 0
            cur = c_oracle.next_state(cur, int(a))
            assert a == N * N or se.key_of(cur) not in keys, r
            keys.add(se.key_of(cur))
        differ += not np.array_equal(ruled['actions'][r], plain['actions'][r])
    assert differ > 0


@pytest.mark.parametrize('reuse', (True, False))
def test_with_gumbel_alone_it_is_the_gumbel_restatement(reuse):
    """tests/test_gpu_gumbel.py's move-loop inputs."""
    N, T, L, m = 5, 4, 2, 4
    A = N * N + 1
    roots = cs.stack(N, ('empty', 'mid0', 'late0', 'passed', 'ended'))
    for g_of in (None, lambda mv, legal: ge.dyadic_g(5, A, mv, salt=9)):
        moves = 5
        kw = dict(komi=0.5, capacity=moves * T * L + 1)
        want, want_final, _ = ge.expected_play(roots, moves, T, L, pe.hash_evaluator_np, m, reuse=reuse, g_of=g_of, **kw)
        got, final, _, _ = ce.expected_play(roots, moves, T, pe.hash_evaluator_np, leaves=L, gumbel=m, g_of=g_of, reuse=reuse, **kw)
        assert np.array_equal(got, want) and np.array_equal(final, want_final), (reuse, g_of is not None)
        if reuse:
            moves = 6
            kw = dict(komi=0.5, capacity=moves * T * L + 1)
            want = ge.expected_selfplay(roots, moves, T, L, pe.hash_evaluator_np, m, g_of, **kw)
            got = ce.expected_selfplay(roots, moves, T, pe.hash_evaluator_np, leaves=L, gumbel=m, g_of=g_of, **kw)
            same(got, want, ('actions', 'pi', 'value', 'lengths', 'final_states'), (g_of is not None,))
            assert got['events'] == collections.Counter({k: v for k, v in want['search'].events().items() if v})


# ---------------------------------------------------------------- 2. the covering set
def test_the_move_loop_cases_cover_every_allowed_pair_of_option_values():
    cases = ce.covering_cases()
    assert all(ce.allowed(c) for c in ce.loop_cases())
    # the pairs, counted here from the factors alone: a pair is allowed if some call can carry it
    keys = [k for k, _ in ce.FACTORS]
    want = set()
    for fn in ('selfplay', 'play'):
        for values in itertools.product(*[v for _, v in ce.FACTORS]):
            c = dict(zip(keys, values))
            g = c['gumbel'] is not None
            ok = (not c['gumbel_noise'] or g) and (not g or (not c['noise'] and c['sample_moves'] == 0))
            ok = ok and (c['reuse'] if fn == 'selfplay' else (not c['noise'] and c['sample_moves'] == 0))
            if ok:
                want |= {frozenset(p) for p in itertools.combinations(sorted(c.items(), key=lambda kv: kv[0]), 2)}
    have = set()
    for c in cases:
        have |= {frozenset(p) for p in itertools.combinations(sorted((k, c[k]) for k in keys), 2)}
    assert have == want and len(want) > 100
    # what the issue names: Gumbel with each mode of the rule, the rule with noise and with the visit-count draw, in self-play
    sp = [c for c in ce.loop_cases() if c['fn'] == 'selfplay']
    assert {c['superko'] for c in sp if c['gumbel'] is not None and c['gumbel_noise']} >= {True, 'tree'}
    assert {c['superko'] for c in sp if c['noise']} >= {True, 'tree'} and {c['superko'] for c in sp if c['sample_moves']} >= {True, 'tree'}


# ---------------------------------------------------------------- 3. the events of every device input
def ends(final):
    ended = np.asarray(final)[:, 5, 0, 0] != 0
    return int(ended.sum()), int((~ended).sum())


def test_the_step_cases_contain_what_they_are_written_for():
    total, running = collections.Counter(), 0
    for case in ce.STEP_CASES:
        s = ce.run_steps(case)
        over, live = ends(np.stack([t.boards[0] for t in s.trees]))
        shown('steps ' + ce.step_id(case), s.tally, 'ended=%d running=%d' % (over, live))
        if case['mode'] is True:
            assert s.tally['root_forbid_kept_child'] >= 1 and s.tally['deep_marks'] == 0, ce.step_id(case)
        else:
            assert s.tally['deep_marks'] >= 1, ce.step_id(case)
        assert s.tally['noise_on_reduced'] >= 1 and over >= 1, ce.step_id(case)
        if case['names'] is not None:                               # the planted sizes: the rule fires on move 0 or 1 of most roots
            _, hist, _, _ = ce.step_inputs(case)
            assert sum(len(h) == 2 for h in hist) >= 3 and live >= 1, ce.step_id(case)
        running += live
        total.update(s.tally)
    for k in ('fallback', 'past', 'collision', 'tie', 'neg_inf'):
        assert total[k] >= 1, k
    assert running >= 1
    assert {c['N'] for c in ce.STEP_CASES} == {2, 3, 9, 19} and {c['N'] for c in ce.STEP_CASES if c['L'] is None} == {2, 9}


@pytest.mark.parametrize('N', (2, 5))
def test_the_move_loop_cases_contain_what_they_are_written_for(N):
    roots, ids = ce.loop_roots(N)
    ev_np = ge.EVALUATORS[ce.LOOP[N]['name']][0]
    total, noise_reduced = collections.Counter(), 0
    for case in ce.loop_cases():
        out = ce.run_loop_case(case, roots, ids, N, ev_np)
        events, final = (out['events'], out['final_states']) if isinstance(out, dict) else (out[3], out[1])
        over, live = ends(final)
        shown('loop N=%d %s' % (N, ce.case_id(case)), events, 'ended=%d running=%d' % (over, live))
        need = ce.needs(case)
        assert need is None or events[need] >= 1, (N, ce.case_id(case), need)
        assert over >= 1 and (live >= 1 or N == 2), (N, ce.case_id(case))
        if case['gumbel'] is not None:
            total.update(events)
        if case['superko'] and (case['noise'] or case['gumbel_noise']):
            noise_reduced += events['noise_on_reduced']
    for k in ('fallback', 'past', 'collision'):
        assert total[k] >= 1, (N, k)
    assert noise_reduced >= 1


@pytest.mark.parametrize('N,gumbel', ce.PLANE_CASES)
def test_the_plane_cases_contain_what_they_are_written_for(N, gumbel):
    roots, hist, g_of, _ = ce.plane_inputs(N, gumbel)
    host = ce.plane_host(N, gumbel)
    marks = []
    for mv in range(ce.PLANE_MOVES):
        ce.plane_move(host, mv, g_of)
        marks.append(host.tally['deep_marks'])
    ce.harvest(host.trees, host.tally)
    over, live = ends(host.boards())
    shown('planes N=%d gumbel=%s' % (N, gumbel), host.tally, 'ended=%d running=%d' % (over, live))
    assert marks[0] >= 1 and sum(len(h) == 2 for h in hist) >= 3 and over >= 1 and live >= 1


@pytest.mark.parametrize('N,gumbel', ce.SHARD_CASES)
def test_the_shard_cases_contain_what_they_are_written_for(N, gumbel):
    import test_gpu_symmetry_io as tsio
    roots, ids, cut = ce.shard_roots(N)
    e = ce.expected_shard(N, gumbel, tsio.point_evaluator)
    over, live = ends(e['final_states'])
    shown('shards N=%d gumbel=%s' % (N, gumbel), e['events'], 'ended=%d running=%d' % (over, live))
    assert e['events']['deep_marks'] >= 1 and over >= 1 and live >= 1
    assert cut % ce.SHARD_L and 0 < cut < len(roots)
    if gumbel is not None:
        assert e['events']['fallback'] >= 1 and e['events']['past'] >= 1 and e['events']['collision'] >= 1
    # the restatement itself concatenates: root r's game depends on root r, its id and its global index alone
    parts = [ce.expected_shard(N, gumbel, tsio.point_evaluator, rows=slice(None, cut)),
             ce.expected_shard(N, gumbel, tsio.point_evaluator, rows=slice(cut, None), first_game=ce.SHARD_FIRST + cut)]
    same({k: np.concatenate([p[k] for p in parts]) for k in FIELDS}, e, FIELDS, (N, gumbel))
