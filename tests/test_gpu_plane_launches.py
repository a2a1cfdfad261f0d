"""-m gpu: WHICH entry points the Python host path queues, in which order and with which pointers NULL - what the docstrings
of gogame promise as "launch for launch" and "one launch more per select()".  A recorder stands in for the loaded library and
notes, per call, the entry point, the pointer parameters that went down as NULL (by the names of the binding table) and the
scalars other than the stream.  Results are not this file's business: the other -m gpu files compare them bit for bit.

The expected sequences are written out from the PuctSearch docstring; the smallest shapes at which an order or a NULL can go
wrong: N = 5, R = 3, two iterations, a constant evaluator on the device, leaves None and 2."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
N, R, ITERATIONS = 5, 3, 2
A = N * N + 1
F16 = 2     # FEATURE_DTYPES[torch.float16]


class Recorder:
    """A proxy of the loaded library: every attribute is the library's; a call of an entry point is noted in `calls` as
    (name, the pointer parameters that were NULL, {scalar parameter: value} without hip_stream)."""

    def __init__(self, real, table):
        self._real, self._table, self.calls = real, table, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        row = self._table.get(name)
        if row is None:
            return fn

        def noted(*args):
            assert len(args) == len(row), (name, len(args), len(row))
            nulls = tuple(p.name for p, a in zip(row, args) if not isinstance(p.kind, type) and a is None)
            scalars = {p.name: a for p, a in zip(row, args) if isinstance(p.kind, type) and p.name != 'hip_stream'}
            self.calls.append((name, nulls, scalars))
            return fn(*args)
        return noted

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def rec(monkeypatch):
    from gymgo_amd import _lib
    real = _lib.lib()
    table = {f: ps for key, t in vars(_lib).items() if key.startswith('ABI') and isinstance(t, dict) for f, ps in t.items()}
    proxy = Recorder(real, table)
    monkeypatch.setattr(_lib, '_lib', proxy)
    return proxy


def names(calls):
    return [c[0] for c in calls]


def roots():
    from gymgo_amd import gogame
    return gogame.batch_init_state(R, N, device='cuda:0')


def evaluate(search, handed):
    """The constant evaluator: uniform priors, zero values, on the device."""
    import torch
    B = handed[0].shape[0]
    search.backup(torch.full((B, A), 1.0 / A, dtype=torch.float32, device='cuda:0'), torch.zeros(B, dtype=torch.float32, device='cuda:0'))


# what a select() queues behind its select launch, what a backup() queues in front of its backup launch, what an advance() queues;
# SELECT / BACKUP stand for the two launches whose entry point depends on leaves= and gumbel=
PLAY, UNTRACK, LEGAL = 'gg_batch_play_moves_tracked', 'gg_batch_untrack_states', 'gg_puct_legal'
ADVANCE = [PLAY, 'gg_puct_advance', UNTRACK]
SETS = {'life': 'gg_batch_life_tracked', 'ladder': 'gg_batch_ladder_tracked', 'outcome': 'gg_batch_move_planes_tracked',
        'area': 'gg_batch_area_tracked'}
VARIANTS = {
    'plain': ({}, ['SELECT', PLAY, UNTRACK, LEGAL], ['BACKUP'], ADVANCE),
    'features': ({'features': 'f16'}, ['SELECT', PLAY, 'gg_batch_features_tracked', LEGAL], ['BACKUP'], ADVANCE),
    'life': ({'features': 'f16', 'life': True}, ['SELECT', PLAY, 'gg_batch_features_tracked', LEGAL, 'gg_batch_life_tracked'],
             ['BACKUP'], ADVANCE),
    'ladder': ({'features': 'f16', 'ladder': True}, ['SELECT', PLAY, 'gg_batch_features_tracked', LEGAL, 'gg_batch_ladder_tracked'],
               ['BACKUP'], ADVANCE),
    'outcome': ({'features': 'f16', 'outcome': True},
                ['SELECT', PLAY, 'gg_batch_features_tracked', LEGAL, 'gg_batch_move_planes_tracked'], ['BACKUP'], ADVANCE),
    'area': ({'features': 'f16', 'area': True}, ['SELECT', PLAY, 'gg_batch_features_tracked', LEGAL, 'gg_batch_area_tracked'],
             ['BACKUP'], ADVANCE),
    'all': ({'features': 'f16', 'life': True, 'ladder': True, 'outcome': True, 'area': True, 'past': True, 'symmetry': 7},
            ['SELECT', PLAY, 'gg_batch_draw_orient', 'gg_batch_features_tracked_oriented', LEGAL, 'gg_batch_symmetry_policy',
             'gg_batch_life_tracked', 'gg_batch_ladder_tracked', 'gg_batch_move_planes_tracked', 'gg_batch_area_tracked', 'gg_puct_past'],
            ['gg_batch_symmetry_policy', 'BACKUP'], ['gg_past_push_tracked'] + ADVANCE),
    'superko': ({'superko': True}, ['SELECT', PLAY, 'gg_puct_superko', UNTRACK, LEGAL], ['BACKUP'],
                [PLAY, 'gg_puct_advance', 'gg_batch_hash_tracked', UNTRACK]),
    'gumbel': ({'gumbel': 2}, ['SELECT', PLAY, UNTRACK, LEGAL], ['BACKUP'], ADVANCE + ['gg_gumbel_begin']),
}


def make_search(kw, leaves, states):
    import torch
    from gymgo_amd import gogame
    kw = dict(kw)
    if 'features' in kw:
        kw['features'] = torch.float16
    if kw.get('past'):
        kw['past'] = gogame.StoneHistory(R, N, 3, moves=True, device=states.device)
    if kw.get('superko'):
        kw['superko'] = gogame.PositionHistory(R, 8, states.device).push(gogame.batch_hash(states))
    return gogame.PuctSearch(states, ITERATIONS, leaves=leaves, **kw)


def entry_points(kw, leaves):
    if kw.get('gumbel') is not None:    # (leaves=None counts as leaves=1 there)
        return 'gg_gumbel_select_leaves', 'gg_puct_backup_leaves'
    return ('gg_puct_select', 'gg_puct_backup') if leaves is None else ('gg_puct_select_leaves', 'gg_puct_backup_leaves')


def check_select(calls, kw, leaves):
    """The NULL pointers and the scalars of the hand-out launches of one select()."""
    B = R * (leaves or 1)
    for name, nulls, scalars in calls:
        if name.startswith('gg_batch_features_tracked'):
            assert nulls == () and scalars == {'out_dtype': F16, 'B': B, 'N': N}, (name, nulls, scalars)
            assert name.endswith('_oriented') == ('symmetry' in kw)
        elif name in SETS.values():
            optional = {'gg_batch_life_tracked': ('settled',), 'gg_batch_ladder_tracked': ('aborted',), 'gg_batch_move_planes_tracked': (),
                        'gg_batch_area_tracked': ('side', 'counts')}[name]
            want = optional + (() if 'symmetry' in kw else ('orient',))
            assert sorted(nulls) == sorted(want) and scalars == {'out_dtype': F16, 'B': B, 'N': N}, (name, nulls, scalars)
        elif name == 'gg_puct_past':
            assert nulls == (() if 'symmetry' in kw else ('orient',)), nulls
            assert scalars == {'R': R, 'N': N, 'C': ITERATIONS * (leaves or 1), 'L': leaves or 1, 'H': 2, 'T': 3, 'moves': 1, 'out_dtype': F16}, scalars
        elif name == 'gg_batch_play_moves_tracked':
            assert nulls == ('played',) and scalars == {'B': B, 'N': N, 'T': 1}, (nulls, scalars)
        elif name == 'gg_batch_symmetry_policy':
            assert nulls == () and scalars == {'elem_size': 1, 'inverse': 0, 'B': B, 'N': N}, (nulls, scalars)
        else:
            assert nulls == (), (name, nulls)


@pytest.mark.parametrize('leaves', [None, 2])
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_search_launches(rec, variant, leaves):
    """Two select() / backup() rounds, one advance(), one more select(): the entry points in order, NULLs and scalars."""
    import torch
    kw, select, backup, advance = VARIANTS[variant]
    states = roots()
    search = make_search(kw, leaves, states)
    torch.cuda.synchronize()
    sel, bak = entry_points(kw, leaves)
    select = [sel if n == 'SELECT' else n for n in select]
    backup = [bak if n == 'BACKUP' else n for n in backup]
    rec.take()
    for _ in range(2):
        handed = search.select()
        calls = rec.take()
        assert names(calls) == select, (variant, leaves, names(calls))
        check_select(calls, kw, leaves)
        assert len(handed) == 2 + sum(k in kw for k in ('life', 'ladder', 'outcome', 'area', 'past'))
        evaluate(search, handed)
        calls = rec.take()
        assert names(calls) == backup, (variant, leaves, names(calls))
        if 'symmetry' in kw:
            assert calls[0][2] == {'elem_size': 4, 'inverse': 1, 'B': R * (leaves or 1), 'N': N}
    search.advance(torch.zeros(R, dtype=torch.int64, device='cuda:0'))
    assert names(rec.take()) == advance, (variant, leaves)
    search.select()
    calls = rec.take()
    assert names(calls) == select, (variant, leaves, names(calls))
    check_select(calls, kw, leaves)
    torch.cuda.synchronize()


def test_all_on_with_superko(rec):
    """Every plane set, past=, symmetry= and superko= with leaves=2: the twelve launches of a select() and the two of a backup()."""
    import torch
    kw = dict(VARIANTS['all'][0], superko=True)
    search = make_search(kw, 2, roots())
    rec.take()
    handed = search.select()
    calls = rec.take()
    assert names(calls) == [
        'gg_puct_select_leaves', 'gg_batch_play_moves_tracked', 'gg_puct_superko', 'gg_batch_draw_orient',
        'gg_batch_features_tracked_oriented', 'gg_puct_legal', 'gg_batch_symmetry_policy', 'gg_batch_life_tracked',
        'gg_batch_ladder_tracked', 'gg_batch_move_planes_tracked', 'gg_batch_area_tracked', 'gg_puct_past']
    check_select(calls, kw, 2)
    evaluate(search, handed)
    assert names(rec.take()) == ['gg_batch_symmetry_policy', 'gg_puct_backup_leaves']
    search.advance(torch.zeros(R, dtype=torch.int64, device='cuda:0'))
    assert names(rec.take()) == ['gg_past_push_tracked', 'gg_batch_play_moves_tracked', 'gg_puct_advance', 'gg_batch_hash_tracked',
                                 'gg_batch_untrack_states']
    torch.cuda.synchronize()


def plane_calls():
    """(tag, call(gogame, boards, tracked: bool, orient or None), entry point of byte planes, NULLs without orient beside orient)."""
    import torch
    own = lambda: torch.zeros((R, 2, N, N), dtype=torch.int32, device='cuda:0')
    side = lambda: torch.ones(R, dtype=torch.uint8, device='cuda:0')
    last = lambda: torch.full((R,), 3, dtype=torch.int32, device='cuda:0')
    t = lambda tracked: '_tracked' if tracked else ''
    fn = lambda g, stem, tracked: getattr(g, stem + t(tracked))
    return [
        ('features', lambda g, b, tr, o: fn(g, 'batch_features', tr)(b, orient=o), 'gg_batch_features', None),
        ('life', lambda g, b, tr, o: fn(g, 'batch_life', tr)(b, orient=o), 'gg_batch_life', ('settled',)),
        ('life settled', lambda g, b, tr, o: fn(g, 'batch_life', tr)(b, orient=o, settled=True), 'gg_batch_life', ()),
        ('ladder', lambda g, b, tr, o: fn(g, 'batch_ladder', tr)(b, orient=o), 'gg_batch_ladder', ('aborted',)),
        ('ladder aborted', lambda g, b, tr, o: fn(g, 'batch_ladder', tr)(b, orient=o, aborted=True), 'gg_batch_ladder', ()),
        ('move planes', lambda g, b, tr, o: fn(g, 'batch_move_planes', tr)(b, orient=o), 'gg_batch_move_planes', ()),
        ('area', lambda g, b, tr, o: fn(g, 'batch_area_planes', tr)(b, orient=o), 'gg_batch_area', ('side', 'counts')),
        ('area side', lambda g, b, tr, o: fn(g, 'batch_area_planes', tr)(b, orient=o, side=side()), 'gg_batch_area', ('counts',)),
        ('area counts', lambda g, b, tr, o: fn(g, 'batch_area_planes', tr)(b, orient=o, counts=True), 'gg_batch_area', ('side',)),
        ('area counts buffer', lambda g, b, tr, o: fn(g, 'batch_area_planes', tr)(
            b, orient=o, side=side(), counts=torch.empty((R, 2), dtype=torch.int32, device='cuda:0')), 'gg_batch_area', ()),
        ('tactics', lambda g, b, tr, o: fn(g, 'batch_tactics', tr)(b, orient=o), 'gg_batch_tactics', ()),
        ('patterns', lambda g, b, tr, o: fn(g, 'batch_patterns', tr)(b, orient=o), 'gg_batch_patterns', ('last',)),
        ('patterns last', lambda g, b, tr, o: fn(g, 'batch_patterns', tr)(b, last(), orient=o), 'gg_batch_patterns', ()),
        ('status', lambda g, b, tr, o: fn(g, 'batch_stone_status', tr)(b, own(), 4, orient=o), 'gg_batch_status', ('side', 'counts')),
        ('status counts', lambda g, b, tr, o: fn(g, 'batch_stone_status', tr)(b, own(), 4, (3, 4), orient=o, counts=True),
         'gg_batch_status', ('side',)),
        ('past', lambda g, b, tr, o: fn(g, 'batch_past_planes', tr)(b, g.StoneHistory(R, N, 3, moves=True, device=b.device), orient=o),
         'gg_batch_past', ()),
    ]


def test_public_plane_calls(rec):
    """Every public plane call queues exactly one entry point: its name, its NULL pointers and its scalars, from byte planes and
    from tracked boards, without and with orient."""
    import torch
    from gymgo_amd import gogame
    states = roots()
    boards = {False: states, True: gogame.batch_track(states)}
    orient = torch.arange(R, dtype=torch.int32, device='cuda:0')
    for tag, call, stem, optional in plane_calls():
        for tracked in (False, True):
            for o in (None, orient):
                rec.take()
                call(gogame, boards[tracked], tracked, o)
                calls = rec.take()
                want = stem + ('_tracked' if tracked else '')
                if optional is None:     # (the feature planes: an entry point of their own with orient, none of them takes NULL)
                    want, nulls = want + ('' if o is None else '_oriented'), ()
                else:
                    nulls = (() if o is not None else ('orient',)) + optional
                assert len(calls) == 1 and calls[0][0] == want and sorted(calls[0][1]) == sorted(nulls), (tag, tracked, o is None, calls)
                scalars = {'out_dtype': 3 if tag != 'features' else F16, 'B': R, 'N': N}
                if tag.startswith('status'):
                    scalars.update(playouts=4, num=3 if 'counts' in tag else 2, den=4 if 'counts' in tag else 3)
                if tag == 'past':
                    scalars.update(H=2, T=3, moves=1)
                assert calls[0][2] == scalars, (tag, calls[0][2])
    torch.cuda.synchronize()


def test_selfplay_batch_launches(rec):
    """selfplay_batch with every set on: the byte-plane entry points in hand-out order behind the oriented feature launch and the
    turn of pi, the history planes after them, the ownership target last."""
    import torch
    from gymgo_amd import gogame
    moves, dev = 2, 'cuda:0'
    states = roots()
    record = gogame.SelfPlay(torch.zeros((R, moves), dtype=torch.int64, device=dev), torch.zeros((R, moves, A), dtype=torch.float32, device=dev),
                             torch.zeros((R, moves), dtype=torch.float32, device=dev), torch.zeros(R, dtype=torch.int8, device=dev),
                             torch.full((R,), moves, dtype=torch.int32, device=dev), states, states[:, None].repeat(1, moves, 1, 1, 1))
    games, at = torch.arange(R, device=dev), torch.ones(R, dtype=torch.int64, device=dev)
    orient = torch.arange(R, dtype=torch.int32, device=dev)
    rec.take()
    res = gogame.selfplay_batch(record, games, at, orient, life=True, ladder=True, outcome=True, area=True, ownership=True, past=(3, True))
    calls = rec.take()
    assert names(calls) == ['gg_batch_features_oriented', 'gg_batch_symmetry_policy', 'gg_batch_life', 'gg_batch_ladder',
                            'gg_batch_move_planes', 'gg_batch_area', 'gg_past_push', 'gg_past_push', 'gg_batch_past', 'gg_batch_area']
    assert [c[1] for c in calls] == [(), (), ('settled',), ('aborted',), (), ('side', 'counts'), (), (), (), ()]
    assert [tuple(x.shape[1:]) for x in res[4:]] == [(4, N, N), (4, N, N), (12, N, N), (3, N, N), (8, N, N), (N, N), ()]
    gogame.selfplay_batch(record, games, at, orient)
    assert names(rec.take()) == ['gg_batch_features_oriented', 'gg_batch_symmetry_policy']
    torch.cuda.synchronize()
