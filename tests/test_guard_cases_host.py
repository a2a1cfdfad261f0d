"""CPU: the case table of tests/guard_cases.py against the five binding tables and the five headers - every entry point with a
device pointer has a case or a named sentinel test, roles follow the headers' `const`, every pointer sees every start residue
its element size allows, and the rollout cells reach every kernel family."""
import collections
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.importorskip('torch')
import guard_arena as ga       # noqa: E402
import guard_cases as gc       # noqa: E402
from test_gpu_dispatch_sizes import families_wanted, rollout_cells   # noqa: E402
from test_host_abi import header_declarations   # noqa: E402

HEADERS = ('gymgo_amd.h', 'gymgo_amd_area.h', 'gymgo_amd_past.h', 'gymgo_amd_gumbel.h', 'gymgo_amd_tactics.h')


def header_pointers():
    """{function: [(parameter name, declared const)]} of the pointer parameters of every `int32_t gg_*(...);` of the five
    headers, by the parser of tests/test_host_abi.py.  The stream is no pointer argument."""
    decls = {}
    for h in HEADERS:
        for fn, ps in header_declarations(h, const=True).items():
            assert fn not in decls, fn
            decls[fn] = [(name, const) for _, pointer, name, const in ps if pointer and name != 'hip_stream']
    return decls


def test_every_entry_point_with_a_device_pointer_has_a_case_or_a_named_sentinel_test():
    """Fails when an entry point is added to a binding table without a case.  gg_gumbel_sequence writes HOST memory and is
    exempt; nothing else is."""
    every = [f for t in gc.tables() for f, ps in t.items() if gc.pointer_params(f)]
    assert len(every) == len(set(every))
    decls = header_pointers()
    assert set(every) == {f for f, ptrs in decls.items() if ptrs}
    covered = {c.fn for c, _ in gc.table()}
    groups = (covered, set(gc.GUARDED_ELSEWHERE), set(gc.EXEMPT))
    count = collections.Counter(f for g in groups for f in g)
    assert sorted(f for f in every if count[f] != 1) == [], 'in none or in several of: the case table, GUARDED_ELSEWHERE, EXEMPT'
    assert sorted(set(count) - set(every)) == []
    assert set(gc.EXEMPT) == {'gg_gumbel_sequence'}
    for n in gc.SIZES:       # every board size runs every entry point of the table
        assert {c.fn for c, _ in gc.table() if c.n == n} == covered, n
    per_size = collections.Counter(c.n for c, _ in gc.table())
    print('guarded cases: %d entry points x %d sizes, %d cases (%s), %d entry points guarded elsewhere'
          % (len(covered), len(gc.SIZES), len(gc.table()), ', '.join('N=%d: %d' % kv for kv in sorted(per_size.items())),
             len(gc.GUARDED_ELSEWHERE)))


def test_every_sentinel_test_named_exists():
    """The named test exists and its own body works with sentinels.  That EVERY written buffer of the entry point stands between
    them there is read by hand (the comment above guard_cases.GUARDED_ELSEWHERE says what was read): the list stays short."""
    assert len(gc.GUARDED_ELSEWHERE) <= 12
    for fn, where in gc.GUARDED_ELSEWHERE.items():
        name, test = where.split('::')
        src = open(os.path.join(ROOT, 'tests', name)).read()
        m = re.search(r'^def %s\(.*?(?=^(?:def |@pytest|# -----)|\Z)' % re.escape(test), src, flags=re.M | re.S)
        assert m, (fn, where)
        assert re.search(r'sentinel|SENTINEL|MARK|room\(|planted\(', m.group(0)), (fn, where)


def test_roles_come_from_the_headers():
    """A pointer's role is `in` exactly when its declaration is const; NULL only where the header allows it; every pointer
    parameter is given in at least one case and every nullable one is NULL in at least one."""
    decls = header_pointers()
    given, null = collections.Counter(), collections.Counter()
    for c, res in gc.table():
        assert [name for name, _ in gc.pointer_params(c.fn)] == [name for name, _ in decls[c.fn]], c.fn
        for name, const in decls[c.fn]:
            role = c.roles[name]
            assert role in ('in', 'out', 'inout', 'null'), (c.fn, name, role)
            if role == 'null':
                assert name in gc.NULLABLE.get(c.fn, ()), (c.fn, name)
                null[c.fn, name] += 1
                assert name not in res
            else:
                assert (role == 'in') == const, (c.fn, name, role, const)
                given[c.fn, name] += 1
    for fn in {c.fn for c, _ in gc.table()}:
        for name, _ in decls[fn]:
            assert given[fn, name] > 0, (fn, name, 'never given')
        for name in gc.NULLABLE.get(fn, ()):
            assert null[fn, name] > 0, (fn, name, 'never NULL')
    assert set(gc.NULLABLE) <= {c.fn for c, _ in gc.table()}


def test_every_pointer_sees_every_residue_its_element_size_allows():
    seen = collections.defaultdict(set)
    sizes = {}
    for c, res in gc.table():
        by_size = collections.defaultdict(list)
        for name, r in res.items():
            dt = gc.pointer_dtype(c, name)
            # what a pointer needs: its element's alignment, a record's (gg_puct_stat starts with a double: 8), or the 16 bytes
            # the Gumbel header demands of stats - such a pointer gets what the header demands and nothing else
            need = gc.pointer_align(c, name)
            assert need >= ga.element_size(dt) and r in ga.residues(dt) and r % need == 0, (c.fn, name, r)
            seen[c.fn, name].add(r)
            sizes.setdefault((c.fn, name), set()).add(need)
            by_size[need].append(r)
        # the pointers of a call that need the SAME alignment stand in different classes while there are classes enough (16 / the
        # alignment of them); pointers of different alignments are not held apart: a byte pointer and a word pointer may both
        # stand at residue 4
        for es, rs in by_size.items():
            assert len(set(rs)) == min(len(rs), 16 // es), (c.fn, es, rs)
    for (fn, name), rs in sorted(seen.items()):
        want = set(range(0, 16, min(sizes[fn, name])))
        assert rs == want, (fn, name, sorted(want - rs))
    print('residues: %d pointer parameters, %d (parameter, residue) pairs' % (len(seen), sum(len(r) for r in seen.values())))


@pytest.mark.parametrize('n', gc.SIZES)
def test_the_rollout_cells_name_every_kernel_family(n):
    """For the batch sizes actually used, raggedness included: the table cannot silently stop reaching k_rollout5 or k_env_step16."""
    import bench
    cells = {(c.b, c.opts['plies'], c.opts['auto']) for c, _ in gc.table() if c.n == n and c.fn == 'gg_batch_rollout'}
    assert len(cells) == 2 * len(rollout_cells(n))
    for fn in ('gg_batch_rollout', 'gg_batch_rollout_ws'):
        mine = [c for c, _ in gc.table() if c.n == n and c.fn == fn]
        assert {(c.b, c.opts['plies'], c.opts['auto']) for c in mine} == cells
        for auto in (1, 0):
            named = {bench.rollout_kernel_name(n, c.b, c.opts['plies'], 1, bool(auto)) for c in mine if c.opts['auto'] == auto}
            # (families_wanted names k_rollout_lat with auto_reset on: its third template argument is the flag)
            want = {w if auto or not w.startswith('k_rollout_lat') else w.replace(', true, 0>', ', false, 0>') for w in families_wanted(n)}
            assert want <= named, (fn, auto, sorted(want - named))
    for (B0, plies), B in zip(rollout_cells(n), [gc.ragged(n, b, p) for b, p in rollout_cells(n)]):
        assert B0 - 3 <= B <= B0 and bench.rollout_kernel_name(n, B, plies, 1) == bench.rollout_kernel_name(n, B0, plies, 1)
    ragged = [B for (B0, _), B in zip(rollout_cells(n), [gc.ragged(n, b, p) for b, p in rollout_cells(n)]) if B != B0]
    assert len(ragged) >= len(rollout_cells(n)) - 1, ragged


def test_the_policy_rollouts_take_policies_0_1_and_2():
    for n in gc.SIZES:
        pol = {(c.fn, c.opts['policy']) for c, _ in gc.table() if c.n == n and 'policy' in c.opts and c.opts['build'] == 'rollout'}
        assert pol == {('gg_batch_rollout_tracked_policy', 0), ('gg_batch_rollout_tracked_policy', 1)} | {
            ('gg_batch_rollout_tracked_policy2', p) for p in (0, 1, 2)}
    halves = {c.dtypes['weights'] for c, _ in gc.table() if c.fn == 'gg_batch_env_step_tracked_weighted'}
    import torch
    assert {torch.bfloat16, torch.float16} <= halves
