"""Every entry point of the old core between guards: no byte written outside its buffers, no `const` input changed.

include/gymgo_amd.h promises both for all entry points ("bytes outside the buffer are read, never written").  The other tests
of these calls run on fresh torch allocations - 256-byte aligned, rounded up to 512 bytes - where a store a few elements past
last_actions[B-1] lands in padding and a board starts only at a few of the sixteen residues.  Here every buffer of a call is
a view of one guarded arena (tests/guard_arena.py) at a start residue that rotates over the table of tests/guard_cases.py
(entry points x board sizes 2, 3, 6, 9, 11, 13, 16, 19 x batch sizes on either side of every take-over of the dispatch, ragged).
Per case, tests/guard_cases.py::run_case asserts:
  1. the call returns 0;
  2. after a device synchronise no guard byte and no byte of an `in` region has changed (the message names the argument, the
     side and the offset);
  3. every `out` / `inout` region is bit-equal to the same call on plain, separately allocated tensors whose `out` tensors
     start from another fill than the arena's - an element neither run writes would differ, so every element of every `out`
     buffer of this table is written (no case declares an element that is left alone: a buffer a call writes only in part,
     such as the boards of a fresh tree or `plan`, is `inout` with content of the caller's);
  4. where oracle/c_oracle.py has the call (rollouts with generators and last actions, next states and status, areas, the
     invalid mask, padded and un-padded children, offsets, update_pieces) the arena's outputs equal the oracle's bit for bit,
     for every game.  For the rest the plain run is the comparison, and the existing tests of those calls tie the plain run to
     the expectation modules;
  5. the same call with B = 0 (R = 0) and all pointers valid returns 0 and changes no byte of the arena, regions included -
     after every region the full call wrote has got the arena's fill back, so that a store of what is there cannot go unseen;
  6. a pointer of which a header demands more than its element's alignment (stats of the Gumbel calls, out of the feature
     planes: 16 bytes) stands where the header wants it, and the same call with it 8 bytes off returns GG_E_BADARG and changes
     no byte of the arena.
Once per child process a byte just past a region is changed with a torch indexing op and violations() must name it.

As tests/test_gpu_dispatch_sizes.py: the library is sized for ONE compute unit (GYMGO_AMD_CUS=1, read once per process) in a
child per board size, so that a few hundred boards reach every kernel family; one more child runs the whole table at the
device's own CU count, where the same batches take the small-batch kernels.  The children run one after another.
The Monte Carlo queue and the UCT / first PUCT / Gumbel calls run on five roots with fewer slots than jobs, each call from the
buffers the calls before it leave (guard_cases.search_cases); the plane, hash and ring-push calls have cases too, since their
own files hold only some of their outputs between sentinels (guard_cases.plane_cases).  Four things are not bit-equal between
two runs or not untouched by an empty call, each by the header's own words, and each is held another way (guard_cases.run_case
says how): `order` of gg_batch_children_offsets (ties in any order: both runs are held against the rule), the opaque working
slots of the playout queue after an advance (which slot a job lands in: the two runs must hold the same whole records as a
multiset), the queue buffers after a begin with R = 0 (an empty queue is written: counter = {0, 0}), and offsets[0] = 0 of
gg_batch_children_offsets / gg_move_playouts_plan with an empty batch (offsets[B] = the total).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 6, 9, 11, 13, 16, 19)

SCRIPT = r'''
import json, sys, time
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import guard_arena, guard_cases
from gymgo_amd import _lib
sizes, one_cu = json.loads(sys.argv[1]), sys.argv[2] == '1'
assert (_lib.lib().gg_device_cus() == 1) == one_cu
assert tuple(guard_cases.SIZES) == %r
x = guard_cases.Ctx('cuda')
# the check can fail: one byte just past a region, one just before it, one inside a read-only one
a = guard_arena.Arena(8192, 'cuda')
probe, fixed = a.take('probe', (5, 3), torch.int32, 4), a.take('fixed', (7,), torch.uint8, 9, readonly=True)
a.snapshot()
assert a.violations() == []
probe.fill_(3)
assert a.violations() == []
r = a.regions['probe']
a.bytes[r.start + r.nbytes] = 0
assert a.violations() == [('probe', 'after', 0)], a.violations()
a.snapshot()
a.bytes[r.start - 1] = 0
fixed[2] = 0
assert a.violations() == [('probe', 'before', 0), ('fixed', 'inside', 2)], a.violations()
failures, count, seconds = [], 0, {}
for n in sizes:
    x.pos(n)
    torch.cuda.synchronize()
    t0 = time.time()
    for c, res in guard_cases.table():
        if c.n != n:
            continue
        count += 1
        try:
            found = guard_cases.run_case(c, res, x)
        except AssertionError as e:          # a mistake in the case itself: reported like a finding, the next case still runs
            found = ['the case could not be made: %%r' %% (e,)]
        if found:
            failures.append([guard_cases.describe(c, res), found])
    torch.cuda.synchronize()
    seconds[n] = round(time.time() - t0, 2)
print('GUARDED ' + json.dumps({'failures': failures, 'cases': count, 'seconds': seconds}))
''' % (ROOT, os.path.join(ROOT, 'tests'), SIZES)


def _child(sizes, cus):
    env = dict(os.environ)
    env.pop('GYMGO_AMD_CUS', None)
    if cus:
        env['GYMGO_AMD_CUS'] = str(cus)
    p = subprocess.run([sys.executable, '-c', SCRIPT, json.dumps(list(sizes)), '1' if cus == 1 else '0'], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('GUARDED ')][-1]
    got = json.loads(line[len('GUARDED '):])
    print('%d cases, seconds per size %s' % (got['cases'], got['seconds']))
    return got


def _report(got):
    lines = ['%s\n      %s' % (what, '\n      '.join(found)) for what, found in got['failures']]
    return '%d of %d cases:\n  %s' % (len(lines), got['cases'], '\n  '.join(lines))


@pytest.mark.parametrize('size', SIZES)
def test_no_byte_outside_the_buffers_at_one_compute_unit(size):
    got = _child([size], 1)
    assert got['cases'] > 280
    assert not got['failures'], _report(got)


def test_no_byte_outside_the_buffers_at_the_devices_cu_count():
    got = _child(SIZES, None)
    assert got['cases'] > 2300
    assert not got['failures'], _report(got)
