"""CPU: the guarded arena of tests/guard_arena.py on host tensors - alignment and guards of every dtype at every residue it may
have, and a changed byte before a region, after it and inside a read-only one each reported with its name, side and offset."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip('torch')
import guard_arena as ga   # noqa: E402

DTYPES = (torch.uint8, torch.bool, torch.float16, torch.bfloat16, torch.int32, torch.float32, torch.int64, torch.float64)


def test_the_fill_holds_neither_0_nor_1_and_depends_on_the_position():
    p = ga.pattern(4096)
    assert int(p.min()) >= 0x80 and p.dtype == torch.uint8
    assert len(set(p[:128].tolist())) == 128 and torch.equal(p[:128], p[128:256])      # 37 is odd: a period of 128 bytes
    assert torch.equal(ga.pattern(64, first=100), p[100:164])


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_take_gives_the_promised_alignment_and_guards(dtype):
    es = ga.element_size(dtype)
    assert ga.residues(dtype) == tuple(range(0, 16, es))
    shapes = ((7,), (5, 3), (2, 6, 19, 19), (1,))
    a = ga.Arena(sum(ga.footprint(s, dtype) for s in shapes) * len(ga.residues(dtype)), 'cpu')
    fill = a.bytes.clone()
    assert torch.equal(fill, ga.pattern(fill.numel()))
    end = 0
    for r in ga.residues(dtype):
        for k, shape in enumerate(shapes):
            name = 'r%d_%d' % (r, k)
            v = a.take(name, shape, dtype, r)
            reg = a.regions[name]
            assert v.data_ptr() % 16 == r and v.is_contiguous() and v.dtype == dtype and tuple(v.shape) == shape
            assert v.data_ptr() == a.bytes.data_ptr() + reg.start and reg.nbytes == v.numel() * es
            record = es
            for s in shape[1:]:
                record *= s
            assert reg.guard >= max(1024, 2 * record) and reg.guard % 16 == 0
            assert reg.start - reg.guard >= end                 # the guards of two regions do not share a byte
            end = reg.start + reg.nbytes + reg.guard
            assert end <= a.bytes.numel()
            # every 16-byte superset of the region lies inside the arena
            assert reg.start // 16 * 16 >= 0 and -(-(reg.start + reg.nbytes) // 16) * 16 <= a.bytes.numel()
    assert torch.equal(a.bytes, fill)                           # take() writes nothing
    a.snapshot()
    assert a.violations() == []
    for bad in (1, 16) if es > 1 else (16, -1):
        with pytest.raises(ValueError):
            a.take('bad', (3,), dtype, bad)
    if es > 1:
        with pytest.raises(ValueError):
            a.take('bad', (3,), dtype, es // 2)
    with pytest.raises(ValueError):
        a.take('r0_0', (3,), dtype, 0)                          # a name is taken once
    with pytest.raises(ValueError):
        a.take('empty', (0, 4), dtype, 0)                       # an empty view has no address to guard


def test_changes_are_reported_with_name_side_and_offset():
    a = ga.Arena(1 << 16, 'cpu')
    src = a.take('src', (4, 6, 3, 3), torch.uint8, 5, readonly=True)
    dst = a.take('dst', (9,), torch.int32, 12)
    tail = a.take('tail', (3, 2), torch.int64, 8)
    with pytest.raises(RuntimeError):
        a.violations()
    src.fill_(1)
    a.snapshot()
    assert a.violations() == []
    dst.fill_(7)                                               # a change inside an out region is not reported
    tail[1, 1] = 5
    assert a.violations() == []
    r = a.regions['dst']
    a.bytes[r.start + r.nbytes] ^= 0xFF                        # the byte just after dst
    assert a.violations() == [('dst', 'after', 0)]
    a.bytes[r.start + r.nbytes + 40] = 0
    assert a.violations() == [('dst', 'after', 0)]             # the first one
    a.snapshot()
    a.bytes[r.start - 1] = 0                                   # the byte just before dst
    a.bytes[r.start - 9] = 0
    assert a.violations() == [('dst', 'before', 0)]
    a.snapshot()
    src[2, 0, 1, 1] = 0                                        # inside a read-only region: byte 2 * 54 + 4
    assert a.violations() == [('src', 'inside', 112)]
    a.snapshot()
    s, t = a.regions['src'], a.regions['tail']
    a.bytes[s.start - s.guard] = 1                             # the far end of the first guard, the far end of the last
    a.bytes[t.start + t.nbytes + t.guard - 1] = 1
    assert a.violations() == [('src', 'before', s.guard - 1), ('tail', 'after', t.guard - 1)]
    a.snapshot()
    a.set_readonly('dst')                                      # the empty batch: every region is read-only
    dst[3] = 8
    assert a.violations() == [('dst', 'inside', 12)]
    a.snapshot()
    a.bytes[a.bytes.numel() - 1] = 0                           # arena bytes behind the last guard count as that guard's
    assert a.violations() == [('tail', 'after', a.bytes.numel() - 1 - (t.start + t.nbytes))]


def test_refill_puts_the_fill_back_into_one_region():
    a = ga.Arena(1 << 14, 'cpu')
    x, y = a.take('x', (5, 7), torch.int32, 4), a.take('y', (9,), torch.uint8, 3)
    fill = a.bytes.clone()
    x.fill_(0)
    y.fill_(1)
    a.refill('x')
    r = a.regions['y']
    assert torch.equal(a.bytes[:r.start], fill[:r.start]) and bool((y == 1).all())
    a.refill('y')
    assert torch.equal(a.bytes, fill)


def test_the_arena_says_when_it_is_full():
    a = ga.Arena(4096, 'cpu')
    a.take('x', (100,), torch.uint8, 3)
    with pytest.raises(ValueError):
        a.take('y', (4096,), torch.uint8, 0)
