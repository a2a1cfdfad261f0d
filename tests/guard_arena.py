"""A guarded arena: every buffer of a call stands at a chosen residue mod 16 inside ONE uint8 tensor, between guards.

include/gymgo_amd.h promises for all entry points that bytes outside a buffer are read, never written, and that what it
declares `const` is left as it was.  A fresh torch allocation cannot show a breach of either: it is 256-byte aligned and
rounded up to 512 bytes, so a stray store lands in padding and most start residues of a board are never tried.  Here the
buffers are views of one tensor filled with a position-dependent pattern that holds neither 0 nor 1 (what boards, flags and
most small outputs are made of), each at the residue the caller names and with untouched pattern on both sides; snapshot()
records the tensor and violations() says which guard, or which read-only region, changed since.

Nothing here leaves an entry point's contract: the views are valid, naturally aligned memory whose 16-byte supersets lie
inside the arena.  A plain helper module (tests/test_guard_arena_host.py holds it on CPU tensors; tests/test_gpu_guarded.py
uses it on the device).
"""
import collections

import torch

ALIGN = 16
MIN_GUARD = 1024       # bytes of pattern on each side of a region, at least; and at least two records of the region

Region = collections.namedtuple('Region', 'name start nbytes guard readonly view')


def pattern(nbytes, device='cpu', first=0):
    """The arena's fill over absolute byte indices first .. first + nbytes: 0x80 | ((i * 37) & 0x7F), never 0 and never 1."""
    i = torch.arange(first, first + nbytes, dtype=torch.int64, device=device)
    return (((i * 37) & 0x7F) | 0x80).to(torch.uint8)


def element_size(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def residues(dtype):
    """The residues mod 16 a pointer to `dtype` may have: the multiples of the element size."""
    return tuple(range(0, ALIGN, element_size(dtype)))


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def guard_bytes(shape, dtype):
    """Pattern on each side of a region: two records (one board, one row of the array) and 1 KiB at least, whole 16-byte units."""
    record = _numel(shape[1:]) * element_size(dtype)
    g = max(2 * record, MIN_GUARD)
    return (g + ALIGN - 1) // ALIGN * ALIGN


def footprint(shape, dtype):
    """Bytes of arena a take() of this shape uses at most, guards and residue included."""
    return 2 * guard_bytes(shape, dtype) + _numel(shape) * element_size(dtype) + 2 * ALIGN


class Arena:
    def __init__(self, nbytes, device='cpu'):
        # (the base of the tensor is brought to a 16-byte boundary by hand: residues are those of the real address)
        self._raw = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=device)
        skip = -self._raw.data_ptr() % ALIGN
        self.bytes = self._raw[skip:skip + nbytes]
        assert self.bytes.data_ptr() % ALIGN == 0
        self.bytes.copy_(pattern(nbytes, device))
        self.regions = {}
        self._cursor = 0
        self._snap = None

    def take(self, name, shape, dtype, residue, readonly=False):
        """A contiguous view of `shape` and `dtype` with data_ptr() % 16 == residue, guards of untouched pattern on both sides.
        readonly: violations() reports a change INSIDE the region too (an `in` buffer; any buffer of an empty batch)."""
        es = element_size(dtype)
        if not 0 <= residue < ALIGN or residue % es:
            raise ValueError('%s: residue %d is no multiple of the element size %d below 16' % (name, residue, es))
        if name in self.regions:
            raise ValueError('%s is taken already' % name)
        shape = tuple(int(s) for s in shape)
        if _numel(shape) < 1:
            raise ValueError('%s: an empty view has no address (shape %r)' % (name, shape))
        guard, nbytes = guard_bytes(shape, dtype), _numel(shape) * es
        start = self._cursor + guard + residue          # cursor and guard are multiples of 16
        end = start + nbytes
        after = (end + guard + ALIGN - 1) // ALIGN * ALIGN
        if after > self.bytes.numel():
            raise ValueError('%s: the arena is full (%d bytes wanted, %d there)' % (name, after, self.bytes.numel()))
        view = self.bytes[start:end].view(dtype).view(shape)
        assert view.data_ptr() % ALIGN == residue and view.is_contiguous()
        self.regions[name] = Region(name, start, nbytes, guard, readonly, view)
        self._cursor = after
        self._snap = None                                # a snapshot describes the regions it was taken with
        return view

    def refill(self, name):
        """Put the arena's fill back into a region (before a call that must not write it: a store of what is already there
        would go unseen)."""
        r = self.regions[name]
        self.bytes[r.start:r.start + r.nbytes] = pattern(r.nbytes, self.bytes.device, r.start)

    def set_readonly(self, name, readonly=True):
        self.regions[name] = self.regions[name]._replace(readonly=readonly)

    def snapshot(self):
        self._snap = self.bytes.clone()

    def violations(self):
        """[(name, side, offset)] since snapshot(): side 'before' / 'after' with the offset of the first changed guard byte counted
        from the region's edge outwards ('after', 0 = the first byte past the region; 'before', 0 = the last byte in front of
        it), or 'inside' with the first changed byte of a read-only region counted from its start.  Bytes of the arena that belong
        to no region and no guard count as the guard of the region before them."""
        if self._snap is None:
            raise RuntimeError('violations() without a snapshot()')
        diff = self.bytes != self._snap
        writable = [r for r in self.regions.values() if not r.readonly]
        if writable:                                     # one reduction on the good path, whatever the number of regions
            diff = diff.clone()
            for r in writable:
                diff[r.start:r.start + r.nbytes] = False
        if not bool(diff.any()):
            return []
        found = []
        regions = sorted(self.regions.values(), key=lambda r: r.start)
        for k, r in enumerate(regions):
            end = r.start + r.nbytes
            hi = regions[k + 1].start - regions[k + 1].guard if k + 1 < len(regions) else diff.numel()
            before = diff[r.start - r.guard:r.start].flip(0).nonzero()
            if before.numel():
                found.append((r.name, 'before', int(before[0])))
            if r.readonly:
                inside = diff[r.start:end].nonzero()
                if inside.numel():
                    found.append((r.name, 'inside', int(inside[0])))
            behind = diff[end:hi].nonzero()
            if behind.numel():
                found.append((r.name, 'after', int(behind[0])))
        assert found, 'a byte changed outside every region and guard'
        return found
