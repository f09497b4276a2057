"""Operands between guard bands, for the tests that hold a kernel-level op to its buffers (tests/test_gpu_ops_bounds.py,
tests/test_gpu_train_ops_bounds.py).

A Guarded holds a (rows, cols) operand of row stride ld >= cols inside ONE allocation: a guard band in front, the rows, a guard
band behind.  The bands and the pad columns cols .. ld-1 of every row carry one fixed quiet-NaN bit pattern, so a read that
reaches the arithmetic poisons the result and a write of any other value -- another NaN included -- shows in an int32
comparison.  A band is max(1024, 128 ld) floats: 128 rows, the tallest tile any body uses, so a stray row of a whole tile
still lands inside the allocation.  `slabs` > 1 lays that many such operands slab_stride floats apart (the partial slabs of a
fused MLP launch, the members of a batched launch); the gaps between them carry the pattern too."""
import torch

GUARD_BITS = 0x7FC5EA7F      # a quiet NaN with a payload no arithmetic produces
NAN = float("nan")
SENTINEL = 12345.678         # the finite half of the canary (tests/test_gpu_linear_bwd.py)


def band_floats(ld):
    """Floats of one guard band for rows of stride ld: 128 rows, never below 1024; rounded up to a multiple of 4, so that the
    operand behind it starts on a 16-byte boundary."""
    return (max(1024, 128 * ld) + 3) // 4 * 4


def canary(*shape):
    """Fill of an output the call must not touch: NaN in the even elements (an overwrite shows), a finite sentinel in the odd
    ones (an accumulation shows as well)."""
    t = torch.full(shape, NAN)
    t.view(-1)[1::2] = SENTINEL
    return t


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).clone()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Guarded:
    """A (rows, cols) operand with row stride ld between two guard bands; `fill` is a tensor of the operand's shape, a number,
    or None for NaN (the regular NaN: an output the call has to write)."""

    def __init__(self, rows, cols, ld=None, fill=None, device="cuda", slabs=1, slab_stride=None):
        ld = cols if ld is None else ld
        one = (rows - 1) * ld + cols                            # first to last float of one slab
        slab_stride = one if slab_stride is None else slab_stride
        assert rows >= 1 and cols >= 1 and ld >= cols and slabs >= 1 and slab_stride >= one
        self.rows, self.cols, self.ld, self.slabs, self.slab_stride = rows, cols, ld, slabs, slab_stride
        self.band = band_floats(ld)
        self.span = (slabs - 1) * slab_stride + one             # first to last float of the operand
        host = torch.empty(2 * self.band + self.span, dtype=torch.float32)
        host.view(torch.int32).fill_(GUARD_BITS)
        body = self._view(host)
        if fill is None:
            body.fill_(NAN)
        elif torch.is_tensor(fill):
            body.view(torch.int32).copy_(fill.to(torch.float32).reshape(body.shape).view(torch.int32))   # bit for bit
        else:
            body.fill_(float(fill))
        valid = torch.zeros(host.numel(), dtype=torch.bool)
        self._view(valid).fill_(True)
        self.initial = bits(body)
        self.buf = host.to(device)
        self.outside = (~valid).to(device)
        self.ptr = self.buf.data_ptr() + 4 * self.band
        assert self.ptr % 16 == 0, "the operand is not 16-byte aligned"

    def _view(self, flat):
        v = flat.as_strided((self.slabs, self.rows, self.cols), (self.slab_stride, self.ld, 1), self.band)
        return v[0] if self.slabs == 1 else v

    @property
    def region(self):
        """The (rows, cols) view of the operand ((slabs, rows, cols) for more than one slab)."""
        return self._view(self.buf)

    def host(self):
        return self.region.cpu()

    def at(self, row=0, col=0):
        """Address of element (row, col): a column block of a wider row (q | k | v, K | V)."""
        return self.ptr + 4 * (row * self.ld + col)

    def first_damage(self):
        """None, or (band, row, column) of the first float outside the operand that lost the guard pattern.  band is "front",
        "pad" (a pad column, or the gap between two slabs) or "behind"; row and column count in rows of ld floats from the
        operand's first element (of its slab, for a pad), negative in front of it."""
        bad = ((self.buf.view(torch.int32) != GUARD_BITS) & self.outside).nonzero()
        if not bad.numel():
            return None
        off = int(bad[0]) - self.band
        if off < 0:
            return ("front", off // self.ld, off % self.ld)
        if off >= self.span:
            off -= (self.slabs - 1) * self.slab_stride
            return ("behind", off // self.ld, off % self.ld)
        off %= self.slab_stride
        return ("pad", off // self.ld, off % self.ld)

    def intact(self):
        """Whether both guard bands, every pad column and every gap still hold the guard pattern (first_damage() names the
        first float that does not)."""
        return self.first_damage() is None

    def keeps(self, want=None):
        """Whether the operand still holds the bits `want` (default: those it started with)."""
        return torch.equal(bits(self.region), self.initial if want is None else bits(want))

    def check(self, what, written=False, unchanged=False):
        """Assert intact(); written: no NaN left inside the operand; unchanged: keeps() its first bits."""
        d = self.first_damage()
        assert d is None, (f"{what}: wrote outside its {self.rows} x {self.cols} rows (stride {self.ld}): "
                           f"{d[0]} band, row {d[1]}, column {d[2]}")
        if written:
            nan = self.region.isnan().nonzero()
            assert not nan.numel(), f"{what}: NaN left at {tuple(int(v) for v in nan[0])} of a region the call had to write"
        if unchanged:
            assert self.keeps(), f"{what}: changed"


class GuardedSet:
    """The operands of one call, by name: check() asserts that every input is intact() and keeps() its bits and that every
    output is intact()."""

    def __init__(self, device="cuda"):
        self.device, self.inputs, self.outputs = device, {}, {}

    def inp(self, name, t, ld=None, slab_stride=None):
        """A (cols,), (rows, cols) or -- with slab_stride -- (slabs, rows, cols) input tensor as a Guarded of row stride ld."""
        t = t.reshape(1, -1) if t.dim() == 1 else t
        slabs = t.shape[0] if t.dim() == 3 else 1
        g = Guarded(t.shape[-2], t.shape[-1], ld, fill=t, device=self.device, slabs=slabs, slab_stride=slab_stride)
        self.inputs[name] = g
        return g

    def out(self, name, rows, cols, ld=None, fill=None, slabs=1, slab_stride=None):
        g = Guarded(rows, cols, ld, fill=fill, device=self.device, slabs=slabs, slab_stride=slab_stride)
        self.outputs[name] = g
        return g

    def check(self, what=""):
        for name, g in self.inputs.items():
            g.check(f"{what}: input {name}", unchanged=True)
        for name, g in self.outputs.items():
            g.check(f"{what}: output {name}")
