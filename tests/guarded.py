"""Guarded device buffers for the tests that call the C ABI directly: an output lives inside a larger allocation that is
pre-filled with a quiet-NaN pattern no arithmetic produces, with canary floats in front of it and behind it, so that an
element the kernel does not write fails its comparison and a store outside the output is seen.  (No arithmetic on
numbers, that is: arithmetic on the pattern itself hands it on.  A test that fences operands and output of one launch
gives each buffer a word of its own, see words().)"""
import torch

CANARY = 0x7FC0BEEF          # a quiet NaN with a payload
MAX_FENCE = 4096             # canary floats on either side: one row of the buffer, at least 64, at most this many


class Guarded:
    """a [rows][C] fp32 tensor `t` = the columns [col0, col0 + C) of a [rows][ld] buffer that is moved `shift` floats off
    its 16-byte alignment, between two canary fences.  With ld > C the columns outside `t` are canaries as well."""

    def __init__(self, rows, C, dev, ld=None, col0=0, shift=0, word=CANARY):
        ld = C if ld is None else ld
        assert 0 <= col0 and col0 + C <= ld and 0 <= shift < 4
        self.rows, self.C, self.ld, self.col0, self.word = rows, C, ld, col0, word
        self.fence = (min(max(ld, 64), MAX_FENCE) + 3) // 4 * 4
        self.lo = self.fence + shift
        self.buf = torch.full((self.lo + rows * ld + self.fence,), word, dtype=torch.int32, device=dev)
        self.t = self.buf.view(torch.float32).as_strided((rows, C), (ld, 1), self.lo + col0)
        assert (self.t.data_ptr() - 4 * (shift + col0)) % 16 == 0

    @classmethod
    def flat(cls, n, dev):
        """n floats in a row"""
        return cls(1, n, dev)

    @classmethod
    def holding(cls, src, dev, ld=None, col0=0, shift=0, word=CANARY):
        """an operand: the 2-D tensor `src` inside the NaN pattern (whatever a kernel reads outside it shows up)"""
        g = cls(src.shape[0], src.shape[1], dev, ld, col0, shift, word)
        g.t.copy_(src)
        return g

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        b = self.buf.cpu()
        assert bool((b[:self.lo] == self.word).all()), f"{what}: the floats in front of the output were written"
        assert bool((b[self.lo + self.rows * self.ld:] == self.word).all()), f"{what}: the floats behind the output were written"
        if self.ld > self.C:
            body = b[self.lo:self.lo + self.rows * self.ld].view(self.rows, self.ld)
            assert bool((body[:, :self.col0] == self.word).all()) and bool((body[:, self.col0 + self.C:] == self.word).all()), \
                f"{what}: columns outside [{self.col0}, {self.col0 + self.C}) of the pitched rows were written"

    def untouched(self):
        return bool((self.buf.cpu() == self.word).all())

    def unwritten(self):
        """elements of the output itself that still hold the pattern"""
        return int((self.t.contiguous().view(torch.int32) == self.word).sum())

    def cpu(self):
        return self.t.detach().cpu().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# outputs that are not flat fp32: other element types, 4-D strided views, workspaces of an exact byte size
# ---------------------------------------------------------------------------------------------------------------------
CANARY16 = 0x7FC1            # two-byte elements: a bf16 quiet NaN with a payload (no conversion produces it)
NAN64_HIGH = 0x7FF8BEEF      # eight-byte elements: this word above the buffer's own, an fp64 quiet NaN with a payload
FINITE = 0x4AC0BEEF          # an in-place operand's fences: a finite float (6.3e6), see words()


def words(k, inplace=False):
    """The pattern of the k-th buffer of one launch.  Arithmetic hands a NaN operand's payload on to its result, so a
    kernel that runs a few elements past the end of operands and output alike computes, from the operands' fences, the
    very word the output's fence holds, and the store shows nowhere.  Every buffer of a launch therefore gets a word
    of its own: CANARY for the first, then quiet NaNs of other payloads.  An operand that is updated in place is its
    own source -- a NaN fence would be rewritten with itself -- so its fences hold finite floats, which any update,
    swap or product with a neighbour's NaN changes."""
    assert 0 <= k < 1000
    return (FINITE if inplace else CANARY) + 0x1000 * k


def _word16(word):
    """the two-byte pattern that goes with a four-byte word: CANARY16 for CANARY, then other bf16 quiet NaNs"""
    return CANARY16 + ((word - CANARY) // 0x1000) % 0x3E


FENCE = 64                   # elements on either side of a GuardedBytes / Guarded4D buffer

# element size -> the integer type the pattern is laid down in
_UNITS = {1: torch.int32, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class GuardedBytes:
    """n elements `t` of any `dtype` (double, int32 / uint32 as int32, uint64 as int64, bf16, uint8) between two fences
    of FENCE elements, moved `shift` elements of that type off the 16-byte alignment of the allocation.  The pattern
    is the CANARY word repeated (CANARY16 for two-byte elements; one-byte elements see its four bytes in turn; eight-byte
    elements have NAN64_HIGH above it, so that a double read from a fence is a NaN as well).  Every
    comparison is bitwise against the pattern as it was laid down."""

    def __init__(self, n, dtype, dev, shift=0, word=CANARY):
        size = torch.empty((), dtype=dtype).element_size()
        unit = _UNITS[size]
        word = {1: word, 2: _word16(word), 4: word, 8: (NAN64_HIGH << 32) | word}[size]
        assert n >= 0 and 0 <= shift and (FENCE * size) % 16 == 0
        self.n, self.dtype, self.size = n, dtype, size
        self.lo = FENCE + shift
        total = self.lo + n + FENCE
        if size == 1:
            raw = torch.full(((total + 3) // 4,), word, dtype=unit, device=dev).view(torch.uint8)
            self.buf, self.total = raw, total
        else:
            self.buf, self.total = torch.full((total,), word, dtype=unit, device=dev), total
        self.pristine = self.buf.cpu().clone()
        self.t = self.buf[self.lo:self.lo + n].view(dtype)
        assert (self.t.data_ptr() - size * shift) % 16 == 0

    @classmethod
    def holding(cls, src, dev, shift=0, word=CANARY):
        """an operand: the 1-D tensor `src` inside the pattern"""
        g = cls(src.numel(), src.dtype, dev, shift, word)
        g.t.copy_(src.reshape(-1))
        return g

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        b, lo, hi = self.buf.cpu(), self.lo, self.lo + self.n
        assert torch.equal(b[:lo], self.pristine[:lo]), f"{what}: the elements in front of the output were written"
        assert torch.equal(b[hi:], self.pristine[hi:]), f"{what}: the elements behind the output were written"

    def untouched(self):
        return torch.equal(self.buf.cpu(), self.pristine)

    def unwritten(self):
        """elements of the output itself that still hold the pattern (meaningless for one-byte elements)"""
        lo, hi = self.lo, self.lo + self.n
        return int((self.buf[lo:hi].cpu() == self.pristine[lo:hi]).sum())

    def cpu(self):
        return self.t.detach().cpu().contiguous()


def workspace(nbytes, dev, word=CANARY):
    """a workspace of exactly `nbytes` bytes (what an entry's *_workspace_bytes function returned) between fences: one
    byte too few in that function and the kernel writes a fence"""
    return GuardedBytes(int(nbytes), torch.uint8, dev, word=word)


class Guarded4D:
    """a [B, C, H, W] fp32 view `t` given by four element strides inside a patterned allocation, `shift` floats off
    its 16-byte alignment; check() verifies that EVERY element outside the view -- the fences and whatever the strides
    leave out between its elements -- still holds the pattern."""

    def __init__(self, shape, strides, dev, shift=0, word=CANARY):
        assert len(shape) == len(strides) == 4 and all(n >= 1 for n in shape) and all(s >= 0 for s in strides)
        self.shape, self.strides, self.word = tuple(shape), tuple(strides), word
        extent = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.lo = FENCE + shift
        self.buf = torch.full((self.lo + extent + FENCE,), word, dtype=torch.int32, device=dev)
        self.t = self.buf.view(torch.float32).as_strided(self.shape, self.strides, self.lo)
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool)
        inside.as_strided(self.shape, self.strides, self.lo).fill_(True)
        self.inside = inside
        assert int(inside.sum()) == shape[0] * shape[1] * shape[2] * shape[3], "the strides make elements overlap"
        assert (self.t.data_ptr() - 4 * shift) % 16 == 0

    @classmethod
    def holding(cls, src, strides, dev, shift=0, word=CANARY):
        """an operand: the 4-D tensor `src` laid out by `strides` inside the NaN pattern"""
        g = cls(tuple(src.shape), strides, dev, shift, word)
        g.t.copy_(src)
        return g

    @staticmethod
    def layout(shape, kind):
        """element strides of a [B, C, H, W] tensor: "nchw", "nhwc" (channels last), or "view" -- a window of an NCHW
        tensor one channel, three rows and five columns larger"""
        B, C, H, W = shape
        if kind == "nchw":
            return (C * H * W, H * W, W, 1)
        if kind == "nhwc":
            return (H * W * C, 1, W * C, C)
        assert kind == "view", kind
        return ((C + 1) * (H + 3) * (W + 5), (H + 3) * (W + 5), W + 5, 1)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        b = self.buf.cpu()
        bad = (b != self.word) & ~self.inside
        assert not bool(bad.any()), \
            f"{what}: {int(bad.sum())} floats outside the strided view were written, the first at {int(bad.nonzero()[0]) - self.lo} from its start"

    def untouched(self):
        return bool((self.buf.cpu() == self.word).all())

    def unwritten(self):
        return int((self.t.contiguous().view(torch.int32) == self.word).sum())

    def cpu(self):
        return self.t.detach().cpu().contiguous()
