"""Guarded device buffers for the tests that call the C ABI directly: an output lives inside a larger allocation that is
pre-filled with a quiet-NaN pattern no arithmetic produces, with canary floats in front of it and behind it, so that an
element the kernel does not write fails its comparison and a store outside the output is seen."""
import torch

CANARY = 0x7FC0BEEF          # a quiet NaN with a payload
MAX_FENCE = 4096             # canary floats on either side: one row of the buffer, at least 64, at most this many


class Guarded:
    """a [rows][C] fp32 tensor `t` = the columns [col0, col0 + C) of a [rows][ld] buffer that is moved `shift` floats off
    its 16-byte alignment, between two canary fences.  With ld > C the columns outside `t` are canaries as well."""

    def __init__(self, rows, C, dev, ld=None, col0=0, shift=0):
        ld = C if ld is None else ld
        assert 0 <= col0 and col0 + C <= ld and 0 <= shift < 4
        self.rows, self.C, self.ld, self.col0 = rows, C, ld, col0
        self.fence = (min(max(ld, 64), MAX_FENCE) + 3) // 4 * 4
        self.lo = self.fence + shift
        self.buf = torch.full((self.lo + rows * ld + self.fence,), CANARY, dtype=torch.int32, device=dev)
        self.t = self.buf.view(torch.float32).as_strided((rows, C), (ld, 1), self.lo + col0)
        assert (self.t.data_ptr() - 4 * (shift + col0)) % 16 == 0

    @classmethod
    def flat(cls, n, dev):
        """n floats in a row"""
        return cls(1, n, dev)

    @classmethod
    def holding(cls, src, dev, ld=None, col0=0, shift=0):
        """an operand: the 2-D tensor `src` inside the NaN pattern (whatever a kernel reads outside it shows up)"""
        g = cls(src.shape[0], src.shape[1], dev, ld, col0, shift)
        g.t.copy_(src)
        return g

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        b = self.buf.cpu()
        assert bool((b[:self.lo] == CANARY).all()), f"{what}: the floats in front of the output were written"
        assert bool((b[self.lo + self.rows * self.ld:] == CANARY).all()), f"{what}: the floats behind the output were written"
        if self.ld > self.C:
            body = b[self.lo:self.lo + self.rows * self.ld].view(self.rows, self.ld)
            assert bool((body[:, :self.col0] == CANARY).all()) and bool((body[:, self.col0 + self.C:] == CANARY).all()), \
                f"{what}: columns outside [{self.col0}, {self.col0 + self.C}) of the pitched rows were written"

    def untouched(self):
        return bool((self.buf.cpu() == CANARY).all())

    def unwritten(self):
        """elements of the output itself that still hold the pattern"""
        return int((self.t.contiguous().view(torch.int32) == CANARY).sum())

    def cpu(self):
        return self.t.detach().cpu().contiguous()
