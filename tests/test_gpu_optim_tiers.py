"""The kernel-argument tiers of the optimizer entries (96 / 224 / 448 gradient addresses per launch) on the GPU:
lic_adam_run, lic_adam_run_scaled, lic_adam_run_ema (with and without clip_state), lic_grad_norm_partial and
lic_swap_run, driven through ctypes at 96, 97, 224, 225 and 448 tensors.

The update is elementwise and every partial sum belongs to one block of one tensor, so cutting the job list into
consecutive chunks of at most 96 jobs, each with its own lic_adam_plan table, cannot change a bit: one launch at any
tier must leave what the chunked launches of the 96 tier leave (the tier the model tests hold to torch and to the
numpy restatements).  A wrong tier reads gradient addresses from beyond the filled part of the argument block.

Tensor i has (1, 3, 4, 5, 8)[i % 5] elements; tensor 1 has 4097 (two blocks, a scalar tail) and a gradient one float
off the 16-byte grid (the scalar path); the average of tensor 2 (4 elements: the 16-byte path) is off the grid too.
Every stream (p, exp_avg, exp_avg_sq, average, gradient) is carved from one buffer with canaries between the tensors,
and whole buffers are compared."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (96, 97, 224, 225, 448)
CHUNK = 96
CANARY = -12345.5
LR, BETA1, BETA2, EPS, WD = 1e-2, 0.9, 0.999, 1e-8, 0.01
VARIANTS = ("plain", "scaled", "ema", "ema_scaled")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _lengths(count):
    return [4097 if i == 1 else (1, 3, 4, 5, 8)[i % 5] for i in range(count)]


def _starts(lengths, off_grid):
    """first element of every tensor in its stream's buffer: on the 16-byte grid, one float behind it for `off_grid`,
    at least 4 canaries before the next tensor.  Returns (starts, buffer length)."""
    starts, at = [], 4
    for i, n in enumerate(lengths):
        starts.append(at + (1 if i in off_grid else 0))
        at += (n + 1 + 3) // 4 * 4 + 4
    return starts, at


@functools.lru_cache(maxsize=None)
def _host_data(count):
    """the CPU images of the streams of `count` tensors, made once: name -> (buffer, starts, mask of live elements)"""
    lengths = _lengths(count)
    gen = torch.Generator(device="cpu").manual_seed(1000 + count)
    out = {}
    for name, off_grid, fill in (("p", (), "randn"), ("m", (), "zero"), ("v", (), "zero"), ("e", (2,), "randn"),
                                 ("g1", (1,), "randn"), ("g2", (1,), "randn")):
        starts, total = _starts(lengths, off_grid)
        buf, live = torch.full((total,), CANARY), torch.zeros(total, dtype=torch.bool)
        for s, n in zip(starts, lengths):
            buf[s:s + n] = torch.randn(n, generator=gen) if fill == "randn" else 0.0
            live[s:s + n] = True
        out[name] = (buf, starts, live)
    return out


class _Streams:
    """one copy of the tensor set on the device"""

    def __init__(self, count, dev):
        self.count, self.lengths, self.dev = count, _lengths(count), dev
        self.buf, self.starts, self.live = {}, {}, {}
        for name, (buf, starts, live) in _host_data(count).items():
            self.buf[name], self.starts[name], self.live[name] = buf.to(dev), starts, live.to(dev)
            assert self.buf[name].data_ptr() % 16 == 0

    def ptr(self, name, i):
        return self.buf[name].data_ptr() + 4 * self.starts[name][i]

    def view(self, name, i):
        s = self.starts[name][i]
        return self.buf[name][s:s + self.lengths[i]]


def _spans(count, chunk):
    return [(a, min(a + chunk, count)) for a in range(0, count, chunk)]


def _tables(lib, st, spans, ema_null=()):
    """per span: (device job table, njobs, blocks, device table of the averages' addresses)"""
    from neural_image_compression_amd import _lib as L
    out = []
    for a, b in spans:
        arr = (L.AdamJob * (b - a))()
        for j, i in zip(arr, range(a, b)):
            j.p, j.m, j.v, j.n = st.ptr("p", i), st.ptr("m", i), st.ptr("v", i), st.lengths[i]
        blocks = lib.lic_adam_plan(arr, b - a)
        assert blocks == sum((st.lengths[i] + 4095) // 4096 for i in range(a, b))
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(st.dev)
        etab = torch.tensor([0 if i in ema_null else st.ptr("e", i) for i in range(a, b)], dtype=torch.int64).to(st.dev)
        out.append((table, b - a, int(blocks), etab))
    return out


def _gptrs(st, name, a, b):
    return (C.c_void_p * (b - a))(*[st.ptr(name, i) for i in range(a, b)])


def _update(lib, variant, st, spans):
    """two steps of `variant` over `st`, one launch per span and step"""
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    clip = torch.tensor([1.0, 0.75, 0.0, 0.0], dtype=torch.float32).to(st.dev)    # norm, coefficient, flag clear, count
    tabs = _tables(lib, st, spans)
    for step in (1, 2):
        for (a, b), (table, njobs, blocks, etab) in zip(spans, tabs):
            head = (C.c_void_p(table.data_ptr()), njobs, blocks, _gptrs(st, f"g{step}", a, b), LR, BETA1, BETA2, EPS,
                    WD, 1.0 - BETA1 ** step, 1.0 - BETA2 ** step)
            w = 1.0 - (1.0 + step) / (10.0 + step)
            if variant == "plain":
                L.check(lib.lic_adam_run(*head, F_._stream()), "lic_adam_run")
            elif variant == "scaled":
                L.check(lib.lic_adam_run_scaled(*head, C.c_void_p(clip.data_ptr()), 1, F_._stream()),
                        "lic_adam_run_scaled")
            elif variant == "ema":
                L.check(lib.lic_adam_run_ema(*head, C.c_void_p(etab.data_ptr()), w, None, 0, F_._stream()),
                        "lic_adam_run_ema")
            else:
                L.check(lib.lic_adam_run_ema(*head, C.c_void_p(etab.data_ptr()), w, C.c_void_p(clip.data_ptr()), 1,
                                             F_._stream()), "lic_adam_run_ema")
    torch.cuda.synchronize()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("count", COUNTS)
def test_one_launch_leaves_the_bits_of_chunked_launches(count, variant):
    dev = _need_gpu()
    from neural_image_compression_amd import _lib as L
    lib = L.load()
    one, chunked = _Streams(count, dev), _Streams(count, dev)
    _update(lib, variant, one, _spans(count, count))
    _update(lib, variant, chunked, _spans(count, CHUNK))
    start = _Streams(count, dev)
    moved = ("p", "m", "v", "e") if variant.startswith("ema") else ("p", "m", "v")
    for name in ("p", "m", "v", "e", "g1", "g2"):
        live = one.live[name]
        for st in (one, chunked):       # nothing written between the tensors
            assert bool((st.buf[name][~live] == CANARY).all()), name
        assert _same_bits(one.buf[name], chunked.buf[name]), name
        if name in moved:               # (every element was updated: the comparison is not between two idle runs)
            assert bool((one.buf[name] != start.buf[name])[live].all()), name
        else:
            assert _same_bits(one.buf[name], start.buf[name]), name


@pytest.mark.parametrize("count", COUNTS)
def test_partial_sums_of_one_launch_are_those_of_chunked_launches(count):
    dev = _need_gpu()
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    lib = L.load()
    st = _Streams(count, dev)

    def partials(spans):
        tabs = _tables(lib, st, spans)
        total, pad = sum(t[2] for t in tabs), 8
        out = torch.full((total + 2 * pad,), CANARY, dtype=torch.float64, device=dev)
        at = pad
        for (a, b), (table, njobs, blocks, _) in zip(spans, tabs):
            L.check(lib.lic_grad_norm_partial(C.c_void_p(table.data_ptr()), njobs, blocks, _gptrs(st, "g1", a, b),
                                              C.c_void_p(out.data_ptr() + 8 * at), F_._stream()), "partial")
            at += blocks
        torch.cuda.synchronize()
        assert bool((out[:pad] == CANARY).all()) and bool((out[pad + total:] == CANARY).all())
        return out[pad:pad + total]

    one, chunked = partials(_spans(count, count)), partials(_spans(count, CHUNK))
    assert one.numel() == count + 1     # (tensor 1 covers two blocks)
    assert torch.equal(one.view(torch.int64), chunked.view(torch.int64))
    # block order is job order: the blocks of tensors 0, 1, 1, 2 hold those tensors' sums of squares (exact products,
    # <= 4096 non-negative terms added in double in two different orders: 2 * 4096 * 2^-53 = 9.1e-13 relative)
    g = [st.view("g1", i).double() for i in range(3)]
    want = torch.stack([(g[0] ** 2).sum(), (g[1][:4096] ** 2).sum(), (g[1][4096:] ** 2).sum(), (g[2] ** 2).sum()])
    assert torch.allclose(one[:4], want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("count", COUNTS)
def test_swap_exchanges_every_tensor_but_the_one_without_an_average(count):
    dev = _need_gpu()
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    lib = L.load()
    st, want = _Streams(count, dev), _Streams(count, dev)
    none = count - 2
    (table, njobs, blocks, etab), = _tables(lib, st, _spans(count, count), ema_null=(none,))
    L.check(lib.lic_swap_run(C.c_void_p(table.data_ptr()), njobs, blocks, C.c_void_p(etab.data_ptr()), F_._stream()),
            "lic_swap_run")
    torch.cuda.synchronize()
    for i in range(count):
        if i != none:
            keep = want.view("p", i).clone()
            want.view("p", i).copy_(want.view("e", i))
            want.view("e", i).copy_(keep)
    for name in ("p", "m", "v", "e", "g1", "g2"):
        assert _same_bits(st.buf[name], want.buf[name]), name
    assert not _same_bits(st.buf["p"], _Streams(count, dev).buf["p"])
