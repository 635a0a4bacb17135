"""lic_prep_run and the stand-alone packers against tests/prep_ref.py, bit for bit.

Hand-built job tables (no model): every case of prep_ref.build_table() in ONE launch -- conv / convT weights on every
(tiled, v4) path of the fp32 and bf16 packers, ragged K and N, a source 4 bytes off alignment, a padded pitch, a
tap-major source, the GDN panels (plain and kperm), the RGB stem / head split-index forms with and without a mask, the
one-launch stem operand, MAP and MASK_INPLACE around their block edge, and masked pack jobs racing the MASK_INPLACE job
of their tensor -- then a few one-job tables.  Destinations are slices of one arena filled with a NaN pattern and
separated by gaps; sources are slices of another.  Everything is compared as bit patterns; the only freedom is whether
v*v - pedestal was contracted to one FMA, and there each element must be one of the two correctly rounded candidates
and the same in prep and in lic_gdn_reparam."""
import ctypes as C

import numpy as np
import pytest
import torch

import prep_ref as R

pytestmark = pytest.mark.gpu

CASES, SOURCES = R.build_table()
NAMES = [c.name for c in CASES]
POISON32 = (R.POISON16 << 16) | R.POISON16


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0]}: " \
                          f"{int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}"


class _Run:
    """the launches, done once per module; the tests below only compare host arrays"""

    def __init__(self):
        from neural_image_compression_amd import _lib as L
        from neural_image_compression_amd import functional as F_
        self.L, self.F_, self.lib, self.dev = L, F_, L.load(), torch.device("cuda:0")
        self.at, nsrc = R.source_layout(SOURCES)
        self.dat, self.nbytes = R.dest_layout(CASES)
        host = np.full(nsrc, POISON32, np.uint32)
        for name, a in SOURCES.items():
            host[self.at[name]:self.at[name] + a.size] = a.view(np.uint32)
        self.src_before = host
        for c in CASES:      # every source read of every job lies inside its buffer
            n = SOURCES[c.src].size
            hi = c.off + (c.N * 75 if c.kind == R.PACK_BF16_STEM else c.N if c.kind in (R.MAP, R.MASK_INPLACE)
                          else int(R.src_offsets(c).max()) + 1)
            assert hi <= n and (c.mask is None or SOURCES[c.mask].size >= hi - c.off), c.name
        self.src_dev = torch.from_numpy(host.view(np.int32)).to(self.dev)
        self.arena = torch.empty(self.nbytes // 2, dtype=torch.int16, device=self.dev)
        self.values = {}
        self.out = self.launch(range(len(CASES)))
        self.planned_all = self.planned
        self.src_after = self.src_dev.cpu().numpy().view(np.uint32)

    def sync(self):
        torch.cuda.synchronize()

    def launch(self, idxs):
        """plans and runs the jobs `idxs` of the table into the freshly poisoned arena; returns the arena's bytes"""
        idxs = list(idxs)
        self.arena.fill_(R.POISON16)
        arr = (self.L.PrepJob * len(idxs))()
        for j, i in zip(arr, idxs):
            R.fill_job(j, CASES[i], self.src_dev.data_ptr(), self.at, self.arena.data_ptr() + self.dat[i])
        total = self.lib.lic_prep_plan(arr, len(idxs))
        assert total > 0, total
        self.planned = arr
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.dev)
        self.L.check(self.lib.lic_prep_run(C.c_void_p(table.data_ptr()), len(idxs), total, self.F_._stream()), "lic_prep_run")
        self.sync()
        return self.arena.cpu().numpy().view(np.uint8)

    def dest(self, out, i):
        c = CASES[i]
        raw = out[self.dat[i]:self.dat[i] + c.dst_bytes()]
        return raw.view(np.uint16 if c.half else np.uint32)

    def upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)

    def fresh(self, n, half):
        t = torch.empty(n, dtype=torch.int16 if half else torch.int32, device=self.dev)
        return t.fill_(R.POISON16 if half else POISON32)

    def value_tensor(self, c):
        """device tensor of value() over the whole source buffer of `c`, made by the STAND-ALONE entry points
        (lic_mul_inplace, lic_gdn_reparam), and the same on the host.  For transform = 1 the host array is the device's
        own result, after each element was checked to be one of the two correctly rounded candidates."""
        key = (c.src, c.mask, c.transform, c.bound, c.pedestal)
        if key not in self.values:
            src = SOURCES[c.src]
            v = self.upload(src)
            pre = R.masked(src, None if c.mask is None else SOURCES[c.mask][:src.size])
            if c.mask is not None:
                m = self.upload(SOURCES[c.mask][:src.size])
                self.L.check(self.lib.lic_mul_inplace(v.data_ptr(), m.data_ptr(), src.size, self.F_._stream()), "mul")
                self.sync()
                _same(v.cpu().numpy().view(np.uint32), R.f32_bits(pre), f"lic_mul_inplace({c.src})")
            host, cands = pre, None
            if c.transform:
                g = self.fresh(src.size, False).view(torch.float32)
                self.L.check(self.lib.lic_gdn_reparam(v.data_ptr(), g.data_ptr(), src.size, c.bound, c.pedestal,
                                                      self.F_._stream()), "reparam")
                self.sync()
                v, host = g, g.cpu().numpy()
                cands = R.reparam_candidates(pre, c.bound, c.pedestal)
            self.values[key] = (v, host, cands)
        return self.values[key]

    def alone(self, c):
        """the destination of `c` by the stand-alone packers, or None where they cannot express the job"""
        if c.kind in (R.MAP, R.MASK_INPLACE) or c.kdiv or c.ndiv:
            return None
        v, _, _ = self.value_tensor(c)
        dst = self.fresh(c.dst_bytes() // (2 if c.half else 4), c.half)
        p = v.data_ptr() + 4 * c.off
        if c.kind == R.PACK_BF16_STEM:
            rc = self.lib.lic_pack_stem_weight_bf16(p, dst.data_ptr(), c.N, self.F_._stream())
        else:
            fn = {R.PACK_F32: self.lib.lic_pack_weight, R.PACK_BF16: self.lib.lic_pack_weight_bf16,
                  R.PACK_BF16_KPERM: self.lib.lic_pack_weight_bf16_kperm}[c.kind]
            rc = fn(p, dst.data_ptr(), c.taps, c.K, c.N, c.s_tap, c.s_kq, c.s_nq, self.F_._stream())
        self.L.check(rc, "stand-alone packer")
        self.sync()
        return dst.cpu().numpy().view(np.uint16 if c.half else np.uint32)


@pytest.fixture(scope="module")
def run():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return _Run()


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_destination_equals_the_reference_and_the_stand_alone_packer(run, i):
    c = CASES[i]
    if c.kind == R.MASK_INPLACE:
        lo = run.at[c.src]
        want = R.f32_bits(R.masked(SOURCES[c.src], SOURCES[c.mask]))
        _same(run.src_after[lo:lo + c.N], want, "the masked tensor")
        return
    _, host, cands = run.value_tensor(c)
    if cands is not None:
        ok = (R.f32_bits(host) == R.f32_bits(cands[0])) | (R.f32_bits(host) == R.f32_bits(cands[1]))
        assert ok.all(), f"lic_gdn_reparam: {np.count_nonzero(~ok)} elements are neither the fused nor the unfused rounding"
    want = R.expected(c, host)
    assert want.size * want.itemsize == c.dst_bytes()
    _same(run.dest(run.out, i), want, "lic_prep_run")       # (a forgotten slot still holds the NaN pattern)
    alone = run.alone(c)
    if alone is not None:
        _same(alone, want, "stand-alone entry point")
    else:
        assert c.kind == R.MAP or c.kdiv or c.ndiv


def test_both_reparam_forms_are_told_apart(run):
    """the candidates differ for some element of some transform case (else the either-or above would hide nothing), and
    every transform case of more than a few elements really had values on both sides of its bound"""
    differ = 0
    for c in CASES:
        if c.transform:
            _, host, cands = run.value_tensor(c)
            differ += int(np.count_nonzero(cands[0] != cands[1]))
            pre = R.masked(SOURCES[c.src], None if c.mask is None else SOURCES[c.mask][:SOURCES[c.src].size])
            assert pre.size < 64 or ((pre < np.float32(c.bound)).any() and (pre > np.float32(c.bound)).any()), c.name
    assert differ > 0


def test_gaps_keep_their_poison_and_sources_are_unchanged(run):
    used = np.zeros(run.nbytes, bool)
    for i, c in enumerate(CASES):
        assert run.dat[i] % 16 == 0 and not used[run.dat[i]:run.dat[i] + c.dst_bytes()].any()
        used[run.dat[i]:run.dat[i] + c.dst_bytes()] = True
    gaps = run.out.view(np.uint16)[~used.reshape(-1, 2).any(axis=1)]
    assert gaps.size >= 8 * len(CASES)
    _same(gaps, np.full(gaps.size, R.POISON16, np.uint16), "the gaps between destinations")
    want = run.src_before.copy()
    inplace = [c for c in CASES if c.kind == R.MASK_INPLACE]
    assert len(inplace) >= len(R.EDGE_N) + 1
    for c in inplace:
        lo = run.at[c.src]
        want[lo:lo + c.N] = R.f32_bits(R.masked(SOURCES[c.src], SOURCES[c.mask]))
        assert c.N < 100 or (want[lo:lo + c.N] == 0x80000000).any(), "a masked negative: the sign of its zero is checked"
    _same(run.src_after, want, "the source arena (gaps and masks included)")


def test_planted_values_reach_the_bf16_destinations(run):
    """the table's sources hold bf16 rounding ties with an even and an odd lower neighbour, and large magnitudes"""
    a = SOURCES["w64x32x3x3"].view(np.uint32)
    tie = (a & 0xFFFF) == 0x8000
    assert (tie & ((a >> 16) & 1 == 0)).any() and (tie & ((a >> 16) & 1 == 1)).any()
    assert (np.abs(SOURCES["w64x32x3x3"]) >= 1e30).any()


def _single_job_indices(run):
    blocks = [j.nblocks for j in run.planned_all]
    one = next(i for i, c in enumerate(CASES) if blocks[i] == 1 and c.kind in R.PACK_KINDS)
    many = int(np.argmax(blocks))
    return [0, len(CASES) - 1, one, many]


@pytest.mark.parametrize("which", ["first", "last", "one-block", "many-block"])
def test_single_job_tables(run, which):
    """a table of one job: the job's destination as in the big launch, and not one other byte of the arena written"""
    i = _single_job_indices(run)[["first", "last", "one-block", "many-block"].index(which)]
    c = CASES[i]
    assert c.kind != R.MASK_INPLACE
    out = run.launch([i])
    assert run.planned[0].block0 == 0
    assert (run.planned[0].nblocks == 1) if which in ("last", "one-block") else (run.planned[0].nblocks > 1)
    lo, hi = run.dat[i], run.dat[i] + c.dst_bytes()
    _same(run.dest(out, i), run.dest(run.out, i), "the job alone against the job in the big launch")
    rest = np.concatenate([out[:lo], out[hi:]]).view(np.uint16)
    _same(rest, np.full(rest.size, R.POISON16, np.uint16), "the rest of the arena")
