"""The kernel-variant tables of the four GEMM families (csrc/lic_conv_plan.h) against the library's own symbols.

The names the `lic_*_kernel_name` functions report carry the variant-coverage net of the GPU suite, the benchmark's
per-kernel attribution and the profiles, so they have to be kernels that exist: (a) every name returned over a sweep
of descriptors is exactly the demangled name of a gfx950 kernel of liblic_hip.so, and (b) every kernel of these
families in the library is returned for at least one descriptor -- an instantiation nothing can reach does not
belong in a table.  The planners never dereference operand pointers, so 16-byte-aligned host buffers stand in for
them.  CPU only."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = "/opt/rocm/lib/llvm/bin"
OBJDUMP = os.path.join(LLVM_BIN, "llvm-objdump")
READELF = os.path.join(LLVM_BIN, "llvm-readelf")
FAMILIES = ("igemm_kernel<", "wgrad_kernel<", "wgrad_glds_kernel<", "igemm_bf16_kernel<", "wgrad_bf16_kernel<",
            "halo_conv_bf16_kernel<", "halo_convt_bf16_kernel<")
(EPI_NONE, EPI_LEAKY, EPI_MUL_LEAKY_MASK, EPI_GDN, EPI_IGDN, EPI_GDN_BWD, EPI_IGDN_BWD, EPI_CONV_GDN,
 EPI_CONV_IGDN) = range(9)

_STANDIN = C.create_string_buffer(256)
ALIGNED = (C.addressof(_STANDIN) + 15) & ~15   # a 16-byte-aligned stand-in operand
UNALIGNED = ALIGNED + 4                        # ... and one that forces the scalar-load variants


def library_kernels(lib_path, workdir):
    """demangled names (no `void `, no parameter list) of every gfx950 kernel of the library"""
    demangler = shutil.which("llvm-cxxfilt", path=LLVM_BIN) or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    assert demangler, "no C++ demangler (llvm-cxxfilt / c++filt) on this machine"
    shutil.copy(lib_path, os.path.join(workdir, "lib.so"))
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=workdir, check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    mangled = set()
    for f in sorted(os.listdir(workdir)):
        if "gfx950" not in f:
            continue
        txt = subprocess.run([READELF, "-sW", f], cwd=workdir, check=True, capture_output=True, text=True).stdout
        for line in txt.splitlines():
            parts = line.split()
            if len(parts) == 8 and parts[3] == "OBJECT" and parts[7].endswith(".kd"):   # a kernel descriptor
                mangled.add(parts[7][:-3])
    assert mangled, "no gfx950 kernels found in the library"
    out = subprocess.run([demangler], input="\n".join(sorted(mangled)) + "\n", check=True, capture_output=True,
                         text=True).stdout
    names = set()
    for line in out.splitlines():
        m = re.match(r"^void (.+)\((?:[^()]*)\)$", line.strip())
        if m:
            names.add(m.group(1))
    return names


# ---- the descriptor sweep ------------------------------------------------------------------------------------------
def _conv_geometries():
    """(B, Hi, Wi, Ho, Wo, k, stride, pad, transposed) of the models' layers: the 5x5 stride-2 stacks, the hyper
    networks' 3x3 / 5x5 layers, the 3x3 residual model, 1x1 layers (GDN contractions, entropy parameters, the RGB
    layers' column matrices), forward and mirrored (= the data gradient of the other direction), at the benchmark
    batches 32 x 256^2 and 16 x 512^2, one image, and ragged sizes."""
    out = []
    for B, S in ((32, 256), (16, 512), (1, 256), (4, 64), (32, 250), (3, 200)):
        for div in (1, 2, 4, 8, 16, 32, 64):
            H, W = -(-S // div), -(-(S if S != 200 else 136) // div)
            if H < 2 or B * H * W > 32 * 256 * 256:
                continue
            out.append((B, H, W, H, W, 1, 1, 0, 0))
            out.append((B, H, W, H, W, 3, 1, 1, 0))
            out.append((B, H, W, H, W, 5, 1, 2, 0))           # the masked context convolution
            for k in (3, 5):
                Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                out.append((B, H, W, Ho, Wo, k, 2, k // 2, 0))    # strided conv
                out.append((B, Ho, Wo, H, W, k, 2, k // 2, 1))    # its data gradient (any output parity)
                out.append((B, H, W, 2 * H, 2 * W, k, 2, k // 2, 1))   # transposed conv, output_padding 1
    return out


_CHANNELS = ((128, 128), (192, 192), (192, 288), (288, 384), (128, 192), (192, 256), (256, 192), (384, 288), (80, 128),
             (80, 192), (192, 80), (128, 80), (768, 640), (640, 640), (640, 576), (640, 1728), (512, 640), (640, 384),
             (64, 64), (192, 128), (320, 320),
             # ragged / unaligned: scalar-load and ragged-N variants, N tiles wider than the problem
             (3, 192), (192, 3), (75, 128), (128, 75), (192, 24), (128, 32), (192, 96), (192, 160), (128, 224),
             (192, 416), (100, 100), (8, 8), (16, 200), (1152, 32), (640, 16))


def _igemm_desc(L, geo, cin, cout, epi=EPI_NONE, prologue=0, tap_mask=0, ws=False, ptr=None, force=(0, 0, 0),
                extra_out=True, in_ld=None):
    B, Hi, Wi, Ho, Wo, k, stride, pad, transposed = geo
    d = L.IgemmDesc()
    p = ALIGNED if ptr is None else ptr
    d.in_, d.w, d.out, d.bias = p, ALIGNED, p, ALIGNED
    d.in_ld, d.out_ld = (cin if in_ld is None else in_ld), cout
    d.out2_ld = d.aux_ld = d.aux2_ld = d.aux3_ld = d.res_ld = d.out3_ld = cout
    d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = B, Hi, Wi, cin, Ho, Wo, cout
    d.kh = d.kw = k
    d.stride, d.pad, d.transposed, d.prologue, d.tap_mask = stride, pad, transposed, prologue, tap_mask
    d.epilogue = EPI_LEAKY if epi == "leaky_res" else epi
    d.slope = 0.01
    if epi in (EPI_MUL_LEAKY_MASK, EPI_GDN, EPI_IGDN):
        d.aux = p
    if epi in (EPI_GDN, EPI_IGDN):
        d.out2 = p
    if epi in (EPI_GDN_BWD, EPI_IGDN_BWD):
        d.aux, d.aux2, d.aux3 = p, p, p
    if prologue in (2, 3):
        d.aux2, d.aux3, d.out2 = p, p, p
        d.aux2_ld = d.aux3_ld = d.out2_ld = cin
    if epi in (EPI_CONV_GDN, EPI_CONV_IGDN):
        d.aux, d.aux2 = ALIGNED, ALIGNED
        if extra_out:
            d.out2, d.out3 = p, p
    if epi == "leaky_res":   # LeakyReLU, then the residual add into out2
        d.res, d.out2 = p, p
    if ws:
        d.workspace, d.workspace_bytes = ALIGNED, (1 << 62)
    d.force_bm, d.force_tn, d.force_split = force
    return d


def igemm_sweep(L):
    """yields (label, IgemmDesc, out_f32)"""
    geos = _conv_geometries()
    for gi, geo in enumerate(geos):
        k = geo[5]
        for cin, cout in _CHANNELS:
            tag = f"g{gi}{geo} {cin}->{cout}"
            for epi, ws in ((EPI_NONE, False), (EPI_LEAKY, True), ("leaky_res", False), (EPI_MUL_LEAKY_MASK, False)):
                yield f"{tag} epi={epi} ws={ws}", _igemm_desc(L, geo, cin, cout, epi, ws=ws), 0
            yield f"{tag} f32out", _igemm_desc(L, geo, cin, cout, EPI_NONE, ws=True), 1
            for epi in (EPI_CONV_GDN, EPI_CONV_IGDN):
                yield f"{tag} fused {epi}", _igemm_desc(L, geo, cin, cout, epi), 0
            if k == 5 and geo[6] == 1:
                yield f"{tag} masked", _igemm_desc(L, geo, cin, cout, tap_mask=0xFFF), 0
                yield f"{tag} masked ws", _igemm_desc(L, geo, cin, cout, tap_mask=0xFFF, ws=True), 0
            if k == 1 and cin == cout:   # GDN / IGDN contraction and its backward
                for epi in (EPI_GDN, EPI_IGDN):
                    yield f"{tag} gdn {epi}", _igemm_desc(L, geo, cin, cout, epi, prologue=1), 0
                yield f"{tag} gdn sq only", _igemm_desc(L, geo, cin, cout, EPI_NONE, prologue=1), 0
                for pro, epi in ((2, EPI_GDN_BWD), (3, EPI_IGDN_BWD), (0, EPI_GDN_BWD)):
                    yield f"{tag} gdn bwd {pro}", _igemm_desc(L, geo, cin, cout, epi, prologue=pro), 0
            yield f"{tag} unaligned", _igemm_desc(L, geo, cin, cout, ptr=UNALIGNED), 0
            yield f"{tag} odd pitch", _igemm_desc(L, geo, cin, cout, in_ld=cin + 2), 0
    # every plan override the planners accept (and a few they refuse), on small and large shapes
    forced_geos = [g for g in geos if g[0] in (4, 32) and g[1] in (4, 16, 64, 128)]
    for geo in forced_geos:
        for cin, cout in ((128, 128), (192, 192), (64, 64), (192, 320), (128, 32)):
            for fb, ft, fs in itertools.product((0, 64, 128, 256, 512, 100), (0, 1, 2, 3, 4), (0, 1, 2, 7, 1000)):
                for epi, pro in ((EPI_NONE, 0), (EPI_CONV_GDN, 0), (EPI_NONE, 1)):
                    if pro == 1 and geo[5] != 1:
                        continue
                    yield (f"forced {geo} {cin}->{cout} bm={fb} tn={ft} split={fs} epi={epi} pro={pro}",
                           _igemm_desc(L, geo, cin, cout, epi, prologue=pro, ws=True, force=(fb, ft, fs)), 0)
    bad = _igemm_desc(L, geos[0], 128, 128)
    bad.kh = bad.kw = 6
    yield "too many taps", bad, 0
    bad = _igemm_desc(L, geos[0], 128, 128)
    bad.stride = 3
    yield "stride 3", bad, 0
    bad = _igemm_desc(L, geos[0], 128, 128)
    bad.w = None
    yield "null weight", bad, 0


def _wgrad_desc(L, B, Hs, Ws, Hl, Wl, k, stride, pad, cp, cg, g_is_row, sq_p=0, sq_g=0, force=(0, 0, 0), ptr=None,
                p_ld=None):
    d = L.WgradDesc()
    q = ALIGNED if ptr is None else ptr
    d.p, d.g, d.dst = q, q, ALIGNED
    d.p_ld, d.g_ld = (cp if p_ld is None else p_ld), cg
    d.dst_sm, d.dst_sn, d.dst_stap = 1, 1, 1
    d.B, d.Hs, d.Ws, d.Cp, d.Hl, d.Wl, d.Cg = B, Hs, Ws, cp, Hl, Wl, cg
    d.kh = d.kw = k
    d.stride, d.pad, d.g_is_row, d.sq_p, d.sq_g, d.scale = stride, pad, g_is_row, sq_p, sq_g, 1.0
    d.force_tm, d.force_tn, d.force_split = force
    return d


def wgrad_sweep(L):
    """yields (label, WgradDesc)"""
    shapes = []
    for B, S in ((32, 256), (16, 512), (1, 256), (4, 64), (32, 250)):
        for div in (2, 4, 8, 16, 32, 64):
            H = -(-S // div)
            shapes.append((B, H, H, H, H, 1, 1, 0))
            shapes.append((B, H, H, H, H, 3, 1, 1))
            shapes.append((B, H, H, H, H, 5, 1, 2))
            for k in (3, 5):
                shapes.append((B, H, H, 2 * H, 2 * H, k, 2, k // 2))
                shapes.append((B, H, H, 2 * H - 1, 2 * H - 1, k, 2, k // 2))
    chans = _CHANNELS + ((76, 128), (128, 76), (76, 192), (192, 76), (384, 384), (192, 384), (384, 192), (320, 128),
                         (128, 320), (64, 192), (192, 64), (64, 128), (128, 64), (320, 64), (64, 320))
    for shp in shapes:
        for cp, cg in chans:
            for g_is_row in (0, 1):
                yield f"{shp} {cp}x{cg} row={g_is_row}", _wgrad_desc(L, *shp, cp, cg, g_is_row)
                yield f"{shp} {cp}x{cg} row={g_is_row} unaligned", _wgrad_desc(L, *shp, cp, cg, g_is_row, ptr=UNALIGNED)
            if shp[5] == 1:
                for g_is_row, sq_p, sq_g in itertools.product((0, 1), (0, 1), (0, 1)):
                    yield (f"{shp} {cp}x{cg} row={g_is_row} sq={sq_p}{sq_g}",
                           _wgrad_desc(L, *shp, cp, cg, g_is_row, sq_p, sq_g))
    for shp in (shapes[0], shapes[7], shapes[-3], shapes[12]):
        for cp, cg in ((192, 192), (128, 128), (384, 192), (100, 200), (64, 64), (192, 320), (76, 192)):
            for tm, tn, fs in itertools.product(range(5), range(5), (0, 1, 5)):
                for g_is_row, sq_p, sq_g in itertools.product((0, 1), (0, 1), (0, 1)):
                    yield (f"forced {shp} {cp}x{cg} tm={tm} tn={tn} split={fs} row={g_is_row} sq={sq_p}{sq_g}",
                           _wgrad_desc(L, *shp, cp, cg, g_is_row, sq_p, sq_g, force=(tm, tn, fs)))
    bad = _wgrad_desc(L, *shapes[0], 128, 128, 0)
    bad.Hs = 0
    yield "empty grid", bad


def sweep_records(lib, env_passes=True):
    """Every observable of the host planners over the sweep, as text lines (one per descriptor and entry point).
    `lib` is the ctypes library with the signatures of _lib.SIGNATURES applied."""
    from neural_image_compression_amd import _lib as L
    buf = C.create_string_buffer(96)
    recs = []

    def name(fn, d):
        buf.value = b""
        rc = fn(C.byref(d), buf, 96)
        return rc, buf.value.decode()

    def conv_pass(tag):
        for label, d, out_f32 in igemm_sweep(L):
            bm, bn, macs = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
            rc, nm = name(lib.lic_igemm_kernel_name, d)
            prc = lib.lic_igemm_plan(C.byref(d), C.byref(bm), C.byref(bn), C.byref(macs))
            recs.append(("igemm", f"{tag}{label}", rc, nm,
                         (prc, bm.value, bn.value, macs.value, lib.lic_igemm_workspace_bytes(C.byref(d)),
                          lib.lic_igemm_fused_gdn_preferred(C.byref(d)))))
            rc, nm = name(lib.lic_igemm_bf16_kernel_name, d)
            recs.append(("igemm_bf16", f"{tag}{label}", rc, nm, (lib.lic_igemm_bf16_workspace_bytes(C.byref(d)),)))

    conv_pass("")
    for label, d in wgrad_sweep(L):
        tm, tn, sk = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        rc, nm = name(lib.lic_wgrad_kernel_name, d)
        prc = lib.lic_wgrad_plan(C.byref(d), C.byref(tm), C.byref(tn), C.byref(sk))
        recs.append(("wgrad", label, rc, nm, (prc, tm.value, tn.value, sk.value,
                                              lib.lic_wgrad_workspace_bytes(C.byref(d)))))
        rc, nm = name(lib.lic_wgrad_bf16_kernel_name, d)
        recs.append(("wgrad_bf16", label, rc, nm, (lib.lic_wgrad_bf16_workspace_bytes(C.byref(d)),)))
    if env_passes:   # the planners' two tuning aids select variants of their own
        for var, val in (("LIC_BF16_RING", "3"), ("LIC_BF16_PP", "0")):
            old = os.environ.get(var)
            os.environ[var] = val
            try:
                conv_pass(f"{var}={val} ")
            finally:
                if old is None:
                    del os.environ[var]
                else:
                    os.environ[var] = old
    return recs


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


@pytest.fixture(scope="module")
def records(lib):
    return sweep_records(lib.load())


@pytest.fixture(scope="module")
def kernels(lib, tmp_path_factory):
    return library_kernels(lib.LIB_PATH, str(tmp_path_factory.mktemp("syms")))


def test_every_reported_name_is_a_kernel_of_the_library(records, kernels):
    ok = [r for r in records if r[2] == 0]
    assert len(ok) > 10000, "the sweep hardly reached the planners"
    assert all(r[2] in (0, -1, -2, -4) for r in records), "a kernel_name call returned an unknown status"
    bad = {}
    for fam, label, rc, nm, _ in ok:
        if nm not in kernels:
            bad.setdefault((fam, nm), label)
    assert not bad, "names reported with LIC_OK that are no kernel of liblic_hip.so (name: first descriptor):\n" + \
        "\n".join(f"  {fam}: {nm!r}: {label}" for (fam, nm), label in sorted(bad.items()))
    assert all(nm == "" for _, _, rc, nm, _ in records if rc != 0), "a failing call wrote a name"


def test_every_kernel_of_the_gemm_families_is_reached_by_some_descriptor(records, kernels):
    in_lib = {k for k in kernels if k.startswith(FAMILIES)}
    assert len(in_lib) >= 90, sorted(in_lib)
    reached = {nm for _, _, rc, nm, _ in records if rc == 0}
    unreached = sorted(in_lib - reached)
    assert not unreached, "instantiated, but no descriptor of the sweep dispatches them:\n  " + "\n  ".join(unreached)
