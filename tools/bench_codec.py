#!/usr/bin/env python3
"""Wall time of ContextCodec.compress / decompress on a Kodak-sized image (GPU only), per coder: warm, median of
RUNS calls, the GPU synchronised around each call only.  Environment: M, K, H, W, CODERS (comma list), RUNS, and
ENCODERS (comma list of host / device, applied to the rans coder in the order given; a name may repeat, so that
`ENCODERS=host,device,host,device` alternates the two in one process), and GROUPS (comma list of sub-stream counts
1..8, applied to the rans coder like ENCODERS, inside every encoder; `GROUPS=1,2,4,8,1,2,4,8` alternates them.
bash keeps a variable GROUPS of its own and ignores an assignment to it: from bash, `env GROUPS=1,2,4,8 python ...`),
and SLICE_ROWS (comma list of latent rows per slice, 0 = no slices, applied to the rans coder outside GROUPS:
`SLICE_ROWS=0,16,8,4`).  A line names the decode steps per image as well.

`--context {raster,checkerboard}` (default raster) builds the model with that context model.  A checkerboard model
decodes in two steps; it has the rans coder only and no slices, so CODERS keeps "rans" alone and
SLICE_ROWS is ignored; its blob modes write LICBITS7 (z_coder="rans").

BLOBS (comma list of blob counts, `BLOBS=1,4,16`) selects the batched-decode mode instead: for every SLICE_ROWS and GROUPS
entry, N `compress_image` blobs of 512x768, 768x512 and 384x512 in turn are decoded once with `decompress_images` and
once as a loop of `decompress_image`, alternating, warm, median of RUNS.  PROFILE=many:3 (or seq:3) skips the timing and
makes just that many calls of one path on the first BLOBS entry, for a kernel trace whose counts can be subtracted.

ENCODE_BLOBS (`ENCODE_BLOBS=1,4,16`) is the same mode for the encoder: N images of those sizes through `compress_images`
and through a loop of `compress_image`, every blob compared with ==; a line also gives the host time of the layout
(`ragged_encode_plan`) per call.  PROFILE works as above.

SCALABLE=<base channels> (`SCALABLE=128`) is the layered codec's mode: ScalableCodec on ScalableImageCoding(M, base, K)
for every SLICE_ROWS and GROUPS entry -- compress, full decode, base-only decode, the full decode with one launch of
the layered entries per layer -- beside ContextCodec(coder="rans", z_coder="rans") on the one-layer model.  A second
line per BLOBS entry (8 if BLOBS is not set) decodes N blobs of that image: `decompress_images` and
`decompress_base_images` (one merged step loop) against loops of `decompress_image` / `decompress_base_image`."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neural_image_compression_amd as nic  # noqa: E402
from neural_image_compression_amd.codec import ContextCodec  # noqa: E402

_ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
_ap.add_argument("--context", choices=("raster", "checkerboard"), default="raster")
CONTEXT = _ap.parse_args().context
M, K = int(os.environ.get("M", "192")), int(os.environ.get("K", "3"))
H, W = int(os.environ.get("H", "512")), int(os.environ.get("W", "768"))
CODERS = os.environ.get("CODERS", "range,rans").split(",")
ENCODERS = os.environ.get("ENCODERS", "host").split(",")
GROUPS = [int(g) for g in os.environ.get("GROUPS", "1").split(",")]
SLICE_ROWS = [int(r) for r in os.environ.get("SLICE_ROWS", "0").split(",")]
RUNS = int(os.environ.get("RUNS", "10"))
BLOBS = [int(n) for n in os.environ.get("BLOBS", "").split(",") if n]
ENCODE_BLOBS = [int(n) for n in os.environ.get("ENCODE_BLOBS", "").split(",") if n]
PROFILE = os.environ.get("PROFILE", "")
BLOB_SIZES = [(512, 768), (768, 512), (384, 512)]
CHECKER = CONTEXT == "checkerboard"
if CHECKER:
    CODERS, SLICE_ROWS = [c for c in CODERS if c == "rans"], [0]
Z_CODER = {"z_coder": "rans"} if CHECKER else {}       # the container of the checkerboard schedule carries rANS z


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def blob_mode(model):
    """decompress_images against a loop of decompress_image on the same N blobs, in one process"""
    for rows, groups in [(r, g) for r in SLICE_ROWS for g in GROUPS]:
        cc = ContextCodec(model, coder="rans", encoder="device", groups=groups, slice_rows=rows or None, **Z_CODER)
        pool = [cc.compress_image(torch.rand(1, 3, h, w, device="cuda")) for h, w in BLOB_SIZES]
        for n in BLOBS:
            blobs = [pool[i % len(pool)] for i in range(n)]
            many = lambda: cc.decompress_images(blobs)
            seq = lambda: [cc.decompress_image(b) for b in blobs]
            if PROFILE:
                path, calls = PROFILE.split(":")
                for _ in range(int(calls)):
                    timed({"many": many, "seq": seq}[path])
                print(f"profile: {calls} calls of {path}, {n} blobs, groups={groups} slice_rows={rows}", flush=True)
                return
            for _ in range(2):                                                   # warm: allocator, weight packs, tuning
                a, b = many(), seq()
            ok = all(torch.equal(u, v) for u, v in zip(a, b))
            t_many, t_seq = [], []
            for _ in range(RUNS):                                                # alternating: same clocks for both
                t_many.append(timed(many)[1])
                t_seq.append(timed(seq)[1])
            mm, ms = statistics.median(t_many), statistics.median(t_seq)
            print(f"JAH({M},{K}) groups={groups} slice_rows={rows} blobs={n}: decompress_images {mm:8.2f} ms "
                  f"(min {min(t_many):.2f}, max {max(t_many):.2f}; {mm / n:6.2f} ms per blob), loop of decompress_image "
                  f"{ms:8.2f} ms (min {min(t_seq):.2f}, max {max(t_seq):.2f}; {ms / n:6.2f} ms per blob), median of {RUNS}, "
                  f"{'bit-equal' if ok else 'MISMATCH'}, {sum(map(len, blobs))} bytes", flush=True)


def encode_blob_mode(model):
    """compress_images against a loop of compress_image on the same N images, in one process"""
    from neural_image_compression_amd.codec import ragged_encode_plan
    for rows, groups in [(r, g) for r in SLICE_ROWS for g in GROUPS]:
        cc = ContextCodec(model, coder="rans", encoder="device", groups=groups, slice_rows=rows or None, **Z_CODER)
        pool = [torch.rand(1, 3, h, w, device="cuda") for h, w in BLOB_SIZES]
        for n in ENCODE_BLOBS:
            xs = [pool[i % len(pool)] for i in range(n)]
            many = lambda: cc.compress_images(xs)
            seq = lambda: [cc.compress_image(x) for x in xs]
            if PROFILE:
                path, calls = PROFILE.split(":")
                for _ in range(int(calls)):
                    timed({"many": many, "seq": seq}[path])
                print(f"profile: {calls} calls of {path}, {n} images, groups={groups} slice_rows={rows}", flush=True)
                return
            for _ in range(2):                                                   # warm: allocator, weight packs, tuning
                a, b = many(), seq()
            ok = len(a) == len(b) and all(u == v for u, v in zip(a, b))
            t_many, t_seq, t_plan = [], [], []
            for _ in range(RUNS):                                                # alternating: same clocks for both
                t_many.append(timed(many)[1])
                t_seq.append(timed(seq)[1])
                t0 = time.perf_counter()
                ragged_encode_plan([(-(-x.shape[2] // 64) * 4, -(-x.shape[3] // 64) * 4) for x in xs], M, cc.pad,
                                   rows or None, groups)
                t_plan.append(1e3 * (time.perf_counter() - t0))
            mm, ms = statistics.median(t_many), statistics.median(t_seq)
            print(f"JAH({M},{K}) groups={groups} slice_rows={rows} images={n}: compress_images {mm:8.2f} ms "
                  f"(min {min(t_many):.2f}, max {max(t_many):.2f}; {mm / n:6.2f} ms per image), loop of compress_image "
                  f"{ms:8.2f} ms (min {min(t_seq):.2f}, max {max(t_seq):.2f}; {ms / n:6.2f} ms per image), median of {RUNS}, "
                  f"layout on the host {statistics.median(t_plan):.2f} ms per call, "
                  f"{'byte-equal' if ok else 'MISMATCH'}, {sum(map(len, a))} bytes", flush=True)


def scalable_mode(base_channels):
    """ScalableCodec on ScalableImageCoding(M, base_channels, K): compress, full decode, base-only decode, the full
    decode with the layered entries launched once per layer (`merge_layers = False`), and -- the yardstick for one
    layer's cost -- ContextCodec(coder="rans", z_coder="rans") on JointAutoregressiveHierarchical(M, K), all in one
    process, the decodes alternating inside every run so that they see the same clocks"""
    from neural_image_compression_amd.codec import ScalableCodec
    torch.manual_seed(0)
    scal = nic.ScalableImageCoding(M, base_channels, K).cuda().eval()
    jah = nic.JointAutoregressiveHierarchical(M, K).cuda().eval()
    x = torch.rand(1, 3, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    for rows, groups in [(r, g) for r in SLICE_ROWS for g in GROUPS]:
        sc = ScalableCodec(scal, groups=groups, slice_rows=rows or None)
        per = ScalableCodec(scal, groups=groups, slice_rows=rows or None)
        per.merge_layers = False
        cc = ContextCodec(jah, coder="rans", encoder="device", groups=groups, slice_rows=rows or None, z_coder="rans")
        enc, one = sc.compress(x), cc.compress(x)
        args, one_args = (enc["strings"], enc["shape"], enc["z_shape"]), (one["strings"], one["shape"], one["z_shape"])
        paths = {"full": lambda: sc.decompress(*args), "base": lambda: sc.decompress_base(*args),
                 "per-layer": lambda: per.decompress(*args), "one-layer": lambda: cc.decompress(*one_args),
                 "compress": lambda: sc.compress(x), "one-layer compress": lambda: cc.compress(x)}
        for _ in range(2):                                                   # warm: allocator, weight packs, tuning
            outs = {k: f() for k, f in paths.items()}
        ok = (torch.equal(outs["full"]["y_hat"], enc["y_in"]) and torch.equal(outs["per-layer"]["y_hat"], enc["y_in"])
              and torch.equal(outs["base"]["y1_hat"], enc["y_in"][:, :base_channels]))
        t = {k: [] for k in paths}
        for _ in range(RUNS):
            for k, f in paths.items():
                t[k].append(timed(f)[1])
        steps = len(sc._wavefront(enc["shape"][2], enc["shape"][3], rows or None))
        line = ", ".join(f"{k} {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f})" for k, v in t.items())
        print(f"Scalable({M},{base_channels},{K}) vs JAH({M},{K}) {H}x{W} groups={groups} slice_rows={rows} steps={steps}: "
              f"{line}; median of {RUNS}, round trip {'ok' if ok else 'MISMATCH'}, bpp coded {enc['bpp_coded']:.4f} "
              f"base {enc['bpp_coded_base']:.4f} est {enc['bpp_est']:.4f}; one-layer bpp coded {one['bpp_coded']:.4f}",
              flush=True)
        # N blobs of this image: the merged step loop against a loop of the single-blob calls (what decompress_images
        # was before the merged loop existed), alternating inside every run
        blob = sc.compress_image(x)
        prefix = blob[:sc.base_bytes_of(blob)]
        for n in BLOBS or [8]:
            many = {"decompress_images": lambda: sc.decompress_images([blob] * n),
                    "loop of decompress_image": lambda: [sc.decompress_image(blob) for _ in range(n)],
                    "decompress_base_images": lambda: sc.decompress_base_images([prefix] * n),
                    "loop of decompress_base_image": lambda: [sc.decompress_base_image(prefix) for _ in range(n)]}
            for _ in range(2):
                outs = {k: f() for k, f in many.items()}
            ok = (all(torch.equal(u, v) for u, v in zip(outs["decompress_images"], outs["loop of decompress_image"]))
                  and all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in
                          zip(outs["decompress_base_images"], outs["loop of decompress_base_image"])))
            t = {k: [] for k in many}
            for _ in range(RUNS):
                for k, f in many.items():
                    t[k].append(timed(f)[1])
            line = ", ".join(f"{k} {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f})" for k, v in t.items())
            print(f"Scalable({M},{base_channels},{K}) {H}x{W} groups={groups} slice_rows={rows} steps={steps} blobs={n}: "
                  f"{line}; median of {RUNS}, {'bit-equal' if ok else 'MISMATCH'}, {n * len(blob)} bytes, "
                  f"{n * len(prefix)} of them base", flush=True)


if os.environ.get("SCALABLE"):
    scalable_mode(int(os.environ["SCALABLE"]))
    sys.exit(0)
torch.manual_seed(0)
model = nic.JointAutoregressiveHierarchical(M, K, context=CONTEXT).cuda().eval()
if BLOBS:
    blob_mode(model)
    sys.exit(0)
if ENCODE_BLOBS:
    encode_blob_mode(model)
    sys.exit(0)
x = torch.rand(1, 3, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
for coder, encoder, rows, groups in [(c, e, r, g) for c in CODERS for e in (ENCODERS if c == "rans" else ["host"])
                                     for r in (SLICE_ROWS if c == "rans" else [0])
                                     for g in (GROUPS if c == "rans" else [1])]:
    cc = ContextCodec(model, coder=coder, encoder=encoder, groups=groups, slice_rows=rows or None)
    for _ in range(2):                                                       # warm: allocator, weight packs, tuning
        enc = cc.compress(x)
        dec = cc.decompress(enc["strings"], enc["shape"], enc["z_shape"])
    ok = torch.equal(dec["y_hat"], enc["y_in"])
    t_enc = [timed(lambda: cc.compress(x))[1] for _ in range(RUNS)]
    t_dec = [timed(lambda: cc.decompress(enc["strings"], enc["shape"], enc["z_shape"]))[1] for _ in range(RUNS)]
    s = enc["strings"]
    nbytes = len(s["z"]) + sum(map(len, s["y"])) + sum(map(len, s.get("y_esc", [])))
    npx = enc["shape"][2] * enc["shape"][3]
    md = statistics.median(t_dec)
    steps = len(cc._wavefront(enc["shape"][2], enc["shape"][3], rows or None))
    print(f"JAH({M},{K}) {H}x{W} context={CONTEXT} coder={coder} encoder={encoder} groups={groups} slice_rows={rows} steps={steps}: compress {statistics.median(t_enc):8.2f} ms "
          f"(min {min(t_enc):.2f}, max {max(t_enc):.2f}), decompress {md:8.2f} ms "
          f"(min {min(t_dec):.2f}, max {max(t_dec):.2f}, median of {RUNS}; {1e3 * md / npx:6.1f} us per latent pixel, "
          f"{npx} pixels), round trip {'ok' if ok else 'MISMATCH'}, {nbytes} bytes, bpp coded {enc['bpp_coded']:.4f} "
          f"est {enc['bpp_est']:.4f}", flush=True)
