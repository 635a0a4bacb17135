#!/usr/bin/env python3
"""Wall time of ContextCodec.compress / decompress on a Kodak-sized image (GPU only), per coder: warm, median of
RUNS calls, the GPU synchronised around each call only.  Environment: M, K, H, W, CODERS (comma list), RUNS, and
ENCODERS (comma list of host / device, applied to the rans coder in the order given; a name may repeat, so that
`ENCODERS=host,device,host,device` alternates the two in one process), and GROUPS (comma list of sub-stream counts
1..8, applied to the rans coder like ENCODERS, inside every encoder; `GROUPS=1,2,4,8,1,2,4,8` alternates them.
bash keeps a variable GROUPS of its own and ignores an assignment to it: from bash, `env GROUPS=1,2,4,8 python ...`),
and SLICE_ROWS (comma list of latent rows per slice, 0 = no slices, applied to the rans coder outside GROUPS:
`SLICE_ROWS=0,16,8,4`).  A line names the decode steps per image as well."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neural_image_compression_amd as nic  # noqa: E402
from neural_image_compression_amd.codec import ContextCodec  # noqa: E402

M, K = int(os.environ.get("M", "192")), int(os.environ.get("K", "3"))
H, W = int(os.environ.get("H", "512")), int(os.environ.get("W", "768"))
CODERS = os.environ.get("CODERS", "range,rans").split(",")
ENCODERS = os.environ.get("ENCODERS", "host").split(",")
GROUPS = [int(g) for g in os.environ.get("GROUPS", "1").split(",")]
SLICE_ROWS = [int(r) for r in os.environ.get("SLICE_ROWS", "0").split(",")]
RUNS = int(os.environ.get("RUNS", "10"))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


torch.manual_seed(0)
model = nic.JointAutoregressiveHierarchical(M, K).cuda().eval()
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
    print(f"JAH({M},{K}) {H}x{W} coder={coder} encoder={encoder} groups={groups} slice_rows={rows} steps={steps}: compress {statistics.median(t_enc):8.2f} ms "
          f"(min {min(t_enc):.2f}, max {max(t_enc):.2f}), decompress {md:8.2f} ms "
          f"(min {min(t_dec):.2f}, max {max(t_dec):.2f}, median of {RUNS}; {1e3 * md / npx:6.1f} us per latent pixel, "
          f"{npx} pixels), round trip {'ok' if ok else 'MISMATCH'}, {nbytes} bytes, bpp coded {enc['bpp_coded']:.4f} "
          f"est {enc['bpp_est']:.4f}", flush=True)
