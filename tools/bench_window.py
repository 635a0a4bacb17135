#!/usr/bin/env python3
"""Window gather against the plain uint8 conversion, and the host cost of the three loaders (GPU only).

(a) lic_window_u8_to_f32 for B = 32 crops of 256^2 from a resident pool of larger images, against
    lic_u8_to_f32 producing the same 25 MB output from 6.3 MB of contiguous bytes: both are streaming kernels, the
    window kernel reads scattered 768-byte row pieces.  Alternating, back to back; time and achieved GB/s
    (bytes read + bytes written) of each.
(b) host time per batch -- wall time between yields with the GPU idle (a synchronize before the clock starts) --
    of ShardLoader on a format-1 shard of 256^2 crops, RandomCropLoader(resident=True) and (resident=False) on a
    ragged shard of the larger images."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_image_compression_amd import _lib as L  # noqa: E402
from neural_image_compression_amd import data as D  # noqa: E402
from neural_image_compression_amd import functional as F_  # noqa: E402

dev = torch.device("cuda:0")
B, CROP, N_IMG = 32, 256, 256
lib = L.load()


def gpu_us(fn, n=200):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def kernels():
    rs = np.random.RandomState(0)
    sizes = np.stack([rs.randint(300, 700, N_IMG), rs.randint(300, 900, N_IMG)], axis=1)
    nbytes = sizes[:, 0] * sizes[:, 1] * 3
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
    pool = torch.randint(0, 256, (int(nbytes.sum()),), device=dev, dtype=torch.uint8)
    img = rs.permutation(N_IMG)[:B]
    y0 = (rs.random_sample(B) * (sizes[img, 0] - CROP + 1)).astype(np.int64)
    x0 = (rs.random_sample(B) * (sizes[img, 1] - CROP + 1)).astype(np.int64)
    out = torch.empty((B, CROP, CROP, 3), device=dev, dtype=torch.float32)
    flat = torch.randint(0, 256, (B, CROP, CROP, 3), device=dev, dtype=torch.uint8)
    tables = {}
    for name, flip in (("window", 0), ("window+flip", 1)):
        jobs = D.window_jobs(offsets[img], sizes[img], y0, x0, flip, CROP, CROP, "zeros", pool_bytes=pool.numel())
        tables[name] = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)

    def window(name):
        L.check(lib.lic_window_u8_to_f32(F_._ptr(pool), F_._ptr(tables[name]), B, CROP, CROP, 3, 0, F_._ptr(out),
                                         F_._stream()), "lic_window_u8_to_f32")

    def plain():
        L.check(lib.lic_u8_to_f32(F_._ptr(flat), F_._ptr(out), flat.numel(), F_._stream()), "lic_u8_to_f32")

    moved = out.numel() * 5                                                 # 1 byte read + 4 written per element
    runs = {"lic_u8_to_f32": [], "window": [], "window+flip": []}
    for _ in range(5):                                                      # alternating, back to back
        runs["lic_u8_to_f32"].append(gpu_us(plain))
        runs["window"].append(gpu_us(lambda: window("window")))
        runs["window+flip"].append(gpu_us(lambda: window("window+flip")))
    print(f"(a) B={B} crops of {CROP}^2, pool {pool.numel() / 1e6:.0f} MB of {N_IMG} images, output {out.numel() * 4 / 1e6:.1f} MB")
    for name, us in runs.items():
        med = float(np.median(us))
        print(f"    {name:14s} median {med:7.1f} us  (runs {' '.join(f'{u:.1f}' for u in us)})  {moved / med / 1e3:7.0f} GB/s",
              flush=True)


def host_ms_per_batch(loader, epochs=3):
    """mean wall time between yields with the GPU idle: the clock runs only while the loader works"""
    list(loader)                                                            # warm-up epoch (pinned-buffer cache, page cache)
    total, n = 0.0, 0
    for _ in range(epochs):
        it = iter(loader)
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch = next(it, None)
            total += time.perf_counter() - t0
            if batch is None:
                break
            n += 1
    return total / n * 1e3


def loaders():
    rs = np.random.RandomState(1)
    with tempfile.TemporaryDirectory() as tmp:
        crops = rs.randint(0, 256, (N_IMG, CROP, CROP, 3)).astype(np.uint8)
        p1 = os.path.join(tmp, "crops.lic")
        D.write_shard(p1, crops)
        big = [rs.randint(0, 256, (int(h), int(w), 3)).astype(np.uint8)
               for h, w in zip(rs.randint(300, 700, N_IMG), rs.randint(300, 900, N_IMG))]
        p2 = os.path.join(tmp, "images.lic2")
        D.write_ragged_shard(p2, big)
        ragged = D.RaggedShardDataset(p2)
        rows = [("ShardLoader (format 1, shuffled)", D.ShardLoader(D.ShardDataset(p1), B, dev, shuffle=True, drop_last=True)),
                ("RandomCropLoader(resident=True)", D.RandomCropLoader(ragged, B, CROP, dev, hflip=True, resident=True)),
                ("RandomCropLoader(resident=False)", D.RandomCropLoader(ragged, B, CROP, dev, hflip=True, resident=False))]
        print(f"(b) host time per batch of {B}, {N_IMG} images per epoch")
        for _ in range(2):                                                  # alternating
            for name, ld in rows:
                print(f"    {name:34s} {host_ms_per_batch(ld):7.3f} ms", flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), flush=True)
    kernels()
    loaders()
