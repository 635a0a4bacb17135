"""Input pipeline at GPU speed.

The reference's `PreprocessedDataset` (Dataloader.py:11-27) decodes one JPEG/PNG per item with PIL
and converts it with `ToTensor()` on the host: fp32 CHW in [0,1].  At ~1100 images/s per MI355X
that decode is the bottleneck, so the preprocessed 256x256 crops (preprocess.py writes them once)
are stored as **uint8 NHWC shards** and a batch is: one gather from a memory-mapped file -> one
pinned H2D copy of uint8 (4x fewer PCIe bytes than fp32) -> `lic_u8_to_f32` on the device
(`float(v) / 255`, bit-identical to `ToTensor()`), already in the channels_last layout the conv
kernels read.

Shard format (little endian): magic b"LICSHRD1", uint32 N, H, W, C, then N*H*W*C bytes.
`ShardLoader` is a drop-in for the `DataLoader` the reference's Trainer / Evaluator iterate
(`for imgs in loader`, `len(loader)`, re-iterable); it yields [B,3,H,W] tensors on the device.

Images of any size: shard format 2 (little endian): magic b"LICSHRD2", uint32 N, C, then N entries
(uint32 H, uint32 W, uint64 byte_offset) and the pixel bytes, image i's [H][W][C] uint8 pixels starting
byte_offset bytes after the end of the entry table.  `RaggedShardDataset` maps such shards and
`RandomCropLoader` draws a fresh random crop (and optional horizontal flip) of every image each epoch
-- what a `transform` of random crops gives the reference's datasets (Dataloader.py:12,32), where
preprocess.py:30-32 fixes one window per image for ever -- with the pixels resident in HBM: a batch is
one 32*B-byte job table and one `lic_window_u8_to_f32` launch.  `load_image_u8` is the evaluation-side
use of the same kernel: one image padded to the multiple of 64 the models need.

Random scale: preprocess.py:23-33 also draws a downscale factor per image and resizes with Pillow's
`Image.BICUBIC` before it crops.  `RandomCropLoader(min_factor=...)` draws the factor per image and epoch and
`lic_resample_u8_to_f32` resizes, crops, flips and converts in one launch, byte for byte what Pillow gives
(`resample_jobs`, `resample_u8_to_f32`).  `shard_from_image_files` applies the reference's two discard rules
(smallest side, saturation) when asked to.
"""
from __future__ import annotations

import os
import struct
from typing import Iterable, Iterator, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import functional as F_

MAGIC = b"LICSHRD1"
_HEADER = struct.Struct("<8sIIII")


def write_shard(path: str, images: np.ndarray) -> None:
    """images: uint8 [N, H, W, C]"""
    a = np.ascontiguousarray(images)
    if a.dtype != np.uint8 or a.ndim != 4:
        raise ValueError(f"images must be uint8 [N,H,W,C], got {a.dtype} {a.shape}")
    with open(path, "wb") as f:
        f.write(_HEADER.pack(MAGIC, *a.shape))
        f.write(a.tobytes())


def is_saturated(image: np.ndarray, threshold: float = 0.95) -> bool:
    """The reference's saturation verdict (preprocess.py:18-21) on a uint8 [H,W,C] image: in float32, more than
    5 % of the pixels have a spread of v/255 over the channels above `threshold`."""
    v = np.asarray(image, np.uint8).astype(np.float32) / np.float32(255.0)
    spread = v.max(axis=2) - v.min(axis=2)
    return bool(np.mean(spread > np.float32(threshold)) > 0.05)


def shard_from_image_files(files: Sequence[str], path: str, ragged: bool = False, min_side: Optional[int] = None,
                           saturation_thresh: Optional[float] = None) -> int:
    """Decode image files (the sorted jpg/jpeg/png list of Dataloader.py:13-18, `.convert("RGB")`)
    once, offline, into a shard.  All images must share one size (preprocess.py crops to 256x256)
    unless `ragged=True`, which writes shard format 2 (`write_ragged_shard`).  `min_side` skips images with
    min(H, W) < min_side and `saturation_thresh` those `is_saturated` at that threshold (preprocess.py:56-62
    discards both kinds); returns the number of images written."""
    from PIL import Image  # offline tool only
    arrs = [np.asarray(Image.open(f).convert("RGB"), np.uint8) for f in files]
    if min_side is not None:
        arrs = [a for a in arrs if min(a.shape[:2]) >= min_side]
    if saturation_thresh is not None:
        arrs = [a for a in arrs if not is_saturated(a, saturation_thresh)]
    if not arrs:
        raise ValueError("no images")
    if ragged:
        write_ragged_shard(path, arrs)
        return len(arrs)
    if any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError("images differ in size; shards hold one size")
    write_shard(path, np.stack(arrs))
    return len(arrs)


class ShardDataset:
    """Memory-mapped uint8 [N,H,W,C] shard(s); `ds[i]` -> uint8 [H,W,C] view."""

    def __init__(self, paths):
        if isinstance(paths, (str, os.PathLike)):
            paths = [paths]
        self._maps, self._starts = [], [0]
        shape = None
        for p in paths:
            with open(p, "rb") as f:
                magic, n, h, w, c = _HEADER.unpack(f.read(_HEADER.size))
            if magic != MAGIC:
                raise ValueError(f"{p}: not a LIC shard")
            if shape is not None and (h, w, c) != shape:
                raise ValueError(f"{p}: image shape {(h, w, c)} differs from {shape}")
            shape = (h, w, c)
            self._maps.append(np.memmap(p, np.uint8, "r", offset=_HEADER.size, shape=(n, h, w, c)))
            self._starts.append(self._starts[-1] + n)
        if shape is None:
            raise ValueError("no shards")
        self.image_shape = shape

    def __len__(self) -> int:
        return self._starts[-1]

    def __getitem__(self, i: int) -> np.ndarray:
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        s = int(np.searchsorted(self._starts, i, side="right")) - 1
        return self._maps[s][i - self._starts[s]]

    def gather(self, idx: Iterable[int], out: Optional[np.ndarray] = None) -> np.ndarray:
        idx = list(idx)
        if out is None:
            out = np.empty((len(idx),) + self.image_shape, np.uint8)
        for k, i in enumerate(idx):
            out[k] = self[i]
        return out


def u8_to_f32(batch_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [B,H,W,C] on the device -> fp32 [B,C,H,W] (channels_last memory), values v/255."""
    if batch_u8.dtype != torch.uint8 or batch_u8.dim() != 4:
        raise ValueError("expected a uint8 [B,H,W,C] tensor")
    if not batch_u8.is_cuda:
        raise L.LicError("lic_u8_to_f32 needs a CUDA tensor (there is no CPU fallback)")
    src = batch_u8.contiguous()
    out = torch.empty(src.shape, device=src.device, dtype=torch.float32)
    L.check(L.load().lic_u8_to_f32(F_._ptr(src), F_._ptr(out), src.numel(), F_._stream()), "lic_u8_to_f32")
    return out.permute(0, 3, 1, 2)


class ShardLoader:
    """Batches of a ShardDataset on `device`.  `rank`/`world_size` take every world_size-th batch slot
    of the (shuffled) order, so data-parallel ranks see disjoint images (the reference has no DP)."""

    def __init__(self, dataset: ShardDataset, batch_size: int, device, shuffle: bool = False, seed: int = 0,
                 drop_last: bool = False, rank: int = 0, world_size: int = 1):
        self.ds, self.bs, self.device = dataset, int(batch_size), torch.device(device)
        self.shuffle, self.seed, self.drop_last = shuffle, int(seed), drop_last
        self.rank, self.world = int(rank), int(world_size)
        self.epoch = 0
        n = len(dataset) // self.world
        self._n_batches = n // self.bs if drop_last else (n + self.bs - 1) // self.bs

    def __len__(self) -> int:
        return self._n_batches

    def order(self) -> np.ndarray:
        idx = np.arange(len(self.ds))
        if self.shuffle:
            np.random.RandomState(self.seed + self.epoch).shuffle(idx)
        per = len(idx) // self.world
        return idx[self.rank * per:(self.rank + 1) * per]

    def __iter__(self) -> Iterator[torch.Tensor]:
        idx = self.order()
        self.epoch += 1
        h, w, c = self.ds.image_shape
        for b in range(self._n_batches):
            sel = idx[b * self.bs:(b + 1) * self.bs]
            host = torch.empty((len(sel), h, w, c), dtype=torch.uint8).pin_memory() \
                if self.device.type == "cuda" else torch.empty((len(sel), h, w, c), dtype=torch.uint8)
            self.ds.gather(sel, host.numpy())
            yield u8_to_f32(host.to(self.device, non_blocking=True))


# ---- images of any size: ragged shards, windows, random-crop batches --------------------------
MAGIC2 = b"LICSHRD2"
_HEADER2 = struct.Struct("<8sII")
_ENTRY2 = np.dtype([("H", "<u4"), ("W", "<u4"), ("offset", "<u8")])
# host mirror of lic_window_job (include/lic.h), as a numpy record so that a table is built without a Python loop
WINDOW_JOB = np.dtype([("src_offset", "<i8"), ("Hs", "<i4"), ("Ws", "<i4"), ("y0", "<i4"), ("x0", "<i4"),
                       ("flags", "<i4"), ("reserved", "<i4")])
# host mirror of lic_resample_job
RESAMPLE_JOB = np.dtype([("src_offset", "<i8"), ("Hs", "<i4"), ("Ws", "<i4"), ("Hn", "<i4"), ("Wn", "<i4"),
                         ("y0", "<i4"), ("x0", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
BORDERS = {"zeros": L.WINDOW_ZERO, "constant": L.WINDOW_ZERO, "replicate": L.WINDOW_REPLICATE,
           "edge": L.WINDOW_REPLICATE, "reflect": L.WINDOW_REFLECT}


def border_code(mode) -> int:
    """'zeros' / 'constant', 'replicate' / 'edge', 'reflect' (torch's and numpy's names) or the integer itself"""
    if isinstance(mode, str):
        if mode not in BORDERS:
            raise ValueError(f"unknown border mode {mode!r}: one of {sorted(BORDERS)}")
        return BORDERS[mode]
    if int(mode) not in (0, 1, 2):
        raise ValueError(f"unknown border code {mode}")
    return int(mode)


def write_ragged_shard(path: str, images: Sequence[np.ndarray]) -> None:
    """images: uint8 [H,W,C] arrays of any sizes, one channel count -> a format-2 shard"""
    arrs = [np.ascontiguousarray(a) for a in images]
    if not arrs:
        raise ValueError("no images")
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != arrs[0].shape[2] or 0 in a.shape:
            raise ValueError(f"images must be non-empty uint8 [H,W,C] with one C, got {a.dtype} {a.shape}")
    table = np.zeros(len(arrs), _ENTRY2)
    table["H"] = [a.shape[0] for a in arrs]
    table["W"] = [a.shape[1] for a in arrs]
    table["offset"] = np.concatenate([[0], np.cumsum([a.size for a in arrs])[:-1]])
    with open(path, "wb") as f:
        f.write(_HEADER2.pack(MAGIC2, len(arrs), arrs[0].shape[2]))
        f.write(table.tobytes())
        for a in arrs:
            f.write(a.tobytes())


class RaggedShardDataset:
    """Memory-mapped format-2 shard(s): `len(ds)`, `ds[i]` -> uint8 [H,W,C] view, `ds.sizes` -> int64 [N,2]
    (H, W).  `ds.offsets[i]` is image i's byte offset in the concatenation of all shards' pixel bytes, the
    layout `pool_chunks()` streams out."""

    def __init__(self, paths):
        if isinstance(paths, (str, os.PathLike)):
            paths = [paths]
        self._maps, self._starts, self._local = [], [0], []
        sizes, offsets, base, channels = [], [], 0, None
        for p in paths:
            with open(p, "rb") as f:
                head = f.read(_HEADER2.size)
                if len(head) < _HEADER2.size or head[:8] != MAGIC2:
                    raise ValueError(f"{p}: not a ragged LIC shard (format 2)")
                _, n, c = _HEADER2.unpack(head)
                table = np.frombuffer(f.read(n * _ENTRY2.itemsize), _ENTRY2)
            if table.size != n or n == 0:
                raise ValueError(f"{p}: truncated entry table")
            if channels is not None and c != channels:
                raise ValueError(f"{p}: {c} channels, earlier shards have {channels}")
            channels = c
            start = _HEADER2.size + n * _ENTRY2.itemsize
            nbytes = table["H"].astype(np.int64) * table["W"].astype(np.int64) * c
            have = os.path.getsize(p) - start
            if np.any(nbytes == 0) or np.any(table["offset"].astype(np.int64) + nbytes > have):
                raise ValueError(f"{p}: an image lies outside the file")
            self._maps.append(np.memmap(p, np.uint8, "r", offset=start, shape=(have,)))
            self._local.append(table["offset"].astype(np.int64))
            self._starts.append(self._starts[-1] + n)
            sizes.append(np.stack([table["H"], table["W"]], axis=1).astype(np.int64))
            offsets.append(self._local[-1] + base)
            base += have
        if channels is None:
            raise ValueError("no shards")
        self.C = int(channels)
        self.sizes = np.concatenate(sizes)
        self.offsets = np.concatenate(offsets)
        self.pool_bytes = int(base)

    def __len__(self) -> int:
        return self._starts[-1]

    def __getitem__(self, i: int) -> np.ndarray:
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        s = int(np.searchsorted(self._starts, i, side="right")) - 1
        h, w = self.sizes[i]
        o = int(self._local[s][i - self._starts[s]])
        return self._maps[s][o:o + h * w * self.C].reshape(h, w, self.C)

    def pool_chunks(self, chunk_bytes: int = 64 << 20):
        """the pixel bytes of all shards, in order, as uint8 arrays of at most chunk_bytes"""
        for m in self._maps:
            for a in range(0, m.shape[0], chunk_bytes):
                yield m[a:a + chunk_bytes]


def window_jobs(offsets, sizes, y0, x0, flip, h: int, w: int, border, C: int = 3, pool_bytes: Optional[int] = None):
    """The host copy of a lic_window_job table (a WINDOW_JOB record array), checked: the library cannot
    inspect a table that lives on the device, so sizes >= 1, offsets inside the pool, 32-bit coordinates and
    the reflect rule (every overhang smaller than the side it reflects about) are verified here."""
    border = border_code(border)
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    n = sizes.shape[0]
    offsets = np.broadcast_to(np.asarray(offsets, np.int64), (n,))
    y0 = np.broadcast_to(np.asarray(y0, np.int64), (n,))
    x0 = np.broadcast_to(np.asarray(x0, np.int64), (n,))
    flip = np.broadcast_to(np.asarray(flip, np.int64), (n,))
    if n == 0 or h <= 0 or w <= 0:
        raise ValueError("empty window table")
    if np.any(sizes < 1) or np.any(sizes >= 2 ** 31):
        raise ValueError("source sizes must be in [1, 2^31)")
    if np.any(offsets < 0) or (pool_bytes is not None and np.any(offsets + sizes[:, 0] * sizes[:, 1] * C > pool_bytes)):
        raise ValueError("an image lies outside the pool")
    lim = 2 ** 30
    if np.any(np.abs(y0) >= lim) or np.any(np.abs(x0) >= lim) or h >= lim or w >= lim:
        raise ValueError("window coordinates out of range")
    if border == L.WINDOW_REFLECT:
        over_y = np.maximum(-y0, y0 + h - sizes[:, 0])
        over_x = np.maximum(-x0, x0 + w - sizes[:, 1])
        if np.any(over_y >= sizes[:, 0]) or np.any(over_x >= sizes[:, 1]):
            raise L.LicError("lic_window_u8_to_f32 failed: LIC_ERR_INVALID (a reflect overhang reaches the source side)")
    jobs = np.zeros(n, WINDOW_JOB)
    jobs["src_offset"], jobs["Hs"], jobs["Ws"] = offsets, sizes[:, 0], sizes[:, 1]
    jobs["y0"], jobs["x0"], jobs["flags"] = y0, x0, (flip != 0) * L.WINDOW_FLIP
    return jobs


def window_u8_to_f32(pool: torch.Tensor, jobs: np.ndarray, h: int, w: int, C: int = 3, border="zeros") -> torch.Tensor:
    """`pool`: uint8 device tensor (any shape; offsets are bytes from its first element); `jobs`: a table from
    `window_jobs`.  One pinned 32*B-byte upload and one lic_window_u8_to_f32 launch -> fp32 [B,C,h,w]
    (channels_last memory)."""
    if not isinstance(pool, torch.Tensor) or pool.dtype != torch.uint8:
        raise ValueError("expected a uint8 tensor")
    if not pool.is_cuda:
        raise L.LicError("lic_window_u8_to_f32 needs a CUDA tensor (there is no CPU fallback)")
    if jobs.dtype != WINDOW_JOB or not pool.is_contiguous():
        raise ValueError("jobs must be a window_jobs() table and the pool contiguous")
    if int((jobs["src_offset"] + jobs["Hs"].astype(np.int64) * jobs["Ws"] * C).max()) > pool.numel():
        raise ValueError("an image lies outside the pool")
    B = jobs.shape[0]
    host = torch.empty(B * WINDOW_JOB.itemsize, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = jobs.view(np.uint8)
    dev = host.to(pool.device, non_blocking=True)
    out = torch.empty((B, h, w, C), device=pool.device, dtype=torch.float32)
    L.check(L.load().lic_window_u8_to_f32(F_._ptr(pool), F_._ptr(dev), B, h, w, C, border_code(border), F_._ptr(out),
                                          F_._stream()), "lic_window_u8_to_f32")
    return out.permute(0, 3, 1, 2)


def resample_jobs(offsets, sizes, new_sizes, y0, x0, flip, h: int, w: int, C: int = 3,
                  pool_bytes: Optional[int] = None):
    """The host copy of a lic_resample_job table (a RESAMPLE_JOB record array), checked: the library cannot
    inspect a table that lives on the device, so everything the kernel assumes is verified here -- sizes >= 1,
    per axis ceil(n_in / 2) <= n_out <= n_in, the h x w window inside the resized image, offsets inside the
    pool."""
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    n = sizes.shape[0]
    new_sizes = np.broadcast_to(np.asarray(new_sizes, np.int64).reshape(-1, 2), (n, 2))
    offsets = np.broadcast_to(np.asarray(offsets, np.int64), (n,))
    y0 = np.broadcast_to(np.asarray(y0, np.int64), (n,))
    x0 = np.broadcast_to(np.asarray(x0, np.int64), (n,))
    flip = np.broadcast_to(np.asarray(flip, np.int64), (n,))
    if n == 0 or h <= 0 or w <= 0:
        raise ValueError("empty resample table")
    if not 1 <= C <= 4:
        raise ValueError("lic_resample_u8_to_f32 takes 1 to 4 channels")
    if np.any(sizes < 1) or np.any(sizes >= 2 ** 30):
        raise ValueError("source sizes must be in [1, 2^30)")
    if np.any(offsets < 0) or (pool_bytes is not None and np.any(offsets + sizes[:, 0] * sizes[:, 1] * C > pool_bytes)):
        raise ValueError("an image lies outside the pool")
    if np.any(new_sizes > sizes) or np.any(new_sizes < (sizes + 1) // 2):
        raise L.LicError("lic_resample_u8_to_f32 failed: LIC_ERR_INVALID (a new size outside [ceil(n / 2), n]: "
                         "downscaling by at most 2 is supported, upscaling is not)")
    if np.any(y0 < 0) or np.any(x0 < 0) or np.any(y0 + h > new_sizes[:, 0]) or np.any(x0 + w > new_sizes[:, 1]):
        raise L.LicError("lic_resample_u8_to_f32 failed: LIC_ERR_INVALID (a window leaves the resized image)")
    jobs = np.zeros(n, RESAMPLE_JOB)
    jobs["src_offset"], jobs["Hs"], jobs["Ws"] = offsets, sizes[:, 0], sizes[:, 1]
    jobs["Hn"], jobs["Wn"] = new_sizes[:, 0], new_sizes[:, 1]
    jobs["y0"], jobs["x0"], jobs["flags"] = y0, x0, (flip != 0) * L.WINDOW_FLIP
    return jobs


def resample_u8_to_f32(pool: torch.Tensor, jobs: np.ndarray, h: int, w: int, C: int = 3) -> torch.Tensor:
    """`pool`: uint8 device tensor (any shape; offsets are bytes from its first element); `jobs`: a table from
    `resample_jobs`.  One pinned 40*B-byte upload and one lic_resample_u8_to_f32 launch -> fp32 [B,C,h,w]
    (channels_last memory): the h x w window of every image resized with Pillow's 8-bit bicubic filter."""
    if not isinstance(pool, torch.Tensor) or pool.dtype != torch.uint8:
        raise ValueError("expected a uint8 tensor")
    if not pool.is_cuda:
        raise L.LicError("lic_resample_u8_to_f32 needs a CUDA tensor (there is no CPU fallback)")
    if jobs.dtype != RESAMPLE_JOB or not pool.is_contiguous():
        raise ValueError("jobs must be a resample_jobs() table and the pool contiguous")
    if int((jobs["src_offset"] + jobs["Hs"].astype(np.int64) * jobs["Ws"] * C).max()) > pool.numel():
        raise ValueError("an image lies outside the pool")
    B = jobs.shape[0]
    host = torch.empty(B * RESAMPLE_JOB.itemsize, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = jobs.view(np.uint8)
    dev = host.to(pool.device, non_blocking=True)
    out = torch.empty((B, h, w, C), device=pool.device, dtype=torch.float32)
    L.check(L.load().lic_resample_u8_to_f32(F_._ptr(pool), F_._ptr(dev), B, h, w, C, F_._ptr(out), F_._stream()),
            "lic_resample_u8_to_f32")
    return out.permute(0, 3, 1, 2)


def load_image_u8(t_u8_hwc: torch.Tensor, multiple: int = 64, mode="replicate", align: str = "topleft"):
    """One uint8 [H,W,C] image on the device -> (x_padded fp32 [1,C,Hp,Wp] channels_last, (H, W, top, left)):
    v/255 and the padding to a multiple of `multiple` in one lic_window_u8_to_f32 launch."""
    if not isinstance(t_u8_hwc, torch.Tensor) or t_u8_hwc.dtype != torch.uint8 or t_u8_hwc.dim() != 3:
        raise ValueError("expected a uint8 [H,W,C] tensor")
    if not t_u8_hwc.is_cuda:
        raise L.LicError("lic_window_u8_to_f32 needs a CUDA tensor (there is no CPU fallback)")
    H, W, C = t_u8_hwc.shape
    Hp, Wp, top, left = F_.pad_geometry(H, W, multiple, align)
    src = t_u8_hwc.contiguous()
    jobs = window_jobs(0, [(H, W)], -top, -left, 0, Hp, Wp, mode, C)
    return window_u8_to_f32(src, jobs, Hp, Wp, C, mode), (H, W, top, left)


class RandomCropLoader:
    """A fresh random `crop` x `crop` window (and, with `hflip`, a coin-flip mirror) of every image each epoch,
    as batches [B,3,crop,crop] fp32 channels_last on `device`: a drop-in for what `Trainer` iterates (`len`,
    re-iterable).

    The schedule is drawn on the host and is a pure function of (seed, epoch, rank).  Draw order, from
    `rs = np.random.RandomState(seed + epoch)` over all N images of the dataset:
      1. `order = rs.permutation(N)`            -- slot k shows image order[k];
      2. `uy = rs.random_sample(N)`, then `ux = rs.random_sample(N)`
                                                -- slot k: y0 = floor(uy[k] * (H - crop + 1)), x0 likewise from W;
      3. `rs.randint(0, 2, N)` for the flips, drawn only when `hflip` is set.
    Rank r of `world_size` takes slots [r * per, (r + 1) * per), per = N // world_size (as `ShardLoader.order`),
    so ranks see disjoint images; `schedule(epoch)` returns this rank's rows (image, y0, x0, flip).

    `min_factor` (0.5 <= min_factor <= 1; None, the default, leaves everything above as it is) adds the random
    downscale of preprocess.py:23-33: every image is resized with Pillow's 8-bit bicubic filter before the crop,
    byte for byte what `Image.resize(..., Image.BICUBIC)` gives.  One more draw follows the ones above:
      4. `us = rs.random_sample(N)`             -- slot k: factor = min_factor + us[k] * (1 - min_factor),
                                                   Hn = int(H * factor), Wn = int(W * factor), and at least
                                                   ceil(H / 2), ceil(W / 2): the kernel downscales by at most 2,
                                                   which an odd side at a factor just above 0.5 would exceed;
    y0 and x0 come from the same uy / ux with (Hn, Wn) in the place of (H, W), and `schedule(epoch)` returns
    rows (image, y0, x0, flip, Hn, Wn).  A batch is then one 40*B-byte table and one lic_resample_u8_to_f32
    launch.  Images with min(H, W) * min_factor < crop are refused (the reference discards them,
    preprocess.py:61).

    `resident=True` uploads all pixel bytes once; a batch is one pinned 32*B-byte job table and one
    lic_window_u8_to_f32 launch.  `resident=False` concatenates the B source images of a batch into a pinned
    staging buffer, copies it once and runs the same kernel with offsets into that buffer."""

    min_factor: Optional[float] = None

    def __init__(self, dataset: RaggedShardDataset, batch_size: int, crop: int = 256, device="cuda", seed: int = 0,
                 hflip: bool = False, resident: bool = True, drop_last: bool = True, rank: int = 0, world_size: int = 1,
                 min_factor: Optional[float] = None):
        self.ds, self.bs, self.crop, self.device = dataset, int(batch_size), int(crop), torch.device(device)
        self.seed, self.hflip, self.resident, self.drop_last = int(seed), bool(hflip), bool(resident), bool(drop_last)
        self.rank, self.world = int(rank), int(world_size)
        self.epoch = 0
        if self.bs <= 0 or self.crop <= 0:
            raise ValueError("batch_size and crop must be positive")
        small = int(np.sum((dataset.sizes < self.crop).any(axis=1)))
        if small:
            raise ValueError(f"{small} of {len(dataset)} images are smaller than the {self.crop}x{self.crop} crop on a side")
        self.min_factor = None if min_factor is None else float(min_factor)
        if self.min_factor is not None:
            if not 0.5 <= self.min_factor <= 1.0:
                raise ValueError(f"min_factor must lie in [0.5, 1], got {min_factor}")
            small = int(np.sum(dataset.sizes.min(axis=1) * self.min_factor < self.crop))
            if small:
                raise ValueError(f"{small} of {len(dataset)} images are too small for a {self.crop}x{self.crop} crop "
                                 f"after a downscale by min_factor={self.min_factor}")
        self._per = len(dataset) // self.world
        self._n_batches = self._per // self.bs if drop_last else (self._per + self.bs - 1) // self.bs
        self._pool = None
        if self.device.type != "cuda":
            raise L.LicError("RandomCropLoader windows on the GPU (lic_window_u8_to_f32): there is no CPU fallback")
        if self.resident:
            free, _ = torch.cuda.mem_get_info(self.device)
            if dataset.pool_bytes > free:
                raise RuntimeError(f"resident=True needs {dataset.pool_bytes} bytes of device memory for the image pool, "
                                   f"{free} are free: use resident=False or fewer shards")
            self._pool = torch.empty(dataset.pool_bytes, device=self.device, dtype=torch.uint8)
            at = 0
            for chunk in dataset.pool_chunks():
                self._pool[at:at + chunk.shape[0]].copy_(torch.from_numpy(np.array(chunk)))
                at += chunk.shape[0]

    def __len__(self) -> int:
        return self._n_batches

    def schedule(self, epoch: int) -> np.ndarray:
        """int64 [n, 4] rows (image, y0, x0, flip) of this rank's slots in `epoch`, n = per-rank image count
        (whole batches only when drop_last); with `min_factor`, [n, 6] rows (image, y0, x0, flip, Hn, Wn)"""
        n_all = len(self.ds)
        rs = np.random.RandomState(self.seed + int(epoch))
        order = rs.permutation(n_all)
        uy, ux = rs.random_sample(n_all), rs.random_sample(n_all)
        flip = rs.randint(0, 2, n_all) if self.hflip else np.zeros(n_all, np.int64)
        sizes = self.ds.sizes[order]
        if self.min_factor is not None:
            factor = self.min_factor + rs.random_sample(n_all) * (1.0 - self.min_factor)
            # int(H * factor), int(W * factor); an odd side at a factor just above 0.5 would land on (n - 1) / 2
            sizes = np.maximum((sizes * factor[:, None]).astype(np.int64), (sizes + 1) // 2)
        room = sizes - self.crop + 1                                    # [N, 2] positions available, >= 1
        y0 = np.minimum((uy * room[:, 0]).astype(np.int64), room[:, 0] - 1)
        x0 = np.minimum((ux * room[:, 1]).astype(np.int64), room[:, 1] - 1)
        cols = [order, y0, x0, flip] + ([sizes[:, 0], sizes[:, 1]] if self.min_factor is not None else [])
        rows = np.stack(cols, axis=1).astype(np.int64)
        rows = rows[self.rank * self._per:(self.rank + 1) * self._per]
        return rows[:self._n_batches * self.bs] if self.drop_last else rows

    def _batch(self, rows: np.ndarray) -> torch.Tensor:
        ds, img = self.ds, rows[:, 0]
        if self.resident:
            pool, offsets = self._pool, ds.offsets[img]
        else:
            nbytes = ds.sizes[img, 0] * ds.sizes[img, 1] * ds.C
            offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
            host = torch.empty(int(nbytes.sum()), dtype=torch.uint8, pin_memory=True)
            flat = host.numpy()
            for i, o, n in zip(img, offsets, nbytes):
                flat[o:o + n] = ds[int(i)].reshape(-1)
            pool = host.to(self.device, non_blocking=True)
        if self.min_factor is not None:
            jobs = resample_jobs(offsets, ds.sizes[img], rows[:, 4:6], rows[:, 1], rows[:, 2], rows[:, 3], self.crop,
                                 self.crop, ds.C)
            return resample_u8_to_f32(pool, jobs, self.crop, self.crop, ds.C)
        jobs = window_jobs(offsets, ds.sizes[img], rows[:, 1], rows[:, 2], rows[:, 3], self.crop, self.crop,
                           L.WINDOW_ZERO, ds.C)
        return window_u8_to_f32(pool, jobs, self.crop, self.crop, ds.C, L.WINDOW_ZERO)

    def __iter__(self) -> Iterator[torch.Tensor]:
        rows = self.schedule(self.epoch)
        self.epoch += 1
        for b in range(self._n_batches):
            yield self._batch(rows[b * self.bs:(b + 1) * self.bs])


# ---- logging statistics without full-tensor D2H copies (Trainer.py:167-217) -------------------
def tensor_stats(t: torch.Tensor, nbins: int = 64, lo: Optional[float] = None, hi: Optional[float] = None) -> dict:
    """count / mean / std / min / max / NaN count and an `nbins` histogram of a device tensor, computed
    on the device; only 6 doubles + nbins counters cross PCIe.  [lo, hi] defaults to the data range
    (one extra tiny pass)."""
    F_._require_cuda(t)
    x = t.detach().float().contiguous().view(-1)
    lib = L.load()
    ws = torch.empty(lib.lic_tensor_stats_workspace_bytes() // 8, device=x.device, dtype=torch.float64)
    stats = torch.empty(6, device=x.device, dtype=torch.float64)
    hist = torch.empty(nbins, device=x.device, dtype=torch.int64)

    def run(a, b):
        L.check(lib.lic_tensor_stats(F_._ptr(x), x.numel(), nbins, float(a), float(b), F_._ptr(stats), F_._ptr(hist),
                                     F_._ptr(ws), ws.numel() * 8, F_._stream()), "lic_tensor_stats")
        return stats.cpu().numpy(), hist.cpu().numpy()

    if lo is None or hi is None:
        s, _ = run(0.0, 1.0)
        lo_, hi_ = (s[3], s[4]) if s[0] > 0 else (0.0, 1.0)
        if not hi_ > lo_:
            hi_ = lo_ + 1.0
        lo, hi = (lo_ if lo is None else lo), (hi_ if hi is None else hi)
    s, h = run(lo, hi)
    n = max(s[0], 1.0)
    mean = s[1] / n
    var = max(s[2] / n - mean * mean, 0.0)
    return {"count": int(s[0]), "mean": float(mean), "std": float(var ** 0.5), "min": float(s[3]), "max": float(s[4]),
            "nan": int(s[5]), "lo": float(lo), "hi": float(hi), "hist": h.tolist()}
