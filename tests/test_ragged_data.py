"""Window rule, ragged shards and the random-crop schedule: host logic, no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_ref as WR  # noqa: E402

from neural_image_compression_amd import _lib as L  # noqa: E402
from neural_image_compression_amd import data as D  # noqa: E402

NP_MODE = {WR.ZERO: "constant", WR.REPLICATE: "edge", WR.REFLECT: "reflect"}


def _image(h, w, seed, c=3):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)


def _by_np_pad(img, y0, x0, h, w, border):
    Hs, Ws = img.shape[:2]
    t, b = max(0, -y0), max(0, y0 + h - Hs)
    l, r = max(0, -x0), max(0, x0 + w - Ws)
    p = np.pad(img, ((t, b), (l, r), (0, 0)), mode=NP_MODE[border])
    return p[y0 + t:y0 + t + h, x0 + l:x0 + l + w]


WINDOWS = [  # (Hs, Ws, y0, x0, h, w)
    (20, 31, 3, 5, 8, 9),          # inside
    (20, 31, 0, 0, 20, 31),        # the whole image
    (20, 31, -4, 2, 10, 10),       # over the top
    (20, 31, 14, 2, 10, 10),       # over the bottom
    (20, 31, 2, -6, 10, 10),       # over the left
    (20, 31, 2, 25, 10, 10),       # over the right
    (20, 31, -3, -5, 12, 12),      # top and left
    (20, 31, 12, 24, 12, 12),      # bottom and right
    (20, 31, -2, -2, 24, 35),      # all four
]


@pytest.mark.parametrize("border", [WR.ZERO, WR.REPLICATE, WR.REFLECT])
@pytest.mark.parametrize("win", WINDOWS)
def test_window_ref_is_np_pad_then_slice(win, border):
    Hs, Ws, y0, x0, h, w = win
    img = _image(Hs, Ws, 1)
    assert np.array_equal(WR.window_ref(img, y0, x0, h, w, border), _by_np_pad(img, y0, x0, h, w, border))
    flipped = WR.window_ref(img, y0, x0, h, w, border, flip=True)
    assert np.array_equal(flipped, _by_np_pad(img, y0, x0, h, w, border)[:, ::-1])


@pytest.mark.parametrize("border", [WR.ZERO, WR.REPLICATE])
def test_window_ref_one_pixel_wide_source(border):
    img = _image(9, 1, 2)
    assert np.array_equal(WR.window_ref(img, -2, -3, 13, 8, border), _by_np_pad(img, -2, -3, 13, 8, border))
    one = _image(1, 1, 3)
    assert np.array_equal(WR.window_ref(one, 0, 0, 64, 64, border), _by_np_pad(one, 0, 0, 64, 64, border))


def test_reflect_overhang_of_a_whole_side_is_rejected():
    img = _image(5, 7, 4)
    assert np.array_equal(WR.window_ref(img, -4, -6, 13, 19, WR.REFLECT), _by_np_pad(img, -4, -6, 13, 19, WR.REFLECT))
    with pytest.raises(ValueError):
        WR.window_ref(img, -5, 0, 8, 7, WR.REFLECT)          # 5 rows above a 5-row image
    with pytest.raises(ValueError):
        WR.window_ref(img, 0, 0, 5, 14, WR.REFLECT)          # 7 columns right of a 7-column image
    with pytest.raises(ValueError):
        WR.window_ref(_image(1, 1, 5), 0, 0, 2, 1, WR.REFLECT)
    # the job-table builder applies the same rule before anything is uploaded
    with pytest.raises(L.LicError, match="LIC_ERR_INVALID"):
        D.window_jobs(0, [(5, 7)], -5, 0, 0, 8, 7, "reflect")
    with pytest.raises(L.LicError, match="LIC_ERR_INVALID"):
        D.window_jobs(0, [(5, 7)], 0, 0, 0, 5, 14, "reflect")
    assert D.window_jobs(0, [(5, 7)], -4, -6, 0, 13, 19, "reflect").shape == (1,)


def test_window_job_mirrors_are_32_bytes():
    assert ctypes.sizeof(L.WindowJob) == 32
    assert D.WINDOW_JOB.itemsize == 32
    assert [n for n, _ in L.WindowJob._fields_] == list(D.WINDOW_JOB.names)
    for name in D.WINDOW_JOB.names:
        assert getattr(L.WindowJob, name).offset == D.WINDOW_JOB.fields[name][1]
    jobs = D.window_jobs([0, 10], [(2, 3), (4, 5)], [0, -1], [1, 0], [0, 1], 2, 2, "zeros")
    c = L.WindowJob.from_buffer_copy(jobs[1].tobytes())
    assert (c.src_offset, c.Hs, c.Ws, c.y0, c.x0, c.flags, c.reserved) == (10, 4, 5, -1, 0, 1, 0)


def test_window_jobs_reject_what_the_kernel_cannot_check():
    with pytest.raises(ValueError):
        D.window_jobs(0, [(0, 3)], 0, 0, 0, 2, 2, "zeros")
    with pytest.raises(ValueError):
        D.window_jobs(-1, [(2, 3)], 0, 0, 0, 2, 2, "zeros")
    with pytest.raises(ValueError):
        D.window_jobs(4, [(2, 3)], 0, 0, 0, 2, 2, "zeros", pool_bytes=21)
    with pytest.raises(ValueError):
        D.window_jobs(0, [(2, 3)], 0, 0, 0, 2, 2, "mirror")


SIZES = [(375, 500), (512, 768), (256, 256), (257, 301)]


@pytest.fixture()
def ragged(tmp_path):
    imgs = [_image(h, w, 10 + i) for i, (h, w) in enumerate(SIZES)]
    path = str(tmp_path / "a.lic2")
    D.write_ragged_shard(path, imgs)
    return path, imgs


def test_ragged_shard_round_trip(ragged, tmp_path):
    path, imgs = ragged
    ds = D.RaggedShardDataset(path)
    assert len(ds) == 4 and ds.C == 3
    assert ds.sizes.tolist() == [list(s) for s in SIZES]
    for i, a in enumerate(imgs):
        assert ds[i].dtype == np.uint8 and np.array_equal(ds[i], a)
    assert np.array_equal(ds[-1], imgs[-1])
    with pytest.raises(IndexError):
        ds[4]
    # two shards: indices run on, offsets address the concatenated pixel bytes
    more = [_image(300, 259, 20), _image(256, 400, 21)]
    p2 = str(tmp_path / "b.lic2")
    D.write_ragged_shard(p2, more)
    both = D.RaggedShardDataset([path, p2])
    assert len(both) == 6 and np.array_equal(both[5], more[1])
    pool = np.concatenate(list(both.pool_chunks(chunk_bytes=100000)))
    assert pool.size == both.pool_bytes == sum(a.size for a in imgs + more)
    for i, a in enumerate(imgs + more):
        assert np.array_equal(pool[both.offsets[i]:both.offsets[i] + a.size].reshape(a.shape), a)


def test_shard_formats_do_not_open_with_each_other(ragged, tmp_path):
    path, _ = ragged
    with pytest.raises(ValueError):
        D.ShardDataset(path)
    p1 = str(tmp_path / "one.lic")
    D.write_shard(p1, np.stack([_image(8, 8, 1), _image(8, 8, 2)]))
    assert len(D.ShardDataset(p1)) == 2
    with pytest.raises(ValueError):
        D.RaggedShardDataset(p1)
    bad = str(tmp_path / "bad.lic2")
    raw = bytearray(open(path, "rb").read())
    raw[0] ^= 1
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(ValueError):
        D.RaggedShardDataset(bad)
    cut = str(tmp_path / "cut.lic2")
    open(cut, "wb").write(bytes(raw[:len(raw) - 1]).replace(raw[:8], D.MAGIC2, 1))
    with pytest.raises(ValueError):
        D.RaggedShardDataset(cut)


def test_shard_from_image_files_ragged_and_default(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    files = []
    for i, (h, w) in enumerate([(20, 30), (17, 23)]):
        f = str(tmp_path / f"{i}.png")
        Image.fromarray(_image(h, w, 30 + i)).save(f)
        files.append(f)
    with pytest.raises(ValueError, match="differ in size"):
        D.shard_from_image_files(files, str(tmp_path / "x.lic"))
    assert D.shard_from_image_files(files, str(tmp_path / "x.lic2"), ragged=True) == 2
    ds = D.RaggedShardDataset(str(tmp_path / "x.lic2"))
    assert np.array_equal(ds[1], _image(17, 23, 31))


class _Sizes:
    """what RandomCropLoader.schedule needs of a dataset"""

    def __init__(self, sizes):
        self.sizes = np.asarray(sizes, np.int64)

    def __len__(self):
        return len(self.sizes)


def _loader(sizes, **kw):
    """a loader without a device: schedule() is host arithmetic"""
    ld = D.RandomCropLoader.__new__(D.RandomCropLoader)
    ld.ds = _Sizes(sizes)
    ld.bs, ld.crop, ld.seed, ld.hflip = kw.get("batch_size", 4), kw.get("crop", 256), kw.get("seed", 0), kw.get("hflip", True)
    ld.rank, ld.world, ld.drop_last = kw.get("rank", 0), kw.get("world_size", 1), kw.get("drop_last", True)
    ld._per = len(ld.ds) // ld.world
    ld._n_batches = ld._per // ld.bs if ld.drop_last else -(-ld._per // ld.bs)
    return ld


def test_schedule_is_a_pure_function_of_seed_epoch_rank():
    rs = np.random.RandomState(0)
    sizes = np.stack([rs.randint(256, 700, 37), rs.randint(256, 900, 37)], axis=1)
    a, b = _loader(sizes, seed=5), _loader(sizes, seed=5)
    s0 = a.schedule(0)
    assert s0.shape == (36, 4) and np.array_equal(s0, b.schedule(0)) and np.array_equal(s0, a.schedule(0))
    assert not np.array_equal(s0, a.schedule(1))
    assert not np.array_equal(s0, _loader(sizes, seed=6).schedule(0))
    assert np.array_equal(a.schedule(1), _loader(sizes, seed=6).schedule(0))     # RandomState(seed + epoch)
    for s in (s0, a.schedule(1), a.schedule(7)):
        img, y0, x0, flip = s.T
        assert len(set(img.tolist())) == len(img)
        assert np.all(y0 >= 0) and np.all(y0 + 256 <= sizes[img, 0])
        assert np.all(x0 >= 0) and np.all(x0 + 256 <= sizes[img, 1])
        assert set(flip.tolist()) <= {0, 1}
    assert len(set(a.schedule(3)[:, 3].tolist())) == 2                            # both flip values occur
    assert not _loader(sizes, hflip=False).schedule(0)[:, 3].any()
    assert _loader(sizes, drop_last=False).schedule(0).shape == (37, 4)
    # images exactly as large as the crop have one position
    assert not _loader([(256, 256)] * 8).schedule(2)[:, 1:3].any()


def test_schedule_ranks_are_disjoint():
    rs = np.random.RandomState(1)
    sizes = np.stack([rs.randint(256, 700, 41), rs.randint(256, 900, 41)], axis=1)
    r0 = _loader(sizes, rank=0, world_size=2, batch_size=5).schedule(4)
    r1 = _loader(sizes, rank=1, world_size=2, batch_size=5).schedule(4)
    assert r0.shape == r1.shape == (20, 4)
    assert not set(r0[:, 0].tolist()) & set(r1[:, 0].tolist())
    whole = _loader(sizes, batch_size=1).schedule(4)
    assert np.array_equal(whole[:20], r0) and np.array_equal(whole[20:40], r1)


def test_batch_ref_matches_plain_slicing():
    imgs = [_image(h, w, 40 + i) for i, (h, w) in enumerate([(300, 311), (256, 257)])]
    rows = np.array([[0, 44, 55, 0], [1, 0, 1, 1]])
    got = WR.batch_ref(imgs, rows, 256)
    assert got.dtype == np.float32
    assert np.array_equal(got[0], imgs[0][44:300, 55:311].astype(np.float32) / np.float32(255))
    assert np.array_equal(got[1], imgs[1][:, 1:257][:, ::-1].astype(np.float32) / np.float32(255))
