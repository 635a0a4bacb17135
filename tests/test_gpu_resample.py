"""lic_resample_u8_to_f32 against the crops recorded from the reference's preprocess.py (Pillow's 8-bit bicubic)
and against the numpy restatement of the definition (resample_ref).  Every comparison is bitwise: the kernel's
coefficients are the definition's integers and its arithmetic is integer up to one exact division."""
import glob
import os

import numpy as np
import pytest
import torch

import resample_ref as RR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILES = sorted(glob.glob(os.path.join(HERE, "golden", "resample_*x*.npz")))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import data as D
    from neural_image_compression_amd import functional as F_
    return L, D, F_, torch.device("cuda:0")


def _image(h, w, seed, c=3):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)


def _pool(images, prefix=0):
    """pixel bytes behind `prefix` filler bytes, one more filler byte wherever it makes an image's offset odd
    -> (uint8 array, offsets)"""
    parts, offsets, at = [np.full(prefix, 0xAB, np.uint8)], [], prefix
    for a in images:
        if at % 2 == 0:
            parts.append(np.full(1, 0xAB, np.uint8))
            at += 1
        offsets.append(at)
        parts.append(a.reshape(-1))
        at += a.size
    return np.concatenate(parts), np.array(offsets, np.int64)


def _run(D, dev, images, rows, h, w, prefix=0):
    """rows: (image, Hn, Wn, y0, x0, flip) -> kernel output as numpy [n,h,w,C], one launch"""
    rows = np.asarray(rows, np.int64)
    pool, offsets = _pool(images, prefix)
    sizes = np.array([images[i].shape[:2] for i in rows[:, 0]])
    C = images[0].shape[2]
    jobs = D.resample_jobs(offsets[rows[:, 0]], sizes, rows[:, 1:3], rows[:, 3], rows[:, 4], rows[:, 5], h, w, C,
                           pool_bytes=pool.size)
    got = D.resample_u8_to_f32(torch.from_numpy(pool).to(dev), jobs, h, w, C)
    assert got.shape == (len(rows), C, h, w) and got.is_contiguous(memory_format=torch.channels_last)
    return got.permute(0, 2, 3, 1).cpu().numpy()


def _ref(images, rows, h, w):
    return np.stack([RR.resample_window_f32(images[i], Hn, Wn, y0, x0, h, w, bool(f)) for i, Hn, Wn, y0, x0, f in rows])


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[9:-4] for f in FILES])
def test_recorded_reference_crops_bit_for_bit(env, path):
    """every recorded case of a fixture file, plain and mirrored; cases of one crop size share a launch"""
    L, D, F_, dev = env
    z = np.load(path)
    src, cases = z["source"], z["cases"]
    assert len(cases) >= 4
    for t in sorted(set(cases[:, 0])):
        idx = [i for i in range(len(cases)) if cases[i, 0] == t]
        for flip in (0, 1):
            rows = [(0, cases[i, 2], cases[i, 1], cases[i, 4], cases[i, 3], flip) for i in idx]
            got = _run(D, dev, [src], rows, int(t), int(t), prefix=1 + flip)
            for k, i in enumerate(idx):
                crop = z[f"crop_{i}"]
                want = np.float32(crop[:, ::-1] if flip else crop) / np.float32(255)
                assert got[k].dtype == np.float32 and np.array_equal(got[k], want), (i, flip, cases[i].tolist())


SHAPES = [(97, 131), (80, 90), (140, 134), (80, 121), (151, 181)]


@pytest.mark.parametrize("crop", [67, 40])
def test_five_jobs_of_different_sources_sizes_and_windows_in_one_launch(env, crop):
    """B = 5 in one pool, every image at an odd byte offset: windows on each of the four borders of the resized
    image (first taps clamp at 0, tap runs end at n_in), a copied image whose bits equal lic_window_u8_to_f32's,
    one axis copied, a factor of exactly 0.5 (8 taps, the most the supported range reaches: a 9th needs a
    downscale beyond 2), mirrored and plain.  Crop 67 has rows of 201 floats -- three rows in four start off a
    16-byte address, every row ends in scalar stores -- and spans several 32 x 64 tiles; crop 40 is narrower than
    a tile."""
    L, D, F_, dev = env
    images = [_image(h, w, 40 + i) for i, (h, w) in enumerate(SHAPES)]
    images[1] = (np.random.RandomState(9).randint(0, 2, (80, 90, 3)) * 255).astype(np.uint8)     # overshoots clamp
    c = crop
    rows = [(0, 73, 99, 0, 99 - c, 0),                 # top and right borders
            (1, 80, 90, 80 - c, 3, 1),                 # Hn == Hs, Wn == Ws: a copy; bottom border, mirrored
            (2, 70, 67, 70 - c, 0, 1),                 # factor exactly 0.5; bottom and left borders, mirrored
            (3, 80, 75, 5, 75 - c, 0),                 # rows copied, columns resized; right border
            (4, 113, 136, 113 - c, 136 - c, 1)]        # bottom and right borders, mirrored
    assert max(len(k) for _, k in RR.axis_coefficients(140, 70)) == 8
    pool, offsets = _pool(images, 3)
    assert np.all(offsets % 2 == 1)
    got = _run(D, dev, images, rows, c, c, prefix=3)
    want = _ref(images, rows, c, c)
    for k in range(5):
        assert np.array_equal(got[k], want[k]), (k, rows[k])
    # the copied job through lic_window_u8_to_f32
    i, Hn, Wn, y0, x0, f = rows[1]
    assert images[i].shape[:2] == (Hn, Wn)
    jobs = D.window_jobs(offsets[i:i + 1], [(Hn, Wn)], y0, x0, f, c, c, "zeros", pool_bytes=pool.size)
    win = D.window_u8_to_f32(torch.from_numpy(pool).to(dev), jobs, c, c, 3, "zeros")
    assert np.array_equal(win.permute(0, 2, 3, 1).cpu().numpy()[0], got[1])


def test_training_size_crops(env):
    """crops of 256^2 (8 x 4 tiles each) from sources of odd and even sides, factors from 0.5 to 1, half mirrored"""
    L, D, F_, dev = env
    shapes = [(375, 501), (512, 768), (300, 259), (511, 640)]
    images = [_image(h, w, 60 + i) for i, (h, w) in enumerate(shapes)]
    rows = [(0, 300, 400, 44, 144, 0), (1, 256, 384, 0, 128, 1), (2, 300, 259, 44, 3, 1), (3, 256, 320, 0, 64, 0),
            (1, 384, 576, 128, 0, 0), (3, 511, 639, 255, 383, 1)]
    got = _run(D, dev, images, rows, 256, 256, prefix=1)
    assert np.array_equal(got, _ref(images, rows, 256, 256))


@pytest.mark.parametrize("C", [1, 2, 4])
def test_other_channel_counts(env, C):
    L, D, F_, dev = env
    images = [_image(61, 83, 70 + C, C), _image(50, 45, 80 + C, C)]
    rows = [(0, 40, 70, 3, 1, 1), (1, 25, 23, 0, 0, 0), (0, 61, 83, 30, 50, 0)]
    got = _run(D, dev, images, rows, 23, 21, prefix=1)
    assert np.array_equal(got, _ref(images, rows, 23, 21))


def test_nothing_is_written_outside_out_and_bad_arguments_launch_nothing(env):
    L, D, F_, dev = env
    lib, ptr, st = L.load(), F_._ptr, F_._stream()
    images = [_image(97, 131, 1), _image(80, 90, 2)]
    rows = np.array([(0, 73, 99, 6, 32, 0), (1, 80, 70, 13, 3, 1), (0, 97, 131, 30, 64, 1)], np.int64)
    h = w = 67
    pool, offsets = _pool(images, 1)
    jobs = D.resample_jobs(offsets[rows[:, 0]], [images[i].shape[:2] for i in rows[:, 0]], rows[:, 1:3], rows[:, 3],
                           rows[:, 4], rows[:, 5], h, w, 3, pool.size)
    n = 3 * h * w * 3
    guard = 4096
    buf = torch.full((guard + n + guard,), -7.0, device=dev)
    out = buf[guard:guard + n]
    assert out.data_ptr() % 16 == 0
    dpool = torch.from_numpy(pool).to(dev)
    djobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    assert lib.lic_resample_u8_to_f32(ptr(dpool), ptr(djobs), 3, h, w, 3, ptr(out), st) == 0
    got = buf.cpu().numpy()
    assert np.all(got[:guard] == -7.0) and np.all(got[guard + n:] == -7.0)
    want = _ref(images, [tuple(r) for r in rows], h, w)
    assert np.array_equal(got[guard:guard + n].reshape(3, h, w, 3), want)
    # entry validation: LIC_ERR_INVALID and nothing launched, so `out` keeps its canary
    buf.fill_(-7.0)
    bad = [(None, ptr(djobs), 3, h, w, 3, ptr(out)), (ptr(dpool), None, 3, h, w, 3, ptr(out)),
           (ptr(dpool), ptr(djobs), 3, h, w, 3, None), (ptr(dpool), ptr(djobs), 0, h, w, 3, ptr(out)),
           (ptr(dpool), ptr(djobs), -1, h, w, 3, ptr(out)), (ptr(dpool), ptr(djobs), 3, 0, w, 3, ptr(out)),
           (ptr(dpool), ptr(djobs), 3, h, -5, 3, ptr(out)), (ptr(dpool), ptr(djobs), 3, h, w, 0, ptr(out)),
           (ptr(dpool), ptr(djobs), 3, h, w, 3, ptr(buf[guard + 1:])),          # out not 16-byte aligned
           (ptr(dpool), ptr(djobs[4:]), 3, h, w, 3, ptr(out))]                  # table not 8-byte aligned
    for args in bad:
        assert lib.lic_resample_u8_to_f32(*args, st) == -1, args
    assert lib.lic_resample_u8_to_f32(ptr(dpool), ptr(djobs), 3, h, w, 5, ptr(out), st) == -2           # C > 4
    assert lib.lic_resample_u8_to_f32(ptr(dpool), ptr(djobs), 1 << 20, 1 << 10, 1 << 10, 3, ptr(out), st) == -2
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())
    with pytest.raises(L.LicError):
        D.resample_u8_to_f32(torch.from_numpy(pool), jobs, h, w)                # CPU tensor: no fallback
    with pytest.raises(ValueError):
        D.resample_u8_to_f32(dpool[:1000], jobs, h, w)                          # an image outside the pool


def test_the_launch_is_captured_into_a_graph_and_replayed_on_a_new_table(env):
    """no allocation, no synchronisation: the launch records as one graph node; the job table is device memory, so a
    replay after the table was overwritten in place computes the new windows"""
    L, D, F_, dev = env
    lib, ptr = L.load(), F_._ptr
    images = [_image(97, 131, 21), _image(80, 90, 22)]
    pool, offsets = _pool(images, 1)
    tables, wants = [], []
    for rows in ([(0, 73, 99, 6, 32, 0), (1, 80, 70, 13, 3, 1)], [(1, 61, 90, 0, 20, 0), (0, 97, 70, 30, 3, 1)]):
        r = np.asarray(rows, np.int64)
        jobs = D.resample_jobs(offsets[r[:, 0]], [images[i].shape[:2] for i in r[:, 0]], r[:, 1:3], r[:, 3], r[:, 4],
                               r[:, 5], 40, 67, 3, pool.size)
        tables.append(torch.from_numpy(jobs.view(np.uint8).copy()).to(dev))
        wants.append(_ref(images, rows, 40, 67))
    dpool = torch.from_numpy(pool).to(dev)
    table = tables[0].clone()
    out = torch.zeros(2, 40, 67, 3, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.check(lib.lic_resample_u8_to_f32(ptr(dpool), ptr(table), 2, 40, 67, 3, ptr(out), F_._stream()), "capture")
    for k in (0, 1, 0):
        table.copy_(tables[k])
        out.zero_()
        g.replay()
        assert np.array_equal(out.cpu().numpy(), wants[k]), k


@pytest.fixture(scope="module")
def small_shard(tmp_path_factory):
    sizes = [(70, 130), (101, 87), (130, 71), (96, 96), (77, 113), (125, 128)]
    imgs = [_image(h, w, 300 + i) for i, (h, w) in enumerate(sizes)]
    path = str(tmp_path_factory.mktemp("resample_gpu") / "six.lic2")
    return path, imgs


@pytest.mark.parametrize("resident", [True, False])
def test_random_crop_loader_with_min_factor(env, small_shard, resident):
    """6 images of 70..130 a side, crop 32, batches of 3, mirrored at random: every batch is resample_ref on
    schedule(epoch)'s rows, resident pool or staged per batch"""
    L, D, F_, dev = env
    path, imgs = small_shard
    D.write_ragged_shard(path, imgs)
    ds = D.RaggedShardDataset(path)
    ld = D.RandomCropLoader(ds, 3, crop=32, device=dev, seed=4, hflip=True, resident=resident, min_factor=0.75)
    assert len(ld) == 2
    for epoch in range(2):
        rows = ld.schedule(epoch)
        assert rows.shape == (6, 6) and sorted(rows[:, 0].tolist()) == list(range(6))
        batches = list(ld)
        assert len(batches) == 2
        for b, x in enumerate(batches):
            assert x.shape == (3, 3, 32, 32) and x.is_contiguous(memory_format=torch.channels_last)
            r = rows[3 * b:3 * b + 3]
            want = _ref(imgs, [(i, Hn, Wn, y0, x0, f) for i, y0, x0, f, Hn, Wn in r], 32, 32)
            assert np.array_equal(x.permute(0, 2, 3, 1).cpu().numpy(), want), (epoch, b)
    assert set(rows[:, 3].tolist()) == {0, 1}
    # without min_factor the loader is the plain window loader
    plain = D.RandomCropLoader(ds, 3, crop=32, device=dev, seed=4, hflip=True, resident=resident)
    assert plain.schedule(0).shape == (6, 4) and next(iter(plain)).shape == (3, 3, 32, 32)
