"""Random-scale crops, host side: the numpy restatement of the 8-bit bicubic resize against the recorded
reference crops, the checks of resample_jobs, the loader's schedule with a scale draw, the shard filters, and the
layout of lic_resample_job.  No GPU."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import resample_ref as RR  # noqa: E402

from neural_image_compression_amd import _lib as L  # noqa: E402
from neural_image_compression_amd import data as D  # noqa: E402

FILES = sorted(glob.glob(os.path.join(HERE, "golden", "resample_*x*.npz")))


def fixture_cases():
    """(id, source, (target, new_w, new_h, left, top, forced), crop) of every recorded case"""
    out = []
    for f in FILES:
        z = np.load(f)
        for i, row in enumerate(z["cases"]):
            out.append((f"{os.path.basename(f)[9:-4]}-{i}", z["source"], tuple(int(v) for v in row), z[f"crop_{i}"]))
    return out


CASES = fixture_cases()


def test_fixtures_cover_what_they_are_meant_to():
    assert len(FILES) == 10 and len(CASES) >= 50
    rows = np.array([c[2] for c in CASES])
    shapes = {c[1].shape[:2] for c in CASES}
    assert shapes == {(37, 53), (64, 90), (97, 131)}
    assert set(rows[:, 0]) == {16, 40, 67}
    mfs = np.concatenate([np.load(f)["min_factors"] for f in FILES])
    assert {0.5, 0.75} <= set(mfs[~np.isnan(mfs)])
    sizes = np.array([(c[1].shape[1], c[1].shape[0]) for c in CASES])
    same = rows[:, 1:3] == sizes                                         # (new_w == W, new_h == H)
    assert np.any(same.all(axis=1))                                      # factor 1.0: nothing is resized
    assert np.any(same[:, 0] & ~same[:, 1]) and np.any(~same[:, 0] & same[:, 1])   # one axis only, either one
    # the two-level sources overshoot: the clamp at both ends shows in the recorded crops
    two = [c[3] for c in CASES if c[0].startswith("twolevel") and c[2][1] != c[1].shape[1]]
    assert any((c == 0).any() and (c == 255).any() and ((c > 0) & (c < 255)).any() for c in two)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_recorded_crop(case):
    _, src, (t, nw, nh, left, top, _), crop = case
    assert np.array_equal(RR.resample_window(src, nh, nw, top, left, t, t), crop)


@pytest.mark.parametrize("case", CASES[::7], ids=[c[0] for c in CASES[::7]])
def test_window_of_the_restatement_is_the_crop_of_the_whole(case):
    _, src, (t, nw, nh, left, top, _), _ = case
    whole = RR.resample_window(src, nh, nw)
    assert whole.shape == (nh, nw, 3)
    assert np.array_equal(RR.resample_window(src, nh, nw, top, left, t, t), whole[top:top + t, left:left + t])
    assert np.array_equal(RR.resample_window(src, nh, nw, top, left, t, t, flip=True),
                          whole[top:top + t, left:left + t][:, ::-1])
    # windows on each border of the resized image
    for y0, x0 in ((0, 0), (nh - t, nw - t), (0, nw - t), (nh - t, 0)):
        assert np.array_equal(RR.resample_window(src, nh, nw, y0, x0, t, t), whole[y0:y0 + t, x0:x0 + t])


def test_tap_counts_of_the_supported_range():
    """downscaling by at most 2 reads at most 9 taps (lic_resample's bound); a copied axis reads 1 of weight 2^22"""
    most = 0
    for n_in in (20, 37, 53, 64, 90, 131):
        for n_out in sorted({(n_in + 1) // 2, (3 * n_in) // 4, n_in - 1}):
            for xmin, k in RR.axis_coefficients(n_in, n_out):
                assert 0 <= xmin and xmin + len(k) <= n_in and 1 <= len(k) <= 9
                assert abs(int(k.sum()) - (1 << 22)) <= len(k)
                most = max(most, len(k))
    assert most >= 8
    assert all(x == i and k.tolist() == [1 << 22] for i, (x, k) in enumerate(RR.axis_coefficients(11, 11)))


def test_resample_job_mirrors_have_the_c_layout(tmp_path):
    names = list(D.RESAMPLE_JOB.names)
    assert ctypes.sizeof(L.ResampleJob) == 40 and D.RESAMPLE_JOB.itemsize == 40
    assert [n for n, _ in L.ResampleJob._fields_] == names
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lic.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(lic_resample_job));\n' +
                   "".join(f'printf("%zu\\n", offsetof(lic_resample_job, {n}));\n' for n in names) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert c[0] == 40
    assert c[1:] == [D.RESAMPLE_JOB.fields[n][1] for n in names] == [getattr(L.ResampleJob, n).offset for n in names]
    jobs = D.resample_jobs([0, 7], [(20, 30), (40, 50)], [(15, 20), (40, 25)], [1, 2], [3, 0], [0, 1], 8, 9)
    j = L.ResampleJob.from_buffer_copy(jobs[1].tobytes())
    assert (j.src_offset, j.Hs, j.Ws, j.Hn, j.Wn, j.y0, j.x0, j.flags, j.reserved) == (7, 40, 50, 40, 25, 2, 0, 1, 0)
    assert "lic_resample_u8_to_f32" in L.SIGNATURES


def test_resample_jobs_reject_what_the_kernel_cannot_check():
    ok = dict(offsets=0, sizes=[(20, 31)], new_sizes=[(10, 16)], y0=2, x0=8, flip=0, h=8, w=8)
    assert D.resample_jobs(**ok).shape == (1,)

    def bad(exc, **kw):
        with pytest.raises(exc):
            D.resample_jobs(**{**ok, **kw})

    bad(ValueError, sizes=[(0, 31)])                       # sizes >= 1
    bad(ValueError, h=0)
    bad(ValueError, w=-1)
    bad(ValueError, C=5)
    bad(ValueError, offsets=-1)                            # offsets inside the pool
    bad(ValueError, offsets=1, pool_bytes=20 * 31 * 3)
    assert D.resample_jobs(**{**ok, "pool_bytes": 20 * 31 * 3}).shape == (1,)
    bad(L.LicError, new_sizes=[(9, 16)])                   # below ceil(20 / 2)
    bad(L.LicError, new_sizes=[(10, 15)])                  # below ceil(31 / 2) = 16
    bad(L.LicError, new_sizes=[(21, 16)])                  # upscaling
    bad(L.LicError, new_sizes=[(10, 32)])
    bad(L.LicError, y0=-1)                                 # the window inside the resized image
    bad(L.LicError, x0=-1)
    bad(L.LicError, y0=3)                                  # 3 + 8 > 10
    bad(L.LicError, x0=9)                                  # 9 + 8 > 16
    assert D.resample_jobs(**{**ok, "new_sizes": [(20, 31)], "y0": 12, "x0": 23}).shape == (1,)   # a plain copy


SIZES = [(342, 420), (512, 768), (344, 343), (401, 377), (600, 350), (345, 900), (350, 350)]


@pytest.fixture(scope="module")
def ragged_ds(tmp_path_factory):
    rs = np.random.RandomState(3)
    path = str(tmp_path_factory.mktemp("resample") / "a.lic2")
    D.write_ragged_shard(path, [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES])
    return D.RaggedShardDataset(path)


def _loader(ds, **kw):
    # resident=False: the constructor touches no device
    return D.RandomCropLoader(ds, kw.pop("batch_size", 2), crop=kw.pop("crop", 256), resident=False, **kw)


@pytest.mark.parametrize("hflip", [False, True])
def test_schedule_without_min_factor_is_the_documented_draw_order(ragged_ds, hflip):
    ld = _loader(ragged_ds, seed=11, hflip=hflip, drop_last=False)
    assert ld.min_factor is None
    for epoch in (0, 3):
        rs = np.random.RandomState(11 + epoch)
        order = rs.permutation(len(SIZES))
        uy, ux = rs.random_sample(len(SIZES)), rs.random_sample(len(SIZES))
        flip = rs.randint(0, 2, len(SIZES)) if hflip else np.zeros(len(SIZES), np.int64)
        want = [(i, int(np.floor(uy[k] * (SIZES[i][0] - 255))), int(np.floor(ux[k] * (SIZES[i][1] - 255))), flip[k])
                for k, i in enumerate(order)]
        got = ld.schedule(epoch)
        assert got.shape == (len(SIZES), 4) and got.dtype == np.int64
        assert got.tolist() == [list(map(int, r)) for r in want]


@pytest.mark.parametrize("min_factor", [0.75, 1.0, 0.8])
def test_schedule_with_min_factor_follows_the_documented_draw_order(ragged_ds, min_factor):
    ld = _loader(ragged_ds, seed=5, hflip=True, min_factor=min_factor, drop_last=False)
    plain = _loader(ragged_ds, seed=5, hflip=True, drop_last=False)
    n = len(SIZES)
    for epoch in (0, 1, 7):
        rs = np.random.RandomState(5 + epoch)
        order = rs.permutation(n)
        uy, ux = rs.random_sample(n), rs.random_sample(n)
        flip = rs.randint(0, 2, n)
        us = rs.random_sample(n)                                         # drawn after the existing draws
        got = ld.schedule(epoch)
        assert got.shape == (n, 6) and got.dtype == np.int64
        assert np.array_equal(got[:, [0, 3]], plain.schedule(epoch)[:, [0, 3]])     # same images, same flips
        for k, i in enumerate(order):
            H, W = SIZES[i]
            factor = min_factor + us[k] * (1 - min_factor)
            Hn, Wn = int(H * factor), int(W * factor)
            y0, x0 = int(uy[k] * (Hn - 256 + 1)), int(ux[k] * (Wn - 256 + 1))
            assert got[k].tolist() == [i, y0, x0, flip[k], Hn, Wn]
            assert 256 <= Hn <= H and 256 <= Wn <= W
            assert 0 <= y0 and y0 + 256 <= Hn and 0 <= x0 and x0 + 256 <= Wn
        # what _batch hands to the kernel passes every check of resample_jobs
        sz = ragged_ds.sizes[got[:, 0]]
        D.resample_jobs(ragged_ds.offsets[got[:, 0]], sz, got[:, 4:6], got[:, 1], got[:, 2], got[:, 3], 256, 256, 3,
                        ragged_ds.pool_bytes)
    if min_factor == 1.0:
        assert np.array_equal(ld.schedule(2)[:, :4], plain.schedule(2))


def test_schedule_at_min_factor_one_half_stays_in_the_supported_range(ragged_ds):
    """odd sides at factors just above 0.5 would give (n - 1) / 2 < n / 2: the schedule holds them at ceil(n / 2)"""
    ld = _loader(ragged_ds, crop=128, seed=1, min_factor=0.5, drop_last=False)
    for epoch in range(40):
        got = ld.schedule(epoch)
        sz = ragged_ds.sizes[got[:, 0]]
        assert np.all(2 * got[:, 4:6] >= sz) and np.all(got[:, 4:6] <= sz)
        D.resample_jobs(0, sz, got[:, 4:6], got[:, 1], got[:, 2], got[:, 3], 128, 128)


def test_ranks_and_batches_with_min_factor(ragged_ds):
    whole = _loader(ragged_ds, seed=2, min_factor=0.75, drop_last=False).schedule(4)
    parts = [_loader(ragged_ds, seed=2, min_factor=0.75, drop_last=False, rank=r, world_size=2).schedule(4) for r in (0, 1)]
    assert np.array_equal(np.concatenate(parts), whole[:6])
    assert _loader(ragged_ds, batch_size=3, seed=2, min_factor=0.75).schedule(4).shape == (6, 6)


def test_constructor_refuses_small_images_and_bad_factors(ragged_ds):
    # min(H, W) * min_factor < crop is refused and the message names the count: the smallest sides are 342 and 343
    with pytest.raises(ValueError, match=r"^1 of 7 images"):
        _loader(ragged_ds, min_factor=0.748)               # 342 * 0.748 = 255.8, 343 * 0.748 = 256.6
    with pytest.raises(ValueError, match=r"^5 of 7 images"):
        _loader(ragged_ds, min_factor=0.7)                 # needs a side of 365.7: 512x768 and 401x377 remain
    with pytest.raises(ValueError, match=r"^7 of 7 images"):
        _loader(ragged_ds, crop=513, min_factor=1.0)       # the plain size check comes first and counts them all
    for f in (0.49, 1.01, -1.0, float("nan")):
        with pytest.raises(ValueError, match="min_factor"):
            _loader(ragged_ds, crop=64, min_factor=f)
    assert _loader(ragged_ds, crop=171, min_factor=0.5).min_factor == 0.5      # 342 * 0.5 = 171: just fits


def test_is_saturated_reproduces_the_recorded_verdicts():
    z = np.load(os.path.join(HERE, "golden", "resample_saturation.npz"))
    verdicts = z["verdicts"].tolist()
    assert True in verdicts and False in verdicts and len(verdicts) >= 6
    for i, (t, want) in enumerate(zip(z["thresholds"], verdicts)):
        assert D.is_saturated(z[f"image_{i}"], float(t)) is want, i


def test_shard_from_image_files_filters(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    z = np.load(os.path.join(HERE, "golden", "resample_saturation.npz"))
    at95 = [i for i, t in enumerate(z["thresholds"]) if t == 0.95]
    files = []
    for i in at95:
        files.append(str(tmp_path / f"s{i:02d}.png"))
        Image.fromarray(z[f"image_{i}"]).save(files[-1])
    keep = [i for i in at95 if not z["verdicts"][i]]
    assert 0 < len(keep) < len(at95)
    out = str(tmp_path / "sat.lic")
    assert D.shard_from_image_files(files, out) == len(at95)                         # defaults change nothing
    assert D.shard_from_image_files(files, out, saturation_thresh=0.95) == len(keep)
    ds = D.ShardDataset(out)
    assert all(np.array_equal(ds[k], z[f"image_{i}"]) for k, i in enumerate(keep))
    # min_side, on a ragged shard
    rs = np.random.RandomState(0)
    sizes = [(30, 50), (29, 80), (40, 30), (64, 29), (30, 30)]
    files = []
    for k, (h, w) in enumerate(sizes):
        files.append(str(tmp_path / f"m{k}.png"))
        Image.fromarray(rs.randint(100, 140, (h, w, 3)).astype(np.uint8)).save(files[-1])
    out = str(tmp_path / "min.lic2")
    assert D.shard_from_image_files(files, out, ragged=True) == 5
    assert D.shard_from_image_files(files, out, ragged=True, min_side=30) == 3
    assert D.RaggedShardDataset(out).sizes.tolist() == [[30, 50], [40, 30], [30, 30]]
    assert D.shard_from_image_files(files, out, ragged=True, min_side=30, saturation_thresh=0.95) == 3
    with pytest.raises(ValueError):
        D.shard_from_image_files(files, out, ragged=True, min_side=65)
