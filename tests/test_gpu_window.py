"""lic_window_u8_to_f32 / lic_window_f32 against the numpy statement of the window rule (window_ref) and
torch.nn.functional.pad.  Every comparison is bitwise: the kernels do one exact division or a copy."""
import numpy as np
import pytest
import torch

import window_ref as WR

pytestmark = pytest.mark.gpu


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
    """concatenated pixel bytes behind `prefix` filler bytes -> (uint8 array, offsets)"""
    sizes = np.array([a.size for a in images])
    offsets = prefix + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return np.concatenate([np.full(prefix, 0xAB, np.uint8)] + [a.reshape(-1) for a in images]), offsets


def _run(D, dev, images, rows, h, w, border, prefix=0):
    """rows: (image, y0, x0, flip) -> (kernel output as numpy [n,h,w,C], reference)"""
    rows = np.asarray(rows, np.int64)
    pool, offsets = _pool(images, prefix)
    sizes = np.array([images[i].shape[:2] for i in rows[:, 0]])
    jobs = D.window_jobs(offsets[rows[:, 0]], sizes, rows[:, 1], rows[:, 2], rows[:, 3], h, w, border,
                         pool_bytes=pool.size)
    got = D.window_u8_to_f32(torch.from_numpy(pool).to(dev), jobs, h, w, 3, border)
    assert got.shape == (len(rows), 3, h, w) and got.is_contiguous(memory_format=torch.channels_last)
    ref = np.stack([WR.window_ref(images[i], y, x, h, w, border, bool(f)) for i, y, x, f in rows])
    return got.permute(0, 2, 3, 1).cpu().numpy(), ref.astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("flip", [0, 1])
def test_training_size_crops_from_a_ragged_pool(env, flip):
    """B = 32 crops of 256^2 (6.3 M floats: the grid-stride loop wraps, 2048 blocks hold 2.1 M) from images of odd
    and even widths at odd byte offsets; first / last row and column windows included"""
    L, D, F_, dev = env
    shapes = [(375, 501), (256, 256), (257, 301), (300, 259), (512, 767), (260, 256), (256, 333), (411, 289)]
    images = [_image(h, w, 100 + i) for i, (h, w) in enumerate(shapes)]
    rs = np.random.RandomState(7 + flip)
    rows = []
    for k in range(32):
        i = k % len(images)
        H, W = shapes[i]
        y0, x0 = rs.randint(0, H - 255), rs.randint(0, W - 255)
        if k < 8:
            y0, x0 = (0, 0) if k % 2 == 0 else (H - 256, W - 256)
        rows.append((i, y0, x0, flip))
    got, ref = _run(D, dev, images, rows, 256, 256, WR.ZERO, prefix=1)
    assert got.size > 2048 * 256 * 4
    assert np.array_equal(got, ref)


def test_a_crop_equal_to_the_whole_image_is_lic_u8_to_f32(env):
    L, D, F_, dev = env
    for (h, w) in [(256, 256), (37, 53)]:
        img = _image(h, w, 5)
        got, ref = _run(D, dev, [img], [(0, 0, 0, 0)], h, w, WR.REPLICATE)
        assert np.array_equal(got, ref)
        plain = D.u8_to_f32(torch.from_numpy(img[None]).to(dev))
        assert np.array_equal(got, plain.permute(0, 2, 3, 1).cpu().numpy())


@pytest.mark.parametrize("align", ["topleft", "center"])
@pytest.mark.parametrize("border", [WR.ZERO, WR.REPLICATE, WR.REFLECT])
def test_pad_windows(env, border, align):
    L, D, F_, dev = env
    img = _image(375, 500, 11)
    Hp, Wp, top, left = F_.pad_geometry(375, 500, 64, align)
    assert (Hp, Wp) == (384, 512) and (top, left) == ((4, 6) if align == "center" else (0, 0))
    got, ref = _run(D, dev, [img], [(0, -top, -left, 0)], Hp, Wp, border, prefix=3)
    assert np.array_equal(got, ref)
    x, meta = D.load_image_u8(torch.from_numpy(img).to(dev), 64, ["zeros", "replicate", "reflect"][border], align)
    assert meta == (375, 500, top, left) and np.array_equal(x.permute(0, 2, 3, 1).cpu().numpy(), ref)
    if border != WR.REFLECT:                      # a 1x1 source has nothing to reflect about
        one = _image(1, 1, 12)
        Hp, Wp, top, left = F_.pad_geometry(1, 1, 64, align)
        got, ref = _run(D, dev, [one], [(0, -top, -left, 0)], 64, 64, border, prefix=2)
        assert np.array_equal(got, ref)
    else:
        with pytest.raises(L.LicError, match="LIC_ERR_INVALID"):
            D.load_image_u8(torch.from_numpy(_image(1, 1, 12)).to(dev), 64, "reflect", align)


@pytest.mark.parametrize("border", [WR.ZERO, WR.REPLICATE, WR.REFLECT])
def test_overhanging_flipped_and_ragged_tail_windows(env, border):
    """windows over one, two and four sides, flipped and not, of widths whose rows are no multiple of 4 floats (the
    4-float lanes then cross rows and images) and a total that is no multiple of 4"""
    L, D, F_, dev = env
    images = [_image(20, 31, 21), _image(33, 17, 22), _image(9, 40, 23)]
    for (h, w) in [(7, 5), (13, 11), (16, 16)]:
        rows = [(0, 3, 5, 0), (1, -4, 2, 1), (2, 1, -3, 0), (0, 12, 24, 1), (1, -2, -2, 0), (2, -5, 30, 1), (0, 0, 0, 1)]
        got, ref = _run(D, dev, images, rows, h, w, border, prefix=5)
        assert np.array_equal(got, ref), (h, w)


def _by_pad(x, y0, x0, h, w, mode):
    H, W = x.shape[2:]
    t, b, l, r = max(0, -y0), max(0, y0 + h - H), max(0, -x0), max(0, x0 + w - W)
    p = torch.nn.functional.pad(x, (l, r, t, b), mode={"zeros": "constant"}.get(mode, mode))
    return p[:, :, y0 + t:y0 + t + h, x0 + l:x0 + l + w]


@pytest.mark.parametrize("mode", ["zeros", "replicate", "reflect"])
def test_window_f32_matches_torch_pad_for_every_layout(env, mode):
    L, D, F_, dev = env
    torch.manual_seed(1)
    big = torch.randn(3, 5, 70, 90, device=dev)
    nchw = torch.randn(2, 3, 45, 61, device=dev)
    cases = [("nchw", nchw), ("channels_last", nchw.contiguous(memory_format=torch.channels_last)),
             ("view", big[1:3, 1:4, 5:50, 7:68]), ("strided view", big[:, ::2, :, 1::2])]
    for name, x in cases:
        H, W = x.shape[2:]
        for (y0, x0, h, w) in [(0, 0, 64, 64), (-3, -4, H + 10, W + 12), (5, 6, 17, 19), (0, 0, H, W), (H - 9, W - 7, 20, 21)]:
            got = F_.window(x, y0, x0, h, w, mode)
            assert got.shape == (x.shape[0], x.shape[1], h, w) and got.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(got, _by_pad(x, y0, x0, h, w, mode)), (name, y0, x0, h, w)
    x = nchw
    for align in ("topleft", "center"):
        Hp, Wp, top, left = F_.pad_geometry(45, 61, 64, align)
        p = F_.pad_to_multiple(x, 64, mode, align)
        assert p.shape == (2, 3, 64, 64) and torch.equal(p, _by_pad(x, -top, -left, 64, 64, mode))
        back = F_.crop_window(p, top, left, 45, 61)
        assert torch.equal(back, x) and back.is_contiguous(memory_format=torch.channels_last)


def test_window_entries_reject_bad_arguments(env):
    L, D, F_, dev = env
    x = torch.zeros(1, 3, 8, 8, device=dev)
    with pytest.raises(L.LicError, match="LIC_ERR_INVALID"):
        F_.window(x, -8, 0, 16, 8, "reflect")             # overhang of a whole side
    with pytest.raises(L.LicError, match="LIC_ERR_INVALID"):
        F_.window(x, 0, 0, 8, 16, "reflect")
    with pytest.raises(L.LicError):
        F_.pad_to_multiple(torch.zeros(1, 3, 8, 8))       # CPU tensor: no fallback
    with pytest.raises(L.LicError):
        F_.crop_window(torch.zeros(1, 3, 8, 8), 0, 0, 4, 4)
    with pytest.raises(L.LicError):
        D.load_image_u8(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        F_.crop_window(x, 4, 4, 8, 8)
    lib = L.load()
    out = torch.empty(1, 8, 8, 3, device=dev)
    ptr, st = F_._ptr, F_._stream()
    assert lib.lic_window_f32(None, 1, 1, 1, 1, 1, 3, 8, 8, 0, 0, 8, 8, 0, ptr(out), st) == -1
    assert lib.lic_window_f32(ptr(x), 192, 64, 8, 1, 1, 3, 8, 8, 0, 0, 8, 8, 3, ptr(out), st) == -1   # border 3
    assert lib.lic_window_f32(ptr(x), 192, 64, 8, 1, 0, 3, 8, 8, 0, 0, 8, 8, 0, ptr(out), st) == -1   # B = 0
    assert lib.lic_window_f32(ptr(x), 192, 64, 8, 1, 1, 3, 8, 8, 0, 0, 0, 8, 0, ptr(out), st) == -1   # h = 0
    assert lib.lic_window_u8_to_f32(None, None, 1, 8, 8, 3, 0, ptr(out), st) == -1
    assert lib.lic_window_u8_to_f32(ptr(x), ptr(x), 1, 8, 8, 3, 0, None, st) == -1
    assert lib.lic_window_u8_to_f32(ptr(x), ptr(x), 1 << 20, 1 << 10, 1 << 10, 3, 0, ptr(out), st) == -2  # > 2^31 - 1 floats
