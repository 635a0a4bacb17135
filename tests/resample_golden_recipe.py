"""Writes tests/golden/resample_*.npz: what the reference's preprocess.py computes (random downscale with
Pillow's Image.BICUBIC, one random crop; the saturation verdict), recorded as data.  Not a test module.

    python tests/resample_golden_recipe.py REFERENCE_DIR        (needs Pillow and the reference's imports)

`random_downsample_crop` and `is_saturated` are imported from REFERENCE_DIR/preprocess.py and called as they
are; the function's `random.uniform` / `random.randint` draws go through recording wrappers, which is how a
fixture knows the factor and the crop origin.  A wrapper can also force the factor (the factor-1.0 cases).

A case in which only ONE axis changes size cannot come out of `random_downsample_crop`: it scales both sides
by one factor f, and int(W * f) == W needs f >= 1.  Those cases ('axis' files) make the function's two Pillow
calls -- `resize((new_w, new_h), Image.BICUBIC)` and `crop` -- directly, with new_w or new_h set to the source
side.

Every file: `source` uint8 [H, W, 3]; `cases` int64 [n, 6] rows (target, new_w, new_h, left, top, forced);
`factors`, `min_factors` float64 [n]; `crop_<i>` uint8 [target, target, 3].
resample_saturation.npz: `image_<i>` uint8, `thresholds` float64 [n], `verdicts` bool [n].
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SIZES = [(37, 53), (64, 90), (97, 131)]                                # (H, W)
# (target, min_factor) per source size: every pair passes the reference's discard rule min(H, W) * min_factor
# >= target, so the function never returns None
PLAN = {(37, 53): [(16, 0.5), (16, 0.75)],
        (64, 90): [(16, 0.5), (16, 0.75), (40, 0.75)],
        (97, 131): [(16, 0.5), (40, 0.5), (40, 0.75), (67, 0.75)]}


def make_source(kind: str, H: int, W: int, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    if kind == "noise":
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "twolevel":                                              # overshoots: exercises the clamp
        return (rs.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 255) // (W - 1), (y * 255) // (H - 1), ((x + y) * 255) // (H + W - 2)], axis=2).astype(np.uint8)


class Recorder:
    """stands in for the `random` module inside preprocess.py"""

    def __init__(self, seed: int, force_factor=None):
        self._r = random.Random(seed)
        self._force = force_factor
        self.uniform_draws, self.randint_draws = [], []

    def uniform(self, a, b):
        v = self._r.uniform(a, b) if self._force is None else self._force
        self.uniform_draws.append(v)
        return v

    def randint(self, a, b):
        v = self._r.randint(a, b)
        self.randint_draws.append(v)
        return v


def run_reference(P, Image, src, target, min_factor, seed, force_factor=None):
    rec = Recorder(seed, force_factor)
    P.random = rec
    try:
        crop = P.random_downsample_crop(Image.fromarray(src), target_size=target, min_factor=min_factor)
    finally:
        P.random = random
    assert crop is not None
    (factor,), (left, top) = rec.uniform_draws, rec.randint_draws
    H, W, _ = src.shape
    row = (target, int(W * factor), int(H * factor), left, top, int(force_factor is not None))
    # lic_resample_u8_to_f32 downscales by at most 2; an odd side at a factor just above 0.5 lands on (n - 1) / 2
    assert 2 * row[1] >= W and 2 * row[2] >= H, "pick another seed: this draw halves an odd side and rounds down"
    return row, factor, np.asarray(crop, np.uint8)


def run_one_axis(Image, src, target, new_w, new_h, seed):
    r = random.Random(seed)
    resized = Image.fromarray(src).resize((new_w, new_h), Image.BICUBIC)
    left, top = r.randint(0, new_w - target), r.randint(0, new_h - target)
    crop = resized.crop((left, top, left + target, top + target))
    return (target, new_w, new_h, left, top, 2), float("nan"), np.asarray(crop, np.uint8)


def save(name, src, results, min_factors):
    arrays = {"source": src, "cases": np.array([r[0] for r in results], np.int64),
              "factors": np.array([r[1] for r in results], np.float64),
              "min_factors": np.array(min_factors, np.float64)}
    for i, r in enumerate(results):
        assert r[2].shape == (r[0][0], r[0][0], 3)
        arrays[f"crop_{i}"] = r[2]
    np.savez_compressed(os.path.join(GOLDEN, name), **arrays)


def main(reference_dir: str) -> None:
    sys.path.insert(0, reference_dir)
    import preprocess as P
    from PIL import Image

    seed = 1000
    for kind in ("noise", "twolevel", "ramp"):
        for (H, W) in SIZES:
            src = make_source(kind, H, W, seed)
            results, mfs = [], []
            for target, mf in PLAN[(H, W)]:
                for rep in range(2 if target == 16 else 1):
                    seed += 1
                    results.append(run_reference(P, Image, src, target, mf, seed))
                    mfs.append(mf)
            seed += 1
            results.append(run_reference(P, Image, src, 16, 0.75, seed, force_factor=1.0))
            mfs.append(0.75)
            save(f"resample_{kind}_{H}x{W}.npz", src, results, mfs)
    # one axis resized, the other copied
    src = make_source("noise", 64, 90, 77)
    results = [run_one_axis(Image, src, 40, 90, 47, 1), run_one_axis(Image, src, 40, 61, 64, 2),
               run_one_axis(Image, src, 16, 90, 32, 3), run_one_axis(Image, src, 16, 45, 64, 4)]
    save("resample_axis_64x90.npz", src, results, [float("nan")] * len(results))

    # is_saturated on both sides of its two thresholds: a pixel counts when max - min over channels exceeds
    # `threshold` (243/255 > 0.95 > 242/255), an image when MORE than 5 % of its pixels count (20 of 400 = 5 %)
    def sat_image(n_pixels, level, seed):
        rs = np.random.RandomState(seed)
        a = rs.randint(100, 140, (20, 20, 3)).astype(np.uint8)
        flat = a.reshape(-1, 3)
        flat[rs.permutation(400)[:n_pixels]] = (level, 0, level // 2)
        return a

    sat = [(sat_image(16, 255, 1), 0.95), (sat_image(20, 255, 2), 0.95), (sat_image(21, 255, 3), 0.95),
           (sat_image(200, 242, 4), 0.95), (sat_image(200, 243, 5), 0.95), (sat_image(0, 255, 6), 0.95),
           (sat_image(21, 128, 7), 0.5), (sat_image(21, 127, 8), 0.5), (sat_image(400, 255, 9), 0.95)]
    arrays = {f"image_{i}": a for i, (a, _) in enumerate(sat)}
    arrays["thresholds"] = np.array([t for _, t in sat], np.float64)
    arrays["verdicts"] = np.array([bool(P.is_saturated(Image.fromarray(a), threshold=t)) for a, t in sat])
    assert arrays["verdicts"].any() and not arrays["verdicts"].all()
    np.savez_compressed(os.path.join(GOLDEN, "resample_saturation.npz"), **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
