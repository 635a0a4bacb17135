"""Plain-loop restatement of the merged decode schedule of several latent planes, written from the
rule's text and not from codec.py: step t of the call is step t of every image that still has one, images in list
order; inside an image, pixel (i, j) belongs to the image's step number j + (pad + 1) * (i mod R), steps that hold
no pixel are left out, and a step lists its pixels by ascending row.  Shared by test_ragged_decode_host.py and the GPU
tests of the ragged kernels."""


def image_steps(h, w, pad, R):
    """[[(i, j), ...] per step] of one image; R None: one slice"""
    R = h if R is None else min(R, h)
    by_step = {}
    for i in range(h):
        for j in range(w):
            by_step.setdefault(j + (pad + 1) * (i % R), []).append((i, j))
    return [sorted(by_step[t]) for t in sorted(by_step)]


def merged(shapes, pad, Rs):
    """-> (T, seg, rows): seg[t][b] = (first row, rows) of image b in step t, rows = [(image, raster pixel index,
    pixel index inside the (h + 2 pad) x (w + 2 pad) frame)] of all steps, one after the other"""
    per = [image_steps(h, w, pad, R) for (h, w), R in zip(shapes, Rs)]
    T = 0
    for steps in per:
        T = max(T, len(steps))
    seg, rows = [], []
    for t in range(T):
        seg.append([])
        first = 0
        for b, steps in enumerate(per):
            n = 0
            if t < len(steps):
                w = shapes[b][1]
                for i, j in steps[t]:
                    rows.append((b, i * w + j, (i + pad) * (w + 2 * pad) + j + pad))
                    n += 1
            seg[t].append((first, n))
            first += n
    return T, seg, rows
