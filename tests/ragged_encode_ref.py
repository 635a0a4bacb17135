"""Plain restatement of the ragged encode (include/lic.h): where the rows, steps, slots and escape
lists of images of different sizes lie, the pick rule that turns tables in raster order into coding order, and the
coding of every block, which is tests/rans_groups_ref.py's (tests/rans_ref.py per sub-stream).  Loops written from
the wording of the rules, independent of codec.ragged_encode_plan, codec.wavefront and codec.rans_group_sizes."""
import numpy as np

import rans_groups_ref as GR

LANES = 64
ERR_RANGE = 1
HARMLESS = 1                     # start 0, freq 1
NO_ESCAPE = 0xFFFFFFFF


def wavefront_order(h, w, pad, R):
    """-> (raster pixel of every coding position, pixels per step): pixel (i, j) belongs to step
    j + (pad + 1) * (i mod R'), R' = min(R, h) or h without slices; steps ascending, rows ascending inside a step;
    step numbers that hold no pixel are left out"""
    Reff = h if R is None else min(R, h)
    steps = {}
    for i in range(h):
        for j in range(w):
            steps.setdefault(j + (pad + 1) * (i % Reff), []).append(i * w + j)
    order, counts = [], []
    for t in sorted(steps):
        order += steps[t]
        counts.append(len(steps[t]))
    return order, counts


def layout(shapes, M, pad, R, G):
    """-> dict of plain lists: images [nimg][4] (ROW0, P, STEP0, NSTEPS), blocks [nimg * G][4] (WORD_OFF, SLOT,
    ESC_OFF, ESC_CAP), row_image, order, step_len, and the totals total_rows, words_len (bytes), esc_len (entries).
    Slots and lists are the tight ones: with n_g the symbols of sub-stream g, 2 * max n_g bytes rounded up to 4 and
    max n_g entries, one behind the other."""
    images, blocks, row_image, order, step_len = [], [], [], [], []
    word_off = esc_off = 0
    for b, (h, w) in enumerate(shapes):
        o, counts = wavefront_order(h, w, pad, R)
        lens = [n * M for n in counts]
        fullest = max(len(pos) for pos, _ in GR.deal(lens, G))
        images.append([len(order), h * w, len(step_len), len(lens)])
        for g in range(G):
            blocks.append([word_off, (2 * fullest + 3) // 4 * 4, esc_off, fullest])
            word_off += blocks[-1][1]
            esc_off += fullest
        row_image += [b] * (h * w)
        order += o
        step_len += lens
    return {"images": images, "blocks": blocks, "row_image": row_image, "order": order, "step_len": step_len,
            "total_rows": len(order), "words_len": word_off, "esc_len": esc_off}


def chunks(costs, budget):
    """consecutive runs of whole items; a run takes the next item while the sum stays within the budget, and always
    takes at least one"""
    out, i = [], 0
    while i < len(costs):
        j, used = i + 1, costs[i]
        while j < len(costs) and used + costs[j] <= budget:
            used += costs[j]
            j += 1
        out.append((i, j))
        i = j
    return out


def pick(tables, center, y, total_rows, images, row_image, order, M, W):
    """lic_rans_encode_pick_ragged.  tables [total_rows * M][2W+2], center and y [total_rows * M] in RASTER order
    -> (sf, exc [total_rows * M] uint32 in coding order, error word per image)"""
    S = 2 * W + 1
    n = total_rows * M
    sf, exc = np.full(n, HARMLESS, np.uint32), np.full(n, NO_ESCAPE, np.uint32)
    err = [0] * len(images)
    for q in range(total_rows):
        b = int(row_image[q])
        if not 0 <= b < len(images):
            continue
        row0, P = int(images[b][0]), int(images[b][1])
        pix = int(order[q])
        fits = row0 >= 0 and P >= 1 and row0 + P <= total_rows and row0 <= q < row0 + P and 0 <= pix < P
        for c in range(M):
            if not fits:
                err[b] |= ERR_RANGE
                continue
            i = (row0 + pix) * M + c
            idx = (int(y[i]) - int(center[i]) + W + 2 ** 31) % 2 ** 32 - 2 ** 31          # 32-bit two's complement
            s = min(max(idx, 0), S - 1)
            if idx <= 0:
                exc[q * M + c] = -idx
            if idx >= S - 1:
                exc[q * M + c] = idx - (S - 1)
            row = [int(v) for v in tables[i]]
            start, end = row[s], row[s + 1]
            if row[0] == 0 and row[S] == 65536 and end > start and end - start < 65536 and start < 65536:
                sf[q * M + c] = (start << 16) | (end - start)
            else:
                err[b] |= ERR_RANGE
    return sf, exc, err


def coding_order(tables, center, y, image, order, M, W):
    """one image's tables and idx = y - center + W in CODING order, for the restatement of the format"""
    row0, P = int(image[0]), int(image[1])
    at = np.array([(row0 + int(order[row0 + q])) * M + c for q in range(P) for c in range(M)], np.int64)
    return np.asarray(tables)[at], np.asarray(y, np.int64)[at] - np.asarray(center, np.int64)[at] + W


def encode_image(tables, center, y, lay, b, M, W, G):
    """-> ([G stream bytes], [G escape-list bytes]) of image b: rans_groups_ref.encode on its coding order"""
    image = lay["images"][b]
    tabs, idx = coding_order(tables, center, y, image, lay["order"], M, W)
    return GR.encode(tabs, idx, lay["step_len"][image[2]:image[2] + image[3]], G)
