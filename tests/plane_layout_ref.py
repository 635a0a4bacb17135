"""Plain-loop restatement of the flat-buffer layout of the ragged codec kernels, written from
the rule's text and not from codec.py.  Two flat fp32 buffers hold every image of a call, one the latent planes and one
the psi planes.  Items come one after the other; an item of B images starts, in either buffer, at the next multiple of 4
floats, and its B planes follow each other without a gap.  A latent plane is (h + 2 f) x (w + 2 f) pixels of y_pix
floats: the h x w image inside a zero frame of f pixels.  A psi plane is h x w pixels of cpsi floats, no frame.  Every
image has a descriptor of 8 words: the float its latent plane starts at, the floats of one framed row, the float of
pixel (0, 0) counted from the plane's start, the float its psi plane starts at, h, w, the rows of a slice (never more
than h; h without slices), and a word that stays 0."""


def round_up_4(n):
    while n % 4:
        n += 1
    return n


def layout(items, y_pix, cpsi, f, slice_rows):
    """items [(B, h, w)], slice_rows per image -> (y_at, psi_at, y_len, psi_len, desc, pixels) as lists"""
    y_at, psi_at, desc, pixels = [], [], [], []
    y_end = psi_end = 0
    image = 0
    for B, h, w in items:
        y_start, psi_start = round_up_4(y_end), round_up_4(psi_end)
        y_at.append(y_start)
        psi_at.append(psi_start)
        framed_w, framed_h = w + f + f, h + f + f
        for b in range(B):
            R = slice_rows[image]
            rows = h if R is None or R > h else R
            first = y_start + b * framed_h * framed_w * y_pix
            origin = f * framed_w * y_pix + f * y_pix              # f framed rows down, f pixels in
            desc.append([first, framed_w * y_pix, origin, psi_start + b * h * w * cpsi, h, w, rows, 0])
            pixels.append(framed_h * framed_w)
            image += 1
        y_end = y_start + B * framed_h * framed_w * y_pix
        psi_end = psi_start + B * h * w * cpsi
    return y_at, psi_at, y_end, psi_end, desc, pixels
