"""lic_rans_encode_pick_ragged + lic_rans_encode_ragged on an MI355X, through the C ABI with hand-made tables: five
images of 1, 5, 70, 130 and 700 pixels (M = 3) in one launch each, every block's states, words and escape list byte
for byte against lic_rans_encode_pick + lic_rans_encode_groups run image by image and against the Python restatement
(tests/ragged_encode_ref.py), with the tight slots and lists of lic.h framed by canaries; then one descriptor or
data failure at a time: the image concerned reports, no other byte moves."""
import numpy as np
import pytest
import torch

import ragged_encode_ref as RE
import test_rans_encode_host as EH

pytestmark = pytest.mark.gpu

M, W_ = 3, 24
S1 = 2 * W_ + 2
PIXELS = [1, 5, 70, 130, 700]
# the image kinds of test_rans_encode_host.make_images: gamma(0.3) with hand-placed escapes up to 2^31, frequency 1
# everywhere (one word per symbol), frequency 65536 - 48 everywhere (no word), gamma(2.0) with escapes, gamma(0.3)
KIND = [0, 3, 4, 2, 0]
# in symbols.  One round only (fewer rounds than G); empty steps; partial rounds; 130 and 195: a partial third and
# fourth round, which is a non-zero group's for G = 3 and 4; 2100 symbols: more than kRing * 64 * G, the ring wraps
STEPS = [[3], [0, 6, 9], [64, 0, 130, 1, 15], [0, 130, 65, 195], [3, 700, 0, 1300, 97]]
NIMG = len(PIXELS)
CANARY = 0xA5
GAP = 8                                        # canary bytes between slots; GAP // 4 canary entries between lists
ERR_RANGE = 1


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import _lib, codec
    from neural_image_compression_amd import functional as F_
    return codec, _lib, F_, torch.device("cuda:0")


@pytest.fixture(scope="module")
def world():
    """the five images in raster order, one unused row in front of, between and behind them"""
    assert [sum(s) for s in STEPS] == [P * M for P in PIXELS]
    r = np.random.RandomState(61)
    rows = sum(PIXELS) + NIMG + 1
    tables, center, y = np.zeros((rows * M, S1), np.uint32), np.zeros(rows * M, np.int32), np.zeros(rows * M, np.int32)
    row_image, order = np.full(rows, -1, np.int64), np.zeros(rows, np.int64)
    images, code, row0, step0 = [], [], 1, 0
    for b, P in enumerate(PIXELS):
        tabs, idx = EH.make_images(steps=[P * M], seed=70 + b, W=W_)
        tabs, idx = tabs[KIND[b]], idx[KIND[b]]
        cen = r.randint(-10, 11, size=P * M).astype(np.int64)
        cen[idx == -2 ** 31] = W_                                             # y = idx + center - W must be an int32
        perm = r.permutation(P).astype(np.int64)
        at = ((row0 + perm)[:, None] * M + np.arange(M)[None, :]).ravel()     # symbol k = q * M + c -> raster element
        tables[at], center[at], y[at] = tabs, cen, idx + cen - W_
        row_image[row0:row0 + P], order[row0:row0 + P] = b, perm
        images.append([row0, P, step0, len(STEPS[b])])
        code.append((tabs, idx))
        row0, step0 = row0 + P + 1, step0 + len(STEPS[b])
    assert row0 == rows
    esc = [EH.escape_count(code[b][1], S1 - 1) for b in range(NIMG)]
    assert esc[0] >= 1 and esc[3] >= 2 and esc[4] >= 7 and (code[4][1] == -2 ** 31).any()
    return {"rows": rows, "tables": tables, "center": center, "y": y, "row_image": row_image, "order": order,
            "images": np.array(images, np.int64), "steps": np.concatenate(STEPS).astype(np.int64), "code": code}


def _blocks(G):
    """the tight slots and lists, a canary gap in front of, between and behind them -> (blocks, words_len, esc_len)"""
    blocks, word_off, esc_off = [], GAP, GAP // 4
    for b in range(NIMG):
        fullest = max(len(pos) for pos, _ in RE.GR.deal(STEPS[b], G))
        for g in range(G):
            blocks.append([word_off, (2 * fullest + 3) // 4 * 4, esc_off, fullest])
            word_off, esc_off = word_off + blocks[-1][1] + GAP, esc_off + fullest + GAP // 4
    return np.array(blocks, np.int64), word_off, esc_off


def _launch(env, world, G, **change):
    """both launches.  `change`: tables / order / row_image / images / steps / blocks replaced for this run
    -> dict of host arrays: state [NIMG * G][67], picked [NIMG][67], words (bytes), esc (uint32), sf, exc, frame"""
    _, _lib, F_, dev = env
    lib = _lib.load()
    blocks, words_len, esc_len = _blocks(G)
    v = dict(world, blocks=blocks)
    v.update(change)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_t, d_c, d_y = up(v["tables"].view(np.int32)), up(v["center"]), up(v["y"])
    d_img, d_blk, d_ri, d_ord, d_steps = up(v["images"]), up(v["blocks"]), up(v["row_image"]), up(v["order"]), up(v["steps"])
    rows, nsym = v["rows"], v["rows"] * M
    sf = torch.full((nsym,), 0x5A5A5A5A, device=dev, dtype=torch.int32)
    exc = torch.full((nsym,), 0x5A5A5A5A, device=dev, dtype=torch.int32)
    words = torch.full((words_len,), CANARY, device=dev, dtype=torch.uint8)
    esc = torch.full((4 * esc_len,), CANARY, device=dev, dtype=torch.uint8)
    frame = torch.full((NIMG * G + NIMG + 2, 67), 0x5A5A5A5A, device=dev, dtype=torch.int32)
    frame[1:-1, 66] = 0                                                       # the caller zeroes the error words
    state, picked = frame[1:1 + NIMG * G], frame[1 + NIMG * G:-1]
    rc = lib.lic_rans_encode_pick_ragged(F_._ptr(d_t), F_._ptr(d_c), F_._ptr(d_y), rows, F_._ptr(d_img), NIMG,
                                         F_._ptr(d_ri), F_._ptr(d_ord), M, W_, F_._ptr(sf), F_._ptr(exc), F_._ptr(picked),
                                         F_._stream())
    assert rc == 0
    picked_sf, picked_exc = sf.cpu().numpy().view(np.uint32), exc.cpu().numpy().view(np.uint32)
    # the rows of no image: pick leaves the harmless word there; a canary instead, which a wave that strays codes
    gaps = torch.from_numpy(np.flatnonzero(np.repeat(world["row_image"] < 0, M))).to(dev)
    sf[gaps] = 0x5A5A5A5A
    exc[gaps] = 0x5A5A5A5A
    rc = lib.lic_rans_encode_ragged(F_._ptr(sf), F_._ptr(exc), F_._ptr(d_steps), v["steps"].size, F_._ptr(d_img),
                                    F_._ptr(d_blk), NIMG, G, rows, M, F_._ptr(words), words_len, F_._ptr(esc), esc_len,
                                    F_._ptr(state), F_._stream())
    assert rc == 0
    torch.cuda.synchronize()
    fr = frame.cpu().numpy().view(np.uint32)
    return {"state": fr[1:1 + NIMG * G], "picked": fr[1 + NIMG * G:-1], "words": words.cpu().numpy(),
            "esc": esc.cpu().numpy().view(np.uint32), "sf": picked_sf, "exc": picked_exc, "frame": fr, "blocks": blocks}


def _block_bytes(out, i):
    """block i as the host assembles it: (stream, escape list)"""
    word_off, slot, esc_off, cap = (int(a) for a in out["blocks"][i])
    nw, ne = int(out["state"][i, 64]), int(out["state"][i, 65])
    assert 2 * nw <= slot and ne <= cap
    return (out["state"][i, :64].astype("<u4").tobytes() + out["words"][word_off + slot - 2 * nw:word_off + slot].tobytes(),
            out["esc"][esc_off:esc_off + ne].astype("<u4").tobytes())


def _canaries_intact(out, written=range(10 ** 6)):
    """nothing but the used words and escapes of the blocks in `written` has changed, and the state frame holds"""
    keep_w, keep_e = np.ones(out["words"].size, bool), np.ones(out["esc"].size, bool)
    for i, (word_off, slot, esc_off, cap) in enumerate(out["blocks"]):
        if i in written:
            keep_w[word_off + slot - 2 * int(out["state"][i, 64]):word_off + slot] = False
            keep_e[esc_off:esc_off + int(out["state"][i, 65])] = False
    assert keep_w.sum() >= GAP * (len(out["blocks"]) + 1) and keep_e.sum() >= GAP // 4 * (len(out["blocks"]) + 1)
    assert (out["words"][keep_w] == CANARY).all(), "bytes outside [slot end - 2 * count, slot end) were written"
    assert (out["esc"][keep_e] == 0xA5A5A5A5).all(), "escape entries beyond the count were written"
    assert (out["frame"][0] == 0x5A5A5A5A).all() and (out["frame"][-1] == 0x5A5A5A5A).all()


@pytest.fixture(scope="module")
def clean(env, world):
    """the undisturbed run for every G, computed once"""
    return {G: _launch(env, world, G) for G in (1, 3, 4)}


def _per_image(env, world, G, b):
    """image b alone through lic_rans_encode_pick + lic_rans_encode_groups -> (state [G][67], [(stream, escapes)])"""
    _, _lib, F_, dev = env
    lib = _lib.load()
    row0, P, step0, nsteps = (int(a) for a in world["images"][b])
    sl = slice(row0 * M, (row0 + P) * M)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_t, d_c, d_y = up(world["tables"][sl].view(np.int32)), up(world["center"][sl]), up(world["y"][sl])
    d_ord, d_steps = up(world["order"][row0:row0 + P]), up(world["steps"][step0:step0 + nsteps])
    nsym = P * M
    fullest = max(len(pos) for pos, _ in RE.GR.deal(STEPS[b], G))
    slot, cap = (2 * fullest + 3) // 4 * 4, fullest
    sf = torch.empty((nsym,), device=dev, dtype=torch.int32)
    exc = torch.empty_like(sf)
    words = torch.zeros((G, slot), device=dev, dtype=torch.uint8)
    esc = torch.zeros((G, cap), device=dev, dtype=torch.int32)
    state = torch.zeros((G, 67), device=dev, dtype=torch.int32)
    picked = torch.zeros((1, 67), device=dev, dtype=torch.int32)
    assert lib.lic_rans_encode_pick(F_._ptr(d_t), F_._ptr(d_c), F_._ptr(d_y), F_._ptr(d_ord), 1, P, M, W_, F_._ptr(sf),
                                    F_._ptr(exc), F_._ptr(picked), F_._stream()) == 0
    assert lib.lic_rans_encode_groups(F_._ptr(sf), F_._ptr(exc), F_._ptr(d_steps), nsteps, 1, G, nsym, F_._ptr(words),
                                      slot, F_._ptr(esc), cap, F_._ptr(state), F_._stream()) == 0
    torch.cuda.synchronize()
    assert picked.cpu().numpy()[0, 66] == 0
    st, h_words, h_esc = state.cpu().numpy().view(np.uint32), words.cpu().numpy(), esc.cpu().numpy().view(np.uint32)
    pairs = [(st[g, :64].astype("<u4").tobytes() + h_words[g, slot - 2 * int(st[g, 64]):].tobytes(),
              h_esc[g, :int(st[g, 65])].astype("<u4").tobytes()) for g in range(G)]
    return st, pairs, sf.cpu().numpy().view(np.uint32), exc.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("G", [1, 3, 4])
def test_five_images_in_one_launch_are_the_per_image_kernels_and_the_restatement(env, world, clean, G):
    out = clean[G]
    assert (out["state"][:, 66] == 0).all() and (out["picked"][:, 66] == 0).all()
    lay = {"images": world["images"].tolist(), "order": world["order"].tolist(), "step_len": world["steps"].tolist()}
    for b in range(NIMG):
        row0, P = int(world["images"][b, 0]), PIXELS[b]
        st, pairs, sf, exc = _per_image(env, world, G, b)
        assert np.array_equal(out["sf"][row0 * M:(row0 + P) * M], sf), f"image {b}: pick words differ"
        assert np.array_equal(out["exc"][row0 * M:(row0 + P) * M], exc), f"image {b}: pick escapes differ"
        assert np.array_equal(out["state"][b * G:(b + 1) * G], st), f"image {b}: state blocks differ"
        streams, escs = RE.encode_image(world["tables"], world["center"], world["y"], lay, b, M, W_, G)
        assert (streams, escs) == world_host(env, world, b, G)
        for g in range(G):
            got = _block_bytes(out, b * G + g)
            assert got == pairs[g], f"image {b} group {g}: differs from lic_rans_encode_groups"
            assert got == (streams[g], escs[g]), f"image {b} group {g}: differs from the restatement"
    # the rows of no image: the harmless word, no escape, no report
    gaps = np.repeat(world["row_image"] < 0, M)
    assert (out["sf"][gaps] == RE.HARMLESS).all() and (out["exc"][gaps] == RE.NO_ESCAPE).all()
    # both ends of the word cursor, the escapes placed by hand, and the image with fewer rounds than G
    sizes = lambda b: [len(pos) for pos, _ in RE.GR.deal(STEPS[b], G)]
    assert [int(v) for v in out["state"][G:2 * G, 64]] == sizes(1) and (out["state"][2 * G:3 * G, 64] == 0).all()
    assert sum(int(v) for v in out["state"][4 * G:, 65]) == EH.escape_count(world["code"][4][1], S1 - 1) >= 7
    assert (out["state"][1:G, :66] == np.array([1 << 16] * 64 + [0, 0], np.uint32)).all()
    assert 2 ** 31 in out["esc"][np.concatenate([np.arange(o, o + int(n)) for (_, _, o, _), n in
                                                 zip(out["blocks"][4 * G:], out["state"][4 * G:, 65])])]
    _canaries_intact(out)


def world_host(env, world, b, G):
    """image b by the host encoder of the format"""
    tabs, idx = world["code"][b]
    return env[0].rans_encode_grouped(tabs, idx.astype(np.int32), STEPS[b], G)


def _only_image_reports(out, base, G, victim, pick=False, encode=True):
    """image `victim` refused (initial states, zero counts, the range bit), every other block byte for byte the clean
    run's, every canary intact"""
    mine = range(victim * G, (victim + 1) * G)
    for i in range(NIMG * G):
        if i in mine:
            if encode:
                assert out["state"][i, 66] & ERR_RANGE
                assert (out["state"][i, :64] == 1 << 16).all() and out["state"][i, 64] == 0 and out["state"][i, 65] == 0
        else:
            assert np.array_equal(out["state"][i], base["state"][i]), i
            assert _block_bytes(out, i) == _block_bytes(base, i), i
    errs = out["picked"][:, 66]
    assert (np.delete(errs, victim) == 0).all() and bool(errs[victim] & ERR_RANGE) == pick
    _canaries_intact(out, written=[i for i in range(NIMG * G) if not (encode and i in mine)])


G_FAIL = 3
VICTIM = 2


def _descriptor_cases(world):
    blocks, words_len, esc_len = _blocks(G_FAIL)
    mine = slice(VICTIM * G_FAIL, (VICTIM + 1) * G_FAIL)

    def images(b, word, value):
        a = world["images"].copy()
        a[b, word] = value
        return {"images": a}

    def blk(word, value):
        a = blocks.copy()
        a[mine, word] = value(a[mine, word]) if callable(value) else value
        return {"blocks": a}

    last = NIMG - 1
    return {
        "rows beyond total_rows": (last, True, images(last, 1, world["rows"] - world["images"][last, 0] + 1)),
        "steps beyond steps_len": (VICTIM, False, images(VICTIM, 3, world["steps"].size - world["images"][VICTIM, 2] + 1)),
        "slot beyond words_len": (VICTIM, False, blk(0, lambda a: words_len - blocks[mine, 1] + 4)),
        "misaligned WORD_OFF": (VICTIM, False, blk(0, lambda a: a + 2)),
        "negative ESC_OFF": (VICTIM, False, blk(2, -1)),
        "negative STEP0": (VICTIM, False, images(VICTIM, 2, -1)),
        "negative ROW0": (VICTIM, True, images(VICTIM, 0, -1)),
        "ESC_CAP 0": (VICTIM, False, blk(3, 0)),
        "list beyond esc_len": (VICTIM, False, blk(2, lambda a: esc_len - blocks[mine, 3] + 1)),
    }


@pytest.mark.parametrize("case", ["rows beyond total_rows", "steps beyond steps_len", "slot beyond words_len",
                                  "misaligned WORD_OFF", "negative ESC_OFF", "negative STEP0", "negative ROW0",
                                  "ESC_CAP 0", "list beyond esc_len"])
def test_a_descriptor_that_does_not_fit_is_refused_by_its_image_alone(env, world, clean, case):
    victim, pick, change = _descriptor_cases(world)[case]
    out = _launch(env, world, G_FAIL, **change)
    _only_image_reports(out, clean[G_FAIL], G_FAIL, victim, pick=pick)


def test_step_lengths_that_do_not_add_up_for_one_image(env, world, clean):
    steps = world["steps"].copy()
    steps[world["images"][VICTIM, 2] + 2] -= 1
    _only_image_reports(_launch(env, world, G_FAIL, steps=steps), clean[G_FAIL], G_FAIL, VICTIM)
    steps = world["steps"].copy()
    steps[world["images"][VICTIM, 2]:world["images"][VICTIM, 2] + 2] = (PIXELS[VICTIM] * M + 64, -64)
    _only_image_reports(_launch(env, world, G_FAIL, steps=steps), clean[G_FAIL], G_FAIL, VICTIM)


def test_data_failures_of_pick_name_their_image_alone(env, world, clean):
    """a malformed table row, an order entry outside [0, P): the symbol is coded as the harmless word, the image's
    pick block reports, the other images do not move.  A row_image entry outside [0, nimg): the same word and no
    report anywhere -- there is no image to name"""
    base, row0 = clean[G_FAIL], int(world["images"][VICTIM, 0])
    tables = world["tables"].copy()
    tables[(row0 + 3) * M + 1, S1 - 1] = 65535                                 # cum[S] != 65536
    out = _launch(env, world, G_FAIL, tables=tables)
    _only_image_reports(out, base, G_FAIL, VICTIM, pick=True, encode=False)
    q = int(np.flatnonzero(world["order"][row0:row0 + PIXELS[VICTIM]] == 3)[0])
    assert out["sf"][(row0 + q) * M + 1] == RE.HARMLESS and (out["state"][:, 66] == 0).all()
    for bad in (PIXELS[VICTIM], -1, 2 ** 40):
        order = world["order"].copy()
        order[row0 + 7] = bad
        out = _launch(env, world, G_FAIL, order=order)
        _only_image_reports(out, base, G_FAIL, VICTIM, pick=True, encode=False)
        k = (row0 + 7) * M
        assert (out["sf"][k:k + M] == RE.HARMLESS).all() and (out["exc"][k:k + M] == RE.NO_ESCAPE).all()
    for bad in (NIMG, -1, 2 ** 40):
        row_image = world["row_image"].copy()
        row_image[row0 + 7] = bad
        out = _launch(env, world, G_FAIL, row_image=row_image)
        assert (out["picked"][:, 66] == 0).all() and (out["state"][:, 66] == 0).all()
        for i in range(NIMG * G_FAIL):
            if i // G_FAIL != VICTIM:
                assert _block_bytes(out, i) == _block_bytes(base, i)
        k = (row0 + 7) * M
        assert (out["sf"][k:k + M] == RE.HARMLESS).all() and (out["exc"][k:k + M] == RE.NO_ESCAPE).all()
        _canaries_intact(out)
    # a row that claims another image's position: outside that image's [ROW0, ROW0 + P), so that image reports
    row_image = world["row_image"].copy()
    row_image[row0 + 7] = VICTIM + 1
    out = _launch(env, world, G_FAIL, row_image=row_image)
    assert [int(e) for e in out["picked"][:, 66]] == [ERR_RANGE if b == VICTIM + 1 else 0 for b in range(NIMG)]
    _canaries_intact(out)


def test_entries_refuse_what_they_can_see(env, world):
    _, _lib, F_, dev = env
    lib = _lib.load()
    buf = torch.zeros(4096, device=dev, dtype=torch.uint8)
    p = buf.data_ptr()
    assert p % 16 == 0
    INVALID = -1
    pick = dict(tables=p, center=p, y=p, rows=8, images=p, nimg=2, row_image=p, order=p, M=3, W=24, sf=p, exc=p,
                state=p, stream=None)
    enc = dict(sf=p, exc=p, steps=p, steps_len=4, images=p, blocks=p, nimg=2, G=2, rows=8, M=3, words=p, words_len=64,
               esc=p, esc_len=16, state=p, stream=None)
    for name in ("tables", "order", "state"):
        assert lib.lic_rans_encode_pick_ragged(*{**pick, name: None}.values()) == INVALID
    assert lib.lic_rans_encode_pick_ragged(*{**pick, "sf": p + 2}.values()) == INVALID
    assert lib.lic_rans_encode_pick_ragged(*{**pick, "images": p + 4}.values()) == INVALID
    for name in ("sf", "blocks", "words"):
        assert lib.lic_rans_encode_ragged(*{**enc, name: None}.values()) == INVALID
    assert lib.lic_rans_encode_ragged(*{**enc, "words": p + 2}.values()) == INVALID
    assert lib.lic_rans_encode_ragged(*{**enc, "steps": p + 4}.values()) == INVALID
    assert lib.lic_rans_encode_ragged(*{**enc, "G": 0}.values()) == INVALID
    assert lib.lic_rans_encode_ragged(*{**enc, "G": 9}.values()) == INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0).all()
