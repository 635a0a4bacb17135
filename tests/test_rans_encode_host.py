"""The device encoder of the "rANS-64" y streams, as far as a CPU can pin it: the constructor rules of
ContextCodec(encoder=...), the two entries' argument checks, and a numpy restatement of the kernels' round-wise
formulation (ballot as a boolean vector, rank as an exclusive cumsum, words placed at wpos - cnt + rank towards
lower addresses, escapes compacted forward) against tests/rans_ref.py on the step list and the five image kinds
that tests/test_gpu_rans_encode.py runs on the device.  CPU only."""
import struct
import types

import numpy as np
import pytest

import rans_ref as RR
from oracle import codec_ref as CR

W_, S_ = 24, 49
LANES = 64
NO_ESCAPE = 0xFFFFFFFF
# a full single round, an empty step, a partial round after two full ones, one symbol, exact multiples, a long step
STEPS = [64, 0, 130, 1, 128, 327]
KINDS = ("gamma 0.3", "gamma 0.02", "gamma 2.0", "freq 1", "freq 65536-48")


def make_images(steps=STEPS, seed=31, W=W_):
    """The five images of the encoder tests in CODING order: tables [5][n][S+1] uint32 and idx [5][n] int64, for the
    window half-width W (S = 2W + 1 symbols).
    (a) gamma(0.3) tables, (b) gamma(0.02): peaked, few words, (c) gamma(2.0), (d) every coded symbol has frequency
    1: one word per symbol, the word cursor ends at its floor, (e) every coded symbol has frequency 65536 - (S - 1):
    no word at all.  Edge symbols are placed by hand in (a) and (c) where they fit into `steps`' n symbols.  At W = 1
    the only interior symbol is 1, so image (d) takes its frequency-1 symbol from the two edge symbols (they come
    with an escape)."""
    S = 2 * W + 1
    r = np.random.RandomState(seed)
    n = int(sum(steps))
    tabs, idx = [], []
    for shape in (0.3, 0.02, 2.0):
        f = r.gamma(shape, 1.0, size=(n, S)) + 1e-9
        F = np.concatenate([np.zeros((n, 1)), np.cumsum(f / f.sum(1, keepdims=True), 1)], 1)
        F[:, -1] = 1.0
        t = CR.quantize_cdf(F)
        u = r.randint(0, 65536, size=n)
        i = np.array([np.searchsorted(t[k], u[k], side="right") - 1 for k in range(n)], np.int64).clip(1, S - 2)
        tabs.append(t)
        idx.append(i)
    big = r.randint(1, S - 1, size=n)
    t = np.zeros((n, S + 1), np.uint32)
    for k in range(n):
        f = np.ones(S, np.int64)
        f[big[k]] = 65536 - (S - 1)
        t[k, 1:] = np.cumsum(f)
    other = np.where(big + 1 <= S - 2, big + 1, big - 1)                  # an interior symbol of frequency 1
    if S == 3:
        other = np.where(r.randint(0, 2, size=n) == 1, S - 1, 0)          # none is interior: symbol 0 or S - 1
    tabs += [t, t.copy()]
    idx += [other.astype(np.int64), big.astype(np.int64)]
    # lane 0 and lane 63 of a full round, the last lane of a partial round (193: step 2's third round; 649: the
    # last symbol), a one-symbol step (194), and the largest excess there is: 2^31, one below the sentinel's range
    for b, places in ((0, {0: 0, 63: -1, 130: -2 ** 31, 193: S - 1, 194: S + 100000, 400: -100000, 649: S}),
                      (2, {127: -7, 193: S - 1, 649: 0})):
        for k, v in places.items():
            if k < n:
                idx[b][k] = v
    return np.stack(tabs), np.stack(idx)


def escape_count(idx, S):
    """escapes of a symbol sequence by the format's rule: one for every idx <= 0 and every idx >= S - 1"""
    idx = np.asarray(idx, np.int64)
    return int(((idx <= 0) | (idx >= S - 1)).sum())


def pick(tables, idx):
    """lic_rans_encode_pick for symbols already in coding order: (start << 16 | freq, excess or the sentinel)"""
    S = tables.shape[-1] - 1
    s = np.clip(idx, 0, S - 1)
    k = np.arange(len(idx))
    start, end = tables[k, s].astype(np.int64), tables[k, s + 1].astype(np.int64)
    assert (tables[:, 0] == 0).all() and (tables[:, S] == 65536).all() and ((end - start > 0) & (end - start < 65536)).all()
    sf = ((start << 16) | (end - start)).astype(np.uint32)
    exc = np.full(len(idx), NO_ESCAPE, np.uint32)
    exc[idx <= 0] = (-idx[idx <= 0]).astype(np.uint32)
    exc[idx >= S - 1] = (idx[idx >= S - 1] - (S - 1)).astype(np.uint32)
    return sf, exc


def roundwise_encode(sf, exc, steps):
    """lic_rans_encode the way its wave executes it.  -> (stream bytes, escape-list bytes, words written at the
    slot's end, whether every symbol cost one word)"""
    n = len(sf)
    # escapes, forward, 64 symbols at a time whatever the steps are
    esc_out, cursor = np.zeros(n, np.uint32), 0
    for k0 in range(0, n, LANES):
        e = np.full(LANES, NO_ESCAPE, np.uint32)
        e[:min(LANES, n - k0)] = exc[k0:k0 + LANES]
        edge = e != NO_ESCAPE                                              # the ballot
        rank = np.cumsum(edge) - edge                                      # set bits below the lane
        esc_out[cursor + rank[edge]] = e[edge]
        cursor += int(edge.sum())
    # states, backward: steps last to first, rounds last to first
    slot = (4 * LANES + 2 * n + 3) // 4 * 4
    wbuf = np.zeros(slot // 2, np.uint16)
    wpos = slot // 2
    x = np.full(LANES, 1 << 16, np.uint64)
    bases = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
    for t in range(len(steps) - 1, -1, -1):
        n_t = int(steps[t])
        for rnd in range((n_t + LANES - 1) // LANES - 1, -1, -1):
            live = min(LANES, n_t - rnd * LANES)
            w = np.zeros(LANES, np.uint64)
            w[:live] = sf[bases[t] + rnd * LANES:bases[t] + rnd * LANES + live]
            freq, start = w & 0xFFFF, w >> 16
            active = freq != 0
            emit = active & ((x >> 16) >= freq)                            # the ballot
            cnt = int(emit.sum())
            rank = np.cumsum(emit) - emit
            assert cnt <= wpos
            wpos -= cnt
            wbuf[wpos + rank[emit]] = (x[emit] & 0xFFFF).astype(np.uint16)
            x[emit] >>= 16
            f = np.where(active, freq, 1)
            x = np.where(active, ((x // f) << 16) + x % f + start, x)
            assert (x < 1 << 32).all() and (x >= 1 << 16).all()
    words = wbuf[wpos:]
    stream = struct.pack("<%dI" % LANES, *[int(v) for v in x]) + words.astype("<u2").tobytes()
    return stream, esc_out[:cursor].astype("<u4").tobytes(), len(words), wpos == (slot // 2 - n)


@pytest.fixture(scope="module")
def images():
    return make_images()


@pytest.mark.parametrize("b", range(5), ids=KINDS)
def test_roundwise_formulation_matches_the_format(images, b):
    tabs, idx = images
    stream, esc, nwords, _ = roundwise_encode(*pick(tabs[b], idx[b]), STEPS)
    ref_stream, ref_esc = RR.encode(tabs[b], idx[b], STEPS)
    assert stream == ref_stream and esc == ref_esc
    assert nwords == (len(ref_stream) - 256) // 2
    assert (RR.decode(stream, esc, tabs[b], STEPS) == idx[b]).all()


def test_the_escape_sentinel_is_no_excess(images):
    tabs, idx = images
    _, exc = pick(tabs[0], idx[0])
    assert exc[130] == 2 ** 31 and exc[0] == 0 and exc[63] == 1 and exc[194] == 100001 and exc[649] == 1
    _, esc = RR.encode(tabs[0], idx[0], STEPS)
    assert struct.unpack("<%dI" % (len(esc) // 4), esc) == (0, 1, 2 ** 31, 0, 100001, 100000, 1)


def test_both_ends_of_the_word_cursor():
    """frequency 1 everywhere: one word per symbol, the stream is the whole slot; frequency 65536 - 48: no word"""
    steps = [64, 0, 130, 1, 128]
    tabs, idx = make_images(steps)
    n = sum(steps)
    stream, esc, nwords, one_each = roundwise_encode(*pick(tabs[3], idx[3]), steps)
    assert (stream, esc) == RR.encode(tabs[3], idx[3], steps)
    assert len(stream) == 256 + 2 * n and nwords == n and one_each and esc == b""
    stream, esc, nwords, _ = roundwise_encode(*pick(tabs[4], idx[4]), steps)
    assert (stream, esc) == RR.encode(tabs[4], idx[4], steps)
    assert len(stream) == 256 and nwords == 0
    for b in (3, 4):
        s, e = RR.encode(tabs[b], idx[b], steps)
        assert (RR.decode(s, e, tabs[b], steps) == idx[b]).all()


def test_prefix_with_channels(images):
    """the M = 32 rerun of the device test: steps of 1 and 3 pixels"""
    tabs, idx = images
    for b in range(5):
        stream, esc, _, _ = roundwise_encode(*pick(tabs[b][:128], idx[b][:128]), [32, 96])
        assert (stream, esc) == RR.encode(tabs[b][:128], idx[b][:128], [32, 96])


# ---- ContextCodec(encoder=...) ---------------------------------------------------------------------
def _stub_model():
    """what ContextCodec's constructor reads: a causal 5x5 mask (type A: the 12 taps before the centre)"""
    masked = types.SimpleNamespace(kernel_size=(5, 5), padding=(2, 2), _tap_mask=(1 << 12) - 1)
    return types.SimpleNamespace(context_model=types.SimpleNamespace(masked=masked))


def test_encoder_argument_rules():
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import codec
    m = _stub_model()
    assert codec.ContextCodec(m).encoder == "host"
    for coder in ("range", "rans"):
        assert codec.ContextCodec(m, coder=coder, encoder="host").encoder == "host"
    assert codec.ContextCodec(m, coder="rans", encoder="device").encoder == "device"
    with pytest.raises(codec.CodecError, match="gpu"):
        codec.ContextCodec(m, coder="rans", encoder="gpu")
    with pytest.raises(codec.CodecError, match="device"):
        codec.ContextCodec(m, coder="range", encoder="device")
    with pytest.raises(codec.CodecError):
        codec.ContextCodec(m, encoder="device")                            # the default coder is "range"


def test_encode_entries_check_their_arguments_without_a_gpu():
    import os
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    INVALID, UNSUPPORTED = -1, -2
    p = 4096                                                               # an aligned non-null address, never used
    assert L.lic_rans_encode_pick(None, None, None, None, 1, 8, 32, 24, None, None, None, None) == INVALID
    assert L.lic_rans_encode_pick(p, p, p, p, 0, 8, 32, 24, p, p, p, None) == INVALID
    assert L.lic_rans_encode_pick(p, p, p, p, 1, 8, 32, 0, p, p, p, None) == INVALID
    assert L.lic_rans_encode_pick(p, p, p, p + 4, 1, 8, 32, 24, p, p, p, None) == INVALID     # order: 8-byte aligned
    assert L.lic_rans_encode_pick(p, p, p, p, 1, 8, 32, 65, p, p, p, None) == UNSUPPORTED
    assert L.lic_rans_encode_pick(p, p, p, p, 1, 1 << 30, 32, 24, p, p, p, None) == UNSUPPORTED
    assert L.lic_rans_encode(None, None, None, 1, 1, 64, None, 384, None, None, None) == INVALID
    assert L.lic_rans_encode(p, p, p, 1, 1, 0, p, 384, p, p, None) == INVALID
    assert L.lic_rans_encode(p, p, p, 1, 1, 64, p, 126, p, p, None) == INVALID                # slot below 2 * nsym
    assert L.lic_rans_encode(p, p, p, 1, 1, 64, p, 386, p, p, None) == INVALID                # slot: whole dwords
    assert L.lic_rans_encode(p, p, p + 2, 1, 1, 64, p, 384, p, p, None) == INVALID
    assert L.lic_rans_encode(p, p, p, 1, 1, 1 << 31, p, 1 << 33, p, p, None) == UNSUPPORTED
