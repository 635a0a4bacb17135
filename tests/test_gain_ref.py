"""Gain units on the host: the plain statements of tests/gain_ref.py on hand-computed cases, the
interpolation rule, the LICRATE1 envelope and its refusals, the argument checks of the three C entries (no GPU: a
refused call launches nothing) and the constructor / argument refusals of model, codec and trainer.  CPU only."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gain_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the statements ---------------------------------------------------------------------------------------------------
def test_forward_statements_on_hand_computed_cases():
    # one image, 2 x 2 pixels, 2 channels; s = (0.5, 2)
    v = np.array([[[[5.0, 1.25], [3.0, -0.75]], [[-5.0, 0.5], [7.0, 1.75]]]], np.float32)
    s = np.array([[0.5, 2.0]], np.float32)
    vg, out, anc = G.forward(v, None, s, G.ROUND)
    assert np.array_equal(vg, [[[[2.5, 2.5], [1.5, -1.5]], [[-2.5, 1.0], [3.5, 3.5]]]])
    # ties go to even: 2.5 -> 2, 1.5 -> 2, -1.5 -> -2, -2.5 -> -2, 3.5 -> 4
    assert np.array_equal(out, [[[[2.0, 2.0], [2.0, -2.0]], [[-2.0, 1.0], [4.0, 4.0]]]])
    # anchors: (0,0) and (1,1)
    assert np.array_equal(anc, [[[[2.0, 2.0], [0.0, 0.0]], [[0.0, 0.0], [4.0, 4.0]]]])
    assert not np.signbit(anc[0, 0, 1]).any()                              # +0, not -0, away from the anchors
    u = np.full_like(v, 0.75)
    vg2, noisy, _ = G.forward(v, u, s, G.NOISE)
    assert np.array_equal(vg2, vg) and np.array_equal(noisy, vg + np.float32(0.25))
    only, none_out, none_anc = G.forward(v, None, s, G.SCALE)
    assert np.array_equal(only, vg) and none_out is None and none_anc is None


def test_forward_rounds_the_product_before_the_sum():
    """v * s is not representable: fl32(fl32(v * s) + h) differs from the once-rounded v * s + h an FMA would give"""
    # v * s = 1 + 2^-22 + 2^-46 -> 1 + 2^-22; + 2^-24 is a tie that goes to even (stays), the unrounded sum lies above it
    v, s, u = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 + 2.0 ** -23), np.float32(0.5 + 2.0 ** -24)
    vg, out, _ = G.forward(np.full((1, 1, 1, 1), v), np.full((1, 1, 1, 1), u), np.full((1, 1), s), G.NOISE)
    half = np.float32(u - np.float32(0.5))
    assert vg[0, 0, 0, 0] == np.float32(v * s) == np.float32(1.0 + 2.0 ** -22)
    fused = np.float32(np.float64(v) * np.float64(s) + np.float64(half))
    assert out[0, 0, 0, 0] == np.float32(np.float32(v * s) + half) and out[0, 0, 0, 0] != fused


def test_per_image_rows_and_one_row_agree():
    rng = np.random.default_rng(0)
    v = rng.standard_normal((3, 2, 3, 5)).astype(np.float32)
    s = rng.uniform(0.5, 2.0, (1, 5)).astype(np.float32)
    a = G.forward(v, None, s, G.ROUND)
    b = G.forward(v, None, np.repeat(s, 3, 0), G.ROUND)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_backward_statements_on_hand_computed_cases():
    v = np.array([[[[1.0, 2.0], [3.0, 4.0]]]], np.float32)                 # 1 x 1 x 2 pixels, 2 channels
    s = np.array([[2.0, 0.5]], np.float32)
    d_vg, d_out, d_anc = np.full_like(v, 1.0), np.full_like(v, 2.0), np.full_like(v, 4.0)
    dv, ds, mag = G.backward64(v, s, d_vg, d_out, d_anc)
    # t = 7 at the anchor (0,0), 3 at (0,1)
    assert np.array_equal(dv, [[[[14.0, 3.5], [6.0, 1.5]]]])
    assert np.array_equal(ds, [[7.0 * 1.0 + 3.0 * 3.0, 7.0 * 2.0 + 3.0 * 4.0]]) and np.array_equal(mag, ds)
    dv1, ds1, _ = G.backward64(v, s, d_vg=d_vg)
    assert np.array_equal(dv1, [[[[2.0, 0.5], [2.0, 0.5]]]]) and np.array_equal(ds1, [[4.0, 6.0]])
    dv32, t = G.dv32(s, d_vg, d_out, d_anc)
    assert dv32.dtype == np.float32 and np.array_equal(dv32, dv) and np.array_equal(t[0, 0, :, 0], [7.0, 3.0])
    with pytest.raises(AssertionError):
        G.backward64(v, s)


# ---- interpolation ----------------------------------------------------------------------------------------------------
def test_interpolation_rule():
    rng = np.random.default_rng(1)
    log_g = rng.standard_normal((4, 6))
    for i in range(4):
        assert np.allclose(G.interpolate(log_g, float(i)), np.exp(log_g[i]), rtol=1e-15, atol=0)
    for i in range(3):
        assert np.allclose(G.interpolate(log_g, i + 0.5), np.sqrt(np.exp(log_g[i]) * np.exp(log_g[i + 1])), rtol=1e-14)
    # floor(q) is clamped to Q - 2: q = Q - 1 is level Q - 1 itself (l = 1), and nothing above it is taken
    assert np.allclose(G.interpolate(log_g, 3.0), np.exp(log_g[3]), rtol=1e-15)
    with pytest.raises(AssertionError):
        G.interpolate(log_g, 3.01)
    assert (G.interpolate(log_g, 1.3) > 0).all()


def test_model_rows_follow_the_rule():
    import neural_image_compression_amd as nic
    m = nic.JointAutoregressiveHierarchical(8, 1, rate_levels=3)
    with torch.no_grad():
        m.log_gain_y.copy_(torch.randn(3, 8, generator=torch.Generator().manual_seed(2)))
    table = m.log_gain_y.detach().double().numpy()
    for q in (0.0, 0.5, 1.0, 1.25, 2.0):
        (got,) = m.gain_rows(m.check_quality(q), m.log_gain_y)
        got = got.detach().numpy()
        assert got.shape == (1, 8) and np.allclose(got[0], G.interpolate(table, q), rtol=1e-5)
    rows, other = m.gain_rows(m.check_quality(torch.tensor([0.0, 1.5, 2.0]), 3), m.log_gain_y, m.log_gain_z)
    assert rows.shape == (3, 8) and bool((rows > 0).all()) and bool((other == 1).all())
    one = m.gain_rows([1.5], m.log_gain_y)[0]
    assert torch.equal(m.gain_rows([1.5, 1.5], m.log_gain_y)[0], torch.cat([one, one]))   # one quality, a constant list
    rows.sum().backward()
    assert m.log_gain_y.grad is not None and bool((m.log_gain_y.grad != 0).any())


# ---- the envelope -----------------------------------------------------------------------------------------------------
INNER = b"LICBITS2" + bytes(range(40))


def test_envelope_round_trip():
    from neural_image_compression_amd import bitstream as bs
    blob = bs.pack_rate_envelope(INNER, 1.25, 4)
    assert blob[:8] == b"LICRATE1" and len(blob) == 20 + len(INNER) + 4
    assert G.read_envelope(blob) == (1.25, 4, 0, len(INNER), INNER, True)
    assert blob == G.make_envelope(INNER, 1.25, 4)
    assert bs.unpack_rate_envelope(blob) == (1.25, 4, INNER) and bs.unpack_rate_envelope(blob, 4)[2] == INNER
    assert bs.quality_of(blob) == 1.25 and bs.is_rate_envelope(blob) and not bs.is_rate_envelope(INNER)
    q = bs.quality_of(bs.pack_rate_envelope(INNER, 0.1, 2))               # the float32 of 0.1 is what travels
    assert q == float(np.float32(0.1))
    for bad_q, bad_Q in ((-0.5, 4), (3.5, 4), (float("nan"), 4), (1.0, 1), (1.0, 70000), ("x", 4)):
        with pytest.raises(bs.CodecError):
            bs.pack_rate_envelope(INNER, bad_q, bad_Q)


@pytest.mark.parametrize("blob, rate_levels, names", [
    (INNER + b"\0" * 24, None, "bad magic"),                                                        # a bare blob
    (G.make_envelope(INNER, 1.0, 4), 3, "4 rate levels; this model has 3"),                         # another model's Q
    (G.make_envelope(INNER, 3.5, 4), None, "outside"),                                              # q above Q - 1
    (G.make_envelope(INNER, -0.25, 4), None, "outside"),
    (G.make_envelope(INNER, float("nan"), 4), None, "outside"),
    (G.make_envelope(INNER, 1.0, 4, crc=0x12345678), None, "CRC-32"),
    (G.make_envelope(INNER, 1.0, 4, length=len(INNER) - 1), None, "length"),
    (G.make_envelope(INNER, 1.0, 4, length=len(INNER) + 1), None, "length"),
    (G.make_envelope(INNER, 1.0, 4) + b"\0", None, "length"),
    (G.make_envelope(INNER, 1.0, 4)[:-1], None, "length"),
    (G.make_envelope(INNER, 1.0, 4)[:16], None, "truncated"),
    (G.make_envelope(INNER, 1.0, 4, pad=1), None, "pad"),
    (G.make_envelope(INNER, 0.0, 1), None, "Q = 1"),
])
def test_envelope_refusals_one_field_at_a_time(blob, rate_levels, names):
    from neural_image_compression_amd import bitstream as bs
    with pytest.raises(bs.CodecError, match=names):
        bs.unpack_rate_envelope(blob, rate_levels)


def test_a_flipped_byte_anywhere_is_a_crc_refusal():
    from neural_image_compression_amd import bitstream as bs
    blob = bs.pack_rate_envelope(INNER, 1.0, 4)
    for at in (8, 12, 14, 20, len(blob) - 5, len(blob) - 1):
        bad = bytearray(blob)
        bad[at] ^= 0x10
        with pytest.raises(bs.CodecError, match="CRC-32"):
            bs.unpack_rate_envelope(bytes(bad))


def test_pinned_container_tables_are_unchanged():
    from neural_image_compression_amd import bitstream as bs
    assert bs.BITSTREAM_FAMILIES == {"JointAutoregressiveHierarchical": 1, "HierarchicalMixtureResidual": 2,
                                     "ScalableImageCoding": 3}
    assert {k: v[0] for k, v in bs._FORMATS.items()} == {("range", False): b"LICBITS1", ("rans", False): b"LICBITS2",
                                                         ("rans", True): b"LICBITS3", ("rans", "sliced"): b"LICBITS4"}
    assert bs._FORMAT_OF_MAGIC == {b"LICBITS1": ("range", False), b"LICBITS2": ("rans", False), b"LICBITS3": ("rans", True),
                                   b"LICBITS4": ("rans", "sliced")}
    assert b"LICRATE1" not in bs._FORMAT_OF_MAGIC and bs._format_of_magic(b"LICRATE1") == ("range", False)


# ---- the C entries: refusals launch nothing ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_gain_entries_refuse_bad_arguments_without_a_gpu(lib):
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    q = lambda v=p, u=None, s=p, stride=0, vg=p, out=p, anc=None, g16=None, o16=None, a16=None, B=1, h=2, w=2, C=4, \
        mode=lib.GAIN_ROUND: L.lic_gain_quantize(v, u, s, stride, vg, out, anc, g16, o16, a16, B, h, w, C, mode, None)
    assert q(v=None) == -1 and q(s=None) == -1 and q(vg=None) == -1 and q(out=None) == -1
    assert q(mode=lib.GAIN_NOISE) == -1                                    # NOISE needs u
    assert q(mode=lib.GAIN_SCALE) == -1 and q(mode=lib.GAIN_SCALE, out=None, u=p) == -1   # SCALE takes neither out nor u
    assert q(mode=lib.GAIN_SCALE, out=None, anc=p) == -1
    assert q(mode=3) == -1 and q(mode=-1) == -1
    assert q(B=0) == -1 and q(h=0) == -1 and q(w=-1) == -1 and q(C=0) == -1
    assert q(stride=3) == -1 and q(stride=1) == -1 and q(stride=-4) == -1   # 0 < s_stride < C, and a negative one
    assert q(h=1 << 15, w=1 << 15, C=2) == -2                               # h * w * C >= 2^31: unsupported
    b = lambda v=p, s=p, stride=0, g=p, o=None, a=None, dv=p, ds=p, B=1, h=2, w=2, C=4, ws=p, nbytes=256: \
        L.lic_gain_bwd(v, s, stride, g, o, a, dv, ds, B, h, w, C, ws, nbytes, None)
    assert b(v=None) == -1 and b(s=None) == -1 and b(dv=None) == -1 and b(ds=None) == -1 and b(ws=None) == -1
    assert b(g=None) == -1                                                  # no gradient at all
    assert b(B=0) == -1 and b(h=-1) == -1 and b(w=0) == -1 and b(C=0) == -1 and b(stride=2) == -1
    need = L.lic_gain_bwd_workspace_bytes(1, 4, 4)
    assert need == 16 and b(nbytes=need - 1) == -1 and b(nbytes=0) == -1    # a workspace that is too small


def test_bwd_workspace_follows_the_slab_constant(lib):
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "lic.h")).read()
    assert f"#define LIC_GAIN_SLAB_PIXELS {lib.GAIN_SLAB_PIXELS}\n" in header
    assert f"#define LIC_GAIN_SLAB_ROWS {lib.GAIN_SLAB_ROWS}\n" in header
    for name, val in (("LIC_GAIN_SCALE", lib.GAIN_SCALE), ("LIC_GAIN_NOISE", lib.GAIN_NOISE), ("LIC_GAIN_ROUND", lib.GAIN_ROUND)):
        assert f"#define {name} {val}\n" in header
    S = lib.GAIN_SLAB_PIXELS
    for B, hw, C in ((1, 1, 1), (2, S - 1, 5), (2, S, 5), (3, S + 1, 8), (32, 256, 192), (1, 2 * S + 5, 12)):
        assert L.lic_gain_bwd_workspace_bytes(B, hw, C) == G.bwd_workspace_bytes(B, hw, C, S) == 4 * B * (-(-hw // S)) * C
    assert L.lic_gain_bwd_workspace_bytes(0, 4, 4) == 0 and L.lic_gain_bwd_workspace_bytes(1, 0, 4) == 0
    assert L.lic_gain_bwd_workspace_bytes(1, 4, -1) == 0


# ---- model, codec, trainer: what they refuse, what stays ----------------------------------------------------------------
def _models():
    import neural_image_compression_amd as nic
    return nic.JointAutoregressiveHierarchical(8, 1), nic.JointAutoregressiveHierarchical(8, 1, rate_levels=3)


def test_rate_levels_none_keeps_the_state_dict():
    import neural_image_compression_amd as nic
    plain, rated = _models()
    tables = {"log_gain_y", "log_inv_gain_y", "log_gain_z", "log_inv_gain_z"}
    assert not tables & set(plain.state_dict()) and plain.rate_levels is None
    assert list(nic.JointAutoregressiveHierarchical(8, 1, rate_levels=None).state_dict()) == list(plain.state_dict())
    assert set(rated.state_dict()) == set(plain.state_dict()) | tables
    for k in tables:
        t = rated.state_dict()[k]
        assert t.shape == (3, 8) and t.dtype == torch.float32 and not t.any()
    assert nic.HierarchicalMixtureResidual(8, 2, "checkerboard", rate_levels=2).log_gain_z.shape == (2, 8)
    for bad in (1, 0, -2, 2.0, True, "3"):
        with pytest.raises(ValueError, match="rate_levels"):
            nic.JointAutoregressiveHierarchical(8, 1, rate_levels=bad)


def test_quality_refusals_of_the_model():
    plain, rated = _models()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="no rate levels"):
        plain(x, quality=1.0)
    with pytest.raises(ValueError, match="no rate levels"):
        plain.analysis_hyperprior(x, training=False, quality=0.0)
    with pytest.raises(ValueError, match="needs `quality`"):
        rated(x)
    with pytest.raises(ValueError, match="needs `quality`"):
        rated.analysis_hyperprior(x, training=False)
    for bad in (-0.01, 2.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="outside"):
            rated(x, quality=bad)
    with pytest.raises(ValueError, match="outside"):
        rated(torch.zeros(2, 3, 64, 64), quality=torch.tensor([0.0, 2.5]))
    with pytest.raises(ValueError, match=r"tensor \[B\]"):
        rated(torch.zeros(2, 3, 64, 64), quality=torch.tensor([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="no rate levels"):
        plain.synthesis(torch.zeros(1, 8, 4, 4), 1.0)
    with pytest.raises(ValueError, match="needs `quality`"):
        rated.hyper_synthesis(torch.zeros(1, 8, 1, 1))


def test_codec_refusals_on_the_host():
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import bitstream as bs
    from neural_image_compression_amd.codec import CodecError, ContextCodec, ScalableCodec
    plain, rated = _models()
    with pytest.raises(CodecError, match="rate-level"):
        ScalableCodec(rated)
    x = torch.zeros(1, 3, 64, 64)
    codec, pcodec = ContextCodec(rated), ContextCodec(plain)
    assert codec.rate_levels == 3 and pcodec.rate_levels is None
    with pytest.raises(CodecError, match="a quality in"):
        codec.compress_image(x)
    with pytest.raises(CodecError, match="outside"):
        codec.compress_image(x, quality=2.5)
    with pytest.raises(CodecError, match="no rate levels"):
        pcodec.compress_image(x, quality=1.0)
    with pytest.raises(CodecError, match="no rate levels"):
        pcodec.compress_image_to(x, 1000)
    # blobs: a rate-level codec reads envelopes only, a plain one none
    env = bs.pack_rate_envelope(INNER, 1.0, 3)
    with pytest.raises(CodecError, match="bad magic"):
        codec.decompress_image(INNER + b"\0" * 24)
    with pytest.raises(CodecError, match="4 rate levels; this model has 3"):
        codec.decompress_image(bs.pack_rate_envelope(INNER, 1.0, 4))
    with pytest.raises(CodecError, match="blob 0: .*CRC-32"):
        codec.decompress_images([env[:-1] + bytes([env[-1] ^ 1]), env])
    with pytest.raises(CodecError, match="no rate levels"):
        pcodec.decompress_image(env)
    with pytest.raises(CodecError, match="blob 0: .*no rate levels"):
        pcodec.decompress_images([env])


class _Loader(list):
    pass


def test_trainer_refusals_and_generator_state(tmp_path):
    import neural_image_compression_amd as nic
    from neural_image_compression_amd.trainer import Trainer
    plain, rated = _models()
    data = _Loader([torch.zeros(1, 3, 64, 64)])
    kw = dict(rd_loss=nic.rd_loss, device="cpu", writer=object(), checkpoint_path=str(tmp_path / "c.pth"), max_steps=4)
    opt = torch.optim.SGD(rated.parameters(), lr=0.0)
    with pytest.raises(ValueError, match="step_plan"):
        Trainer(rated, opt, data, rate_points=[(0.0, 0.01)], step_plan=True, **kw)
    with pytest.raises(ValueError, match="rate_levels"):
        Trainer(plain, torch.optim.SGD(plain.parameters(), lr=0.0), data, rate_points=[(0.0, 0.01)], **kw)
    with pytest.raises(ValueError, match="outside"):
        Trainer(rated, opt, data, rate_points=[(0.0, 0.01), (5.0, 0.1)], **kw)
    with pytest.raises(ValueError, match="at least one"):
        Trainer(rated, opt, data, rate_points=[], **kw)
    # the generator: seeded, saved with the checkpoint, restored on resume
    pts = [(0.0, 0.001), (1.0, 0.01), (2.0, 0.1)]
    a = Trainer(rated, opt, data, rate_points=pts, rate_seed=5, **kw)
    b = Trainer(rated, opt, data, rate_points=pts, rate_seed=5, **kw)
    first = [a._rate_rng.choice(a.rate_points) for _ in range(6)]
    assert first == [b._rate_rng.choice(b.rate_points) for _ in range(6)] and len(set(first)) > 1
    a.save_checkpoint()
    want = [a._rate_rng.choice(a.rate_points) for _ in range(8)]
    c = Trainer(rated, opt, data, rate_points=pts, rate_seed=99, resume=True, **kw)
    assert [c._rate_rng.choice(c.rate_points) for _ in range(8)] == want
    assert "rate_rng" not in Trainer(plain, torch.optim.SGD(plain.parameters(), lr=0.0), data, **kw)._checkpoint_state()
