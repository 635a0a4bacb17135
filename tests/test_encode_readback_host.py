"""The host half of an encode's read-back, `codec.rans_streams_of`, and the block layout it reads, `rans_block_layout`:
buffers laid out as the encoder kernels leave them give back exactly the host encoder's streams and escape lists; every
refusal names its image; the layout is the one `ragged_encode_plan` and `z_encode_plan` return.  CPU only."""
import numpy as np
import pytest

import test_ragged_encode_host as RH
import test_rans_encode_host as EH

SIZES = [130, 700, 64]                                 # symbols of the three images; the last one gets no escape
NAME = lambda img: f"picture {img}"


@pytest.fixture(scope="module")
def codec():
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import codec
    return codec


def _encoded(codec, G):
    """three images through the grouped host encoder and the buffers a device encoder would leave of them
    -> (step lengths, h_state, h_words, h_esc, blocks, streams, escape lists)"""
    from neural_image_compression_amd import _lib
    steps = [[n // 3, n - n // 3] for n in SIZES]
    all_tabs, all_idx = EH.make_images(steps=[max(SIZES)], seed=17)
    # images (a) and (c) of the encoder tests carry edge symbols, (b) has interior symbols only
    tabs = [all_tabs[k][:n] for k, n in zip((0, 2, 1), SIZES)]
    idx = [np.where(all_idx[k][:n] == -2 ** 31, -5, all_idx[k][:n]).astype(np.int32) for k, n in zip((0, 2, 1), SIZES)]
    pairs = [codec.rans_encode_grouped(t, i, s, G) for t, i, s in zip(tabs, idx, steps)]
    streams, escs = [s for p in pairs for s in p[0]], [e for p in pairs for e in p[1]]
    assert any(escs[:2 * G]) and not any(escs[2 * G:])
    blocks, words_len, esc_len = codec.rans_block_layout([codec.rans_group_sizes(s, G).max() for s in steps], G)
    h_state = np.zeros((3 * G, _lib.RANS_STATE_WORDS), np.uint32)
    h_words, h_esc = np.full(words_len, 0xA5, np.uint8), np.full(esc_len, 0xDEADBEEF, np.uint32)
    for i, (s, e) in enumerate(zip(streams, escs)):
        off, slot, e_off, cap = blocks[i]
        nw, ne = (len(s) - 256) // 2, len(e) // 4
        assert 2 * nw <= slot and ne <= cap
        h_state[i, :64], h_state[i, 64], h_state[i, 65] = np.frombuffer(s[:256], "<u4"), nw, ne
        h_words[off + slot - 2 * nw:off + slot] = np.frombuffer(s[256:], np.uint8)
        h_esc[e_off:e_off + ne] = np.frombuffer(e, "<u4")
    return steps, h_state, h_words, h_esc, blocks, streams, escs


@pytest.mark.parametrize("G", [1, 3])
def test_the_cut_gives_back_the_host_encoders_bytes(codec, G):
    _, h_state, h_words, h_esc, blocks, streams, escs = _encoded(codec, G)
    assert codec.rans_streams_of(h_state, h_words, h_esc, blocks, G) == (streams, escs)
    # the copies as functions, called once the counts have passed; pick words of 0, one per call and one per image
    calls = []
    words_of = lambda lo: calls.append(("words", lo)) or h_words[lo:]          # from the first used byte on
    esc_of = lambda used: calls.append("esc") or h_esc[used]
    for picked in (0, np.zeros(1, np.int32), np.zeros(3, np.uint32)):
        assert codec.rans_streams_of(h_state.view(np.int32), words_of, esc_of, blocks, G, picked, NAME) == (streams, escs)
    first_used = int((blocks[:, 0] + blocks[:, 1] - 2 * h_state[:, 64].astype(np.int64)).min())
    assert calls == [("words", first_used), "esc"] * 3
    # no escape at all: nothing is gathered
    quiet = h_state.copy()
    quiet[:, 65] = 0
    got = codec.rans_streams_of(quiet, h_words, lambda used: calls.append("never"), blocks, G)
    assert got == (streams, [b""] * (3 * G)) and "never" not in calls


@pytest.mark.parametrize("G", [1, 3])
def test_every_refusal_names_its_image(codec, G):
    _, h_state, h_words, h_esc, blocks, _, _ = _encoded(codec, G)
    never = lambda *a: pytest.fail("a buffer was copied before the counts had passed")
    y, z = "the rANS encoder", "the rANS encoder of z"
    y_fault = " met a malformed table, a pixel index outside the image or step lengths that do not add up "
    z_fault = " met a malformed table or step lengths that do not add up "

    def refused(state, picked, coder, message):
        with pytest.raises(codec.CodecError) as err:
            codec.rans_streams_of(state, never, never, blocks, G, picked, NAME, coder)
        assert str(err.value) == message

    bad = h_state.copy()
    bad[2 * G + G - 1, 66] = 2                                             # the last block of image 2
    refused(bad, None, y, f"picture 2: {y}{y_fault}(error word 2)")
    refused(bad, None, z, f"picture 2: {z}{z_fault}(error word 2)")
    bad[1 * G, 66] = 1                                                     # the first bad block speaks
    refused(bad, None, y, f"picture 1: {y}{y_fault}(error word 1)")
    refused(h_state, [0, 4, 0], y, f"picture 1: {y}{y_fault}(error word 4)")   # pick's word of another image
    refused(bad, [0, 4, 0], y, f"picture 1: {y}{y_fault}(error word 5)")
    refused(h_state, 8, z, f"picture 0: {z}{z_fault}(error word 8)")           # the word of the whole call
    for coder in (y, z):
        bad = h_state.copy()
        bad[1 * G, 64] = blocks[1 * G, 1] // 2 + 1                         # 2 nw > SLOT
        refused(bad, None, coder, f"picture 1: {coder} reports impossible counts ({bad[G, 64]} words, {bad[G, 65]} "
                                  "escapes)")
        bad = h_state.copy()
        bad[3 * G - 1, 65] = blocks[3 * G - 1, 3] + 1                      # ne > ESC_CAP
        refused(bad, None, coder, f"picture 2: {coder} reports impossible counts ({bad[3 * G - 1, 64]} words, "
                                  f"{bad[3 * G - 1, 65]} escapes)")
        bad[0, 66] = 16                                                    # an error word comes before any count
        refused(bad, None, coder, f"picture 0: {coder}{y_fault if coder == y else z_fault}(error word 16)")


@pytest.mark.parametrize("G", [1, 3, 4, 8])
def test_the_layout_is_the_one_the_plans_return(codec, G):
    for R in (None, 1, 2, 8):
        plan = codec.ragged_encode_plan(RH.SHAPES, RH.M, RH.PAD, R, G)
        fullest = [codec.rans_group_sizes([len(ii) * RH.M for ii, _ in codec.wavefront(h, w, RH.PAD, R)], G).max()
                   for h, w in RH.SHAPES]
        blocks, words_len, esc_len = codec.rans_block_layout(fullest, G)
        assert blocks.dtype == np.int64 and blocks.flags["C_CONTIGUOUS"]
        assert np.array_equal(blocks, plan.blocks) and (words_len, esc_len) == (plan.words_len, plan.esc_len)
    M, pixels = 5, [1, 7, 40]                                              # test_rans_z_host.py's
    _, want, _, _, want_words, want_esc = codec.z_encode_plan(pixels, M, G)
    blocks, words_len, esc_len = codec.rans_block_layout([codec.rans_group_sizes([P * M], G).max() for P in pixels], G)
    assert np.array_equal(blocks, want) and (words_len, esc_len) == (want_words, want_esc)
    # an image without symbols still owns a slot and a list of one entry; no image, no block
    assert codec.rans_block_layout([0], G)[0].tolist() == [[4 * g, 4, g, 1] for g in range(G)]
    assert codec.rans_block_layout([], G)[0].shape == (0, 4)
    # the single-item kernels' table: images of one size, slots with room for the 64 states (lic_rans_bound)
    blocks, words_len, esc_len = codec.rans_block_layout([5] * 3, G, head=256)
    want = [[i * 268, 268, i * 5, 5] for i in range(3 * G)]
    assert blocks.tolist() == want and (words_len, esc_len) == (3 * G * 268, 3 * G * 5)
    assert 268 == (codec._codec().lic_rans_bound(5) + 3) // 4 * 4
