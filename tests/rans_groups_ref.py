"""Plain Python restatement of the "rANS-64 x G" dealing rule (include/lic_codec.h), written as loops from the
rule's wording and independent of codec.rans_deal: the symbols of an image keep their coding order; symbol k of a step
lies in round k // 64 of that step; round r of every step belongs to sub-stream r % G.  Grouped encode / decode are the
restatement of the rANS-64 format (tests/rans_ref.py) applied to every sub-stream."""
import struct

import numpy as np

import rans_ref as RR

LANES = 64


def deal(step_len, G):
    """-> [(positions, step_len_g) for g in range(G)] as plain lists"""
    pos = [[] for _ in range(G)]
    lens = [[] for _ in range(G)]
    at = 0
    for n_t in step_len:
        for g in range(G):
            lens[g].append(0)
        for k in range(int(n_t)):
            g = (k // LANES) % G
            pos[g].append(at)
            lens[g][-1] += 1
            at += 1
    return [(pos[g], lens[g]) for g in range(G)]


def encode(tables, idx, step_len, G):
    """-> ([G stream bytes], [G escape-list bytes])"""
    tables, idx = np.asarray(tables), np.asarray(idx).ravel()
    streams, escs = [], []
    for pos, lens in deal(step_len, G):
        p = np.array(pos, np.int64)
        s, e = RR.encode(tables[p].reshape(len(p), tables.shape[-1]), idx[p], lens)
        streams.append(s)
        escs.append(e)
    return streams, escs


def decode(streams, escs, tables, step_len):
    """the inverse; G = len(streams); raises rans_ref.Corrupt as rans_ref.decode does"""
    tables = np.asarray(tables)
    out = np.zeros(int(sum(step_len)), np.int64)
    for (pos, lens), s, e in zip(deal(step_len, len(streams)), streams, escs):
        p = np.array(pos, np.int64)
        out[p] = RR.decode(s, e, tables[p].reshape(len(p), tables.shape[-1]), lens)
    return out


# the four consecutive launches of tests/test_gpu_rans.py as (M, pixels of the step), and a fifth of 9 rounds
LAUNCHES = [(32, 1), (32, 3), (1, 327), (1, 1), (192, 3)]
STEPS = [M * n for M, n in LAUNCHES]


def synthetic_images(W=24, steps=STEPS, seed=21):
    """The recipe of tests/test_gpu_rans.py's make_synthetic on `steps`: three images of gamma(0.3), gamma(0.02) and
    gamma(2.0) tables (so three stream lengths), interior symbols drawn from the tables, edge symbols placed by hand
    in images 0 and 2 -- among them the last lane of the 327-symbol step's partial round 5 and both ends of the
    nine-round step; image 1 ends in symbols that cost no word (see below).  -> (tables [3][n][S+1] uint32, idx [3][n] int32)"""
    from oracle import codec_ref as CR
    S = 2 * W + 1
    r = np.random.RandomState(seed)
    nsym = sum(steps)
    tabs, idx = [], []
    for shape in (0.3, 0.02, 2.0):
        f = r.gamma(shape, 1.0, size=(nsym, S)) + 1e-9
        F = np.concatenate([np.zeros((nsym, 1)), np.cumsum(f / f.sum(1, keepdims=True), 1)], 1)
        F[:, -1] = 1.0
        t = CR.quantize_cdf(F)
        u = r.randint(0, 65536, size=nsym)
        i = np.array([np.searchsorted(t[k], u[k], side="right") - 1 for k in range(nsym)], np.int32).clip(1, S - 2)
        tabs.append(t)
        idx.append(i)
    for b, places in ((0, {3: 0, 40: -1, 130: S - 1, 131: S + 100000, 454: -100000, 455: S, 456: -2, 1031: S + 7}),
                      (2, {31: -7, 127: S - 1, 128 + 64 * 5 + 6: 0, 456 + 64 * 4: -3, 456 + 64 * 7 + 63: S - 1})):
        for k, v in places.items():
            if k < nsym:
                idx[b][k] = v
    # image 1, rounds 5 to 8 of the nine-round step: every table's most probable interior symbol.  With these peaked
    # tables such a symbol costs no word as a rule, so a sub-stream of image 1 reads its last word before it decodes
    # them and, cut by one word, has symbols left to get wrong: `symbols_after_the_last_word` says how many
    late = np.arange(sum(steps[:4]) + 5 * LANES, nsym)
    if len(steps) == 5 and late.size:
        idx[1][late] = 1 + np.diff(tabs[1][late].astype(np.int64), axis=1)[:, 1:S - 1].argmax(1)
    return np.stack(tabs), np.stack(idx)


def symbols_after_the_last_word(stream, tables, step_len):
    """how many symbols of one rANS-64 stream are decoded in rounds AFTER the round that reads its last word: the
    decoder of the format, round by round, keeping only the states and the word cursor"""
    tables = np.asarray(tables, np.int64)
    x = list(struct.unpack_from("<%dI" % LANES, stream, 0))
    nwords = (len(stream) - 4 * LANES) // 2
    words = struct.unpack_from("<%dH" % nwords, stream, 4 * LANES)
    ptr = base = done = 0
    at_last = None
    for n_t in step_len:
        for rnd in range((int(n_t) + LANES - 1) // LANES):
            active = [lane for lane in range(LANES) if rnd * LANES + lane < n_t]
            for lane in active:
                row = tables[base + rnd * LANES + lane]
                slot = x[lane] & 0xFFFF
                s = int(np.searchsorted(row, slot, side="right")) - 1
                x[lane] = int(row[s + 1] - row[s]) * (x[lane] >> 16) + slot - int(row[s])
            need = [lane for lane in active if x[lane] < 1 << 16]
            for rank, lane in enumerate(need):
                x[lane] = (x[lane] << 16) | words[ptr + rank]
            ptr += len(need)
            done += len(active)
            if need and ptr == nwords:
                at_last = done
        base += int(n_t)
    assert ptr == nwords and nwords > 0
    return done - at_last
