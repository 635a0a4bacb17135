"""Plain Python restatement of the "rANS-64" y-stream format (include/lic_codec.h), written from the format's
description, not from the C++: 64 interleaved 32-bit states in [2^16, 2^32), 16-bit probabilities, renormalisation
by 16-bit little-endian words (at most one per symbol per lane), symbol k of a step on lane k % 64 in round k / 64,
rounds never straddling steps, escapes in a separate list of uint32 in symbol order.

The decoder is written round by round with the ballot-and-rank rule spelled out (who needs a word, how many needing
lanes have a smaller id), the way a 64-lane wave executes it; the encoder is its mirror."""
import struct

import numpy as np

LANES = 64
LOW = 1 << 16


class Corrupt(Exception):
    pass


def _edge(v, S):
    """(coded symbol, excess or None)"""
    if v <= 0:
        return 0, -v
    if v >= S - 1:
        return S - 1, v - (S - 1)
    return v, None


def encode(tables, idx, step_len):
    """tables [n][S+1], idx [n], step_len: symbols per step -> (stream bytes, escape-list bytes)"""
    tables = np.asarray(tables, np.int64)
    idx = [int(v) for v in np.asarray(idx).ravel()]
    S = tables.shape[-1] - 1 if tables.ndim == 2 else 0
    assert sum(step_len) == len(idx)
    esc = [ex for ex in (_edge(v, S)[1] for v in idx) if ex is not None]        # symbol order
    x = [LOW] * LANES
    words = []                                                                   # in emission order = reverse reading order
    bases = np.concatenate([[0], np.cumsum(step_len)]).astype(np.int64)
    for t in range(len(step_len) - 1, -1, -1):
        n_t = int(step_len[t])
        for rnd in range((n_t + LANES - 1) // LANES - 1, -1, -1):
            for lane in range(LANES - 1, -1, -1):
                k = rnd * LANES + lane
                if k >= n_t:
                    continue                                                     # partial last round: the lane does nothing
                i = int(bases[t]) + k
                s, _ = _edge(idx[i], S)
                start, freq = int(tables[i, s]), int(tables[i, s + 1] - tables[i, s])
                assert 1 <= freq < 65536
                if x[lane] >= freq << 16:
                    words.append(x[lane] & 0xFFFF)
                    x[lane] >>= 16
                x[lane] = ((x[lane] // freq) << 16) + (x[lane] % freq) + start
                assert LOW <= x[lane] < 1 << 32
    words.reverse()
    stream = struct.pack("<%dI" % LANES, *x) + struct.pack("<%dH" % len(words), *words)
    return stream, struct.pack("<%dI" % len(esc), *esc)


def decode(stream, esc_bytes, tables, step_len):
    """the inverse; raises Corrupt for a cursor past the end, trailing words / escapes, or final states != 2^16"""
    tables = np.asarray(tables, np.int64)
    S = tables.shape[-1] - 1 if tables.ndim == 2 else 0
    if len(stream) < 4 * LANES or len(stream) % 2 or len(esc_bytes) % 4:
        raise Corrupt("impossible length")
    x = list(struct.unpack_from("<%dI" % LANES, stream, 0))
    nwords = (len(stream) - 4 * LANES) // 2
    words = struct.unpack_from("<%dH" % nwords, stream, 4 * LANES)
    esc = struct.unpack("<%dI" % (len(esc_bytes) // 4), esc_bytes)
    ptr = eptr = 0
    out = []
    base = 0
    for n_t in step_len:
        n_t = int(n_t)
        for rnd in range((n_t + LANES - 1) // LANES):
            active = [lane for lane in range(LANES) if rnd * LANES + lane < n_t]
            sym = {}
            for lane in active:
                row = tables[base + rnd * LANES + lane]
                slot = x[lane] & 0xFFFF
                s = int(np.searchsorted(row, slot, side="right")) - 1            # cum[s] <= slot < cum[s+1]
                x[lane] = int(row[s + 1] - row[s]) * (x[lane] >> 16) + slot - int(row[s])
                sym[lane] = s
            need = [lane for lane in active if x[lane] < LOW]                    # the ballot
            for rank, lane in enumerate(need):                                   # rank = needing lanes with a smaller id
                if ptr + rank >= nwords:
                    raise Corrupt("word cursor past the end")
                x[lane] = (x[lane] << 16) | words[ptr + rank]
            ptr += len(need)
            edge = [lane for lane in active if sym[lane] in (0, S - 1)]          # the second cursor, same rule
            excess = {}
            for rank, lane in enumerate(edge):
                if eptr + rank >= len(esc):
                    raise Corrupt("escape cursor past the end")
                excess[lane] = esc[eptr + rank]
            eptr += len(edge)
            for lane in active:
                s = sym[lane]
                out.append(-excess[lane] if s == 0 else (s + excess[lane] if s == S - 1 else s))
        base += n_t
    if ptr != nwords or eptr != len(esc) or any(v != LOW for v in x):
        raise Corrupt("stream not used up exactly")
    return np.array(out, np.int64)


def ideal_bits(tables, idx):
    """-sum log2(freq / 65536) + 32 bits per escape"""
    tables = np.asarray(tables, np.int64)
    S = tables.shape[-1] - 1
    bits = 0.0
    for i, v in enumerate(np.asarray(idx).ravel()):
        s, ex = _edge(int(v), S)
        bits += 16.0 - np.log2(float(tables[i, s + 1] - tables[i, s])) + (32.0 if ex is not None else 0.0)
    return bits
