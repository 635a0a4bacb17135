"""The self-describing container of `ContextCodec.compress_image` (host only, no torch): one byte string per batch
of images of any size.  Six formats, one per (coder, grouping) pair of the y streams, one for rANS-coded z and one for
the checkerboard schedule; `_FORMATS`, `_FORMAT_ZRANS_ROW` and `_FORMAT_CHECKER_ROW` below describe them, `_pack` writes
and `_unpack` reads all six, and the twelve public functions are their wrappers.

Every format, little endian:
  magic (8 bytes) | uint32 family (1 = JointAutoregressiveHierarchical, 2 = HierarchicalMixtureResidual)
  | uint32 M, K | int32 z_lo | uint32 z_S, y_W, B, H, W, top, left | uint32 z-stream length | [uint32 lanes]
  | [uint32 slice_rows]
  | image table: B rows | block table: B*G rows, image-major (row b * G + g)
  | z stream | for every block: its y stream, then its escape list (uint32 each) | uint32 CRC-32 of all before it
The padded size is the next multiple of 64 of (H, W); the latent is [B, M, Hp/16, Wp/16], z [B, M, Hp/64, Wp/64].

  magic     coder  lanes word        image table row   block table row                    blocks per image
  LICBITS1  range  absent            none              y length, symbol CRC-32            1
  LICBITS2  rans   64                none              y length, symbol CRC-32, escapes   1
  LICBITS3  rans   64 G, G in 1..8   symbol CRC-32     sub-stream length, escapes         G ("rANS-64 x G", `rans_deal`)
  LICBITS4  rans   64 G, G in 1..8   symbol CRC-32     sub-stream length, escapes         G, and the slice_rows word
  LICBITS5  rans   64 G, G in 1..8   symbol CRC-32     sub-stream length, escapes         G, slice_rows word, z section
  LICBITS7  rans   64 G, G in 1..8   symbol CRC-32     sub-stream length, escapes         G, slice_rows word = 0, z section

"symbol CRC-32" is `compress`'s y_crc32 of that image's latent symbols, "escapes" the number of uint32 in the block's
escape list.  `lanes` is the interleaving of an image's y streams.  A LICBITS2 reader refuses any value but 64: wider
interleaving has LICBITS3, whose tables have another shape.  A LICBITS3 reader takes the multiples of 64 up to 512
(64 is legal there, though `compress_image` writes LICBITS2 for one group) and refuses a sub-stream shorter than its 64
states or of odd length.  LICBITS4 is LICBITS3 with one more header word: `slice_rows` = R >= 1, the latent rows per slice
of the context model (codec.ContextCodec: no context tap crosses a boundary between bands of R rows, and the bands
decode side by side); `compress_image` writes it only for a codec with slices, for any G.  Its reader refuses what
LICBITS3's does, and R = 0 as a damaged header; R comes back as head["slice_rows"].
LICBITS5 is the container of a codec with z_coder="rans" (codec.ContextCodec), for any G, with or without slices: the
header is LICBITS4's, and its slice_rows word may be 0 = no slices (head then has no "slice_rows").  The hyper-latent
is not one range-coder stream for the batch but "rANS-64 x G" sub-streams per image, so where the other formats have
the z stream LICBITS5 has a z SECTION, and the header's "z-stream length" is the section's length:
  z block table: B*G rows (sub-stream length, escapes), image-major | for every z block: its stream, then its escape list
Its reader refuses what LICBITS3's does, for the z blocks too -- a z sub-stream shorter than its 64 states or of odd
length -- and a z section whose table and blocks do not add up to its length.
LICBITS7 is byte for byte LICBITS5's layout under its own magic, and names the SCHEDULE of the y symbols: the two passes
of the checkerboard context (codec.two_pass: the anchors, latent pixels with i + j even, in raster order, then the
others) where LICBITS1 to 5 mean the raster wavefront.  A checkerboard model has no slices: its slice_rows word is 0,
and its reader refuses anything else as a damaged header, besides what LICBITS5's reader refuses.

LICBITS6 is the layered container of codec.ScalableCodec (family 3 = ScalableImageCoding): the latent's M channels are
two layers, the base one of M1 channels, each coded as "rANS-64 x G" sub-streams of its own.  Its header is LICBITS5's
plus `uint32 M1, base_bytes`, and the blob is
  header | image table: B rows (symbol CRC-32 of layer 0, of layer 1) | z section (LICBITS5's)
  | base section: block table, B*G rows (sub-stream length, escapes), then the blocks | uint32 CRC-32 of all before it
  | enhancement section: the same for layer 1 | uint32 CRC-32 of all before it
`base_bytes` is the offset just behind the first CRC-32, so blob[:base_bytes] is a valid input of the base reader
(`unpack_bitstream_layered_base`), which looks at nothing behind it; the full reader (`unpack_bitstream_layered`)
refuses that prefix as truncated.  Both refuse what LICBITS5's reader does, M1 outside 0 < M1 < M, and a `base_bytes`
that is not where the tables put the end of the base section.
"""
from __future__ import annotations

import struct
import zlib
from itertools import accumulate
from typing import Dict

import numpy as np

RANS_LANES = 64
RANS_MAX_GROUPS = 8                              # sub-streams per image of the "rANS-64 x G" format


class CodecError(RuntimeError):
    pass


def _groups(G) -> int:
    """G as an int in 1..RANS_MAX_GROUPS, or CodecError"""
    if isinstance(G, bool) or not isinstance(G, (int, np.integer)) or not 1 <= int(G) <= RANS_MAX_GROUPS:
        raise CodecError(f"groups = {G!r}: expected an integer from 1 to {RANS_MAX_GROUPS}")
    return int(G)


BITSTREAM_FAMILIES = {"JointAutoregressiveHierarchical": 1, "HierarchicalMixtureResidual": 2, "ScalableImageCoding": 3}
BITSTREAM_MAGIC, BITSTREAM_MAGIC_RANS, BITSTREAM_MAGIC_GROUPED = b"LICBITS1", b"LICBITS2", b"LICBITS3"
BITSTREAM_MAGIC_SLICED = b"LICBITS4"
BITSTREAM_MAGIC_ZRANS = b"LICBITS5"
_BITS_FIELDS = ("family", "M", "K", "z_lo", "z_S", "y_W", "B", "H", "W", "top", "left")
_BITS_HEAD, _BITS_HEAD_RANS = struct.Struct("<8s3Ii8I"), struct.Struct("<8s3Ii9I")          # without / with `lanes`
_BITS_HEAD_SLICED = struct.Struct("<8s3Ii10I")                                                # `lanes`, `slice_rows`
# (coder, grouping: False = one stream per image, True = G sub-streams, "sliced" = those and slices)
# -> (magic, header, image table columns, block table columns, what `_pack` expects)
_FORMATS = {
    ("range", False): (BITSTREAM_MAGIC, _BITS_HEAD, (), ("len", "crc"), "one y stream and one checksum per image"),
    ("rans", False): (BITSTREAM_MAGIC_RANS, _BITS_HEAD_RANS, (), ("len", "crc", "esc"),
                      "one y stream, one escape list and one checksum per image"),
    ("rans", True): (BITSTREAM_MAGIC_GROUPED, _BITS_HEAD_RANS, ("crc",), ("len", "esc"),
                     "one sub-stream and one escape list per image and group, one checksum per image"),
    ("rans", "sliced"): (BITSTREAM_MAGIC_SLICED, _BITS_HEAD_SLICED, ("crc",), ("len", "esc"),
                         "one sub-stream and one escape list per image and group, one checksum per image"),
}
_FORMAT_OF_MAGIC = {f[0]: key for key, f in _FORMATS.items()}
# the four above carry z as ONE range-coder stream; LICBITS5 carries a z section and is kept beside them
_FORMAT_ZRANS = ("rans", "zrans")
_FORMAT_ZRANS_ROW = (BITSTREAM_MAGIC_ZRANS, _BITS_HEAD_SLICED, ("crc",), ("len", "esc"),
                     "one y and one z sub-stream and escape list per image and group, one checksum per image")
# LICBITS7: LICBITS5's layout for the two-pass schedule of a checkerboard context model
BITSTREAM_MAGIC_CHECKER = b"LICBITS7"
_FORMAT_CHECKER = ("rans", "checker")
_FORMAT_CHECKER_ROW = (BITSTREAM_MAGIC_CHECKER,) + _FORMAT_ZRANS_ROW[1:]
_Z_SECTION_FORMATS = (_FORMAT_ZRANS, _FORMAT_CHECKER)


def _format_of_magic(magic: bytes):
    """the key `_pack` / `_unpack` take for a blob that starts with `magic`; an unknown magic: LICBITS1's reader says so"""
    beside = {BITSTREAM_MAGIC_ZRANS: _FORMAT_ZRANS, BITSTREAM_MAGIC_CHECKER: _FORMAT_CHECKER}
    return beside.get(bytes(magic)) or _FORMAT_OF_MAGIC.get(bytes(magic), ("range", False))


def _format(fmt):
    return {_FORMAT_ZRANS: _FORMAT_ZRANS_ROW, _FORMAT_CHECKER: _FORMAT_CHECKER_ROW}.get(fmt) or _FORMATS[fmt]


def _pack(fmt, head: Dict, z_bytes: bytes, ys, escs, crcs, G: int = 1, lanes: int = None) -> bytes:
    """`head`: the _BITS_FIELDS; B * G y streams and escape lists (bytes; None where the format has none), image-major,
    and one symbol checksum per image.  The sliced format takes head["slice_rows"] as well."""
    magic, st, img_cols, blk_cols, expects = _format(fmt)
    zrans = fmt in _Z_SECTION_FORMATS
    R = head.get("slice_rows", 0) if st is _BITS_HEAD_SLICED else 0
    R = 0 if zrans and R is None else R
    if fmt == _FORMAT_CHECKER and not (isinstance(R, (int, np.integer)) and not isinstance(R, bool) and int(R) == 0):
        raise CodecError(f"slice_rows = {R!r}: a checkerboard bitstream has no slices")
    if st is _BITS_HEAD_SLICED and (isinstance(R, bool) or not isinstance(R, (int, np.integer))
                                    or not (0 if zrans else 1) <= int(R) <= 0xFFFFFFFF):
        raise CodecError(f"slice_rows = {R!r}: a sliced bitstream needs a whole number of rows per slice, at least 1")
    B = int(head["B"])
    if zrans:
        z_bytes = _pack_z_section(z_bytes, B * G, expects)
    escs = [b""] * len(ys) if escs is None else escs
    if len(ys) != B * G or len(escs) != B * G or len(crcs) != B:
        raise CodecError(expects + " expected")
    if any(len(e) % 4 for e in escs):
        raise CodecError("an escape list is not a whole number of uint32")
    words = (len(z_bytes), RANS_LANES * G if lanes is None else int(lanes), int(R))
    parts = [st.pack(magic, *(int(head[k]) for k in _BITS_FIELDS), *words[:1 + (st.size - _BITS_HEAD.size) // 4])]
    rows = [{"crc": int(c) & 0xFFFFFFFF} for c in crcs]
    blocks = [dict(rows[i // G], len=len(s), esc=len(e) // 4) for i, (s, e) in enumerate(zip(ys, escs))]
    parts += [struct.pack("<%dI" % len(cols), *(r[k] for k in cols)) for cols, t in ((img_cols, rows), (blk_cols, blocks))
              for r in t]
    parts += [bytes(z_bytes)] + [bytes(p) for s, e in zip(ys, escs) for p in (s, e)]
    body = b"".join(parts)
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def _pack_z_section(z, nblocks: int, expects: str) -> bytes:
    """z = ([sub-stream per image and group], [escape list likewise]) -> LICBITS5's z section"""
    try:
        zs, zes = z
        zs, zes = [bytes(s) for s in zs], [bytes(e) for e in zes]
    except (TypeError, ValueError):
        raise CodecError(expects + " expected") from None
    if len(zs) != nblocks or len(zes) != nblocks:
        raise CodecError(expects + " expected")
    if any(len(e) % 4 for e in zes):
        raise CodecError("an escape list is not a whole number of uint32")
    return b"".join([struct.pack("<2I", len(s), len(e) // 4) for s, e in zip(zs, zes)]
                    + [p for s, e in zip(zs, zes) for p in (s, e)])


def _unpack_z_section(sec: bytes, nblocks: int):
    """the inverse -> ([sub-stream], [escape list]); CodecError for a section that does not add up or a sub-stream
    shorter than its 64 states or of odd length"""
    if len(sec) < 8 * nblocks:
        raise CodecError("bitstream is truncated (z block table)")
    rows = [struct.unpack_from("<2I", sec, 8 * i) for i in range(nblocks)]
    cuts = list(accumulate([n for ln, ne in rows for n in (ln, 4 * ne)], initial=8 * nblocks))
    if cuts[-1] != len(sec):
        raise CodecError("bitstream z section does not add up (its block table and its length disagree)")
    if any(ln < 4 * RANS_LANES or ln % 2 for ln, _ in rows):
        raise CodecError("bitstream names a z sub-stream shorter than its 64 states or of odd length")
    payload = [sec[a:b] for a, b in zip(cuts, cuts[1:])]
    return payload[0::2], payload[1::2]


def _unpack(fmt, data: bytes):
    """-> (head dict, z_bytes, [y stream per block], [escape list per block], [symbol checksum per image], G); for
    LICBITS5 z_bytes is the pair ([z sub-stream per block], [z escape list per block]).
    CodecError, in this order, for a buffer shorter than its header or tables, another magic, a total length that is
    not the one the header and tables name, a failing CRC-32, a header that cannot be right, and what the format itself
    refuses (module docstring) -- except that LICBITS3 must know G to find its tables, so its `lanes` rule comes first."""
    magic, st, img_cols, blk_cols, _ = _format(fmt)
    data = bytes(data)
    if len(data) < st.size + 4:
        raise CodecError("bitstream is truncated (shorter than its header)")
    vals = st.unpack_from(data, 0)
    if vals[0] != magic:
        raise CodecError(f"not a {magic.decode()} bitstream (bad magic)")
    head = dict(zip(_BITS_FIELDS, vals[1:12]))
    z_len, lanes, B, G = vals[12], RANS_LANES if st is _BITS_HEAD else vals[13], head["B"], 1
    if fmt[1]:
        if lanes % RANS_LANES or not RANS_LANES <= lanes <= RANS_LANES * RANS_MAX_GROUPS:
            raise CodecError(f"bitstream interleaves {lanes} coder states; this decoder implements multiples of "
                             f"{RANS_LANES} up to {RANS_LANES * RANS_MAX_GROUPS}")
        G = lanes // RANS_LANES
    at = st.size
    if B == 0 or len(data) < at + 4 * (len(img_cols) + len(blk_cols) * G) * B + 4:
        raise CodecError("bitstream is truncated (per-image table%s)" % ("s" if img_cols else ""))
    tables = []
    for cols, n in ((img_cols, B), (blk_cols, B * G)):
        row = struct.Struct("<%dI" % len(cols))
        tables.append([dict(zip(cols, row.unpack_from(data, at + row.size * i))) for i in range(n)])
        at += row.size * n
    rows, blocks = tables
    # where the z stream, then every block's y stream and escape list, begin and end
    cuts = list(accumulate([z_len] + [n for r in blocks for n in (r["len"], 4 * r.get("esc", 0))], initial=at))
    if len(data) != cuts[-1] + 4:
        raise CodecError("bitstream is truncated or has trailing bytes (its length does not match its header)")
    _check_crc_and_head(data, head)
    if not fmt[1] and lanes != RANS_LANES:
        raise CodecError(f"bitstream interleaves {lanes} coder states; this decoder implements {RANS_LANES}")
    if fmt[1] and any(r["len"] < 4 * RANS_LANES or r["len"] % 2 for r in blocks):
        raise CodecError("bitstream names a sub-stream shorter than its 64 states or of odd length")
    zrans = fmt in _Z_SECTION_FORMATS
    if st is _BITS_HEAD_SLICED:
        if vals[14] < 1 and not zrans:
            raise CodecError("bitstream header is damaged (slice_rows = 0)")
        if vals[14] and fmt == _FORMAT_CHECKER:
            raise CodecError(f"bitstream header is damaged (slice_rows = {vals[14]} in a checkerboard bitstream)")
        if vals[14] >= 1:
            head["slice_rows"] = vals[14]
    payload = [data[a:b] for a, b in zip(cuts, cuts[1:])]
    z = _unpack_z_section(payload[0], B * G) if zrans else payload[0]
    return head, z, payload[1::2], payload[2::2], [r["crc"] for r in (rows if img_cols else blocks)], G


def _check_crc_and_head(data: bytes, head: Dict):
    """the checks all containers share: the trailing CRC-32 and a header that can be right"""
    if zlib.crc32(data[:-4]) & 0xFFFFFFFF != struct.unpack_from("<I", data, len(data) - 4)[0]:
        raise CodecError("bitstream is damaged (CRC-32 mismatch)")
    if not (head["H"] > 0 and head["W"] > 0 and head["top"] < 64 and head["left"] < 64
            and head["top"] + head["H"] <= -(-head["H"] // 64) * 64 and head["left"] + head["W"] <= -(-head["W"] // 64) * 64
            and head["M"] > 0 and head["K"] > 0 and head["z_S"] > 0 and head["y_W"] > 0):
        raise CodecError("bitstream header is inconsistent")


# ---- LICBITS6: the layered container of codec.ScalableCodec --------------------------------------------------------
# It sits beside the five above as LICBITS5 sits beside the first four: `_FORMAT_OF_MAGIC` stays what it is.
BITSTREAM_MAGIC_LAYERED = b"LICBITS6"
_BITS_HEAD_LAYERED = struct.Struct("<8s3Ii12I")                        # LICBITS5's header, then `M1`, `base_bytes`
_LAYERED_EXPECTS = ("two layers of one sub-stream and one escape list per image and group and one checksum per image, "
                    "and one z sub-stream and escape list per image and group")


def _pack_block_section(ys, escs) -> bytes:
    """block table (sub-stream length, escapes per block), then every block's stream and escape list"""
    return b"".join([struct.pack("<2I", len(s), len(e) // 4) for s, e in zip(ys, escs)]
                    + [bytes(p) for s, e in zip(ys, escs) for p in (s, e)])


def pack_bitstream_layered(head: Dict, z_streams, z_esc, layers, groups: int, slice_rows: int = None) -> bytes:
    """LICBITS6.  `head`: the _BITS_FIELDS and "M1"; `layers`: two dicts {"y": [B*G sub-streams], "y_esc": [B*G escape
    lists], "y_crc32": [B]}, base layer first; z as for LICBITS5; slice_rows None or 0: no slices.  Layout (module
    docstring): header | image table | z section | base section | CRC-32 | enhancement section | CRC-32, and
    header word `base_bytes` = the offset just behind the first CRC-32, so blob[:base_bytes] decodes the base alone."""
    G, B = _groups(groups), int(head["B"])
    R = 0 if slice_rows is None else slice_rows
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 0 <= int(R) <= 0xFFFFFFFF:
        raise CodecError(f"slice_rows = {R!r}: expected None or a whole number of rows per slice")
    try:
        if len(layers) != 2:
            raise CodecError(_LAYERED_EXPECTS + " expected")
        secs = [([bytes(s) for s in ly["y"]], [bytes(e) for e in ly["y_esc"]], list(ly["y_crc32"])) for ly in layers]
    except (TypeError, KeyError):
        raise CodecError(_LAYERED_EXPECTS + " expected") from None
    if any(len(ys) != B * G or len(es) != B * G or len(crc) != B for ys, es, crc in secs):
        raise CodecError(_LAYERED_EXPECTS + " expected")
    if any(len(e) % 4 for _, es, _ in secs for e in es):
        raise CodecError("an escape list is not a whole number of uint32")
    z_sec = _pack_z_section((z_streams, z_esc), B * G, _LAYERED_EXPECTS)
    images = b"".join(struct.pack("<2I", int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF) for a, b in zip(secs[0][2], secs[1][2]))
    base_sec, enh_sec = _pack_block_section(*secs[0][:2]), _pack_block_section(*secs[1][:2])
    base_bytes = _BITS_HEAD_LAYERED.size + len(images) + len(z_sec) + len(base_sec) + 4
    if base_bytes + len(enh_sec) + 4 > 0xFFFFFFFF:
        raise CodecError("the bitstream is too long for its 32-bit lengths")
    front = _BITS_HEAD_LAYERED.pack(BITSTREAM_MAGIC_LAYERED, *(int(head[k]) for k in _BITS_FIELDS), len(z_sec),
                                    RANS_LANES * G, int(R), int(head["M1"]), base_bytes) + images + z_sec + base_sec
    front += struct.pack("<I", zlib.crc32(front) & 0xFFFFFFFF)
    body = front + enh_sec
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def _block_table(data: bytes, at: int, nblocks: int):
    """the block table at `at` -> ([(length, escapes)], the cuts of its blocks' streams and escape lists behind it)"""
    rows = [struct.unpack_from("<2I", data, at + 8 * i) for i in range(nblocks)]
    return rows, list(accumulate([n for ln, ne in rows for n in (ln, 4 * ne)], initial=at + 8 * nblocks))


def _unpack_layered(data: bytes, base_only: bool):
    """Both LICBITS6 readers.  -> (head with "M1", "base_bytes" and, if slicing, "slice_rows"; [z sub-stream per block];
    [z escape list per block]; the layers read: [{"y", "y_esc", "y_crc32"}] -- one for the base reader, two for the
    full one; G).  The base reader takes the whole blob, its prefix blob[:base_bytes] or either with anything behind
    base_bytes, and looks at nothing there.  CodecError in `_unpack`'s order: a buffer shorter than its header, another
    magic, a `lanes` word that names no G, a buffer shorter than its tables, lengths that do not add up (`base_bytes`
    against the tables; for the full reader the total, so it refuses a prefix as truncated), a failing CRC-32 (the
    base reader: the one at base_bytes - 4 only), a header that cannot be right (0 < M1 < M included), a sub-stream
    shorter than its 64 states or of odd length, and what the z section refuses."""
    st = _BITS_HEAD_LAYERED
    data = bytes(data)
    if len(data) < st.size + 4:
        raise CodecError("bitstream is truncated (shorter than its header)")
    vals = st.unpack_from(data, 0)
    if vals[0] != BITSTREAM_MAGIC_LAYERED:
        raise CodecError(f"not a {BITSTREAM_MAGIC_LAYERED.decode()} bitstream (bad magic)")
    head = dict(zip(_BITS_FIELDS, vals[1:12]))
    z_len, lanes, R, M1, base_bytes = vals[12:17]
    B = head["B"]
    if lanes % RANS_LANES or not RANS_LANES <= lanes <= RANS_LANES * RANS_MAX_GROUPS:
        raise CodecError(f"bitstream interleaves {lanes} coder states; this decoder implements multiples of "
                         f"{RANS_LANES} up to {RANS_LANES * RANS_MAX_GROUPS}")
    G = lanes // RANS_LANES
    z_at = st.size + 8 * B
    base_at = z_at + z_len
    if B == 0 or len(data) < base_at + 8 * B * G + 4:
        raise CodecError("bitstream is truncated (per-image tables)")
    rows = [struct.unpack_from("<2I", data, st.size + 8 * i) for i in range(B)]
    base_rows, base_cuts = _block_table(data, base_at, B * G)
    if base_bytes != base_cuts[-1] + 4:
        raise CodecError("bitstream header is damaged (base_bytes does not match the base layer's tables)")
    if len(data) < base_bytes:
        raise CodecError("bitstream is truncated (shorter than its base layer)")
    sections = [(base_rows, base_cuts)]
    if not base_only:
        if len(data) < base_bytes + 8 * B * G + 4:
            raise CodecError("bitstream is truncated (it ends with its base layer: only the base decodes)"
                             if len(data) == base_bytes else "bitstream is truncated (enhancement layer table)")
        enh_rows, enh_cuts = _block_table(data, base_bytes, B * G)
        if len(data) != enh_cuts[-1] + 4:
            raise CodecError("bitstream is truncated or has trailing bytes (its length does not match its header)")
        sections.append((enh_rows, enh_cuts))
    if zlib.crc32(data[:base_bytes - 4]) & 0xFFFFFFFF != struct.unpack_from("<I", data, base_bytes - 4)[0]:
        raise CodecError("bitstream is damaged (CRC-32 mismatch in the base layer)")
    if not base_only:
        _check_crc_and_head(data, head)
    else:
        _check_crc_and_head(data[:base_bytes], head)
    if not 0 < M1 < head["M"]:
        raise CodecError("bitstream header is inconsistent (M1 outside 0 < M1 < M)")
    if any(ln < 4 * RANS_LANES or ln % 2 for sec_rows, _ in sections for ln, _ in sec_rows):
        raise CodecError("bitstream names a sub-stream shorter than its 64 states or of odd length")
    head.update(M1=M1, base_bytes=base_bytes)
    if R >= 1:
        head["slice_rows"] = R
    zs, zes = _unpack_z_section(data[z_at:base_at], B * G)
    layers = []
    for l, (_, cuts) in enumerate(sections):
        payload = [data[a:b] for a, b in zip(cuts, cuts[1:])]
        layers.append({"y": payload[0::2], "y_esc": payload[1::2], "y_crc32": [r[l] for r in rows]})
    return head, zs, zes, layers, G


def unpack_bitstream_layered(data: bytes):
    """-> (head dict with "M1" and "base_bytes", [z sub-stream per image and group], [z escape list likewise],
    [base layer, enhancement layer] as {"y", "y_esc", "y_crc32"}, groups, slice_rows or None).  Refuses a prefix."""
    head, zs, zes, layers, G = _unpack_layered(data, False)
    return head, zs, zes, layers, G, head.get("slice_rows")


def unpack_bitstream_layered_base(data: bytes):
    """The same from a whole LICBITS6 blob or from its prefix blob[:base_bytes], with the base layer alone in the
    list; bytes behind base_bytes are not looked at."""
    head, zs, zes, layers, G = _unpack_layered(data, True)
    return head, zs, zes, layers, G, head.get("slice_rows")


def pack_bitstream(head: Dict, z_bytes: bytes, y_streams, y_crc32) -> bytes:
    return _pack(("range", False), head, z_bytes, y_streams, None, y_crc32)


def unpack_bitstream(data: bytes):
    """-> (head dict, z_bytes, [y stream per image], [symbol checksum per image])"""
    head, z_bytes, ys, _, crcs, _ = _unpack(("range", False), data)
    return head, z_bytes, ys, crcs


def pack_bitstream_rans(head: Dict, z_bytes: bytes, y_streams, y_esc, y_crc32, lanes: int = RANS_LANES) -> bytes:
    return _pack(("rans", False), head, z_bytes, y_streams, y_esc, y_crc32, lanes=lanes)


def unpack_bitstream_rans(data: bytes):
    """-> (head dict, z_bytes, [y stream per image], [escape list per image], [symbol checksum per image])"""
    return _unpack(("rans", False), data)[:5]


def pack_bitstream_grouped(head: Dict, z_bytes: bytes, y_streams, y_esc, y_crc32, groups: int) -> bytes:
    return _pack(("rans", True), head, z_bytes, y_streams, y_esc, y_crc32, _groups(groups))


def unpack_bitstream_grouped(data: bytes):
    """-> (head dict, z_bytes, [sub-stream per image and group], [escape list likewise], [symbol checksum per image],
    groups)"""
    return _unpack(("rans", True), data)


def pack_bitstream_sliced(head: Dict, z_bytes: bytes, y_streams, y_esc, y_crc32, groups: int, slice_rows: int) -> bytes:
    return _pack(("rans", "sliced"), dict(head, slice_rows=slice_rows), z_bytes, y_streams, y_esc, y_crc32,
                 _groups(groups))


def unpack_bitstream_sliced(data: bytes):
    """-> `unpack_bitstream_grouped`'s six, then slice_rows (head["slice_rows"] too)"""
    out = _unpack(("rans", "sliced"), data)
    return out + (out[0]["slice_rows"],)


def pack_bitstream_zrans(head: Dict, z_streams, z_esc, y_streams, y_esc, y_crc32, groups: int,
                         slice_rows: int = None) -> bytes:
    """LICBITS5: z as B * groups rANS sub-streams and escape lists, image-major; slice_rows None or 0: no slices"""
    return _pack(_FORMAT_ZRANS, dict(head, slice_rows=slice_rows or 0), (z_streams, z_esc), y_streams, y_esc,
                 y_crc32, _groups(groups))


def unpack_bitstream_zrans(data: bytes):
    """-> (head dict, [z sub-stream per image and group], [z escape list likewise], [y sub-stream likewise],
    [y escape list likewise], [symbol checksum per image], groups, slice_rows or None)"""
    head, (zs, zes), ys, escs, crcs, G = _unpack(_FORMAT_ZRANS, data)
    return head, zs, zes, ys, escs, crcs, G, head.get("slice_rows")


def pack_bitstream_checker(head: Dict, z_streams, z_esc, y_streams, y_esc, y_crc32, groups: int) -> bytes:
    """LICBITS7: `pack_bitstream_zrans` without slices, for y symbols in the two-pass order of a checkerboard context"""
    return _pack(_FORMAT_CHECKER, dict(head, slice_rows=0), (z_streams, z_esc), y_streams, y_esc, y_crc32, _groups(groups))


def unpack_bitstream_checker(data: bytes):
    """-> `unpack_bitstream_zrans`'s first seven: (head dict, [z sub-stream per image and group], [z escape list
    likewise], [y sub-stream likewise], [y escape list likewise], [symbol checksum per image], groups)"""
    head, (zs, zes), ys, escs, crcs, G = _unpack(_FORMAT_CHECKER, data)
    return head, zs, zes, ys, escs, crcs, G


# ---- LICRATE1: the quality envelope of a rate-level codec ----------------------------------------------------------
# A variable-rate model (models: rate_levels = Q) codes at any real quality q in [0, Q-1], and its decoder needs q for the
# two inverse gains.  q travels AROUND the container, not in it: the tables above stay what they are.  Little endian:
#   magic LICRATE1 | float32 q | uint16 Q | uint16 zero | uint32 inner length | the inner LICBITS1-5/7 blob, verbatim
#   | uint32 CRC-32 of all before it
BITSTREAM_MAGIC_RATE = b"LICRATE1"
_RATE_HEAD = struct.Struct("<8sfHHI")


def _rate_quality(quality, Q):
    """(q as the float32 the envelope holds, Q) or CodecError"""
    if isinstance(Q, bool) or not isinstance(Q, (int, np.integer)) or not 2 <= int(Q) <= 0xFFFF:
        raise CodecError(f"rate_levels = {Q!r}: expected an integer from 2 to 65535")
    try:
        q = float(np.float32(quality))
    except (TypeError, ValueError):
        raise CodecError(f"quality = {quality!r}: expected a number") from None
    if not 0.0 <= q <= int(Q) - 1:
        raise CodecError(f"quality {quality!r} outside [0, {int(Q) - 1}]")
    return q, int(Q)


def pack_rate_envelope(inner: bytes, quality: float, rate_levels: int) -> bytes:
    q, Q = _rate_quality(quality, rate_levels)
    inner = bytes(inner)
    if len(inner) > 0xFFFFFFFF:
        raise CodecError("the bitstream is too long for its 32-bit length")
    body = _RATE_HEAD.pack(BITSTREAM_MAGIC_RATE, q, Q, 0, len(inner)) + inner
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def is_rate_envelope(data: bytes) -> bool:
    return bytes(data[:8]) == BITSTREAM_MAGIC_RATE


def unpack_rate_envelope(data: bytes, rate_levels: int = None):
    """-> (quality, Q, inner blob).  CodecError, in this order, for a buffer shorter than the envelope, another magic (a
    bare LICBITS blob), an inner length that is not the buffer's, a failing CRC-32, a non-zero pad, Q < 2, q outside
    [0, Q-1] (or no number), and -- `rate_levels` given -- a Q that is not the model's."""
    data = bytes(data)
    if len(data) < _RATE_HEAD.size + 4:
        raise CodecError("rate envelope is truncated (shorter than its header)")
    magic, q, Q, pad, n = _RATE_HEAD.unpack_from(data, 0)
    if magic != BITSTREAM_MAGIC_RATE:
        raise CodecError(f"not a {BITSTREAM_MAGIC_RATE.decode()} rate envelope (bad magic): a rate-level codec reads "
                         "only envelopes")
    if len(data) != _RATE_HEAD.size + n + 4:
        raise CodecError("rate envelope is truncated or has trailing bytes (its length does not match its header)")
    if zlib.crc32(data[:-4]) & 0xFFFFFFFF != struct.unpack_from("<I", data, len(data) - 4)[0]:
        raise CodecError("rate envelope is damaged (CRC-32 mismatch)")
    if pad != 0:
        raise CodecError(f"rate envelope header is damaged (pad word = {pad}, not zero)")
    if Q < 2:
        raise CodecError(f"rate envelope header is damaged (Q = {Q} rate levels)")
    if not 0.0 <= q <= Q - 1:
        raise CodecError(f"rate envelope names quality {q} outside [0, {Q - 1}]")
    if rate_levels is not None and Q != rate_levels:
        raise CodecError(f"rate envelope was written by a model of {Q} rate levels; this model has {rate_levels}")
    return float(q), int(Q), data[_RATE_HEAD.size:_RATE_HEAD.size + n]


def quality_of(blob: bytes) -> float:
    """the quality a rate envelope was coded at"""
    return unpack_rate_envelope(blob)[0]
