"""Entropy coding of the latents.  The reference only ESTIMATES bits
(RateDistortionLoss.py:13-18; no coder or bitstream exists there); this module turns
the same distributions into real byte strings and checks that estimate against them.

Division of labour: the MI355X builds the 16-bit cumulative tables for every latent element in
parallel (`lic_factorized_cdf_tables` from the factorised prior's per-channel CDF,
EntropyModels.py:153-184; `lic_gmm_cdf_tables` from the Gaussian / mixture parameters,
EntropyModels.py:192-233) and the serial range coder runs on the host CPU
(`liblic_codec.so`, include/lic_codec.h), as the north star prescribes.

`LatentCodec`: `compress` (y and z streams), `decompress_z` (the hyper-latent has a parameter-free
prior, so it decodes without context) and `decode_y_with_tables` (decodes y from the tables the encoder
used -- the coder's inverse).  `ContextCodec`: the full round trip; its decoder rebuilds the tables from
already-decoded pixels through the masked 5x5 context model, wavefront by wavefront.
`ContextCodec.compress_image` / `decompress_image` wrap that round trip, for images of any size, in one
self-describing byte string: header, per-image lengths and checksums, streams, CRC-32.  bitstream.py holds the five
containers (LICBITS1/2/3/4, one per coder and grouping, and LICBITS5 for rANS-coded z), their one writer and one reader;
its names are this module's too.

`ContextCodec(..., coder="rans")` codes the y streams with the 64-lane interleaved rANS coder of lic_codec.h
instead: its decoder is a device kernel (`lic_rans_decode_step`), so the decode loop has no host in it.  The range
coder stays the default and codes z, unless `z_coder="rans"` (below).
With `encoder="device"` that coder's encoder runs on the device as well (`lic_rans_encode_pick` + `lic_rans_encode`):
the same bytes, and no table is copied to the host.

`ContextCodec(..., coder="rans", groups=G)` deals every image's rounds to G independent rANS-64 sub-streams
(`rans_deal`: round r of a step goes to sub-stream r % G), so G waves per image decode and encode them
(`lic_rans_decode_step_groups`, `lic_rans_encode_groups`); each sub-stream costs its 256 bytes of states.  G = 1,
the default, is the format above.

`ContextCodec(..., coder="rans", slice_rows=R)` cuts the latent plane into slices of R rows whose contexts do not see
each other, so all slices decode side by side: w + 3 (min(R, h) - 1) dependent steps instead of w + 3 (h - 1), paid
for in rate by the first rows of every slice (DESIGN 1.1 f.2e has the rule).  Both sides build the rows their
per-pixel layers read with one gather, `lic_ctx_gather`, which applies that rule.

`ContextCodec.decompress_images(blobs)` decodes many `compress_image` blobs of different sizes together: step t of
every image shares one gather (`lic_ctx_gather_ragged`), one pass through the per-pixel layers and one decode launch
(`lic_rans_decode_step_ragged`), by the schedule of `merged_wavefront`; entry i is bit for bit `decompress_image(blobs[i])`.

`ContextCodec(..., coder="rans", z_coder="rans")` codes the hyper-latent z on the device as well: every image's z is one
step of all its symbols dealt to the same G sub-streams ("rANS-64 x G"), symbol k using row k % M of the factorised
tables, which `lic_rans_z_decode` keeps in LDS for the whole stream.  `lic_rans_z_pick` + `lic_rans_encode_ragged` encode
(`encoder="host"`: `rans_encode_shared`, the same bytes); `decompress_many` decodes every item's z in one launch ahead
of its step loop and checks the z state blocks in the read-back it already has.  The container is LICBITS5; y streams,
checksums, z_hat, y_hat and x_hat are those of `z_coder="range"`, only the z bytes differ.

`ContextCodec.compress_images(images)` is its counterpart: images of different sizes share one gather, one pass through
the per-pixel layers, one table launch and one launch of each encoder kernel (`lic_rans_encode_pick_ragged`,
`lic_rans_encode_ragged`); entry i is byte for byte `compress_image(images[i])`.

A model built with `context="checkerboard"` decodes in TWO steps whatever its size (`two_pass`): the
anchors -- latent pixels with i + j even -- from the hyperprior alone, then the others from the anchors around them.
Both sides gather every pixel's window from anchor(y_hat); the decoder's plane starts as zeros, so step 0 reads zeros
and step 1 only anchors, through the same gather, per-pixel layers, table and rANS kernels as the raster schedule.
`CodecLayer` reads the schedule off the mask; such a codec needs coder="rans", has no slices, and its container is
LICBITS7, which a raster codec refuses as this one refuses LICBITS1 to 5.

`ScalableCodec` is the codec of `models.ScalableImageCoding`: base and enhancement latent are two layers (`CodecLayer`)
with their own rANS sub-streams, the container (LICBITS6) puts the base layer first, and `decompress_base` /
`decompress_base_image` decode z and the base layer alone.  `_LayeredCodec` holds what it shares with `ContextCodec`,
the one-layer case: gather, front end and step loop over a list of layers (`lic_ctx_gather_layers`,
`lic_rans_decode_step_layers`: all layers of a step in one launch each), the decode of many bitstreams in one loop
(`_decompress_many`), the z coder and the y encoders.  The layouts of the ragged calls are pure numpy functions here:
`merged_wavefront`, `ragged_encode_plan`, `plane_layout`, `z_plan`, and `rans_block_layout` for the slots of every
encode.  Every device encode (y of one item, y of a chunk, z) builds its inputs and leaves buffers and launches to
`_RansEncoding` and the one read-back to `rans_read_back` (host half: `rans_streams_of`), as every decode leaves them to
`_RansStaging`.
"""
from __future__ import annotations

import ctypes as C
import functools
import struct
import zlib
import os
from typing import Dict, List, NamedTuple, Sequence

import numpy as np
import torch

from . import _lib as L
from . import functional as F_
from .bitstream import (BITSTREAM_FAMILIES, BITSTREAM_MAGIC, BITSTREAM_MAGIC_GROUPED,  # noqa: F401
                        BITSTREAM_MAGIC_RANS, BITSTREAM_MAGIC_SLICED, BITSTREAM_MAGIC_ZRANS, RANS_LANES, RANS_MAX_GROUPS,
                        CodecError, BITSTREAM_MAGIC_CHECKER, _FORMAT_CHECKER, pack_bitstream_checker,
                        unpack_bitstream_checker,
                        BITSTREAM_MAGIC_LAYERED, _BITS_HEAD_LAYERED,
                        _BITS_FIELDS, _BITS_HEAD, _BITS_HEAD_RANS, _FORMAT_OF_MAGIC, _FORMAT_ZRANS, _FORMATS,
                        _check_crc_and_head, _format_of_magic, is_rate_envelope, pack_rate_envelope, quality_of,
                        unpack_rate_envelope,
                        _groups, _pack, _unpack, pack_bitstream, pack_bitstream_grouped, pack_bitstream_layered,
                        pack_bitstream_rans,
                        pack_bitstream_sliced, pack_bitstream_zrans, unpack_bitstream, unpack_bitstream_grouped,
                        unpack_bitstream_layered, unpack_bitstream_layered_base,
                        unpack_bitstream_rans, unpack_bitstream_sliced, unpack_bitstream_zrans)

_CODEC = None


def _codec():
    global _CODEC
    if _CODEC is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "liblic_codec.so")
        if not os.path.exists(path):
            raise CodecError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(path)
        u32p, i32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        lib.lic_rc_bound.restype, lib.lic_rc_bound.argtypes = C.c_size_t, [C.c_int64]
        lib.lic_rc_encode.restype = C.c_int
        lib.lic_rc_encode.argtypes = [u32p, i32p, C.c_int32, i32p, C.c_int64, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.lic_rc_decode.restype = C.c_int
        lib.lic_rc_decode.argtypes = [u8p, C.c_size_t, u32p, i32p, C.c_int32, C.c_int64, i32p]
        lib.lic_rc_ideal_bits.restype = C.c_double
        lib.lic_rc_ideal_bits.argtypes = [u32p, i32p, C.c_int32, i32p, C.c_int64]
        lib.lic_codec_version.restype = C.c_int
        lib.lic_rc_decoder_new.restype, lib.lic_rc_decoder_new.argtypes = C.c_void_p, [u8p, C.c_size_t]
        lib.lic_rc_decoder_next.restype = C.c_int
        lib.lic_rc_decoder_next.argtypes = [C.c_void_p, u32p, i32p, C.c_int32, C.c_int64, i32p]
        lib.lic_rc_decoder_free.argtypes = [C.c_void_p]
        i64p, szp = C.POINTER(C.c_int64), C.POINTER(C.c_size_t)
        lib.lic_rans_bound.restype, lib.lic_rans_bound.argtypes = C.c_size_t, [C.c_int64]
        lib.lic_rans_encode.restype = C.c_int
        lib.lic_rans_encode.argtypes = [u32p, C.c_int32, i32p, C.c_int64, i64p, C.c_int64, u8p, C.c_size_t, szp, u32p,
                                        C.c_size_t, szp]
        lib.lic_rans_decode.restype = C.c_int
        lib.lic_rans_decode.argtypes = [u8p, C.c_size_t, u32p, C.c_size_t, u32p, C.c_int32, C.c_int64, i64p, C.c_int64,
                                        i32p]
        lib.lic_rans_ideal_bits.restype = C.c_double
        lib.lic_rans_ideal_bits.argtypes = [u32p, i32p, C.c_int32, i32p, C.c_int64]
        lib.lic_rans_encode_shared.restype = C.c_int
        lib.lic_rans_encode_shared.argtypes = [u32p, i32p, C.c_int32, C.c_int32, i32p, C.c_int64, i64p, C.c_int64, u8p,
                                               C.c_size_t, szp, u32p, C.c_size_t, szp]
        lib.lic_rans_decode_shared.restype = C.c_int
        lib.lic_rans_decode_shared.argtypes = [u8p, C.c_size_t, u32p, C.c_size_t, u32p, i32p, C.c_int32, C.c_int32,
                                               C.c_int64, i64p, C.c_int64, i32p]
        _CODEC = lib
    return _CODEC


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def rc_encode(tables: np.ndarray, idx: np.ndarray, table_of: np.ndarray = None) -> bytes:
    """tables [T][S+1] uint32, idx [n] int32 (value - window_lo), table_of [n] int32 or None (T == n)."""
    tables = np.ascontiguousarray(tables, np.uint32)
    idx = np.ascontiguousarray(idx, np.int32).ravel()
    tof = None if table_of is None else np.ascontiguousarray(table_of, np.int32).ravel()
    S = tables.shape[-1] - 1
    lib = _codec()
    cap = lib.lic_rc_bound(idx.size)
    out = np.empty(cap, np.uint8)
    nb = C.c_size_t(0)
    rc = lib.lic_rc_encode(_p(tables, C.c_uint32), _p(tof, C.c_int32), S, _p(idx, C.c_int32), idx.size,
                           _p(out, C.c_uint8), cap, C.byref(nb))
    if rc != 0:
        raise CodecError(f"lic_rc_encode failed with status {rc}")
    return out[:nb.value].tobytes()


def rc_decode(data: bytes, tables: np.ndarray, n: int, table_of: np.ndarray = None) -> np.ndarray:
    tables = np.ascontiguousarray(tables, np.uint32)
    tof = None if table_of is None else np.ascontiguousarray(table_of, np.int32).ravel()
    S = tables.shape[-1] - 1
    buf = np.frombuffer(data, np.uint8)
    out = np.empty(n, np.int32)
    rc = _codec().lic_rc_decode(_p(buf, C.c_uint8), buf.size, _p(tables, C.c_uint32), _p(tof, C.c_int32), S, n,
                                _p(out, C.c_int32))
    if rc != 0:
        raise CodecError(f"lic_rc_decode failed with status {rc}")
    return out


def rc_ideal_bits(tables: np.ndarray, idx: np.ndarray, table_of: np.ndarray = None) -> float:
    tables = np.ascontiguousarray(tables, np.uint32)
    idx = np.ascontiguousarray(idx, np.int32).ravel()
    tof = None if table_of is None else np.ascontiguousarray(table_of, np.int32).ravel()
    return float(_codec().lic_rc_ideal_bits(_p(tables, C.c_uint32), _p(tof, C.c_int32), tables.shape[-1] - 1,
                                            _p(idx, C.c_int32), idx.size))


# ---- the interleaved rANS coder of the y streams (lic_codec.h "rANS-64") ---------------------
CODERS = ("range", "rans")
ENCODERS = ("host", "device")
Z_CODERS = ("range", "rans")                     # who codes the hyper-latent z: the host range coder, or rANS-64 x G kernels
RANS_MAX_W = 64                                  # widest window lic_rans_decode_step / lic_rans_encode_pick take


def rans_encode(tables: np.ndarray, idx: np.ndarray, step_len) -> tuple:
    """tables [n][S+1] uint32 (one per symbol), idx [n] int32, step_len: symbols per wavefront step (sums to n)
    -> (stream bytes, escape list bytes: little-endian uint32, in symbol order)"""
    tables = np.ascontiguousarray(tables, np.uint32)
    idx = np.ascontiguousarray(idx, np.int32).ravel()
    steps = np.ascontiguousarray(step_len, np.int64).ravel()
    S = tables.shape[-1] - 1
    lib = _codec()
    cap = lib.lic_rans_bound(idx.size)
    out, esc = np.empty(cap, np.uint8), np.empty(max(idx.size, 1), np.dtype("<u4"))
    nb, ne = C.c_size_t(0), C.c_size_t(0)
    rc = lib.lic_rans_encode(_p(tables, C.c_uint32), S, _p(idx, C.c_int32), idx.size, _p(steps, C.c_int64), steps.size,
                             _p(out, C.c_uint8), cap, C.byref(nb), _p(esc, C.c_uint32), idx.size, C.byref(ne))
    if rc != 0:
        raise CodecError(f"lic_rans_encode failed with status {rc}")
    return out[:nb.value].tobytes(), esc[:ne.value].tobytes()


def rans_decode(data: bytes, esc: bytes, tables: np.ndarray, step_len) -> np.ndarray:
    """the inverse of `rans_encode` for known tables"""
    tables = np.ascontiguousarray(tables, np.uint32)
    steps = np.ascontiguousarray(step_len, np.int64).ravel()
    n = int(steps.sum())
    S = tables.shape[-1] - 1
    if len(esc) % 4:
        raise CodecError("escape list is not a whole number of uint32")
    buf = np.frombuffer(data, np.uint8)
    ebuf = np.frombuffer(esc, np.dtype("<u4")).astype(np.uint32)
    out = np.empty(n, np.int32)
    rc = _codec().lic_rans_decode(_p(buf, C.c_uint8), buf.size, _p(ebuf, C.c_uint32), ebuf.size, _p(tables, C.c_uint32),
                                  S, n, _p(steps, C.c_int64), steps.size, _p(out, C.c_int32))
    if rc != 0:
        raise CodecError(f"lic_rans_decode failed with status {rc}")
    return out


def rans_encode_shared(tables: np.ndarray, idx: np.ndarray, step_len, table_of: np.ndarray = None) -> tuple:
    """`rans_encode` for symbols that share tables, `rc_encode`'s convention: tables [T][S+1] uint32, table_of [n] int32
    (None: table n, which is `rans_encode`) -> (stream bytes, escape list bytes)"""
    tables = np.ascontiguousarray(tables, np.uint32)
    idx = np.ascontiguousarray(idx, np.int32).ravel()
    steps = np.ascontiguousarray(step_len, np.int64).ravel()
    tof = None if table_of is None else np.ascontiguousarray(table_of, np.int32).ravel()
    if tof is not None and tof.size != idx.size:
        raise CodecError("one table_of entry per symbol expected")
    T, S = tables.shape[0], tables.shape[-1] - 1
    lib = _codec()
    cap = lib.lic_rans_bound(idx.size)
    out, esc = np.empty(cap, np.uint8), np.empty(max(idx.size, 1), np.dtype("<u4"))
    nb, ne = C.c_size_t(0), C.c_size_t(0)
    rc = lib.lic_rans_encode_shared(_p(tables, C.c_uint32), _p(tof, C.c_int32), T, S, _p(idx, C.c_int32), idx.size,
                                    _p(steps, C.c_int64), steps.size, _p(out, C.c_uint8), cap, C.byref(nb),
                                    _p(esc, C.c_uint32), idx.size, C.byref(ne))
    if rc != 0:
        raise CodecError(f"lic_rans_encode_shared failed with status {rc}")
    return out[:nb.value].tobytes(), esc[:ne.value].tobytes()


def rans_decode_shared(data: bytes, esc: bytes, tables: np.ndarray, step_len, table_of: np.ndarray = None) -> np.ndarray:
    """the inverse of `rans_encode_shared` for known tables"""
    tables = np.ascontiguousarray(tables, np.uint32)
    steps = np.ascontiguousarray(step_len, np.int64).ravel()
    n = int(steps.sum())
    tof = None if table_of is None else np.ascontiguousarray(table_of, np.int32).ravel()
    if tof is not None and tof.size != n:
        raise CodecError("one table_of entry per symbol expected")
    T, S = tables.shape[0], tables.shape[-1] - 1
    if len(esc) % 4:
        raise CodecError("escape list is not a whole number of uint32")
    buf = np.frombuffer(data, np.uint8)
    ebuf = np.frombuffer(esc, np.dtype("<u4")).astype(np.uint32)
    out = np.empty(n, np.int32)
    rc = _codec().lic_rans_decode_shared(_p(buf, C.c_uint8), buf.size, _p(ebuf, C.c_uint32), ebuf.size,
                                         _p(tables, C.c_uint32), _p(tof, C.c_int32), T, S, n, _p(steps, C.c_int64),
                                         steps.size, _p(out, C.c_int32))
    if rc != 0:
        raise CodecError(f"lic_rans_decode_shared failed with status {rc}")
    return out


def rans_deal(step_len, G: int):
    """The "rANS-64 x G" format (lic_codec.h): symbol k of a step lies in round k // 64 of that step, and round r of
    every step belongs to sub-stream r % G.  step_len: symbols per step of one image, in coding order.
    -> [(positions, step_len_g) for g in range(G)]: the positions (int64, ascending) of sub-stream g's symbols in the
    image's coding order, and how many of them every step contributes (int64, one entry per step, zeros included)."""
    G = _groups(G)
    steps = np.ascontiguousarray(step_len, np.int64).ravel()
    if (steps < 0).any():
        raise CodecError("negative step length")
    pos = np.arange(int(steps.sum()), dtype=np.int64)
    step_of = np.repeat(np.arange(steps.size, dtype=np.int64), steps)
    in_step = pos - np.repeat(np.cumsum(steps) - steps, steps)
    group_of = (in_step // RANS_LANES) % G
    counts = np.bincount(step_of * G + group_of, minlength=steps.size * G).reshape(steps.size, G).astype(np.int64)
    return [(pos[group_of == g], np.ascontiguousarray(counts[:, g])) for g in range(G)]


def rans_group_sizes(step_len, G: int) -> np.ndarray:
    """[G] int64: the symbols of every sub-stream of `rans_deal(step_len, G)`, from the step lengths alone.  Of a
    step's R rounds, (R + G - 1 - g) // G are group g's; all are full but the step's last, round R - 1."""
    G = _groups(G)
    n = np.ascontiguousarray(step_len, np.int64).ravel()[:, None]
    R = (n + RANS_LANES - 1) // RANS_LANES
    g = np.arange(G, dtype=np.int64)[None, :]
    short = np.where((n % RANS_LANES != 0) & ((R - 1) % G == g), RANS_LANES - n % RANS_LANES, 0)
    return (RANS_LANES * ((R + G - 1 - g) // G) - short).sum(0)


def rans_encode_grouped(tables: np.ndarray, idx: np.ndarray, step_len, G: int) -> tuple:
    """`rans_encode` per sub-stream of `rans_deal` -> ([G stream bytes], [G escape-list bytes])"""
    tables = np.ascontiguousarray(tables, np.uint32)
    idx = np.ascontiguousarray(idx, np.int32).ravel()
    pairs = [rans_encode(tables[pos], idx[pos], steps_g) for pos, steps_g in rans_deal(step_len, G)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def rans_decode_grouped(streams, escs, tables: np.ndarray, step_len) -> np.ndarray:
    """the inverse of `rans_encode_grouped` for known tables; G = len(streams)"""
    if len(streams) != len(escs):
        raise CodecError("one escape list per sub-stream expected")
    tables = np.ascontiguousarray(tables, np.uint32)
    out = np.empty(int(np.asarray(step_len, np.int64).sum()), np.int32)
    for (pos, steps_g), data, esc in zip(rans_deal(step_len, len(streams)), streams, escs):
        out[pos] = rans_decode(data, esc, tables[pos], steps_g)
    return out


def rans_ideal_bits(tables: np.ndarray, idx: np.ndarray) -> float:
    tables = np.ascontiguousarray(tables, np.uint32)
    idx = np.ascontiguousarray(idx, np.int32).ravel()
    return float(_codec().lic_rans_ideal_bits(_p(tables, C.c_uint32), None, tables.shape[-1] - 1, _p(idx, C.c_int32),
                                              idx.size))


# ---- device side: tables --------------------------------------------------------------------
def factorized_tables(fe_model, lo: int, S: int) -> torch.Tensor:
    """[C][S+1] uint32 (as int64-safe torch.int32 view) for symbols lo .. lo+S-1 of every channel."""
    params = fe_model.packed_params().detach().contiguous()
    Cc = params.shape[0]
    out = torch.empty((Cc, S + 1), device=params.device, dtype=torch.int32)
    L.check(L.load().lic_factorized_cdf_tables(F_._ptr(params), Cc, int(lo), int(S), F_._ptr(out), F_._stream()),
            "lic_factorized_cdf_tables")
    return out


def gmm_tables(act: torch.Tensor, M: int, K: int, W: int):
    """act: the packed activated parameters [B,G*K*M,h,w] (EntropyParameters.packed); returns
    (center [B,h,w,M] int32, tables [B*h*w*M][2W+2] int32-viewed uint32)."""
    a = F_._nhwc(act.detach())  # [B,h,w,G*K*M] contiguous
    P = a.numel() // a.shape[-1]
    center = torch.empty((P, M), device=a.device, dtype=torch.int32)
    tables = torch.empty((P * M, 2 * W + 2), device=a.device, dtype=torch.int32)
    L.check(L.load().lic_gmm_cdf_tables(F_._ptr(a), P, M, K, int(W), F_._ptr(center), F_._ptr(tables), F_._stream()),
            "lic_gmm_cdf_tables")
    return center, tables


def _slice_rows(R) -> int:
    """R as an int >= 1 (latent rows per slice), or CodecError"""
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or int(R) < 1:
        raise CodecError(f"slice_rows = {R!r}: expected None (no slices) or an integer of at least 1")
    return int(R)


def wavefront(h: int, w: int, pad: int, slice_rows: int = None):
    """The decode schedule of an h x w latent plane under a causal mask of half-width `pad`, cut into slices of
    `slice_rows` rows (None: one slice).  Pixel (i, j) belongs to step t = j + (pad + 1) * (i mod R): its own row's
    taps lie in earlier steps, and so do the rows above it INSIDE its slice up to column j + pad; rows above the slice
    are not context (ContextCodec).  -> [(rows, cols)] per step, rows ascending: w + (pad + 1)(min(R, h) - 1) steps."""
    k = pad + 1
    R = h if slice_rows is None else min(_slice_rows(slice_rows), h)
    rows = np.arange(h, dtype=np.int64)
    steps = []
    for t in range(w + k * (R - 1)):
        jj = t - k * (rows % R)
        keep = (jj >= 0) & (jj < w)
        if keep.any():
            steps.append((rows[keep], jj[keep]))
    return steps


SCHEDULES = ("raster", "checkerboard")


def two_pass(h: int, w: int):
    """The decode schedule of an h x w latent plane under the checkerboard context: step 0 holds the anchors (i + j
    even), step 1 the other pixels, each in raster order; a plane of one pixel has one step.  -> [(rows, cols)] per
    step, as `wavefront`."""
    i, j = np.repeat(np.arange(h, dtype=np.int64), w), np.tile(np.arange(w, dtype=np.int64), h)
    odd = ((i + j) & 1).astype(bool)
    return [(i[keep], j[keep]) for keep in (~odd, odd) if keep.any()]


def _schedule(schedule) -> str:
    if schedule not in SCHEDULES:
        raise CodecError(f"unknown schedule {schedule!r}: expected one of {SCHEDULES}")
    return schedule


def _steps_of(h: int, w: int, pad: int, slice_rows, schedule: str):
    """`wavefront` or `two_pass`, by the schedule (a checkerboard plane has no slices)"""
    if _schedule(schedule) == "raster":
        return wavefront(h, w, pad, slice_rows)
    if slice_rows is not None:
        raise CodecError(f"slice_rows = {slice_rows!r}: the checkerboard schedule has no slices")
    return two_pass(h, w)


def _z_size(strings) -> int:
    """bytes of the coded hyper-latent in `compress`'s strings: one stream, or sub-streams and escape lists"""
    if strings.get("z_coder", "range") == "rans":
        return sum(len(s) for s in strings["z"]) + sum(len(e) for e in strings["z_esc"])
    return len(strings["z"])


def _image_name(img: int) -> str:
    return f"image {img}"


def _state_blocks(d_state: torch.Tensor, G: int, problem, name=_image_name):
    """The one read-back of a rANS kernel's state blocks [blocks][RANS_STATE_WORDS] (lic.h: 64 coder states, word
    count, escape count, error word), image-major with G blocks per image -> [(states uint32 [64], words, escapes)].
    `problem(i, states, words, escapes, error word)` says what is wrong with block i, if anything: the first such
    block raises CodecError, named by its image (`name(image)`, `_image_name` by default)."""
    blocks = []
    for i, row in enumerate(d_state.cpu().numpy().view(np.uint32)):
        blocks.append((row[:RANS_LANES], int(row[RANS_LANES]), int(row[RANS_LANES + 1])))
        what = problem(i, *blocks[-1], int(row[RANS_LANES + 2]))
        if what:
            raise CodecError(f"{name(i // G)}: {what}")
    return blocks


class MergedSchedule(NamedTuple):
    """what `merged_wavefront` returns, uploaded once per call.  Image b's step lengths, as `compress` orders its
    symbols and `rans_deal` reads them, are seg[:, b, 1] * M up to the image's last step."""
    T: int                    # steps of the call: the largest step count of any image
    seg: np.ndarray           # [T][nimg][2] int32: (first row, rows) of image b inside step t's row batch
    rows: np.ndarray          # [3][sum of h*w] int64, steps concatenated: image index, raster pixel index inside the
    #                           image, destination pixel index inside its zero-framed (h + 2 pad) x (w + 2 pad) plane
    step_off: np.ndarray      # [T + 1] int64: step t's rows are rows[:, step_off[t]:step_off[t + 1]]


def merged_wavefront(shapes, pad: int, slice_rows_list, schedule: str = "raster") -> MergedSchedule:
    """The decode schedule of several latent planes advanced together.  shapes: [(h, w)] per image; slice_rows_list:
    each image's slice_rows (None: no slices).  Step t of the call is step t of every image that still has one, images
    in list order; inside an image the order is exactly `wavefront(h, w, pad, R)`'s -- `two_pass(h, w)`'s for
    schedule "checkerboard" (every entry of slice_rows_list None), so T = 2 unless every plane is one pixel.  An image
    that has finished keeps a segment of 0 rows whose first row is the running sum, so every segment is well defined.
    No loop over steps: every pixel gets its step number, and one stable sort by (step, image) of the pixels in
    raster order, image after image, leaves them step by step, image by image, rows ascending."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    slice_rows_list = list(slice_rows_list)
    if len(slice_rows_list) != len(shapes):
        raise CodecError("one slice_rows entry per image expected")
    nimg, k = len(shapes), pad + 1
    checker = _schedule(schedule) == "checkerboard"
    if checker and any(R is not None for R in slice_rows_list):
        raise CodecError("slice_rows: the checkerboard schedule has no slices")
    kinds, per = {}, []                                          # images of one shape and slice height share their arrays
    for (h, w), R in zip(shapes, slice_rows_list):
        if (h, w, R) not in kinds:
            Reff = h if R is None else min(_slice_rows(R), h)
            i, j = np.repeat(np.arange(h, dtype=np.int64), w), np.tile(np.arange(w, dtype=np.int64), h)
            # `wavefront` leaves out the steps that hold no pixel (w < pad + 1 only): number the ones that remain
            # (`two_pass`: the parity is the step; a plane of one pixel has step 0 only)
            _, t = np.unique((i + j) & 1 if checker else j + k * (i % Reff), return_inverse=True)
            kinds[h, w, R] = (t.astype(np.int64).ravel(), i * w + j, (i + pad) * (w + 2 * pad) + j + pad)
        per.append(kinds[h, w, R])
    if not per:
        return MergedSchedule(0, np.zeros((0, 0, 2), np.int32), np.zeros((3, 0), np.int64), np.zeros(1, np.int64))
    step = np.concatenate([a[0] for a in per])
    image = np.repeat(np.arange(nimg, dtype=np.int64), [a[0].size for a in per])
    T = int(step.max()) + 1
    key = step * nimg + image
    order = np.argsort(key, kind="stable")
    rows = np.stack([image, np.concatenate([a[1] for a in per]), np.concatenate([a[2] for a in per])])[:, order]
    count = np.bincount(key, minlength=T * nimg).reshape(T, nimg)
    seg = np.stack([np.cumsum(count, 1) - count, count], 2).astype(np.int32)
    step_off = np.concatenate([[0], np.cumsum(count.sum(1))]).astype(np.int64)
    return MergedSchedule(T, seg, np.ascontiguousarray(rows), step_off)


def _step_indices(steps, w: int, pad: int) -> np.ndarray:
    """[2][pixels] int64 for the steps of one plane (`wavefront`), concatenated: the raster index i * w + j of every
    pixel and its index inside the zero-framed (h + 2 pad) x (w + 2 pad) plane"""
    Wp = w + 2 * pad
    return np.stack([np.concatenate([ii * w + jj for ii, jj in steps]),
                     np.concatenate([(ii + pad) * Wp + jj + pad for ii, jj in steps])])


class RaggedEncodePlan(NamedTuple):
    """what `ragged_encode_plan` returns: the arguments of `lic_rans_encode_pick_ragged` / `lic_rans_encode_ragged`
    that the host knows before the device has run (lic.h has the descriptor words)"""
    images: np.ndarray        # [nimg][4] int64: ROW0, P, STEP0, NSTEPS
    blocks: np.ndarray        # [nimg * G][4] int64, image-major: WORD_OFF (bytes), SLOT (bytes), ESC_OFF, ESC_CAP (entries)
    row_image: np.ndarray     # [total_rows] int64: the image of every row, which is the image of every coding position
    order: np.ndarray         # [total_rows] int64: the raster pixel, inside its image, of every coding position
    step_len: np.ndarray      # int64, the images' step lengths one after the other
    total_rows: int
    words_len: int            # bytes of all slots
    esc_len: int              # entries of all escape lists


def rans_block_layout(fullest, G: int, head: int = 0):
    """The block table of one encode: the one rule for slots and escape lists.  fullest: per image, the symbols of its
    fullest sub-stream (`rans_group_sizes(step_len, G).max()`; an image without symbols counts as 1).  Every one of an
    image's G blocks gets the smallest slot and escape list that cannot run out -- one 16-bit word and one escape per
    symbol at the most (lic.h): head + 2 * fullest bytes rounded up to 4, and fullest entries --, one behind the other,
    so every slot starts on a multiple of 4 bytes.  head: 0 for the ragged entries; 4 * RANS_LANES for the single-item
    kernels, whose slots are `lic_rans_bound`'s and, the images being of one size, uniform.
    -> (blocks [nimg * G][4] int64, image-major: WORD_OFF (bytes), SLOT (bytes), ESC_OFF, ESC_CAP (entries);
        words_len: bytes of all slots; esc_len: entries of all escape lists)"""
    cap = np.repeat(np.maximum(np.asarray(fullest, np.int64).ravel(), 1), _groups(G))
    slot = (head + 2 * cap + 3) // 4 * 4
    return np.stack([np.cumsum(slot) - slot, slot, np.cumsum(cap) - cap, cap], 1), int(slot.sum()), int(cap.sum())


@functools.lru_cache(maxsize=64)
def _encode_layout_of(h: int, w: int, M: int, pad: int, slice_rows, G: int, schedule: str = "raster"):
    """what `compress` and `ragged_encode_plan` need of one image shape, kept between calls (a folder has few shapes;
    the arrays are read only): (raster pixel of every coding position, step lengths, symbols of the fullest sub-stream)"""
    steps = _steps_of(h, w, pad, slice_rows, schedule)
    step_len = np.array([len(ii) * M for ii, _ in steps], np.int64)
    order = np.concatenate([ii * w + jj for ii, jj in steps]).astype(np.int64)
    order.setflags(write=False)
    step_len.setflags(write=False)
    return order, step_len, int(rans_group_sizes(step_len, G).max())


def ragged_encode_plan(shapes, M: int, pad: int, slice_rows, G: int, schedule: str = "raster") -> RaggedEncodePlan:
    """The layout of one ragged encode.  shapes: [(h, w)] per image, all coded with this `slice_rows` and G (schedule
    "checkerboard": `two_pass(h, w)` where this text says `wavefront`, slice_rows None).  Image b
    owns rows [ROW0, ROW0 + h w) of the tables, centres and symbols, in raster order, and the same range of coding
    positions: position ROW0 + q is pixel `wavefront(h, w, pad, slice_rows)`[concatenated][q], its step lengths are
    len(rows_t) * M, exactly `compress`'s.  Slots and escape lists are `rans_block_layout`'s."""
    G = _groups(G)
    shapes = [(int(h), int(w)) for h, w in shapes]
    kinds = {(h, w): _encode_layout_of(h, w, int(M), int(pad), slice_rows, G, _schedule(schedule)) for h, w in set(shapes)}
    nimg = len(shapes)
    images = np.zeros((nimg, L.RANS_IMAGE_WORDS), np.int64)
    row0 = step0 = 0
    for b, (h, w) in enumerate(shapes):
        order, step_len, _ = kinds[h, w]
        images[b] = (row0, order.size, step0, step_len.size)
        row0, step0 = row0 + order.size, step0 + step_len.size
    blocks, words_len, esc_len = rans_block_layout([kinds[s][2] for s in shapes], G)
    cat = lambda k: (np.concatenate([kinds[s][k] for s in shapes]) if nimg else np.zeros(0, np.int64))
    return RaggedEncodePlan(images, blocks, np.repeat(np.arange(nimg, dtype=np.int64), images[:, 1]), cat(0), cat(1),
                            row0, words_len, esc_len)


def z_encode_plan(pixels, M: int, G: int):
    """`lic_rans_encode_ragged`'s layout for the hyper-latents of several images (z_coder="rans"): image b is pixels[b]
    rows of M symbols in raster order and ONE step of pixels[b] * M symbols; slots and escape lists are
    `rans_block_layout`'s.
    -> (images [nimg][4], blocks [nimg * G][4], step_len [nimg], total_rows, words_len, esc_len), as RaggedEncodePlan"""
    G = _groups(G)
    step_len = np.array([int(P) * M for P in pixels], np.int64)
    images = np.zeros((len(pixels), L.RANS_IMAGE_WORDS), np.int64)
    images[:, 1], images[:, 2], images[:, 3] = step_len // M, np.arange(len(pixels)), 1
    images[:, 0] = np.cumsum(images[:, 1]) - images[:, 1]
    blocks, words_len, esc_len = rans_block_layout([rans_group_sizes([n], G).max() for n in step_len], G)
    return images, blocks, step_len, int(images[:, 1].sum()), words_len, esc_len


class PlaneLayout(NamedTuple):
    """what `plane_layout` returns: where the planes of every item lie in the two flat fp32 buffers of a ragged call"""
    y_at: np.ndarray          # [items] int64: the float of the latent buffer item i's first plane starts at
    psi_at: np.ndarray        # [items] int64: likewise in the psi buffer
    y_len: int                # floats of the latent buffer
    psi_len: int              # floats of the psi buffer
    desc: np.ndarray          # [nimg][CTX_IMAGE_WORDS] int64 (lic.h): Y_BASE, Y_ROW, Y_ORIGIN, PSI_BASE, H, W, R, 0
    pixels: np.ndarray        # [nimg] int64: the pixels of every framed plane, (h + 2 frame)(w + 2 frame)


def plane_layout(items, y_pix: int, cpsi: int, frame: int, slice_rows_list) -> PlaneLayout:
    """The flat buffers of the ragged kernels.  items: [(B, h, w)]; item after item, each on a multiple of 4 floats of
    either buffer, its B planes one behind the other: latent planes of y_pix floats per pixel inside a zero frame of
    `frame` pixels (the codec's pad when decoding, 0 when encoding: plain NHWC planes), psi planes of cpsi floats per
    pixel without a frame.  slice_rows_list: the slice_rows of every IMAGE (None: no slices), items' images in order.
    Image b of an item gets the descriptor (first float of its plane, floats per framed row, the float of pixel (0, 0)
    inside the plane, first float of its psi plane, h, w, min(R, h))."""
    items = [(int(B), int(h), int(w)) for B, h, w in items]
    slice_rows_list = list(slice_rows_list)
    nimg = sum(B for B, _, _ in items)
    if len(slice_rows_list) != nimg:
        raise CodecError("one slice_rows entry per image expected")
    y_at, psi_at = np.zeros(len(items), np.int64), np.zeros(len(items), np.int64)
    desc, pixels = np.zeros((nimg, L.CTX_IMAGE_WORDS), np.int64), np.zeros(nimg, np.int64)
    y_len = psi_len = img = 0
    for i, (B, h, w) in enumerate(items):
        y_at[i], psi_at[i] = (y_len + 3) // 4 * 4, (psi_len + 3) // 4 * 4
        Wp, plane = w + 2 * frame, (h + 2 * frame) * (w + 2 * frame)
        for b in range(B):
            R = slice_rows_list[img]
            desc[img, :7] = (y_at[i] + b * plane * y_pix, Wp * y_pix, (frame * Wp + frame) * y_pix,
                             psi_at[i] + b * h * w * cpsi, h, w, h if R is None else min(R, h))
            pixels[img] = plane
            img += 1
        y_len, psi_len = int(y_at[i]) + B * plane * y_pix, int(psi_at[i]) + B * h * w * cpsi
    return PlaneLayout(y_at, psi_at, y_len, psi_len, desc, pixels)


class ZPlan(NamedTuple):
    """what `z_plan` returns: `lic_rans_z_decode`'s per-image arguments and where every item's z lies"""
    windows: list             # (z_lo, z_S) per image
    nsyms: list               # its symbols
    bases: list               # the float of the flat z buffer its plane starts at
    z_len: int                # floats of that buffer
    at: list                  # per item: the float its first plane starts at; None for an item without rANS-coded z


def z_plan(z_items, M: int) -> ZPlan:
    """The flat buffer the rANS-coded hyper-latents of a call are decoded into.  z_items: per item (z_shape, (z_lo,
    z_S)), or None for an item whose z is range-coded and takes no room.  Item after item, each on a multiple of 4
    floats, its B planes of h4 * w4 * M floats (pixel by pixel, channel by channel) one behind the other."""
    windows, nsyms, bases, at, z_len = [], [], [], [], 0
    for entry in z_items:
        if entry is None:
            at.append(None)
            continue
        (B, _, h4, w4), win = entry
        z_len = (z_len + 3) // 4 * 4
        at.append(z_len)
        for b in range(B):
            windows.append((int(win[0]), int(win[1])))
            nsyms.append(h4 * w4 * M)
            bases.append(z_len)
            z_len += h4 * w4 * M
    return ZPlan(windows, nsyms, bases, z_len, at)


def _crc32_of(a) -> int:
    """CRC-32 of an array's elements in C order: the checksum of an image's latent symbols (int32)"""
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _check_latents(got: np.ndarray, c0: int, c1: int, want, what: str = ""):
    """got [B, h, w, channels] int32: the rounded decoded latents; want [B]: the encoder's CRC-32 of channels [c0, c1)
    of every image.  A decoder whose tables differ from the encoder's by one count decodes garbage silently; with the
    checksum it fails loudly instead, naming the image and `what` (", layer l" for a layered codec)."""
    for b in range(got.shape[0]):
        if _crc32_of(got[b, :, :, c0:c1]) != int(want[b]):
            raise CodecError(f"image {b}{what}: decoded latents do not match the encoder's checksum "
                             "(encoder and decoder built different probability tables, or the stream is damaged)")


def table_chunks(costs, budget: int):
    """Consecutive runs [(first, end)] of whole items whose costs (table bytes) add up to `budget` at the most; an
    item that is larger than the budget runs alone."""
    chunks, first, used = [], 0, 0
    for i, c in enumerate(costs):
        if i > first and used + c > budget:
            chunks.append((first, i))
            first, used = i, 0
        used += c
    if len(costs) > first:
        chunks.append((first, len(costs)))
    return chunks


class _RansStaging:
    """The streams, escape lists and state blocks of `nimg * G` rANS blocks (image-major) as the decode kernels take
    them: every stream on a 4-byte boundary of one buffer, offsets, lengths and seeds in one array each.  The
    constructor is host only and refuses what cannot be staged; `upload` sends the six arrays once; `check` is the one
    read-back after the last step.  `name(image)` labels an image in the messages."""

    def __init__(self, ys, escs, nimg: int, G: int, name=_image_name):
        B = nimg * G
        if escs is None or len(ys) != B or len(escs) != B:
            raise CodecError("one y stream and one escape list per image and group expected")
        head = 4 * RANS_LANES
        for b in range(B):
            if len(ys[b]) < head or len(ys[b]) % 2 or len(escs[b]) % 4:
                raise CodecError(f"{name(b // G)}: y stream or escape list has an impossible length")
        # staging: every stream starts on a 4-byte boundary; offsets, lengths and seeds in one upload each
        s_off = np.zeros(B + 1, np.int64)
        for b in range(B):
            s_off[b + 1] = s_off[b] + (len(ys[b]) + 3) // 4 * 4
        s_len = np.array([len(s) for s in ys], np.int64)
        buf = np.zeros(int(s_off[B]), np.uint8)
        state = np.zeros((B, L.RANS_STATE_WORDS), np.uint32)
        for b in range(B):
            buf[s_off[b]:s_off[b] + len(ys[b])] = np.frombuffer(ys[b], np.uint8)
            state[b, :RANS_LANES] = np.frombuffer(ys[b][:head], np.dtype("<u4"))
        e_off = np.concatenate([[0], np.cumsum([len(e) // 4 for e in escs])]).astype(np.int64)
        e_all = np.frombuffer(b"".join(escs) + b"\0\0\0\0", np.dtype("<u4")).astype(np.uint32)
        self.ys, self.escs, self.G, self.name = ys, escs, G, name
        self.host = (buf, s_off, s_len, e_all.view(np.int32), e_off, state.view(np.int32))

    def upload(self, dev):
        """-> the kernels' first six arguments: streams, stream_off, stream_bytes, escapes, esc_off, state"""
        self.dev = tuple(torch.from_numpy(a).to(dev) for a in self.host)
        return tuple(F_._ptr(t) for t in self.dev)

    def blocks_from(self, first: int):
        """the same six arguments for the blocks from `first` on (after `upload`): the offsets stay absolute, so only
        the per-block arrays move"""
        s, s_off, s_len, e, e_off, state = self.dev
        return tuple(F_._ptr(t) for t in (s, s_off[first:], s_len[first:], e, e_off[first:], state[first:]))

    def check(self):
        ys, escs, head = self.ys, self.escs, 4 * RANS_LANES

        def problem(b, states, nw, ne, err):
            if err:
                return (f"the rANS decoder ran past the end of its stream or escape list (error word {err}): "
                        "the stream is damaged")
            if nw != (len(ys[b]) - head) // 2 or ne != len(escs[b]) // 4 or (states != 1 << 16).any():
                return ("the rANS stream was not used up exactly (trailing words or escapes, or final states that are "
                        "not the encoder's start): the stream is damaged")
        _state_blocks(self.dev[5], self.G, problem, self.name)                            # the one read-back


# what an encoder's error word means, by the coder the message speaks of
_ENCODER_FAULTS = {
    "the rANS encoder": "a malformed table, a pixel index outside the image or step lengths that do not add up",
    "the rANS encoder of z": "a malformed table or step lengths that do not add up"}


def rans_streams_of(h_state, h_words, h_esc, blocks, G: int, picked=None, name=_image_name, coder="the rANS encoder"):
    """The host half of an encode's read-back, pure numpy: what the encoder kernels left -> the bytes, or CodecError.
    h_state: the encoder's state blocks [nimg * G][RANS_STATE_WORDS] uint32, image-major (`_state_blocks` has the
    words); blocks: their table (`rans_block_layout`); picked: pick's error words -- None, one for the call, or one
    per image --, OR-ed into every block of their image.  First every block's error word, then every block's counts
    against its slot and list: the first block that fails raises, named `name(image)`.  h_words: the word buffer
    (uint8), a block's words right-aligned in its slot; h_esc: the escape buffer (uint32).  Either may be a function,
    called once the counts have passed -- h_words(lo) -> the buffer from byte lo, the first used one, on; h_esc(used)
    -> the entries at the indices `used` --, so `rans_read_back` copies from the device no more than is used.
    -> ([stream bytes per image and group, image-major], [escape-list bytes likewise, little-endian uint32])"""
    h_state, nb = np.asarray(h_state).view(np.uint32), blocks.shape[0]
    pick = np.broadcast_to(np.asarray(0 if picked is None else picked).astype(np.uint32).ravel(), (nb // G,))
    err = h_state[:nb, RANS_LANES + 2] | np.repeat(pick, G)
    nw, ne = h_state[:nb, RANS_LANES].astype(np.int64), h_state[:nb, RANS_LANES + 1].astype(np.int64)
    for i in np.flatnonzero(err)[:1]:
        raise CodecError(f"{name(i // G)}: {coder} met {_ENCODER_FAULTS[coder]} (error word {err[i]})")
    for i in np.flatnonzero((2 * nw > blocks[:, 1]) | (ne > blocks[:, 3]))[:1]:
        raise CodecError(f"{name(i // G)}: {coder} reports impossible counts ({nw[i]} words, {ne[i]} escapes)")
    end = blocks[:, 0] + blocks[:, 1]
    lo = int((end - 2 * nw).min())
    h_words = h_words(lo) if callable(h_words) else h_words[lo:]
    used = np.concatenate([off + np.arange(n, dtype=np.int64) for off, n in zip(blocks[:, 2], ne)])
    if used.size:
        h_esc = np.asarray(h_esc(used) if callable(h_esc) else h_esc[used]).view(np.uint32)
    e_at = np.cumsum(ne) - ne
    return ([h_state[i, :RANS_LANES].astype("<u4").tobytes() + h_words[end[i] - 2 * nw[i] - lo:end[i] - lo].tobytes()
             for i in range(nb)],
            [h_esc[e_at[i]:e_at[i] + ne[i]].astype("<u4").tobytes() if ne[i] else b"" for i in range(nb)])


class _RansEncoding:
    """The device side of one pick + encode over the nimg * G blocks of a block table (`rans_block_layout`), as
    `_RansStaging` is of a decode.  kind "single": `lic_rans_encode_pick` + `lic_rans_encode` (`lic_rans_encode_groups`
    for G > 1) over `images` images of one size; "ragged": `lic_rans_encode_pick_ragged` + `lic_rans_encode_ragged`;
    "z": `lic_rans_z_pick` + `lic_rans_encode_ragged`.  The constructor allocates what they write -- a start|freq and an
    escape word per symbol, slots, escape lists, and the zeroed state blocks: the encoder's, then pick's (one per image;
    one for the whole z pick), so one read-back brings both -- and uploads the int64 arrays of `index` in ONE copy."""

    def __init__(self, dev, kind: str, layout, G: int, nsym: int, images: int, index: Dict):
        self.kind, self.G, self.images, (self.blocks, self.words_len, self.esc_len) = kind, G, images, layout
        parts = [np.ascontiguousarray(a, np.int64).ravel() for a in index.values()]     # int64: all 8-byte aligned
        self.d = dict(zip(index, torch.split(torch.from_numpy(np.concatenate(parts)).to(dev), [a.size for a in parts])))
        self.sf = torch.empty(nsym, device=dev, dtype=torch.int32)
        self.exc = torch.empty_like(self.sf)
        self.words = torch.empty(self.words_len, device=dev, dtype=torch.uint8)
        self.esc = torch.empty(self.esc_len, device=dev, dtype=torch.int32)
        self.state = torch.zeros((len(self.blocks) + (1 if kind == "z" else images), L.RANS_STATE_WORDS), device=dev,
                                 dtype=torch.int32)

    def launch(self, tables, center, syms, M: int, window, rows: int):
        """The two launches; nothing waits.  tables, center (None for z), syms: what pick reads; window: y_W, or (z_lo,
        z_S); rows: pixels of one image ("single") or of all.  `index` held "steps", and what the entries index with."""
        lib, d, G, nimg, st = L.load(), self.d, self.G, self.images, F_._stream()
        sf, exc, words, esc, state = (F_._ptr(t) for t in (self.sf, self.exc, self.words, self.esc, self.state))
        picked, steps, nsteps = F_._ptr(self.state[len(self.blocks):]), F_._ptr(d["steps"]), d["steps"].numel()
        if self.kind == "single":
            nsym, (_, slot, _, cap) = rows * M, self.blocks[0].tolist()
            L.check(lib.lic_rans_encode_pick(F_._ptr(tables), F_._ptr(center), F_._ptr(syms), F_._ptr(d["order"]), nimg,
                                             rows, M, window, sf, exc, picked, st), "lic_rans_encode_pick")
            if G == 1:
                return L.check(lib.lic_rans_encode(sf, exc, steps, nsteps, nimg, nsym, words, slot, esc, state, st),
                               "lic_rans_encode")
            return L.check(lib.lic_rans_encode_groups(sf, exc, steps, nsteps, nimg, G, nsym, words, slot, esc, cap, state,
                                                      st), "lic_rans_encode_groups")
        if self.kind == "z":
            L.check(lib.lic_rans_z_pick(F_._ptr(tables), M, window[0], window[1], F_._ptr(syms), syms.numel(), sf, exc,
                                        picked, st), "lic_rans_z_pick")
        else:
            L.check(lib.lic_rans_encode_pick_ragged(
                F_._ptr(tables), F_._ptr(center), F_._ptr(syms), rows, F_._ptr(d["images"]), nimg, F_._ptr(d["row_image"]),
                F_._ptr(d["order"]), M, window, sf, exc, picked, st), "lic_rans_encode_pick_ragged")
        L.check(lib.lic_rans_encode_ragged(sf, exc, steps, nsteps, F_._ptr(d["images"]), F_._ptr(d["blocks"]), nimg, G, rows,
                                           M, words, self.words_len, esc, self.esc_len, state, st), "lic_rans_encode_ragged")

    def read_back(self, name=_image_name):
        """`rans_read_back` of these buffers -> (streams, escape lists), image-major"""
        z = self.kind == "z"
        return rans_read_back(self.state, self.words, self.esc, self.blocks, self.G, 0 if z else RANS_LANES + 2, name,
                              "the rANS encoder of z" if z else "the rANS encoder")


def rans_read_back(state, words, esc, blocks, G: int, pick_word: int, name=_image_name, coder="the rANS encoder"):
    """The one read-back of an encode, `_RansStaging.check`'s sibling.  state, words, esc: the device buffers the
    encoder kernels wrote (`_RansEncoding`); state holds the encoder's nimg * G blocks and behind them pick's, whose
    word `pick_word` is pick's error word (0 of the z pick's one block, RANS_LANES + 2 of the y picks' one per image).
    The waiting copy of the state blocks, then `rans_streams_of`: pick's words OR-ed in on the host, the refusals, ONE
    copy of the word buffer from its first used byte on, ONE gather of the used escape entries (none when there is no
    escape), the cut."""
    nb = blocks.shape[0]
    h_state = state.cpu().numpy()                                                 # the read-back that waits
    return rans_streams_of(h_state[:nb], lambda lo: words[lo:].cpu().numpy(),
                           lambda used: esc[torch.from_numpy(used).to(esc.device)].cpu().numpy(), blocks, G,
                           h_state[nb:, pick_word], name, coder)


def _z_coder_of(strings) -> str:
    """who coded the hyper-latent of these strings: "range" if they do not say; CodecError for what cannot be"""
    z_coder = strings.get("z_coder", "range")
    if z_coder not in Z_CODERS:
        raise CodecError(f"unknown z_coder {z_coder!r} in the strings")
    if z_coder == "rans" and strings.get("coder", "range") != "rans":
        raise CodecError("the strings name z_coder 'rans' without coder 'rans': only 'rans' streams carry rANS z streams")
    return z_coder


def _z_streams(strings, n: int):
    """the n rANS sub-streams of the hyper-latent in `strings` and their escape lists, or CodecError"""
    zs, zescs = strings["z"], strings.get("z_esc")
    if zescs is None or isinstance(zs, (bytes, bytearray)) or len(zs) != n or len(zescs) != n:
        raise CodecError("one z stream and one escape list per image and group expected")
    return list(zs), list(zescs)


def _stage_y_and_z(ys, escs, nimg: int, zs, zescs, nz: int, G: int, name=_image_name, zname=None) -> _RansStaging:
    """One staging for the nimg * G y blocks and, behind them, the nz * G z blocks of the images whose hyper-latent is
    rANS-coded: one upload, one read-back.  `name(image)` / `zname(z image)` label them in the messages."""
    if escs is None or len(ys) != nimg * G or len(escs) != nimg * G:
        raise CodecError("one y stream and one escape list per image and group expected")
    if zescs is None or isinstance(zs, (bytes, bytearray)) or len(zs) != nz * G or len(zescs) != nz * G:
        raise CodecError("one z stream and one escape list per image and group expected")
    zname = name if zname is None else zname
    return _RansStaging(list(ys) + list(zs), list(escs) + list(zescs), nimg + nz, G,
                        lambda img: name(img) if img < nimg else zname(img - nimg) + " (hyper-latent)")


def _rounded_nhwc(t: torch.Tensor) -> torch.Tensor:
    """[B,C,h,w] latents -> [B,h,w,C] int32: the symbols, pixel by pixel, channel by channel"""
    return t.permute(0, 2, 3, 1).contiguous().round().to(torch.int32)


def rc_encode_z(zt: np.ndarray, z_idx: np.ndarray) -> bytes:
    """the range coder's one call for z: symbol k (value - z_lo, `_rounded_nhwc`'s order) uses row k % M of the
    factorised tables zt [M][z_S+1]"""
    return rc_encode(zt, z_idx, np.tile(np.arange(len(zt), dtype=np.int32), z_idx.size // len(zt)))


class LatentCodec:
    """compress / decompress the (y, z) latents of a JointAutoregressiveHierarchical /
    HierarchicalMixtureResidual model.  `z_lo`, `z_S`: symbol window of the hyper-latent tables;
    `y_W`: half-width of the per-element window around the mixture mean."""

    def __init__(self, model, z_lo: int = -64, z_S: int = 129, y_W: int = 32):
        self.model, self.z_lo, self.z_S, self.y_W = model, int(z_lo), int(z_S), int(y_W)

    @torch.no_grad()
    def compress(self, x: torch.Tensor) -> Dict:
        m = self.model
        out = m.analysis_hyperprior(x, training=False, with_packed_params=True)
        y_in, z_in = out["y_in"], out["z_in"]                      # NCHW-logical, NHWC-physical, integer valued
        B, M, h, w = y_in.shape
        zt, z_idx, z_tab = self._z_symbols(z_in)
        z_bytes = rc_encode_z(zt, z_idx)
        act = out["_act"]
        center, yt = gmm_tables(act, M, m.K, self.y_W)
        y_idx = (_rounded_nhwc(y_in).reshape(-1, M) - center + self.y_W).cpu().numpy().ravel()
        yt_h = yt.cpu().numpy().view(np.uint32)
        y_bytes = rc_encode(yt_h, y_idx)
        npix = x.shape[0] * x.shape[2] * x.shape[3]
        return {"strings": {"y": y_bytes, "z": z_bytes}, "shape": (B, M, h, w),
                "z_shape": tuple(z_in.shape),
                "bpp_coded_y": 8.0 * len(y_bytes) / npix, "bpp_coded_z": 8.0 * len(z_bytes) / npix,
                "bpp_ideal_y": rc_ideal_bits(yt_h, y_idx) / npix, "bpp_ideal_z": rc_ideal_bits(zt, z_idx, z_tab) / npix,
                "bpp_est_y": float(-out["logp_y"].double().sum() / np.log(2.0) / npix),
                "bpp_est_z": float(-out["logp_z"].double().sum() / np.log(2.0) / npix),
                "y_in": y_in, "z_in": z_in, "_y_tables": yt_h, "_y_center": center}

    def _z_tables(self, n: int):
        """(factorised tables [M][z_S+1] uint32, table of each of the n z symbols: pixel by pixel, channel by channel)"""
        zt = factorized_tables(self.model.factorized_entropy_model, self.z_lo, self.z_S).cpu().numpy().view(np.uint32)
        return zt, np.tile(np.arange(len(zt), dtype=np.int32), n // len(zt))

    def _z_symbols(self, z_in: torch.Tensor):
        """z_in [B,M,h4,w4] -> `rc_encode`'s arguments: (tables, symbol - z_lo in coding order, table of each symbol)"""
        zt, z_tab = self._z_tables(z_in.numel())
        return zt, (_rounded_nhwc(z_in) - self.z_lo).cpu().numpy().ravel(), z_tab

    def encode_z(self, z_in: torch.Tensor) -> bytes:
        return rc_encode_z(*self._z_symbols(z_in)[:2])

    @torch.no_grad()
    def decompress_z(self, z_bytes: bytes, z_shape) -> torch.Tensor:
        """The hyper-latent: parameter-free prior, decodes in one pass.  Returns z_in [B,M,h4,w4]."""
        B, M, h4, w4 = z_shape
        dev = next(self.model.parameters()).device
        n = B * M * h4 * w4
        zt, z_tab = self._z_tables(n)
        idx = rc_decode(z_bytes, zt, n, z_tab)
        z = torch.from_numpy((idx + self.z_lo).astype(np.float32)).view(B, h4, w4, M).to(dev)
        return z.permute(0, 3, 1, 2)

    @staticmethod
    def decode_y_with_tables(y_bytes: bytes, tables: np.ndarray, center: torch.Tensor, y_W: int, shape):
        """The coder's inverse for y, given the tables / centres the encoder used."""
        B, M, h, w = shape
        idx = rc_decode(y_bytes, tables, B * M * h * w)
        y = torch.from_numpy(idx.astype(np.int32)).view(-1, M) + center.cpu() - int(y_W)
        return y.view(B, h, w, M).permute(0, 3, 1, 2).float()


# ---------------------------------------------------------------------------------------------
# Full bitstream with the autoregressive context: the serial step
# ---------------------------------------------------------------------------------------------
class _StreamDecoder:
    """lic_rc_decoder_* wrapper (one per image stream)."""

    def __init__(self, data: bytes):
        self._buf = np.frombuffer(data, np.uint8).copy()
        self._h = _codec().lic_rc_decoder_new(_p(self._buf, C.c_uint8), self._buf.size)
        if not self._h:
            raise CodecError("lic_rc_decoder_new failed")

    def next(self, tables: np.ndarray, n: int) -> np.ndarray:
        tables = np.ascontiguousarray(tables, np.uint32)
        out = np.empty(n, np.int32)
        rc = _codec().lic_rc_decoder_next(self._h, _p(tables, C.c_uint32), None, tables.shape[-1] - 1, n,
                                          _p(out, C.c_int32))
        if rc != 0:
            raise CodecError(f"lic_rc_decoder_next failed with status {rc}")
        return out

    def close(self):
        if self._h:
            _codec().lic_rc_decoder_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


class CodecLayer:
    """A layer as the codec sees it: a masked context convolution and an entropy-parameter MLP (three 1x1
    convolutions) over the channels [c0, c0 + M) of the latent, with K mixture components.  `ContextCodec` has one,
    over all channels; `ScalableCodec` has the base and the enhancement layer.  Everything per-pixel a codec evaluates
    goes through here, so encoder and decoder of every codec build their tables with the same calls."""

    def __init__(self, model, context: str, mlp: str, c0: int = 0, channels: str = "M"):
        """`context`, `mlp`, `channels`: the names of the model's attributes that hold the layer's context model, its
        entropy-parameter MLP and its channel count; only the context model's mask is read here, the rest when used"""
        self.model, self._context, self._mlp, self.c0, self._channels = model, context, mlp, int(c0), channels
        mc = self.context_model.masked
        k = mc.kernel_size[0]
        self.taps = [(r, s) for r in range(k) for s in range(k) if (mc._tap_mask >> (r * k + s)) & 1]
        self.k, self.pad = k, mc.padding[0]
        # the wavefront schedule (`wavefront`) needs every live tap strictly earlier: ds + (pad + 1) * dr < 0; the
        # two-pass schedule (`two_pass`) needs every live tap to change the parity of i + j: dr + ds odd
        if not any((s - self.pad) + (self.pad + 1) * (r - self.pad) >= 0 for (r, s) in self.taps):
            self.kind = "raster"
        elif all(((r - self.pad) + (s - self.pad)) % 2 == 1 for (r, s) in self.taps):
            self.kind = "checkerboard"
        else:
            raise CodecError("context mask is not causal in raster order and not a checkerboard mask (every live tap "
                             "(dr, ds) with dr + ds odd): the codec has a schedule for these two kinds only")

    context_model = property(lambda self: getattr(self.model, self._context))
    entropy_parameters = property(lambda self: getattr(self.model, self._mlp))
    M = property(lambda self: int(getattr(self.model, self._channels)))
    K = property(lambda self: int(self.model.K))

    @property
    def cctx(self) -> int:
        """columns the context GEMM writes in front of psi in the first 1x1 layer's input"""
        return self.context_model.masked.out_channels

    def ctx_weight(self):
        mc = self.context_model.masked
        w = (mc.weight * mc.mask).detach()                                     # [2M, M, k, k]
        cols = [w[:, :, r, s] for (r, s) in self.taps]                         # each [2M, M]
        return torch.cat(cols, dim=1).reshape(w.shape[0], -1, 1, 1).contiguous(), mc.bias.detach()

    def prepack(self):
        """The four per-pixel layers (context GEMM + the 1x1 MLP) with their weights packed ONCE: the decoder
        runs them h*w times; packing per call moved ~10 MB per latent pixel."""
        wg, bg = self.ctx_weight()
        net = self.entropy_parameters.net
        convs = [net[0], net[2], net[4]]
        slopes = [net[1].negative_slope, net[3].negative_slope]
        layers = [(F_.pack_conv_weight(wg), bg, wg.shape[0], False, 0.01)]
        for i, c in enumerate(convs):
            if c.kernel_size != (1, 1):
                raise CodecError("entropy-parameter layers are expected to be 1x1 convolutions")
            layers.append((F_.pack_conv_weight(c.weight), None if c.bias is None else c.bias.detach(), c.out_channels,
                           i < 2, slopes[i] if i < 2 else 0.01))
        return layers

    def act_at(self, windows: torch.Tensor, psi_px: torch.Tensor, layers, comb: torch.Tensor = None) -> torch.Tensor:
        """windows [N, 12M, 1, 1], psi_px [N, 2M, 1, 1] -> the activated entropy parameters [N, G*K*M, 1, 1].
        `comb` [N, 4M]: the input of the first 1x1 layer with psi already in its last 2M columns (`_gather`), instead
        of psi_px; the context GEMM writes its 2M columns beside them, so no `cat` (Models.py:73) runs."""
        wp, b, co, _, _ = layers[0]
        N = windows.shape[0]
        if comb is None:
            comb = torch.empty((N, co + psi_px.shape[1]), device=windows.device, dtype=torch.float32)
            comb[:, co:] = psi_px.reshape(N, -1)
        comb = comb.view(N, 1, 1, -1)
        F_.conv2d_prepacked(windows, wp, b, co, 1, pin_tile=True, out=comb[..., :co])
        x = comb.permute(0, 3, 1, 2)
        for wp, b, co, leaky, slope in layers[1:]:
            x = F_.conv2d_prepacked(x, wp, b, co, 1, leaky=leaky, slope=slope, pin_tile=True)
        return F_.entropy_params_activation(x, self.M, self.K)

    def params_at(self, windows: torch.Tensor, psi_px: torch.Tensor, layers, comb: torch.Tensor, y_W: int):
        """`act_at`'s arguments -> (center [N, M], tables [N*M, S+1]) on the device"""
        return gmm_tables(self.act_at(windows, psi_px, layers, comb), self.M, self.K, y_W)


class _LayeredCodec:
    """What `ContextCodec` (one layer over all channels) and `ScalableCodec` (two layers) share: the gather of every
    layer's rows from the one latent plane, the per-step front end and the rANS step loop, written once over
    `self.layers`.  A single layer that covers the whole plane goes through `lic_ctx_gather` and
    `lic_rans_decode_step_groups`; anything else through `lic_ctx_gather_layers` and `lic_rans_decode_step_layers`,
    one launch each for all layers of a step.

    `_decompress_many` is `decompress_many` of both: many bitstreams of different sizes in one loop,
    `_run_merged_steps`, whose gather (`_gather_rows`) and decode launch are `lic_ctx_gather_ragged` and
    `lic_rans_decode_step_ragged` for the codec of one layer, `lic_ctx_gather_layers_ragged` and
    `lic_rans_decode_step_layers_ragged` for a layered one.  A class adds `_item_streams` (an item's refusals, where its
    streams sit in its strings, whether z may be range-coded) and `_finish` (checksums and what a result holds).
    The layouts are module functions: `plane_layout`, `z_plan`, `merged_wavefront`.

    Also here, because they do not know how many layers y has: the rANS coder of z (`_z_symbols`, `_encode_z`,
    `_decode_z`), the two encoders of one layer's y streams (`_encode_y_device`, `_encode_y_host` over `_coding_order`:
    the same arguments, the same bytes), the optional keys of the strings (`_optional_keys`), and what the containers
    of both codecs share (`_family`, `_shapes`, `_one_window_one_G`, `_pack_padded`).  The device encoders build their
    inputs only: buffers and launches are `_RansEncoding`'s, the read-back is `rans_read_back`."""

    # False: the layered entries are launched once per layer instead of once per step (tools/bench_codec.py measures
    # what the merged launches save); bytes and results are the same
    merge_layers = True
    # what the layers' masks say (`CodecLayer.kind`, `_set_layers`): "raster" (`wavefront`) or "checkerboard" (`two_pass`)
    schedule = "raster"

    # ---- rate levels (models: rate_levels = Q): the quality an item is coded at rides in its strings ----
    @property
    def rate_levels(self):
        return getattr(self.model, "rate_levels", None)

    def _quality(self, quality):
        """one item's quality as this codec's model takes it: None for a plain model, a float in [0, Q-1] for a
        rate-level one; CodecError otherwise"""
        Q = self.rate_levels
        if Q is None:
            if quality is not None:
                raise CodecError(f"quality = {quality!r}: this codec's model has no rate levels")
            return None
        if quality is None:
            raise CodecError(f"this codec's model has {Q} rate levels: a quality in [0, {Q - 1}] is needed")
        if isinstance(quality, bool) or not isinstance(quality, (int, float, np.integer, np.floating)):
            raise CodecError(f"quality = {quality!r}: expected one number per item")
        q = float(np.float32(quality))          # what the envelope holds: encoder and decoder scale by the same gains
        if not 0.0 <= q <= Q - 1:
            raise CodecError(f"quality {quality!r} outside [0, {Q - 1}]")
        return q

    def _qualities(self, quality, n: int, what: str = "item"):
        """`quality` of a many-item call -> one per item: a number for all of them or a list of n"""
        if quality is None or isinstance(quality, (int, float, np.integer, np.floating)):
            return [self._quality(quality)] * n
        qs = list(quality)
        if len(qs) != n:
            raise CodecError(f"{len(qs)} qualities for {n} {what}s: one number, or one per {what}")
        out = []
        for i, q in enumerate(qs):
            try:
                out.append(self._quality(q))
            except CodecError as err:
                raise CodecError(f"{what} {i}: {err}") from None
        return out

    def _hyper_synthesis(self, z_hat: torch.Tensor, quality=None) -> torch.Tensor:
        """psi of one item: the hyper-decoder behind the inverse gain of its quality (the bare module for a plain model)"""
        m = self.model
        return m.hyper_synthesis(z_hat, quality) if hasattr(m, "hyper_synthesis") else m.hyper_decoder(z_hat)

    def _set_layers(self, layers):
        """the codec's layers; they share one wavefront schedule and one tap table, so their masks must agree"""
        self.layers = list(layers)
        first = self.layers[0]
        for ly in self.layers[1:]:
            if (ly.taps, ly.k, ly.pad) != (first.taps, first.k, first.pad):
                raise CodecError("the layers' context masks differ in their live taps: one gather and one wavefront "
                                 "schedule serve all layers, so they must agree")
            if ly.kind != first.kind:
                raise CodecError(f"the layers' context masks differ in kind ({first.kind} and {ly.kind}): one schedule "
                                 "serves all layers")
        self.taps, self.k, self.pad, self.schedule = first.taps, first.k, first.pad, first.kind

    @staticmethod
    def _whole_plane(layers, y_pix: int) -> bool:
        return len(layers) == 1 and layers[0].c0 == 0 and layers[0].M == y_pix

    def _wavefront(self, h: int, w: int, slice_rows: int = None):
        """Decode schedule.  With mask type A a pixel (i, j) sees rows above it up to column j + pad and its own
        row up to j - 1, so for t = j + (pad + 1) * i every pixel's context lies in steps < t: the pixels of one
        step are independent and go through the GPU as one batch -- w + (pad + 1)(h - 1) dependent steps
        instead of h * w (141 instead of 1536 for a 512x768 image).  With slices of `slice_rows` rows i counts
        inside the pixel's slice (`wavefront`).  Returns [(rows, cols)] per step, rows
        ascending; encoder and decoder order the symbols step by step, pixel by pixel, channel by channel.
        A checkerboard mask has `two_pass`'s two steps instead, and no slices."""
        return _steps_of(h, w, self.pad, slice_rows, self.schedule)

    def _context_plane(self, y_in: torch.Tensor) -> torch.Tensor:
        """the plane the ENCODER gathers every pixel's window from: y_hat itself, or anchor(y_hat) under a checkerboard
        mask (lic_quantize_anchor on rounded values: rint changes nothing) -- what the decoder's plane holds when it
        reaches the pixel: zeros in step 0, the anchors alone in step 1"""
        return F_.quantize_anchor(y_in, None, False)[1] if self.schedule == "checkerboard" else y_in

    def _refuse_other_schedule(self, strings):
        got = strings.get("schedule", "raster")
        if got != self.schedule:
            raise CodecError(f"schedule mismatch: the strings were coded in the {got} schedule, this codec's context "
                             f"model decodes the {self.schedule} schedule")

    def _taps_on(self, dev) -> torch.Tensor:
        """the live taps as (dr, ds) int32 pairs on `dev`, uploaded once"""
        if getattr(self, "_taps_dev", None) is None or self._taps_dev.device != dev:
            self._taps_dev = torch.tensor([(r - self.pad, s - self.pad) for (r, s) in self.taps], dtype=torch.int32,
                                          device=dev)
        return self._taps_dev

    def _gather_layers(self, y: torch.Tensor, y_pix: int, geometry, h: int, w: int, pix: torch.Tensor, slice_rows,
                       psi_flat=None, layers=None):
        """One gather launch for all `layers` (default: the codec's).  y: fp32 latents of B images with y_pix channels
        per pixel, pixel (i, j) of image b at float b * batch + origin + i * row + j * y_pix for geometry = (batch,
        row, origin); pix: int64 raster indices (device) of the n pixels wanted; psi_flat [B, h*w, 2M] or None.
        -> per layer (windows [B*n, 12 M_l, 1, 1] with zeros for taps outside the image or the pixel's slice,
                      comb [B*n, cctx_l + 2M] whose last 2M columns hold the pixels' psi, the first cctx_l still
                      unwritten; None without psi)"""
        layers = self.layers if layers is None else layers
        B, n, nt, dev = y.shape[0], pix.numel(), len(self.taps), y.device
        taps = self._taps_on(dev)
        cpsi = 0 if psi_flat is None else psi_flat.shape[2]
        outs = []
        for ly in layers:
            win = torch.empty((B * n, nt * ly.M, 1, 1), device=dev, dtype=torch.float32)
            comb = None if psi_flat is None else torch.empty((B * n, ly.cctx + cpsi), device=dev, dtype=torch.float32)
            outs.append((win, comb))
        batch, row, origin = geometry
        R = h if slice_rows is None else min(slice_rows, h)
        first_col = lambda ly, comb: None if comb is None else C.c_void_p(comb.data_ptr() + 4 * ly.cctx)
        if self._whole_plane(layers, y_pix):
            (win, comb), ly = outs[0], layers[0]
            L.check(L.load().lic_ctx_gather(
                F_._ptr(y), batch, row, y_pix, origin, B, h, w, ly.M, F_._ptr(taps), nt, R, F_._ptr(pix), n, F_._ptr(win),
                F_._ptr(psi_flat), cpsi, first_col(ly, comb), 0 if comb is None else comb.shape[1], L.CTX_AUTO,
                F_._stream()), "lic_ctx_gather")
            return outs
        if len(layers) > L.MAX_LAYERS:
            raise CodecError(f"{len(layers)} layers: the layered kernels take {L.MAX_LAYERS} at the most")
        table = (L.CtxLayer * len(layers))()
        for t, ly, (win, comb) in zip(table, layers, outs):
            t.win, t.comb, t.comb_ld = win.data_ptr(), first_col(ly, comb), 0 if comb is None else comb.shape[1]
            t.c0, t.M = ly.c0, ly.M
        # merge_layers False: one launch per layer, for tools/bench_codec.py's comparison; the same bytes
        for rows in ([table] if self.merge_layers else [(L.CtxLayer * 1)(t) for t in table]):
            L.check(L.load().lic_ctx_gather_layers(
                F_._ptr(y), batch, row, y_pix, origin, B, h, w, F_._ptr(taps), nt, R, F_._ptr(pix), n, F_._ptr(psi_flat),
                cpsi, rows, len(rows), L.CTX_AUTO, F_._stream()), "lic_ctx_gather_layers")
        return outs

    def _windows_layers(self, y_hat: torch.Tensor, slice_rows: int = None, psi: torch.Tensor = None, layers=None):
        """[B, M, h, w] -> `_gather_layers`' result for every pixel of every image, in raster order"""
        F_._require_cuda(y_hat, psi)
        B, M, h, w = y_hat.shape
        y = F_._nhwc(y_hat)
        pix = torch.arange(h * w, device=y.device, dtype=torch.int64)
        return self._gather_layers(y, M, (h * w * M, w * M, 0), h, w, pix, slice_rows,
                                   None if psi is None else F_._nhwc(psi).view(B, h * w, -1), layers)

    def _step_front_end(self, steps, yflat, psi, slice_rows=None, layers=None):
        """What the decoders do per wavefront step before their coder runs.  Here, once: the layers are packed and
        one array uploaded, the raster index and the index into yflat of every step's pixels.  Then, per step of
        `steps` (`_wavefront`) as the returned generator is advanced: one gather of every layer's windows from `yflat`
        (the zero-framed latents [B, (h+2p)(w+2p), y_pix], which the coder fills in between) and of the pixels'
        columns of `psi` [B, 2M, h, w], then per layer the per-pixel layers and the table kernel
        -> (n pixels, their n indices into yflat, [(center [B*n, M_l], tables [B*n*M_l, S+1]) per layer])"""
        layers = self.layers if layers is None else layers
        B, y_pix, p = yflat.shape[0], yflat.shape[2], self.pad
        h, w = psi.shape[2], psi.shape[3]
        packed = [ly.prepack() for ly in layers]
        psi_flat = F_._nhwc(psi).view(B, h * w, -1)                                       # [B, h*w, 2M]
        Wp = w + 2 * p
        idx = torch.from_numpy(_step_indices(steps, w, p)).to(yflat.device)
        geometry = (yflat.shape[1] * y_pix, Wp * y_pix, (p * Wp + p) * y_pix)

        def run():
            off = 0
            for ii, _ in steps:
                n = len(ii)
                rows = self._gather_layers(yflat, y_pix, geometry, h, w, idx[0, off:off + n], slice_rows, psi_flat, layers)
                yield n, idx[1, off:off + n], [ly.params_at(win, None, pk, comb, self.y_W)
                                               for ly, pk, (win, comb) in zip(layers, packed, rows)]
                off += n
        return run()

    def _run_steps(self, front, yflat, blocks, G: int, layers=None):
        """The step loop of the rANS coder: every step of `front` (`_step_front_end`: gather -> per-pixel layers +
        tables) ends in ONE decode launch for all layers, which writes the decoded values into `yflat` where the next
        gather reads them.  Nothing in the loop waits for the device.  blocks: the six staging arguments
        (`_RansStaging.upload`), one block per layer, image and group, layer-major."""
        layers = self.layers if layers is None else layers
        nimg, npad, y_pix = yflat.shape
        lib = L.load()
        if self._whole_plane(layers, y_pix):
            for n, own, ((center, tables),) in front:
                L.check(lib.lic_rans_decode_step_groups(*blocks, F_._ptr(tables), F_._ptr(center), nimg, G, n, y_pix,
                                                        self.y_W, F_._ptr(own), F_._ptr(yflat), npad, F_._stream()),
                        "lic_rans_decode_step_groups")
            return
        table = (L.RansLayer * len(layers))()
        s, s_off, s_len, e, e_off, state = blocks
        per = nimg * G                                                      # blocks of one layer
        shift = lambda p, l, size: C.c_void_p(p.value + l * per * size)
        for n, own, params in front:
            for t, ly, (center, tables) in zip(table, layers, params):
                t.tables, t.center, t.c0, t.M = tables.data_ptr(), center.data_ptr(), ly.c0, ly.M
            if self.merge_layers:
                L.check(lib.lic_rans_decode_step_layers(*blocks, table, len(layers), nimg, G, n, self.y_W, F_._ptr(own),
                                                        F_._ptr(yflat), npad, y_pix, F_._stream()),
                        "lic_rans_decode_step_layers")
                continue
            for l, t in enumerate(table):                                   # one launch per layer (bench_codec.py)
                L.check(lib.lic_rans_decode_step_layers(
                    s, shift(s_off, l, 8), shift(s_len, l, 8), e, shift(e_off, l, 8),
                    shift(state, l, 4 * L.RANS_STATE_WORDS), (L.RansLayer * 1)(t), 1, nimg, G, n, self.y_W, F_._ptr(own),
                    F_._ptr(yflat), npad, y_pix, F_._stream()), "lic_rans_decode_step_layers")

    def _one_layer_ragged(self, layers, y_pix: int) -> bool:
        """Which entries a ragged call launches: `_whole_plane`'s rule for a codec of one layer.  A layered codec keeps
        the `_layers_ragged` entries for its base layer alone too, which `_whole_plane` alone would hand to the
        one-layer entries: the same bytes, but they are the launches tests/test_gpu_scalable_decode_many.py counts."""
        return len(self.layers) == 1 and self._whole_plane(layers, y_pix)

    def _gather_rows(self, layers, yflat: torch.Tensor, y_pix: int, d_desc: torch.Tensor, row_image: torch.Tensor,
                     row_pix: torch.Tensor, psiflat: torch.Tensor, cpsi: int):
        """One gather launch for rows of different images: `_gather_layers` over the flat buffers of `plane_layout`.
        yflat, psiflat: the buffers all planes lie in; d_desc [nimg, CTX_IMAGE_WORDS] int64 (device): where, and h, w,
        R of each; row_image, row_pix [n] int64 (device): the image and raster index of every row
        -> per layer (windows [n, 12 M_l, 1, 1], comb [n, cctx_l + cpsi]) as `_gather_layers`.  `lic_ctx_gather_ragged`
        for the codec of one layer, `lic_ctx_gather_layers_ragged` for a layered one (`_one_layer_ragged`)."""
        n, nt, nimg, dev = row_pix.numel(), len(self.taps), d_desc.shape[0], yflat.device
        taps = self._taps_on(dev)
        rows = [(torch.empty((n, nt * ly.M, 1, 1), device=dev, dtype=torch.float32),
                 torch.empty((n, ly.cctx + cpsi), device=dev, dtype=torch.float32)) for ly in layers]
        if self._one_layer_ragged(layers, y_pix):
            (win, comb), ly = rows[0], layers[0]
            L.check(L.load().lic_ctx_gather_ragged(
                F_._ptr(yflat), yflat.numel(), y_pix, F_._ptr(d_desc), nimg, ly.M, F_._ptr(taps), nt, F_._ptr(row_image),
                F_._ptr(row_pix), n, F_._ptr(win), F_._ptr(psiflat), psiflat.numel(), cpsi,
                C.c_void_p(comb.data_ptr() + 4 * ly.cctx), comb.shape[1], L.CTX_AUTO, F_._stream()), "lic_ctx_gather_ragged")
            return rows
        if len(layers) > L.MAX_LAYERS:
            raise CodecError(f"{len(layers)} layers: the layered kernels take {L.MAX_LAYERS} at the most")
        ctx = (L.CtxLayer * len(layers))()
        for c, ly, (win, comb) in zip(ctx, layers, rows):
            c.win, c.comb, c.comb_ld, c.c0, c.M = win.data_ptr(), comb.data_ptr() + 4 * ly.cctx, comb.shape[1], ly.c0, ly.M
        L.check(L.load().lic_ctx_gather_layers_ragged(
            F_._ptr(yflat), yflat.numel(), y_pix, F_._ptr(d_desc), nimg, F_._ptr(taps), nt, F_._ptr(row_image),
            F_._ptr(row_pix), n, F_._ptr(psiflat), psiflat.numel(), cpsi, ctx, len(layers), L.CTX_AUTO, F_._stream()),
            "lic_ctx_gather_layers_ragged")
        return rows

    def _run_merged_steps(self, sched: MergedSchedule, layers, blocks, G: int, yflat: torch.Tensor, y_pix: int,
                          layout: PlaneLayout, psiflat: torch.Tensor, cpsi: int):
        """The step loop of many latents of different sizes (`merged_wavefront`), every layer of `layers` in it: per
        step ONE gather (`_gather_rows`) from the flat buffers `yflat` (zero-framed planes of y_pix channels per pixel)
        and `psiflat`, per layer the per-pixel layers and the table kernel over the step's rows of every image, and ONE
        decode launch, which writes the values where the next gather reads them: `lic_rans_decode_step_ragged` for the
        codec of one layer, `lic_rans_decode_step_layers_ragged` for a layered one (`_one_layer_ragged`).  layout: the
        buffers' `plane_layout`; blocks: the six staging arguments, one block per layer, image and group, layer-major.
        Schedule and layout go up once; nothing in the loop copies, waits for the device or computes on the host."""
        dev, nimg, lib = yflat.device, layout.desc.shape[0], L.load()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        one = self._one_layer_ragged(layers, y_pix)
        d_desc, d_rows, d_seg, d_pixels = up(layout.desc), up(sched.rows), up(sched.seg), up(layout.pixels)
        # the planes' first floats: an upload for the one-layer entries, a device copy of the column for the layered
        # ones, as each loop did before they became one (their kernel traces stay what they were)
        d_ybase = up(layout.desc[:, 0]) if one else d_desc[:, 0].contiguous()
        packed = [ly.prepack() for ly in layers]
        rans, off = (L.RansLayer * len(layers))(), sched.step_off
        for t in range(sched.T):
            a, e = int(off[t]), int(off[t + 1])
            rows = self._gather_rows(layers, yflat, y_pix, d_desc, d_rows[0, a:e], d_rows[1, a:e], psiflat, cpsi)
            params = [ly.params_at(win, None, pk, comb, self.y_W) for ly, pk, (win, comb) in zip(layers, packed, rows)]
            if one:
                ((center, tables),) = params
                L.check(lib.lic_rans_decode_step_ragged(
                    *blocks, F_._ptr(tables), F_._ptr(center), F_._ptr(d_seg[t]), nimg, G, e - a, y_pix, self.y_W,
                    F_._ptr(d_rows[2, a:e]), F_._ptr(yflat), F_._ptr(d_ybase), F_._ptr(d_pixels), yflat.numel(),
                    F_._stream()), "lic_rans_decode_step_ragged")
                continue
            for r, ly, (center, tables) in zip(rans, layers, params):
                r.tables, r.center, r.c0, r.M = tables.data_ptr(), center.data_ptr(), ly.c0, ly.M
            L.check(lib.lic_rans_decode_step_layers_ragged(
                *blocks, rans, len(layers), F_._ptr(d_seg[t]), nimg, G, e - a, self.y_W, F_._ptr(d_rows[2, a:e]),
                F_._ptr(yflat), F_._ptr(d_ybase), F_._ptr(d_pixels), yflat.numel(), y_pix, F_._stream()),
                "lic_rans_decode_step_layers_ragged")

    # ---- many bitstreams in one step loop -------------------------------------------------------
    def _what(self, l: int) -> str:
        """how a message names layer l of an image: not at all in the codec of one layer"""
        return f", layer {l}" if len(self.layers) > 1 else ""

    def _decompress_many(self, items, use, z_windows, names) -> List[Dict]:
        """`decompress_many` of both codecs, for the layers `use` (the codec's first ones).  A class supplies
        `_item_streams` (an item's refusals and its streams) and `_finish` (its result).

        Host first, item by item, lowest index first and inside an item G, then y, then z: every refusal, the blocks of all
        layers staged layer-major (block (l * nimg + image) * G + g) with the z blocks of the items whose hyper-latent
        is rANS-coded behind them (`_stage_y_and_z`), the schedule (`merged_wavefront`) and the z buffer (`z_plan`).
        Then the device: those z in one `lic_rans_z_decode` launch per window (`_decode_z`), a range-coded z on the
        host, the hyper-decoder per item exactly as `decompress` runs it; all psi planes and all zero-framed latent
        planes in two flat buffers (`plane_layout`); ONE loop of T steps (`_run_merged_steps`): no copy, no
        synchronisation, no host arithmetic; one read-back of the state blocks; `_finish` per item on a view of its
        planes."""
        m, p, M = self.model, self.pad, self.model.M
        items = list(items)
        if not items:
            return []
        y_pix = sum(ly.M for ly in use)                    # the layers are consecutive from channel 0
        names = [f"item {i}" for i in range(len(items))] if names is None else list(names)
        z_windows = [(self.z_lo, self.z_S)] * len(items) if z_windows is None else list(z_windows)
        G, shapes, Rs, owner, zowner, z_items = None, [], [], [], [], []
        ys, escs, zs, zescs = [[] for _ in use], [[] for _ in use], [], []
        for i, ((strings, shape, z_shape), win) in enumerate(zip(items, z_windows)):
            try:
                g = _groups(strings.get("groups", 1))
                if G is not None and g != G:
                    raise CodecError(f"{g} sub-streams per image, {names[0]} has {G}: one call decodes one G")
                self._refuse_other_schedule(strings)
                coded, z = self._item_streams(strings, shape, z_shape, g, len(use))
                R = None if strings.get("slice_rows") is None else _slice_rows(strings["slice_rows"])
            except CodecError as err:
                raise CodecError(f"{names[i]}: {err}") from None
            G, (B, _, h, w) = g, shape
            shapes += [(h, w)] * B
            Rs += [R] * B
            owner += [(i, b) for b in range(B)]
            for l, (y, esc, _) in enumerate(coded):
                ys[l] += list(y)
                escs[l] += list(esc)
            z_items.append(None if z is None else (z_shape, win))
            if z is not None:                              # its z blocks ride behind the y blocks in the one staging
                zowner += [(i, b) for b in range(B)]
                zs += z[0]
                zescs += z[1]
        nimg = len(shapes)
        of = lambda own: (lambda img: f"{names[own[img][0]]}: image {own[img][1]}")
        yname = lambda img: of(owner)(img % nimg) + self._what(img // nimg)
        ys, escs = [s for y in ys for s in y], [e for esc in escs for e in esc]
        if zowner:
            staged = _stage_y_and_z(ys, escs, len(use) * nimg, zs, zescs, len(zowner), G, yname, of(zowner))
        else:
            staged = _RansStaging(ys, escs, len(use) * nimg, G, yname)
        sched = merged_wavefront(shapes, p, Rs, self.schedule)
        zp = z_plan(z_items, M)
        # ---- the device from here on
        dev = next(m.parameters()).device
        blocks = staged.upload(dev)
        if zowner:
            zflat = self._decode_z(staged, len(use) * nimg * G, zp, dev)          # every such item's z, one launch
        z_hats, psis = [], []
        for i, ((strings, _, z_shape), (z_lo, z_S)) in enumerate(zip(items, z_windows)):
            if zp.at[i] is not None:
                z_hat = self._z_view(zflat, zp.at[i], z_shape)
            else:
                try:
                    z_hat = LatentCodec(m, z_lo, z_S, self.y_W).decompress_z(strings["z"], z_shape)
                except CodecError as err:
                    raise CodecError(f"{names[i]}: {err}") from None
            z_hats.append(z_hat.contiguous(memory_format=torch.channels_last))
            psis.append(self._hyper_synthesis(z_hats[-1], strings.get("quality")).float())
        cpsi = psis[0].shape[1]
        lay = plane_layout([(B, h, w) for _, (B, _, h, w), _ in items], y_pix, cpsi, p, Rs)
        yflat = torch.zeros(lay.y_len, device=dev, dtype=torch.float32)            # decoded latents inside zero frames
        psiflat = torch.empty(lay.psi_len, device=dev, dtype=torch.float32)
        for (_, (B, _, h, w), _), at, psi in zip(items, lay.psi_at.tolist(), psis):
            psiflat[at:at + B * h * w * cpsi].view(B, h * w, cpsi).copy_(F_._nhwc(psi).view(B, h * w, -1))
        self._run_merged_steps(sched, use, blocks, G, yflat, y_pix, lay, psiflat, cpsi)
        staged.check()
        out = []
        for (strings, (B, _, h, w), _), at, z_hat, name in zip(items, lay.y_at.tolist(), z_hats, names):
            ypad = yflat[at:at + B * (h + 2 * p) * (w + 2 * p) * y_pix].view(B, h + 2 * p, w + 2 * p, y_pix)
            try:
                out.append(self._finish(strings, ypad, z_hat, (B, M, h, w)))
            except CodecError as err:
                raise CodecError(f"{name}: {err}") from None
        return out

    def _z_view(self, zflat: torch.Tensor, at: int, z_shape) -> torch.Tensor:
        """an item's z_hat [B, M, h4, w4] inside the flat buffer `_decode_z` filled (`z_plan`)"""
        B, _, h4, w4 = z_shape
        M = self.model.M
        return zflat[at:at + B * h4 * w4 * M].view(B, h4, w4, M).permute(0, 3, 1, 2)

    # ---- what the containers of both codecs share ---------------------------------------------------
    @staticmethod
    def _shapes(head, M: int):
        """a container header -> (shape, z_shape) of the image padded to multiples of 64, as `decompress` takes them"""
        Hp, Wp = -(-head["H"] // 64) * 64, -(-head["W"] // 64) * 64
        return (head["B"], M, Hp // 16, Wp // 16), (head["B"], M, Hp // 64, Wp // 64)

    @staticmethod
    def _one_window_one_G(opened) -> int:
        """opened: [(header, strings)] of the blobs of one batched decode, at least one.  CodecError, naming the blob,
        for a y_W, then for a G (sub-streams per image), that is not blob 0's -> the y_W of them all"""
        y_W, G = opened[0][0]["y_W"], opened[0][1].get("groups", 1)
        for i, (head, strings) in enumerate(opened):
            if head["y_W"] != y_W:
                raise CodecError(f"blob {i}: y_W = {head['y_W']}, blob 0 has y_W = {y_W}: one call decodes one window")
        for i, (head, strings) in enumerate(opened):
            if strings.get("groups", 1) != G:
                raise CodecError(f"blob {i}: G = {strings.get('groups', 1)} sub-streams per image, blob 0 has G = {G}: "
                                 "one call decodes one G")
        return y_W

    def _pack_padded(self, x: torch.Tensor, strings: Dict, align: str) -> bytes:
        """the codec's container (`_pack_image`) around the strings `compress` gave for x padded to multiples of 64"""
        B, _, H, W = x.shape
        _, _, top, left = F_.pad_geometry(H, W, 64, align)
        return self._pack_image(strings, B, H, W, top, left)

    def _family(self) -> int:
        name = type(self.model).__name__
        if name not in BITSTREAM_FAMILIES:
            raise CodecError(f"no bitstream family id for {name}")
        return BITSTREAM_FAMILIES[name]

    # ---- the z coder and the device y encoder: they do not know how many layers y has ---------------
    @staticmethod
    def _z_symbols(z_in: torch.Tensor):
        """z_in [B,M,h4,w4] -> [B][h4*w4*M] int32 on its device: every image's rounded hyper-latents, pixel by pixel,
        channel by channel (`LatentCodec._z_symbols`' order)"""
        return _rounded_nhwc(z_in).reshape(z_in.shape[0], -1)

    def _encode_z(self, z_syms, name=_image_name):
        """The hyper-latents as "rANS-64 x G" streams (z_coder="rans").  z_syms: one flat int32 tensor per image
        (`_z_symbols`), of any sizes.  An image is ONE step of all its symbols dealt to G sub-streams
        (`rans_deal([n], G)`); symbol k uses row k % M of the factorised tables.
        -> ([stream bytes per image and group, image-major], [escape-list bytes likewise]), the same bytes from
        `encoder="host"` (`rans_encode_shared`) and from "device" (`lic_rans_z_pick` + `lic_rans_encode_ragged`)."""
        M, G = self.model.M, self.groups
        tables = factorized_tables(self.model.factorized_entropy_model, self.z_lo, self.z_S)
        if self.encoder != "device":
            zt = tables.cpu().numpy().view(np.uint32)
            pairs = [rans_encode_shared(zt, idx[pos], steps_g, (pos % M).astype(np.int32))
                     for idx in ((z.reshape(-1) - self.z_lo).cpu().numpy() for z in z_syms)
                     for pos, steps_g in rans_deal([idx.size], G)]
            return [p[0] for p in pairs], [p[1] for p in pairs]
        dev, nimg = tables.device, len(z_syms)
        images, blocks, step_len, rows, words_len, esc_len = z_encode_plan([z.numel() // M for z in z_syms], M, G)
        z_all = torch.cat([z.reshape(-1) for z in z_syms]) if nimg > 1 else z_syms[0].reshape(-1).contiguous()
        enc = _RansEncoding(dev, "z", (blocks, words_len, esc_len), G, z_all.numel(), nimg,
                            dict(images=images, blocks=blocks, steps=step_len))
        enc.launch(tables, None, z_all, M, (self.z_lo, self.z_S), rows)
        return enc.read_back(name)

    def _decode_z(self, staged, first: int, plan: ZPlan, dev) -> torch.Tensor:
        """The hyper-latents of the images of `plan` (`z_plan`) from their staged "rANS-64 x G" blocks (blocks `first`
        on of `staged`, after `upload`), every image in ONE `lic_rans_z_decode` launch per z window (one launch when
        all share it: an image of another window has 0 symbols in that launch and its blocks stay as they are)
        -> the flat fp32 buffer of plan.z_len floats (`_z_view` cuts an item out of it).  Nothing waits: the blocks
        are checked with the y blocks, by `staged.check()`."""
        M, G, nz, lib = self.model.M, staged.G, len(plan.nsyms), L.load()
        zflat = torch.zeros(plan.z_len, device=dev, dtype=torch.float32)
        kinds = list(dict.fromkeys(plan.windows))
        desc = np.array([[n if win == kind else 0 for n, win in zip(plan.nsyms, plan.windows)] for kind in kinds]
                        + [list(plan.bases)], np.int64)
        d_desc = torch.from_numpy(desc).to(dev)
        blocks = staged.blocks_from(first)
        for i, (z_lo, z_S) in enumerate(kinds):
            tables = factorized_tables(self.model.factorized_entropy_model, z_lo, z_S)
            L.check(lib.lic_rans_z_decode(*blocks, F_._ptr(tables), M, int(z_lo), int(z_S), nz, G, F_._ptr(d_desc[i]),
                                          F_._ptr(d_desc[len(kinds)]), F_._ptr(zflat), plan.z_len, L.RANS_Z_AUTO,
                                          F_._stream()), "lic_rans_z_decode")
        return zflat

    def _encode_y_device(self, tables, center, y_sym, order, step_len, B: int, P: int, M: int):
        """The y streams of the "rans" coder without the host encoder: `lic_rans_encode_pick` turns tables (raster
        order, where `params_at` left them), centres and symbols into one start|freq word and one escape word per
        symbol in wavefront order, `lic_rans_encode` (`lic_rans_encode_groups` for G > 1) codes them, one wave per image
        and group.  Here: the slot rule of these kernels as a block table; buffers, the one upload
        of order and step lengths and the launches are `_RansEncoding`'s, the read-back is `rans_read_back`.
        -> ([stream bytes per image and group, image-major], [escape-list bytes likewise])"""
        G = self.groups
        # B images of one size: uniform slots, with room for the states (lic_rans_bound); G = 1: cap = all symbols
        layout = rans_block_layout([rans_group_sizes(step_len, G).max()] * B, G, 4 * RANS_LANES)
        enc = _RansEncoding(tables.device, "single", layout, G, B * P * M, B, dict(order=order, steps=step_len))
        enc.launch(tables, center, y_sym.contiguous(), M, self.y_W, P)
        return enc.read_back()

    def _coding_order(self, tables, center, y_sym, order, B: int, P: int, M: int):
        """tables and symbols of B images on the host, in coding order: (tables [B][P * M][S + 1] uint32, symbol -
        window start [B][P * M] int32), what the host coders take"""
        perm = torch.from_numpy(np.array(order, np.int64)).to(tables.device)
        idx = (y_sym - center + self.y_W).view(B, P, M)[:, perm].cpu().numpy().reshape(B, P * M)
        return tables.view(B, P, M, -1)[:, perm].cpu().numpy().view(np.uint32).reshape(B, P * M, -1), idx

    def _encode_y_host(self, tables, center, y_sym, order, step_len, B: int, P: int, M: int):
        """`_encode_y_device`'s arguments and result from the host encoder: tables and symbols are permuted into
        coding order on the device, copied, and coded image by image (`rans_encode_grouped`).  The same bytes."""
        tabs, idx = self._coding_order(tables, center, y_sym, order, B, P, M)
        pairs = [rans_encode_grouped(tabs[b], idx[b], step_len, self.groups) for b in range(B)]
        return [s for p in pairs for s in p[0]], [e for p in pairs for e in p[1]]

    def _optional_keys(self, z_esc=None) -> Dict:
        """the keys of `compress`'s strings that are there only when they say something: z_coder and z_esc, groups,
        slice_rows, schedule, coder"""
        keys = {"z_coder": "rans", "z_esc": z_esc} if self.z_coder == "rans" else {}
        said = {"groups": self.groups > 1, "slice_rows": self.slice_rows is not None,
                "schedule": self.schedule != "raster", "coder": self.coder == "rans"}
        return dict(keys, **{key: getattr(self, key) for key, yes in said.items() if yes})


class ContextCodec(_LayeredCodec):
    """compress(x) -> byte strings, decompress(strings) -> x_hat, through the model's masked-conv
    context (ContextModels.py:3-36): the parameters of pixel (i, j) of y depend on the already decoded
    pixels above / left of it, so decoding is serial -- but only along a wavefront: pixels with equal
    j + 3 i are independent (see _wavefront), so it takes w + 3 (h - 1) dependent steps of {12-tap context
    GEMM -> entropy-parameter MLP -> table kernel} on the GPU, each over a batch of pixels, and their
    symbols on the host coder in between.

    Encoder and decoder must build BIT-IDENTICAL tables, so both evaluate the context as the same
    per-pixel GEMM over the 12 live taps ([N, 12M, 1, 1] "images": the kernels' results for one row do
    not depend on the batch it sits in, and their split-K choice depends on per-image geometry only --
    the property tests/test_gpu_fullsize.py pins); the encoder simply has all N = B*h*w pixels at
    once.  One y stream per image (symbols step by step, pixel by pixel, channel by channel) + one z stream
    for the batch.

    `coder`: "range" (the default) codes y with the host range coder as described above; "rans" codes y with
    the 64-lane interleaved rANS coder of lic_codec.h, whose decoder is a device kernel
    (`lic_rans_decode_step`): the step loop is then {gather -> per-pixel layers -> tables -> decode}, all
    asynchronous launches, and the host reads back one small block after the last step.  z keeps the range coder
    unless `z_coder` says otherwise.
    Its kernels take `y_W` from 1 to 64 (RANS_MAX_W); the constructor refuses a wider window for this coder.

    `encoder`: where `compress` codes the y streams.  "host" (the default) gathers the tables into wavefront order,
    copies them to the host and runs the C++ encoder, one image after the other; "device" (coder "rans" only) runs
    `lic_rans_encode_pick` + `lic_rans_encode` on the tables where they were built and copies back state blocks,
    streams and escape lists only.  Both write the same bytes.

    `groups`: sub-streams per image of the "rans" coder (1 to 8, `rans_deal`).  1 (the default) is the rANS-64
    format; with G > 1 `strings["groups"]` is G and `strings["y"]`, `strings["y_esc"]` hold B * G entries,
    image-major (entry b * G + g), coded and decoded by G waves per image.  `decompress` reads G from the strings.

    `slice_rows`: None (the default) or R >= 1, coder "rans" only: latent rows per slice.  A context tap (dr, ds) with
    dr < 0 of pixel (i, j) contributes y_hat[i + dr, j + ds] only if (i mod R) + dr >= 0 and zero otherwise, exactly
    as a tap above the image does; taps of the pixel's own row are untouched.  The slices then advance together
    (`wavefront`): fewer, wider steps, for the rate the first rows of every slice lose with their context.  The model
    is not told: encoder and decoder evaluate the same layers on the same masked windows, so their tables agree and
    y_hat, x_hat are what the codec without slices reconstructs; only the bytes differ.  R >= h is that codec, byte
    for byte.  `strings["slice_rows"]` is R when slicing is on; `decompress` reads it from the strings.

    `z_coder`: "range" (the default: one host range-coder stream for the batch's z) or "rans" (coder "rans" only): every
    image's z as `groups` rANS-64 sub-streams of its own, coded by kernels (`_encode_z`, `_decode_z`) for any window
    z_S >= 2.  Then `strings["z_coder"]` is "rans" and `strings["z"]`, `strings["z_esc"]` are lists of B * G byte
    strings, image-major; the decoders read `z_coder` from the strings.  Nothing else changes: y streams, `y_crc32`
    and the decoded z_hat, y_hat, x_hat are bit for bit those of "range".

    A model with a checkerboard context (`context="checkerboard"`) is coded in the two steps of `two_pass` instead of
    the wavefront: every window is gathered from anchor(y_hat), nothing else differs.  It takes coder="rans" only and no
    `slice_rows`; `strings["schedule"]` is "checkerboard", the container is LICBITS7 (which needs z_coder="rans"), and
    either kind of codec refuses the other's strings and blobs on the host.

    A rate-level model (`rate_levels=Q`) codes at the quality given to `compress(x, quality)` and its kin:
    `strings["quality"]` holds it (as the float32 the container keeps), the decoders read it there, and
    `compress_image` wraps its container in a LICRATE1 envelope (bitstream.py) that carries q and Q.  Such a codec
    writes and reads envelopes only; a plain codec refuses them.  Blobs of different qualities decode together: only
    the two inverse gains are per item.

    This is the one-layer case of `_LayeredCodec`, which holds the gathers, the step loops and the whole of
    `decompress_many`, and both y encoders; what is written here is what one layer makes different: the range coder's
    loop, the containers LICBITS1 to 5, the batched encoder (`_compress_chunk`: its inputs only), the result of a
    compress (`_compressed`, for `compress` and `compress_many`), and for `decompress_many` `_item_streams` and
    `_finish`."""

    def __init__(self, model, z_lo: int = -64, z_S: int = 129, y_W: int = 32, coder: str = "range",
                 encoder: str = "host", groups: int = 1, slice_rows: int = None, z_coder: str = "range"):
        if z_coder not in Z_CODERS:
            raise CodecError(f"unknown z_coder {z_coder!r}: expected one of {Z_CODERS}")
        if z_coder == "rans" and coder != "rans":
            raise CodecError(f"z_coder='rans' needs coder='rans': the {coder!r} coder has no container for rANS z streams")
        if z_coder == "rans" and int(z_S) < 2:
            raise CodecError(f"z_S = {int(z_S)}: z_coder='rans' needs a window of at least 2 symbols")
        self.z_coder = z_coder
        if coder not in CODERS:
            raise CodecError(f"unknown coder {coder!r}: expected one of {CODERS}")
        if encoder not in ENCODERS:
            raise CodecError(f"unknown encoder {encoder!r}: expected one of {ENCODERS}")
        if encoder == "device" and coder != "rans":
            raise CodecError(f"encoder='device' needs coder='rans': the {coder!r} coder has no device encoder")
        if int(y_W) < 1:
            raise CodecError(f"y_W = {int(y_W)}: the window half-width must be at least 1")
        if coder == "rans" and int(y_W) > RANS_MAX_W:
            # the only rANS decoder is the device kernel: a wider stream could be written but never read
            raise CodecError(f"y_W = {int(y_W)}: coder='rans' takes windows of 1 to {RANS_MAX_W} "
                             "(the limit of its device kernels); the range coder has no such limit")
        self.model, self.z_lo, self.z_S, self.y_W, self.coder = model, int(z_lo), int(z_S), int(y_W), coder
        self.encoder = encoder
        self.groups = _groups(groups)
        if self.groups > 1 and coder != "rans":
            raise CodecError(f"groups={self.groups} needs coder='rans': the {coder!r} coder has one stream per image")
        self.slice_rows = None if slice_rows is None else _slice_rows(slice_rows)
        if self.slice_rows is not None and coder != "rans":
            raise CodecError(f"slice_rows={self.slice_rows} needs coder='rans': the {coder!r} coder has no sliced format")
        # the one-layer case of `_LayeredCodec`: all M channels, the model's one context model and MLP
        self._set_layers([CodecLayer(model, "context_model", "entropy_parameters")])
        if self.schedule == "checkerboard":
            if coder != "rans":
                raise CodecError(f"coder={coder!r}: a checkerboard context model needs coder='rans' (its two wide steps "
                                 "are for the device coder; the range coder has no container for them)")
            if self.slice_rows is not None:
                raise CodecError(f"slice_rows={self.slice_rows}: a checkerboard context model has no slices (slice_rows "
                                 "must be None): it decodes in two steps already")

    def _prepack(self):
        """the per-pixel layers of the codec's one layer, packed once (`CodecLayer.prepack`)"""
        return self.layers[0].prepack()

    def _act_at(self, windows: torch.Tensor, psi_px: torch.Tensor, layers, comb: torch.Tensor = None) -> torch.Tensor:
        """`CodecLayer.act_at` of the codec's one layer; `layers` is what `_prepack` gave"""
        return self.layers[0].act_at(windows, psi_px, layers, comb)

    def _params_at(self, windows: torch.Tensor, psi_px: torch.Tensor, layers, comb: torch.Tensor = None):
        """`_act_at`'s arguments -> (center [N, M], tables [N*M, S+1]) on the device"""
        return self.layers[0].params_at(windows, psi_px, layers, comb, self.y_W)

    def _windows_all(self, y_hat: torch.Tensor, slice_rows: int = None, psi: torch.Tensor = None):
        """[B, M, h, w] -> [B*h*w, 12M, 1, 1]: the live taps of every pixel (zeros outside the image and, with
        `slice_rows`, outside the pixel's slice).  With psi [B, 2M, h, w]: -> (those windows, the comb [B*h*w, 4M] whose
        last 2M columns hold the pixels' psi, the first 2M still unwritten): `_windows_layers` for the one layer"""
        ((win, comb),) = self._windows_layers(y_hat, slice_rows, psi)
        return win if psi is None else (win, comb)

    @torch.no_grad()
    def compress(self, x: torch.Tensor, quality: float = None) -> Dict:
        m = self.model
        q = self._quality(quality)
        out = m.analysis_hyperprior(x, training=False, quality=q)
        y_in, z_in = out["y_in"].contiguous(), out["z_in"]
        B, M, h, w = y_in.shape
        if self.z_coder == "rans":
            z_bytes, z_esc = self._encode_z(list(self._z_symbols(z_in)))
        else:
            z_bytes, z_esc = LatentCodec(m, self.z_lo, self.z_S, self.y_W).encode_z(z_in), None
        psi = self._hyper_synthesis(z_in, q).float()
        win, comb = self._windows_all(self._context_plane(out["y_in"]), self.slice_rows, psi)
        center, tables = self._params_at(win, None, self._prepack(), comb)
        y_sym = _rounded_nhwc(y_in).reshape(B * h * w, M)
        # symbols leave in the decoder's wavefront order (see _wavefront), M channels per pixel
        order, step_len, _ = _encode_layout_of(h, w, M, self.pad, self.slice_rows, self.groups, self.schedule)
        if self.coder == "rans":
            encode = self._encode_y_device if self.encoder == "device" else self._encode_y_host
            y_streams, y_esc = encode(tables, center, y_sym, order, step_len, B, h * w, M)
        else:
            tabs, idx = self._coding_order(tables, center, y_sym, order, B, h * w, M)
            y_streams, y_esc = [rc_encode(tabs[b], idx[b]) for b in range(B)], []
        return self._compressed(x, dict(self._optional_keys(z_esc), z=z_bytes, **self._quality_key(q)), y_streams, y_esc,
                                y_sym.cpu().numpy(), out["logp_y"].double().sum() + out["logp_z"].double().sum(), y_in, z_in)

    @staticmethod
    def _quality_key(q) -> Dict:
        return {} if q is None else {"quality": q}

    def _compressed(self, x, strings, y_streams, y_esc, h_sym: np.ndarray, logp, y_in, z_in) -> Dict:
        """What `compress` and `compress_many` return for one item, from its coded streams.  strings: z and the
        optional keys; h_sym: the item's latent symbols on the host, int32 in raster order; logp: the fp64 sum of its
        log-likelihoods -- a device scalar from `compress`, a host one from `compress_many`, and the estimate is
        divided where the sum lies (the two differ in the last bit now and then)."""
        B, M, h, w = y_in.shape
        npix = x.shape[0] * x.shape[2] * x.shape[3]
        if self.coder == "rans":
            strings["y_esc"] = y_esc
        coded = 8.0 * (_z_size(strings) + sum(len(s) for s in y_streams) + sum(len(e) for e in y_esc)) / npix
        # CRC-32 of every image's latent symbols, which the decoder checks (`_check_latents`)
        strings.update(y=y_streams, y_crc32=[_crc32_of(a) for a in h_sym.reshape(B, h * w * M)])
        return {"strings": strings, "shape": (B, M, h, w), "z_shape": tuple(z_in.shape), "bpp_coded": coded,
                "bpp_est": float(-logp / np.log(2.0) / npix), "y_in": y_in, "z_in": z_in}

    # ---- many images in one encode pass -----------------------------------------------------------
    @torch.no_grad()
    def compress_many(self, xs: Sequence[torch.Tensor], table_budget_bytes: int = 2 << 30, names=None,
                      quality=None) -> List[Dict]:
        """`compress` for several inputs at once (coder "rans", encoder "device").  xs: [B_i, 3, H_i, W_i] tensors as
        `compress` takes them (sides already multiples of 64), of any sizes; names: what to call an item in a message
        (default "item i").  -> one `compress` result per item: the same strings byte for byte, shape, z_shape,
        bpp_coded, bpp_est, y_in, z_in.

        Per item the transforms run exactly as in `compress`; the factorised z tables are built and copied once per
        call.  `table_budget_bytes` cuts the list into chunks, consecutive runs of whole items whose y tables
        (rows * M * (2 y_W + 2) * 4 bytes) fit the budget together, an item above it alone (`table_chunks`); a chunk
        is one pass of `_compress_chunk`, and chunking changes no byte.  `quality` (a rate-level model): one number for
        all items or one per item.  Everything the host can refuse is refused before the device is touched."""
        xs = list(xs)
        names = [f"item {i}" for i in range(len(xs))] if names is None else list(names)
        self._refuse_items(xs, names)
        qs = self._qualities(quality, len(xs))
        if not xs:
            return []
        M = self.model.M
        costs = [x.shape[0] * (x.shape[2] // 16) * (x.shape[3] // 16) * M * (2 * self.y_W + 2) * 4 for x in xs]
        zt = factorized_tables(self.model.factorized_entropy_model, self.z_lo, self.z_S).cpu().numpy().view(np.uint32)
        out = []
        for first, end in table_chunks(costs, int(table_budget_bytes)):
            out += self._compress_chunk(xs[first:end], zt, names[first:end], qs[first:end])
        return out

    def _compress_chunk(self, xs, zt: np.ndarray, names, qs) -> List[Dict]:
        """One pass of `compress_many`.  After every item's transforms: all y_in and psi planes in two flat buffers
        (every item on a multiple of 4 floats, plain NHWC planes), ONE `lic_ctx_gather_ragged` over every pixel of
        every image (rows image-major, raster order inside an image), ONE `_params_at` over all rows, ONE
        `lic_rans_encode_pick_ragged` and ONE `lic_rans_encode_ragged`.  Written here: the inputs of those calls
        (`ragged_encode_plan`, `plane_layout`).  Buffers, the one upload and the launches are `_RansEncoding`'s, the
        read-back is `rans_read_back`, every item's result is `_compressed`'s.  The device -> host copies that wait do
        not grow with the images: the z symbols of all items, the state blocks, the word buffer, the used escape
        entries, the symbols for the checksums and the rate estimates."""
        m, G, R = self.model, self.groups, self.slice_rows
        M, dev = m.M, xs[0].device
        outs, psis, sums = [], [], []
        for x, q in zip(xs, qs):
            out = m.analysis_hyperprior(x, training=False, quality=q)
            outs.append((out["y_in"].contiguous(), out["z_in"], self._context_plane(out["y_in"])))
            psis.append(self._hyper_synthesis(out["z_in"], q).float())
            sums.append(out["logp_y"].double().sum() + out["logp_z"].double().sum())
        owner = [(i, b) for i, (y_in, _, _) in enumerate(outs) for b in range(y_in.shape[0])]
        name = lambda im: f"{names[owner[im][0]]}: image {owner[im][1]}"
        # z: the symbols of all items in one read-back, one host range coder run per item as `compress` has it -- or,
        # with z_coder="rans", every image of every item in one pick and one encode launch, cut per item below
        zs, zes, at = [], None, 0
        if self.z_coder == "rans":
            zs, zes = self._encode_z([row for _, z, _ in outs for row in self._z_symbols(z)], name)
        else:
            z_sym = [(_rounded_nhwc(z) - self.z_lo).reshape(-1) for _, z, _ in outs]
            z_all = torch.cat(z_sym).cpu().numpy()
            for z in z_sym:
                zs.append(rc_encode_z(zt, z_all[at:at + z.numel()]))
                at += z.numel()
        cpsi = psis[0].shape[1]
        shapes = [(y_in.shape[2], y_in.shape[3]) for y_in, _, _ in outs for _ in range(y_in.shape[0])]
        nimg = len(shapes)
        plan = ragged_encode_plan(shapes, M, self.pad, R, G, self.schedule)
        lay = plane_layout([(y_in.shape[0], y_in.shape[2], y_in.shape[3]) for y_in, _, _ in outs], M, cpsi, 0,
                           [R] * nimg)                                     # no frame: the gather never leaves a plane
        yflat = torch.empty(lay.y_len, device=dev, dtype=torch.float32)
        psiflat = torch.empty(lay.psi_len, device=dev, dtype=torch.float32)
        y_syms = []
        for (y_in, _, y_raw), psi, y_at, psi_at in zip(outs, psis, lay.y_at.tolist(), lay.psi_at.tolist()):
            B, _, h, w = y_in.shape
            yflat[y_at:y_at + B * h * w * M].view(B, h, w, M).copy_(F_._nhwc(y_raw))
            psiflat[psi_at:psi_at + B * h * w * cpsi].view(B, h * w, cpsi).copy_(F_._nhwc(psi).view(B, h * w, -1))
            y_syms.append(_rounded_nhwc(y_in).reshape(B * h * w, M))
        y_sym = torch.cat(y_syms) if len(y_syms) > 1 else y_syms[0]
        # one upload of everything the kernels index with, the gather's descriptors and rows included
        row_pix = np.concatenate([np.arange(h * w, dtype=np.int64) for h, w in shapes])
        enc = _RansEncoding(dev, "ragged", (plan.blocks, plan.words_len, plan.esc_len), G, plan.total_rows * M, nimg,
                            dict(desc=lay.desc, images=plan.images, blocks=plan.blocks, row_image=plan.row_image,
                                 row_pix=row_pix, order=plan.order, steps=plan.step_len))
        ((win, comb),) = self._gather_rows(self.layers, yflat, M, enc.d["desc"].view(nimg, -1), enc.d["row_image"],
                                           enc.d["row_pix"], psiflat, cpsi)
        center, tables = self._params_at(win, None, self._prepack(), comb)
        enc.launch(tables, center, y_sym, M, self.y_W, plan.total_rows)
        streams, escs = enc.read_back(name)
        h_sym = y_sym.cpu().numpy()
        h_sums = torch.stack(sums).cpu().numpy()
        res, img = [], 0
        for i, ((y_in, z_in, _), x) in enumerate(zip(outs, xs)):
            B, _, h, w = y_in.shape
            row0, cut = int(plan.images[img, 0]), slice(img * G, (img + B) * G)
            strings = self._optional_keys(zes[cut]) if zes is not None else self._optional_keys()
            strings.update(self._quality_key(qs[i]))
            res.append(self._compressed(x, dict(strings, z=zs[cut] if zes is not None else zs[i]), streams[cut], escs[cut],
                                        h_sym[row0:row0 + B * h * w], h_sums[i], y_in, z_in))
            img += B
        return res

    @torch.no_grad()
    def decompress(self, strings: Dict, shape, z_shape, quality: float = None) -> Dict:
        """`quality` (a rate-level model): the quality the strings were coded at; default: strings["quality"]"""
        m = self.model
        B, M, h, w = shape
        self._refuse_other_schedule(strings)
        if quality is not None:
            strings = dict(strings, quality=quality)
        strings = self._with_quality(strings)
        dev = next(m.parameters()).device
        z_coder, staged = _z_coder_of(strings), None
        if z_coder == "rans":
            # y and z blocks are staged together: z decodes in one launch ahead of the step loop and its state blocks
            # come back with the y blocks', in the one read-back after the last step
            G = _groups(strings.get("groups", 1))
            staged = _stage_y_and_z(strings["y"], strings.get("y_esc"), B, strings["z"], strings.get("z_esc"), B, G)
            staged.upload(dev)
            zflat = self._decode_z(staged, B * G, z_plan([(z_shape, (self.z_lo, self.z_S))], M), dev)
            z_hat = self._z_view(zflat, 0, z_shape)
        else:
            z_hat = LatentCodec(m, self.z_lo, self.z_S, self.y_W).decompress_z(strings["z"], z_shape)
        z_hat = z_hat.contiguous(memory_format=torch.channels_last)
        psi = self._hyper_synthesis(z_hat, strings.get("quality")).float()
        p = self.pad
        # decoded latents, pixel-major, inside a zero frame
        ypad = torch.zeros((B, h + 2 * p, w + 2 * p, M), device=dev, dtype=torch.float32)
        yflat = ypad.view(B, -1, M)
        coder = strings.get("coder", "range")
        if coder not in CODERS:
            raise CodecError(f"unknown coder {coder!r} in the strings")
        R = None if strings.get("slice_rows") is None else _slice_rows(strings["slice_rows"])
        if R is not None and coder != "rans":
            raise CodecError(f"the strings name slice_rows with coder {coder!r}: only 'rans' streams have slices")
        steps = self._wavefront(h, w, R)
        front = self._step_front_end(steps, yflat, psi, R)
        if coder == "rans":
            self._decode_y_rans(strings, front, yflat, staged)
            return self._finish(strings, ypad, z_hat, shape)
        pin = dev.type == "cuda"
        nmax, S1 = max(len(ii) for ii, _ in steps), 2 * self.y_W + 2
        tabs_host = torch.empty((B, nmax * M, S1), dtype=torch.int32, pin_memory=pin)
        c_host = torch.empty((B, nmax * M), dtype=torch.int32, pin_memory=pin)
        vals_host = torch.empty((B, nmax * M), dtype=torch.float32, pin_memory=pin)
        tabs_np, c_np, vals_np = tabs_host.numpy().view(np.uint32), c_host.numpy(), vals_host.numpy()
        decs = [_StreamDecoder(s) for s in strings["y"]]
        try:
            for n, own, ((center, tables),) in front:
                tabs_host[:, :n * M].copy_(tables.view(B, n * M, S1), non_blocking=True)
                c_host[:, :n * M].copy_(center.view(B, n * M), non_blocking=True)
                torch.cuda.current_stream().synchronize()
                for b in range(B):
                    vals_np[b, :n * M] = decs[b].next(tabs_np[b, :n * M], n * M) + c_np[b, :n * M] - self.y_W
                yflat.index_copy_(1, own, vals_host[:, :n * M].to(dev, non_blocking=True).view(B, n, M))
        finally:
            for d in decs:
                d.close()
        return self._finish(strings, ypad, z_hat, shape)

    def _decode_y_rans(self, strings, front, yflat, staged=None):
        """The step loop of the "rans" coder (`_run_steps`): streams, escape lists and state blocks go up once, then
        every step of `front` ends in lic_rans_decode_step_groups.  Nothing in the loop waits for the
        device; the state blocks (error words, cursors, final states) come back once, after the last step.  One block
        per image and group (`strings["groups"]`, 1 if absent), image-major.  `staged`: the
        staging `decompress` has already uploaded, with the z blocks behind the y blocks (z_coder="rans")."""
        G = _groups(strings.get("groups", 1))
        if staged is None:
            staged = _RansStaging(strings["y"], strings.get("y_esc"), yflat.shape[0], G)
            blocks = staged.upload(yflat.device)
        else:
            blocks = staged.blocks_from(0)
        self._run_steps(front, yflat, blocks, G)
        staged.check()

    def _finish(self, strings, ypad, z_hat, shape) -> Dict:
        """checksum of the decoded latents, then the synthesis transform"""
        m, p = self.model, self.pad
        B, M, h, w = shape
        if "y_crc32" in strings:
            got = ypad[:, p:p + h, p:p + w, :].reshape(B, h * w * M).round().to(torch.int32).cpu().numpy()
            _check_latents(got.reshape(B, h, w, M), 0, M, strings["y_crc32"])
        y_hat = ypad[:, p:p + h, p:p + w, :].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        x_hat = m.synthesis(y_hat, strings.get("quality"))
        return {"x_hat": x_hat, "y_hat": y_hat, "z_hat": z_hat}

    def _with_quality(self, strings: Dict) -> Dict:
        """the strings with their quality as this codec's model takes it (`_quality`'s refusals)"""
        q = self._quality(strings.get("quality"))
        return strings if q is None else dict(strings, quality=q)

    # ---- many bitstreams in one step loop -------------------------------------------------------
    @torch.no_grad()
    def decompress_many(self, items, z_windows=None, names=None) -> List[Dict]:
        """`decompress` for several bitstreams at once.  items: [(strings, shape, z_shape)] as `decompress` takes
        them, all of the "rans" coder, this codec's y_W and one G; they may differ in B, h, w and slice_rows.
        z_windows: [(z_lo, z_S)] per item (default: this codec's); names: what to call an item in a message (default
        "item i").  -> one `decompress` result per item, bit for bit what `decompress` gives for it alone.

        `_LayeredCodec._decompress_many` is the body, here with the one layer: every step of its loop is
        {lic_ctx_gather_ragged -> per-pixel layers and tables over the step's rows of every image ->
        lic_rans_decode_step_ragged}.  An item's z may be range-coded (decoded on the host, as `decompress` does) or
        rANS-coded (`strings["z_coder"]`; those decode together).  Everything the host can refuse is refused before the
        device is touched."""
        items = list(items)
        for i, (strings, shape, z_shape) in enumerate(items):
            try:
                if strings.get("coder", "range") != "rans":
                    raise CodecError("only streams of the 'rans' coder decode together (the range coder's loop waits for "
                                     "the host at every step)")
                items[i] = (self._with_quality(strings), shape, z_shape)
            except CodecError as err:
                raise CodecError(f"{f'item {i}' if names is None else names[i]}: {err}") from None
        return self._decompress_many(items, self.layers, z_windows, names)

    def _item_streams(self, strings, shape, z_shape, G: int, nlayers: int):
        """`_decompress_many`'s view of one item, after this codec's refusals -> ([(y streams, escape lists, checksums
        or None)] for the one layer, (z streams, escape lists) or None for a range-coded z)"""
        B, Mi = shape[0], shape[1]
        if Mi != self.model.M:
            raise CodecError(f"{Mi} latent channels, this model has {self.model.M}")
        if strings.get("y_esc") is None or len(strings["y"]) != B * G or len(strings["y_esc"]) != B * G:
            raise CodecError("one y stream and one escape list per image and group expected")
        y = [(strings["y"], strings["y_esc"], strings.get("y_crc32"))]
        if _z_coder_of(strings) != "rans":
            return y, None
        if z_shape[0] != B:
            raise CodecError("z_shape and shape name different batch sizes")
        return y, _z_streams(strings, B * G)

    # ---- self-describing container: one byte string per batch, any image size ---------------------
    @torch.no_grad()
    def compress_image(self, x: torch.Tensor, mode: str = "replicate", align: str = "topleft",
                       coder: str = None, quality: float = None) -> bytes:
        """x [B,3,H,W] of ANY size -> one byte string that `decompress_image` decodes by itself.  The image is padded
        to multiples of 64 (`functional.pad_to_multiple`) and the payload is exactly what `compress` produces for
        the padded tensor; the header (bitstream.py) carries everything the decoder needs to rebuild the
        shapes and to crop back.  bpp_coded of the result is 8 * len(data) / (B * H * W): header and checksums
        included, per ORIGINAL pixel.  `coder`: None = this codec's own; the container is the one `_FORMATS` has for
        (coder, groups > 1): LICBITS1 for "range", LICBITS2 for "rans", LICBITS3 for "rans" with groups -- and LICBITS4
        for a codec with slices, whatever its groups, LICBITS5 for one with z_coder="rans", whatever its groups and
        slices.  Slices, groups and z_coder do not follow to another coder.  A rate-level model: coded at `quality`, and
        the container sits in a LICRATE1 envelope that carries it."""
        if x.dim() != 4:
            raise CodecError("expected a [B,3,H,W] tensor")
        quality = self._quality(quality)
        if coder is not None and coder != self.coder:
            # encoder and groups go with the coder they belong to: only a coder that has a grouped format ("rans")
            # has a device encoder
            enc, G = (self.encoder, self.groups) if (coder, True) in _FORMATS else ("host", 1)
            return ContextCodec(self.model, self.z_lo, self.z_S, self.y_W, coder, enc, G).compress_image(
                x, mode, align, quality=quality)
        self._refuse_checkerboard_without_zrans()
        return self._pack_padded(x, self.compress(F_.pad_to_multiple(x, 64, mode, align), quality)["strings"], align)

    def _pack_image(self, s: Dict, B: int, H: int, W: int, top: int, left: int) -> bytes:
        """the container of `compress_image` around the strings `compress` gave for the padded image; for a rate-level
        model inside the envelope that carries the quality"""
        inner = self._pack_container(s, B, H, W, top, left)
        if self.rate_levels is None:
            return inner
        return pack_rate_envelope(inner, s["quality"], self.rate_levels)

    def _pack_container(self, s: Dict, B: int, H: int, W: int, top: int, left: int) -> bytes:
        head = {"family": self._family(), "M": self.model.M, "K": self.model.K, "z_lo": self.z_lo, "z_S": self.z_S,
                "y_W": self.y_W, "B": B, "H": H, "W": W, "top": top, "left": left}
        if self.schedule == "checkerboard":
            self._refuse_checkerboard_without_zrans()
            return _pack(_FORMAT_CHECKER, dict(head, slice_rows=0), (s["z"], s["z_esc"]), s["y"], s["y_esc"],
                         s["y_crc32"], self.groups)
        if self.z_coder == "rans":
            return _pack(_FORMAT_ZRANS, dict(head, slice_rows=self.slice_rows or 0), (s["z"], s["z_esc"]), s["y"],
                         s["y_esc"], s["y_crc32"], self.groups)
        if self.slice_rows is not None:
            return _pack((self.coder, "sliced"), dict(head, slice_rows=self.slice_rows), s["z"], s["y"], s["y_esc"],
                         s["y_crc32"], self.groups)
        return _pack((self.coder, self.groups > 1), head, s["z"], s["y"], s.get("y_esc"), s["y_crc32"], self.groups)

    def _refuse_checkerboard_without_zrans(self):
        if self.schedule == "checkerboard" and self.z_coder != "rans":
            raise CodecError(f"z_coder={self.z_coder!r}: the container of the checkerboard schedule (LICBITS7) carries z as "
                             "rANS sub-streams, as LICBITS5 does: build the codec with z_coder='rans'")

    def _refuse_items(self, xs, names, also=lambda: None):
        """what `compress_many` refuses of its items before the device is touched, item by item, named; `also`: what a
        caller refuses of the codec besides"""
        for x, name in zip(xs, names):
            try:
                self._refuse_unless_batched_encoder()
                also()
                if not isinstance(x, torch.Tensor) or x.dim() != 4:
                    raise CodecError("expected a [B,3,H,W] tensor")
                if not x.is_cuda:
                    raise CodecError("expected a tensor on the GPU: the device encoder runs where the tables are built")
            except CodecError as err:
                raise CodecError(f"{name}: {err}") from None

    def _refuse_unless_batched_encoder(self):
        if self.coder != "rans" or self.encoder != "device":
            raise CodecError(f"this codec has coder={self.coder!r}, encoder={self.encoder!r}: images are encoded "
                             "together by the device encoder of the 'rans' coder only (coder='rans', encoder='device'); "
                             "encode them one by one with compress_image")

    @torch.no_grad()
    def compress_images(self, images: Sequence[torch.Tensor], mode: str = "replicate", align: str = "topleft",
                        table_budget_bytes: int = 2 << 30, quality=None) -> List[bytes]:
        """Many images of any sizes in one encode pass: entry i is byte for byte `compress_image(images[i], mode,
        align)`, the container of this codec's groups, slice_rows and z_coder (LICBITS2 / 3 / 4 / 5).  All images of a
        chunk share
        one gather, one pass through the per-pixel layers, one table launch and one launch of each encoder kernel
        (`compress_many`, which also says what `table_budget_bytes` does).  Needs coder="rans", encoder="device".
        Raises CodecError before any GPU work, every message naming its entry ("image i: ..."): a codec with another
        coder or encoder, an entry that is not a [B,3,H,W] tensor, a tensor that is not on the GPU.  An empty list
        gives an empty list.  `quality` (a rate-level model): one number for all images or a list, one per image."""
        images = list(images)
        names = [f"image {i}" for i in range(len(images))]
        self._refuse_items(images, names, self._refuse_checkerboard_without_zrans)
        qs = self._qualities(quality, len(images), "image")
        if not images:
            return []
        rs = self.compress_many([F_.pad_to_multiple(x, 64, mode, align) for x in images], table_budget_bytes, names, qs)
        return [self._pack_padded(x, r["strings"], align) for x, r in zip(images, rs)]

    @torch.no_grad()
    def compress_image_to(self, x: torch.Tensor, max_bytes: int, steps: int = 16, **kw):
        """-> (blob, quality): `compress_image(x, quality=q, **kw)` at the highest q of the grid k (Q-1) / steps,
        k = 0..steps, whose blob has at most `max_bytes` bytes (a rate-level model).  Bisection over k, which assumes
        that the size grows with q; the blob returned is measured, and if it does not fit the grid is walked down from
        it until one does.  CodecError when not even q = 0 fits."""
        Q = self.rate_levels
        if Q is None:
            raise CodecError("compress_image_to picks a quality: this codec's model has no rate levels")
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
            raise CodecError(f"steps = {steps!r}: expected an integer >= 1")
        blobs = {}

        def at(k):
            if k not in blobs:
                blobs[k] = self.compress_image(x, quality=k * (Q - 1) / steps, **kw)
            return blobs[k]

        lo, hi = 0, int(steps)                    # the bisection keeps: grid point lo is the answer so far
        if len(at(hi)) <= max_bytes:
            lo = hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if len(at(mid)) <= max_bytes:
                lo = mid
            else:
                hi = mid
        while lo > 0 and len(at(lo)) > max_bytes:  # (the size did not grow with q after all)
            lo -= 1
        if len(at(lo)) > max_bytes:
            raise CodecError(f"the image takes {len(at(0))} bytes at quality 0: it does not fit max_bytes = {max_bytes}")
        return at(lo), quality_of(at(lo))

    @torch.no_grad()
    def decompress_image(self, data: bytes) -> torch.Tensor:
        """The inverse of `compress_image`: x_hat [B,3,H,W] (channels_last).  Raises CodecError, before any GPU
        work, for a bad magic, a truncated buffer, a failing CRC or a header whose family / M / K are not this
        model's.  The magic selects the coder, whatever this codec's own is."""
        head, strings = self._open_blob(data)
        m = self.model
        dec = self
        if (head["z_lo"], head["z_S"], head["y_W"]) != (self.z_lo, self.z_S, self.y_W):
            dec = ContextCodec(m, head["z_lo"], head["z_S"], head["y_W"], strings.get("coder", "range"))
        out = dec.decompress(strings, *self._shapes(head, m.M))
        return F_.crop_window(out["x_hat"], head["top"], head["left"], head["H"], head["W"])

    def _open_blob(self, data: bytes):
        """`decompress_image`'s host half -> (header, the strings `decompress` takes).  Its refusals, in order: the
        container reader's (`_unpack`), a window the rANS decoder does not take, a model that is not this one."""
        quality = None
        if self.rate_levels is not None:
            quality, _, data = unpack_rate_envelope(data, self.rate_levels)
        elif is_rate_envelope(data):
            raise CodecError("a LICRATE1 rate envelope: this codec's model has no rate levels (rate_levels=None) and reads "
                             "bare bitstreams only")
        fmt = _format_of_magic(data[:8])                                      # an unknown magic: LICBITS1's reader says so
        head, z_bytes, y_streams, y_esc, y_crc, G = _unpack(fmt, data)
        strings = {"y": y_streams, "z": z_bytes, "y_crc32": y_crc, **self._quality_key(quality)}
        if (fmt == _FORMAT_CHECKER) != (self.schedule == "checkerboard"):
            raise CodecError(f"schedule mismatch: a {bytes(data[:8]).decode()} bitstream is coded in the "
                             f"{'checkerboard' if fmt == _FORMAT_CHECKER else 'raster'} schedule, this codec's context "
                             f"model decodes the {self.schedule} schedule")
        if fmt == _FORMAT_CHECKER:
            strings["schedule"] = "checkerboard"
        if fmt in (_FORMAT_ZRANS, _FORMAT_CHECKER):
            if not 2 <= head["z_S"] <= L.RANS_Z_MAX_S:
                raise CodecError(f"bitstream names z_S = {head['z_S']}; the rANS decoder of z takes windows of 2 to "
                                 f"{L.RANS_Z_MAX_S} symbols")
            strings.update(z_coder="rans", z=z_bytes[0], z_esc=z_bytes[1])
        if fmt[0] == "rans":
            if head["y_W"] > RANS_MAX_W:
                raise CodecError(f"bitstream names y_W = {head['y_W']}; the rANS decoder takes windows of 1 to "
                                 f"{RANS_MAX_W}")
            strings.update(coder="rans", y_esc=y_esc, **({"groups": G} if G > 1 else {}))
            if "slice_rows" in head:
                strings["slice_rows"] = head["slice_rows"]
        m = self.model
        if (head["family"], head["M"], head["K"]) != (self._family(), m.M, m.K):
            raise CodecError(f"bitstream was written by family {head['family']} with M={head['M']}, K={head['K']}; "
                             f"this model is family {self._family()} with M={m.M}, K={m.K}")
        return head, strings

    @torch.no_grad()
    def decompress_images(self, blobs: Sequence[bytes]) -> List[torch.Tensor]:
        """Many `compress_image` blobs in one decode loop: entry i is bit for bit `decompress_image(blobs[i])`,
        [B_i, 3, H_i, W_i], channels_last, cropped.  The blobs may differ in size, batch, crop, slice_rows, z window and
        between LICBITS2 / 3 / 4 / 5; step t of all their images shares its launches (`decompress_many`), so a folder of
        blobs costs about one blob's step loop plus every blob's transforms.  Raises CodecError before any GPU work,
        every message naming its blob ("blob i: ..."): whatever `decompress_image` refuses for blob i; a LICBITS1 blob
        (the range coder's loop waits for the host at every step: nothing to merge); a y_W or a G (sub-streams per
        image; 1 for LICBITS2) that is not blob 0's.  An empty list gives an empty list."""
        blobs = list(blobs)
        opened = []
        for i, data in enumerate(blobs):
            try:
                opened.append(self._open_blob(data))
            except CodecError as err:
                raise CodecError(f"blob {i}: {err}") from None
        if not opened:
            return []
        for i, (head, strings) in enumerate(opened):
            if strings.get("coder", "range") != "rans":
                raise CodecError(f"blob {i}: a LICBITS1 blob (range coder) cannot join a batched decode: its loop waits "
                                 "for the host at every step; decode it with decompress_image")
        y_W = self._one_window_one_G(opened)
        m = self.model
        items = [(strings, *self._shapes(head, m.M)) for head, strings in opened]
        dec = self if y_W == self.y_W else ContextCodec(m, self.z_lo, self.z_S, y_W, "rans")
        outs = dec.decompress_many(items, [(head["z_lo"], head["z_S"]) for head, _ in opened],
                                   [f"blob {i}" for i in range(len(opened))])
        return [F_.crop_window(out["x_hat"], head["top"], head["left"], head["H"], head["W"])
                for out, (head, _) in zip(outs, opened)]


class ScalableCodec(_LayeredCodec):
    """The bitstream of `models.ScalableImageCoding`: the base latent y1 (the model's first `base_channels` channels)
    and the enhancement latent y2 travel as separate, separately decodable bytes, so a vision client downloads and
    decodes z and y1 and stops there (`decompress_base`, `decompress_base_image`).

    Two layers (`CodecLayer`): layer l's tables come from `context_model_l` on y_l ALONE plus the shared psi, so layer 0
    never reads y2, and layer l codes its symbols in wavefront step order, pixel by pixel, over its own M_l channels --
    exactly what a one-layer codec over those channels does.  rANS only: every layer's y as "rANS-64 x G" sub-streams
    of its own, z as rANS sub-streams (`ContextCodec(z_coder="rans")`'s), groups and slice_rows as there.  The decode
    loop runs both layers' steps together: per step ONE gather (`lic_ctx_gather_layers`) from the one M-channel plane
    and the one psi, the per-pixel layers and tables per layer, and ONE decode launch (`lic_rans_decode_step_layers`)
    whose waves of both layers run side by side.  A base-only decode is the one-layer loop over an M1-channel plane.
    `encoder`: "device" (the default) or "host" (`rans_encode_grouped` from tables copied back); the same bytes.

    `compress` returns strings with `layers` = [{"y": [B*G], "y_esc": [B*G], "y_crc32": [B]}, the same for layer 1],
    `z`, `z_esc`, `z_coder`, `coder`, and `groups` / `slice_rows` when set; `bpp_coded` and `bpp_coded_base` count the
    LICBITS6 container (bitstream.py) that `compress_image` writes, header and checksums included: all of it, and its
    first `base_bytes` (header, z and layer 0).

    Many blobs decode in ONE step loop: `decompress_images` (the pictures) and `decompress_base_images` (whole blobs or
    base prefixes, the base layer alone) advance step t of every image of every blob together (`decompress_many`, which
    is `_LayeredCodec._decompress_many` with this codec's `_item_streams` and `_finish`): per step one
    `lic_ctx_gather_layers_ragged` and one `lic_rans_decode_step_layers_ragged` for all images and layers, so N blobs
    cost about one blob's step loop plus every blob's transforms; every entry is bit for bit the single-blob call's.
    One call decodes one depth.  Several images are still encoded one after the other (`compress_images`)."""

    def __init__(self, model, z_lo: int = -64, z_S: int = 129, y_W: int = 32, encoder: str = "device", groups: int = 1,
                 slice_rows: int = None):
        from .models import ScalableImageCoding
        if getattr(model, "rate_levels", None) is not None:
            raise CodecError(f"ScalableCodec takes no rate-level model (rate_levels={model.rate_levels}): the layered "
                             "bitstream has one rate; ContextCodec codes a rate-level model")
        if not isinstance(model, ScalableImageCoding):
            raise CodecError(f"ScalableCodec codes a ScalableImageCoding model, not a {type(model).__name__}: "
                             "the one-layer models have ContextCodec")
        if encoder not in ENCODERS:
            raise CodecError(f"unknown encoder {encoder!r}: expected one of {ENCODERS}")
        if int(z_S) < 2:
            raise CodecError(f"z_S = {int(z_S)}: the rANS coder of z needs a window of at least 2 symbols")
        if int(y_W) < 1:
            raise CodecError(f"y_W = {int(y_W)}: the window half-width must be at least 1")
        if int(y_W) > RANS_MAX_W:
            raise CodecError(f"y_W = {int(y_W)}: the rANS coder takes windows of 1 to {RANS_MAX_W} (the limit of its "
                             "device kernels)")
        self.model, self.z_lo, self.z_S, self.y_W, self.encoder = model, int(z_lo), int(z_S), int(y_W), encoder
        self.coder = self.z_coder = "rans"
        self.groups = _groups(groups)
        self.slice_rows = None if slice_rows is None else _slice_rows(slice_rows)
        self._set_layers([CodecLayer(model, "context_model_1", "entropy_parameters_1", 0, "M1"),
                          CodecLayer(model, "context_model_2", "entropy_parameters_2", model.M1, "M2")])
        if self.schedule != "raster":
            raise CodecError(f"the layered codec has the raster schedule only, these context masks are {self.schedule}")

    @torch.no_grad()
    def compress(self, x: torch.Tensor) -> Dict:
        m = self.model
        if x.dim() != 4 or x.shape[2] % 64 or x.shape[3] % 64:
            raise CodecError("expected a [B,3,H,W] tensor with H and W multiples of 64 (compress_image pads any size)")
        if m.use_step_prep and x.is_cuda:
            m.step_prep().run()
        y = m.encoder(x)
        z_in, y_in = F_.quantize(m.hyper_encoder(y), None, False), F_.quantize(y, None, False).contiguous()
        B, M, h, w = y_in.shape
        z_bytes, z_esc = self._encode_z(list(self._z_symbols(z_in)))
        psi = m.hyper_decoder(z_in).float()
        y_sym_all = _rounded_nhwc(y_in).reshape(B * h * w, M)
        encode = self._encode_y_device if self.encoder == "device" else self._encode_y_host
        logp = m.factorized_entropy_model.likelihood_and_log(z_in)[1].double().sum()
        coded = []
        for ly, (win, comb) in zip(self.layers, self._windows_layers(y_in, self.slice_rows, psi)):
            act = ly.act_at(win, None, ly.prepack(), comb)
            center, tables = gmm_tables(act, ly.M, ly.K, self.y_W)
            y_sym = y_sym_all[:, ly.c0:ly.c0 + ly.M].contiguous()
            order, step_len, _ = _encode_layout_of(h, w, ly.M, self.pad, self.slice_rows, self.groups, self.schedule)
            streams, escs = encode(tables, center, y_sym, order, step_len, B, h * w, ly.M)
            coded.append({"y": streams, "y_esc": escs,
                          "y_crc32": [_crc32_of(a) for a in y_sym.reshape(B, h * w * ly.M).cpu().numpy()]})
            y_l = y_in[:, ly.c0:ly.c0 + ly.M]
            logp = logp + m.conditional.packed_likelihood_and_log(
                y_l, act.reshape(B, h, w, -1).permute(0, 3, 1, 2), ly.K)[1].double().sum()
        strings = dict(self._optional_keys(z_esc), layers=coded, z=z_bytes)
        npix = B * x.shape[2] * x.shape[3]
        blob = self._pack_image(strings, B, x.shape[2], x.shape[3], 0, 0)      # the ledger counts the container
        base_bytes = self.base_bytes_of(blob)
        return {"strings": strings, "shape": (B, M, h, w), "z_shape": tuple(z_in.shape),
                "bpp_coded": 8.0 * len(blob) / npix, "bpp_coded_base": 8.0 * base_bytes / npix,
                "bpp_est": float(-logp / np.log(2.0) / npix), "y_in": y_in, "z_in": z_in}

    def _item_streams(self, strings, shape, z_shape, G: int, nlayers: int):
        """One item's streams after this codec's refusals, for `_decode` and `_decompress_many` -> ([(y streams, escape
        lists, checksums)] of the first `nlayers` layers, (z streams, escape lists)).  Later layers are not touched."""
        B, M = shape[0], shape[1]
        if M != self.model.M or z_shape[0] != B:
            raise CodecError(f"shape names {M} latent channels and z_shape {z_shape[0]} images; this model has "
                             f"{self.model.M} channels and shape {B} images")
        coded = strings.get("layers")
        if not isinstance(coded, (list, tuple)) or len(coded) < nlayers:
            raise CodecError(f"the strings hold {0 if not isinstance(coded, (list, tuple)) else len(coded)} layers; "
                             f"{nlayers} are to be decoded")
        for l, c in enumerate(coded[:nlayers]):
            if c.get("y_esc") is None or len(c["y"]) != B * G or len(c["y_esc"]) != B * G or len(c["y_crc32"]) != B:
                raise CodecError(f"layer {l}: one y stream and one escape list per image and group and one checksum "
                                 "per image expected")
        return [(c["y"], c["y_esc"], c["y_crc32"]) for c in coded[:nlayers]], _z_streams(strings, B * G)

    def _decode(self, strings: Dict, shape, z_shape, nlayers: int) -> Dict:
        """z, then the first `nlayers` layers in one step loop, then `_finish`"""
        m, p = self.model, self.pad
        B, M, h, w = shape
        dev = next(m.parameters()).device
        use = self.layers[:nlayers]
        G = _groups(strings.get("groups", 1))
        coded, (zs, zescs) = self._item_streams(strings, shape, z_shape, G, nlayers)
        R = None if strings.get("slice_rows") is None else _slice_rows(strings["slice_rows"])
        # layer-major blocks, the z blocks behind them: one upload, one read-back
        staged = _stage_y_and_z([s for y, _, _ in coded for s in y], [e for _, esc, _ in coded for e in esc], nlayers * B,
                                zs, zescs, B, G, lambda i: f"image {i % B}{self._what(i // B)}", _image_name)
        blocks = staged.upload(dev)
        zflat = self._decode_z(staged, nlayers * B * G, z_plan([(z_shape, (self.z_lo, self.z_S))], M), dev)
        z_hat = self._z_view(zflat, 0, z_shape).contiguous(memory_format=torch.channels_last)
        psi = m.hyper_decoder(z_hat).float()
        y_pix = sum(ly.M for ly in use)                    # the layers are consecutive from channel 0
        ypad = torch.zeros((B, h + 2 * p, w + 2 * p, y_pix), device=dev, dtype=torch.float32)
        yflat = ypad.view(B, -1, y_pix)
        front = self._step_front_end(self._wavefront(h, w, R), yflat, psi, R, use)
        self._run_steps(front, yflat, blocks, G, use)
        staged.check()
        return self._finish(strings, ypad, z_hat, shape)

    def _finish(self, strings, ypad, z_hat, shape) -> Dict:
        """The checksums of the layers whose channels `ypad` holds, then what `decompress` returns for both layers
        (after the synthesis transform) and `decompress_base` for the base layer alone"""
        m, p = self.model, self.pad
        B, _, h, w = shape
        use = [ly for ly in self.layers if ly.c0 + ly.M <= ypad.shape[3]]
        inner = ypad[:, p:p + h, p:p + w, :]
        got = inner.round().to(torch.int32).cpu().numpy()
        for l, (ly, c) in enumerate(zip(use, strings["layers"])):
            _check_latents(got, ly.c0, ly.c0 + ly.M, c["y_crc32"], self._what(l))
        y_hat = inner.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        if len(use) == 1:
            return {"y1_hat": y_hat, "z_hat": z_hat, "F_tilde": m.LST(y_hat)}
        return {"x_hat": m.decoder(y_hat), "y_hat": y_hat, "z_hat": z_hat, "F_tilde": m.LST(y_hat[:, :m.M1])}

    @torch.no_grad()
    def decompress(self, strings: Dict, shape, z_shape) -> Dict:
        """-> {"x_hat", "y_hat", "z_hat", "F_tilde"}: both layers, the picture and the base layer's vision features"""
        return self._decode(strings, shape, z_shape, 2)

    @torch.no_grad()
    def decompress_base(self, strings: Dict, shape, z_shape) -> Dict:
        """-> {"y1_hat", "z_hat", "F_tilde"} from z and layer 0 alone; layer 1's strings may be absent"""
        return self._decode(strings, shape, z_shape, 1)

    # ---- the LICBITS6 container ---------------------------------------------------------------------
    def _pack_image(self, s: Dict, B: int, H: int, W: int, top: int, left: int) -> bytes:
        m = self.model
        head = {"family": self._family(), "M": m.M, "K": m.K, "z_lo": self.z_lo, "z_S": self.z_S, "y_W": self.y_W,
                "B": B, "H": H, "W": W, "top": top, "left": left, "M1": m.M1}
        return pack_bitstream_layered(head, s["z"], s["z_esc"], s["layers"], self.groups, self.slice_rows)

    @torch.no_grad()
    def compress_image(self, x: torch.Tensor, mode: str = "replicate", align: str = "topleft") -> bytes:
        """x [B,3,H,W] of ANY size -> one LICBITS6 byte string that `decompress_image` decodes by itself, and whose
        first `base_bytes` (header word; `base_bytes_of(blob)`) `decompress_base_image` decodes by themselves"""
        if x.dim() != 4:
            raise CodecError("expected a [B,3,H,W] tensor")
        return self._pack_padded(x, self.compress(F_.pad_to_multiple(x, 64, mode, align))["strings"], align)

    @staticmethod
    def base_bytes_of(blob: bytes) -> int:
        """how many leading bytes of a LICBITS6 blob the base decode needs (from the header alone)"""
        if len(blob) < _BITS_HEAD_LAYERED.size or bytes(blob[:8]) != BITSTREAM_MAGIC_LAYERED:
            raise CodecError("not a LICBITS6 bitstream (bad magic or shorter than its header)")
        return struct.unpack_from("<I", blob, _BITS_HEAD_LAYERED.size - 4)[0]

    def _open_blob(self, data: bytes, base_only: bool):
        """the host half of the container decoders -> (header, strings, the codec that decodes them).  Refusals, in
        order: the reader's (bitstream.py), a window the rANS decoders do not take, a model that is not this one."""
        head, zs, zes, layers, G, R = (unpack_bitstream_layered_base if base_only else unpack_bitstream_layered)(data)
        if not 2 <= head["z_S"] <= L.RANS_Z_MAX_S:
            raise CodecError(f"bitstream names z_S = {head['z_S']}; the rANS decoder of z takes windows of 2 to "
                             f"{L.RANS_Z_MAX_S} symbols")
        if head["y_W"] > RANS_MAX_W:
            raise CodecError(f"bitstream names y_W = {head['y_W']}; the rANS decoder takes windows of 1 to {RANS_MAX_W}")
        m = self.model
        if (head["family"], head["M"], head["K"], head["M1"]) != (self._family(), m.M, m.K, m.M1):
            raise CodecError(f"bitstream was written by family {head['family']} with M={head['M']}, M1={head['M1']}, "
                             f"K={head['K']}; this model is family {self._family()} with M={m.M}, M1={m.M1}, K={m.K}")
        strings = {"layers": layers, "z": zs, "z_esc": zes, "z_coder": "rans", "coder": "rans"}
        if G > 1:
            strings["groups"] = G
        if R is not None:
            strings["slice_rows"] = R
        dec = self
        if (head["z_lo"], head["z_S"], head["y_W"]) != (self.z_lo, self.z_S, self.y_W):
            dec = ScalableCodec(m, head["z_lo"], head["z_S"], head["y_W"])
        return head, strings, dec

    @torch.no_grad()
    def decompress_image(self, data: bytes) -> torch.Tensor:
        """The inverse of `compress_image`: x_hat [B,3,H,W], cropped back.  CodecError before any GPU work for a bad
        magic, a truncated buffer -- the base prefix included --, a failing CRC or a header that is not this model's."""
        head, strings, dec = self._open_blob(data, False)
        out = dec.decompress(strings, *self._shapes(head, self.model.M))
        return F_.crop_window(out["x_hat"], head["top"], head["left"], head["H"], head["W"])

    @torch.no_grad()
    def decompress_base_image(self, data: bytes):
        """A whole `compress_image` blob or its prefix blob[:base_bytes] -> (y1_hat [B, M1, Hp/16, Wp/16], F_tilde).
        Nothing behind base_bytes is looked at; damage before it is refused."""
        head, strings, dec = self._open_blob(data, True)
        out = dec.decompress_base(strings, *self._shapes(head, self.model.M))
        return out["y1_hat"], out["F_tilde"]

    def compress_images(self, images: Sequence[torch.Tensor], mode: str = "replicate", align: str = "topleft") -> List[bytes]:
        """`compress_image` per entry, one after the other (no merged pass for layered blobs)"""
        return [self.compress_image(x, mode, align) for x in images]

    # ---- many layered bitstreams in one step loop -----------------------------------------------------
    @torch.no_grad()
    def decompress_many(self, items, nlayers: int = 2, z_windows=None, names=None) -> List[Dict]:
        """`decompress` (nlayers = 2) or `decompress_base` (nlayers = 1) for several bitstreams at once.  items:
        [(strings, shape, z_shape)] as those take them, of this codec's y_W and one G; they may differ in B, h, w and
        slice_rows.  z_windows: [(z_lo, z_S)] per item (default: this codec's); names: what to call an item in a message
        (default "item i").  -> one result per item, bit for bit what the single call gives for it alone.

        `_LayeredCodec._decompress_many` is the body, here with the first `nlayers` layers: the latent planes hold their
        channels, and every step of its loop is {lic_ctx_gather_layers_ragged -> per-pixel layers and tables per layer
        -> lic_rans_decode_step_layers_ragged}, for one layer as for two.  Everything the host can refuse is refused
        before the device is touched."""
        items = list(items)
        if items and nlayers not in (1, 2):
            raise CodecError(f"nlayers = {nlayers!r}: 1 decodes the base layer, 2 both layers")
        return self._decompress_many(items, self.layers[:nlayers], z_windows, names)

    def _open_blobs(self, blobs, base_only: bool):
        """The host half of `decompress_images` / `decompress_base_images` -> ([(header, strings)], the codec that
        decodes them all).  CodecError, naming the blob: what `_open_blob` refuses for it, a y_W or a G that is not
        blob 0's.  An empty list gives ([], self)."""
        opened = []
        for i, data in enumerate(blobs):
            try:
                opened.append(self._open_blob(data, base_only)[:2])
            except CodecError as err:
                raise CodecError(f"blob {i}: {err}") from None
        if not opened:
            return [], self
        y_W = self._one_window_one_G(opened)
        return opened, (self if y_W == self.y_W else ScalableCodec(self.model, self.z_lo, self.z_S, y_W))

    def _decompress_blobs(self, blobs, nlayers: int):
        opened, dec = self._open_blobs(list(blobs), nlayers == 1)
        if not opened:
            return [], []
        items = [(strings, *self._shapes(head, self.model.M)) for head, strings in opened]
        return opened, dec.decompress_many(items, nlayers, [(head["z_lo"], head["z_S"]) for head, _ in opened],
                                           [f"blob {i}" for i in range(len(opened))])

    @torch.no_grad()
    def decompress_images(self, blobs: Sequence[bytes]) -> List[torch.Tensor]:
        """Many `compress_image` blobs in one decode loop: entry i is bit for bit `decompress_image(blobs[i])`,
        [B_i, 3, H_i, W_i], channels_last, cropped.  The blobs may differ in size, batch, crop, slice_rows and z window;
        step t of all their images and both layers shares its launches (`decompress_many`), so N blobs cost about one
        blob's step loop plus every blob's transforms.  Raises CodecError before any GPU work, every message naming its
        blob ("blob i: ..."): whatever `decompress_image` refuses for blob i -- a base prefix included --, a y_W or a
        G that is not blob 0's.  An empty list gives an empty list."""
        opened, outs = self._decompress_blobs(blobs, 2)
        return [F_.crop_window(out["x_hat"], head["top"], head["left"], head["H"], head["W"])
                for out, (head, _) in zip(outs, opened)]

    @torch.no_grad()
    def decompress_base_images(self, blobs: Sequence[bytes]):
        """Whole `compress_image` blobs or their prefixes blob[:base_bytes], mixed freely, in one decode loop of the
        base layer alone: entry i is bit for bit `decompress_base_image(blobs[i])`, (y1_hat, F_tilde).  Nothing behind
        base_bytes is looked at.  Differences between blobs and refusals as for `decompress_images`."""
        _, outs = self._decompress_blobs(blobs, 1)
        return [(out["y1_hat"], out["F_tilde"]) for out in outs]
