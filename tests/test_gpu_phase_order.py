"""Phase-sorted four-phase launches of lic_igemm (transposed, stride 2, at least 128 M tiles per phase) on the GPU, at
the group sizes phase_order() (csrc/lic_conv_plan.h) now derives from the XCD ranges: k = ceil(MT / 512) groups per XCD
of g = ceil(MT / 8k) M tiles, MT padded to 8 k g.  A reordering of workgroups must leave every output byte what it was,
and it can go wrong only by running a tile twice, not at all, or past a phase's rows -- so the operands are integers in
the exact regime of tests/conv_ref64.py (S < 2^24: fp32 forms every partial sum without rounding, in any order), the
outputs live in tests/guarded.py buffers (a NaN pattern that an unwritten element keeps, canaries around the
allocation) and the required relation is equality with float64, bit for bit.  tests/test_phase_order_host.py holds the
order itself on the CPU; here each case's grid is read back from the same probe, so that the case is known to be what its
comment says.  The launch helpers are those of tests/test_gpu_conv_fp32.py.

xcd_contiguous()'s `r != 0` branch (a grid that is no multiple of 8): a phase-sorted launch never takes it, its grid
is 8 k g x 4 phases x NT x K splits.  The B = 3 cases stand on both sides: 169 tiles padded to 176, and 127 tiles --
one below the threshold -- whose rotated launch of 508 workgroups does take it."""
import ctypes
import functools

import pytest
import torch

import conv_ref64 as R
from test_gpu_conv_fp32 import OK, IgemmOperands, env, igemm_desc, run_igemm, sync_clean  # noqa: F401
from guarded import Guarded

pytestmark = pytest.mark.gpu

_ic = R.ICase
# (case, M tiles per phase, groups per XCD k, tiles per group g (0: rotated, below the threshold), N tiles, K slices)
CASES = [
    # 2 * 64 * 64 = 8192 rows per phase: 128 tiles of 64, the smallest sorted launch
    (_ic("po-t5-64", "convT", 5, 2, 2, 1, 2, 64, 64, 16, 64, tiles=[(64, 1)]), 128, 1, 16, 1, 1),
    # 2 * 72 * 72 / 64 = 162 tiles, padded to 8 * 21 = 168
    (_ic("po-t5-72", "convT", 5, 2, 2, 1, 2, 72, 72, 16, 64, tiles=[(64, 1)]), 162, 1, 21, 1, 1),
    # output_padding 0: 127 x 127 outputs, phases of 64 x 64, 64 x 63, 63 x 64 and 63 x 63 pixels (128 126 126 125 tiles)
    (_ic("po-t5-64-odd", "convT", 5, 2, 2, 0, 2, 64, 64, 16, 64, tiles=[(64, 1)]), 128, 1, 16, 1, 1),
    # 128-row tiles: 2 * 128 * 64 / 128 = 128 of them
    (_ic("po-t5-128x64-bm128", "convT", 5, 2, 2, 1, 2, 128, 64, 16, 64, tiles=[(128, 1)]), 128, 1, 16, 1, 1),
    # two N tiles, which run faster than the M tile
    (_ic("po-t5-64-nt2", "convT", 5, 2, 2, 1, 2, 64, 64, 16, 128, tiles=[(64, 1)]), 128, 1, 16, 2, 1),
    # three K slices (of 9 chunks), which run fastest, and the finish kernel
    (_ic("po-t5-64-split3", "convT", 5, 2, 2, 1, 2, 64, 64, 16, 64, tiles=[(64, 1)], splits=(3,)), 128, 1, 16, 1, 3),
    # 3x3: phases of 1 / 2 / 2 / 4 taps
    (_ic("po-t3-64", "convT", 3, 2, 1, 1, 2, 64, 64, 16, 64, tiles=[(64, 1)]), 128, 1, 16, 1, 1),
    # B = 3: 3 * 60 * 60 / 64 = 168.75 -> 169 tiles, padded to 8 * 22 = 176
    (_ic("po-t5-60-b3", "convT", 5, 2, 2, 1, 3, 60, 60, 16, 64, tiles=[(64, 1)]), 169, 1, 22, 1, 1),
    # B = 3, 3 * 52 * 52 / 64 = 126.75 -> 127 tiles: rotated, 508 workgroups, 4 XCDs hold one id more
    (_ic("po-t5-52-b3-rotated", "convT", 5, 2, 2, 1, 3, 52, 52, 16, 64, tiles=[(64, 1)]), 127, 0, 0, 1, 1),
]
BY_NAME = {c[0].name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _cpu(name):
    """integer inputs and the float64 reference of a case: computed once, left unchanged"""
    c = BY_NAME[name][0]
    inp = R.igemm_inputs(c, True)
    ref = R.igemm_reference(c, inp)
    assert R.exact_ok(ref["S"])
    return inp, ref


def _grid(env, c, ops, tile, split):
    """workgroups of the launch, from lic_igemm_tile_order (the sizes alone)"""
    F_, L, lib, dev = env
    d = igemm_desc(env, c, ops, "fwd", tile, split, Guarded(1, 4, dev), None, Guarded(1, 4, dev), 1 << 50)
    n = ctypes.c_int64(-1)
    assert lib.lic_igemm_tile_order(ctypes.byref(d), None, 0, ctypes.byref(n), None, None) == OK
    return n.value


@pytest.mark.parametrize("name", [c[0].name for c in CASES])
def test_phase_sorted_launch_exact(env, name):
    c, MT, k, g, NT, S = BY_NAME[name]
    (which, tile, split), = c.launches()
    inp, ref = _cpu(name)
    ops = IgemmOperands(env, c, inp)
    rows = c.B * ((c.Ho + 1) // 2) * ((c.Wo + 1) // 2)
    assert -(-rows // tile[0]) == MT and (MT >= R.PGROUP_TILES) == (g > 0)
    nwg = _grid(env, c, ops, tile, split)
    assert nwg == (8 * k * g if g else MT) * 4 * NT * S, (name, nwg)
    assert (nwg % 8 == 0) == (g > 0)
    out, _, slices = run_igemm(env, c, ops, which, tile, split)
    assert slices == S
    differ = int((out.double() != ref["out"]).sum())
    print(f"PHASE ORDER {name}: {nwg} workgroups, {differ} elements differ from float64")
    assert R.same_bits(out, ref["out"])


def test_a_second_launch_gives_the_same_bytes(env):
    c = BY_NAME["po-t5-72"][0]
    ops = IgemmOperands(env, c, _cpu(c.name)[0])
    a, _, _ = run_igemm(env, c, ops, "fwd", (64, 1), 0)
    b, _, _ = run_igemm(env, c, ops, "fwd", (64, 1), 0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
