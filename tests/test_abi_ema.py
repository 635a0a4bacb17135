"""lic_adam_run_ema / lic_swap_run: exported, bound, and refusing bad arguments with status codes before anything is
launched.  CPU only, as tests/test_abi.py."""
import ctypes
import os

import pytest

INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _args(n=3):
    """stand-ins that pass the null checks: nothing is dereferenced before the argument checks are through"""
    table = (ctypes.c_uint64 * 64)()
    grads = (ctypes.c_void_p * n)(*[ctypes.addressof(table)] * n)
    ema = (ctypes.c_void_p * n)()
    return table, grads, ema


def test_adam_run_ema_refuses_bad_arguments(lib):
    L = lib.load()
    table, grads, ema = _args()
    t, e = ctypes.addressof(table), ctypes.addressof(ema)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001)

    def run(jobs=t, njobs=3, blocks=3, g=grads, hp=hyper, ema_p=e, w=0.001, clip=None, skip=0):
        return L.lic_adam_run_ema(jobs, njobs, blocks, g, *hp, ema_p, w, clip, skip, None)

    assert run(jobs=None) == INVALID
    assert run(g=None) == INVALID
    assert run(njobs=0) == INVALID and run(blocks=0) == INVALID and run(blocks=2 ** 31) == INVALID
    assert run(ema_p=None) == INVALID                                  # no table of averages
    assert run(ema_p=e + 4) == INVALID and run(ema_p=e + 1) == INVALID   # not aligned to a pointer
    for w in (-1e-9, 1.0 + 1e-9, 2.0, float("nan"), float("inf"), -float("inf")):
        assert run(w=w) == INVALID, w
    assert run(hp=hyper[:5] + (0.0, 0.001)) == INVALID                   # bias corrections must be positive
    assert run(hp=hyper[:5] + (0.1, float("nan"))) == INVALID
    assert run(njobs=449, g=(ctypes.c_void_p * 449)(*[t] * 449)) == UNSUPPORTED
    holes = (ctypes.c_void_p * 3)(t, None, t)
    assert run(g=holes) == INVALID                                       # a missing gradient
    assert run(g=holes, clip=t, skip=1) == INVALID                       # ... with a clip state as well


def test_swap_run_refuses_bad_arguments(lib):
    L = lib.load()
    table, _, ema = _args()
    t, e = ctypes.addressof(table), ctypes.addressof(ema)
    assert L.lic_swap_run(None, 3, 3, e, None) == INVALID
    assert L.lic_swap_run(t, 3, 3, None, None) == INVALID
    assert L.lic_swap_run(t, 3, 3, e + 4, None) == INVALID
    assert L.lic_swap_run(t, 0, 3, e, None) == INVALID
    assert L.lic_swap_run(t, 3, 0, e, None) == INVALID and L.lic_swap_run(t, 3, 2 ** 31, e, None) == INVALID
    assert L.lic_swap_run(t, 449, 449, e, None) == UNSUPPORTED


def test_new_entries_are_declared_exported_and_bound(lib):
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lic.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for name in ("lic_adam_run_ema", "lic_swap_run"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in lib.SIGNATURES
    # the job layout the new entries share with lic_adam_run has not moved
    assert ctypes.sizeof(lib.AdamJob) == 48
    assert [f[0] for f in lib.AdamJob._fields_] == ["p", "g", "m", "v", "n", "block0", "nblocks"]
