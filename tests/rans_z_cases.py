"""Synthetic hyper-latent streams for the z_coder="rans" tests: M shared tables [M][S+1], symbols in raster order
(symbol k uses table k % M), one step per image dealt to G sub-streams.  The expected bytes come from the plain
restatement of the format (tests/rans_groups_ref.py) applied to the EXPANDED tables t[arange(n) % M]: that is the
definition of a z stream."""
import numpy as np

import rans_groups_ref as GR


def shared_tables(M, S, seed, shape=0.5):
    """[M][S+1] uint32, cum[0] = 0 < ... < cum[S] = 65536, every frequency >= 1"""
    from oracle import codec_ref as CR
    r = np.random.RandomState(seed)
    f = r.gamma(shape, 1.0, size=(M, S)) + 1e-9
    F = np.concatenate([np.zeros((M, 1)), np.cumsum(f / f.sum(1, keepdims=True), 1)], 1)
    F[:, -1] = 1.0
    return CR.quantize_cdf(F).astype(np.uint32)


def symbols(S, n, seed, far=True):
    """idx [n] int32 drawn from [-3, S+3): interior, edge and escaping symbols; with `far`, +-100000 by hand"""
    r = np.random.RandomState(seed)
    idx = r.randint(-3, S + 3, size=n).astype(np.int32)
    if far and n >= 2:
        idx[n // 2] = -100000
        idx[n - 1] = S + 100000
    elif far:
        idx[0] = -100000
    return idx


def reference(tables, idx, G):
    """-> ([G stream bytes], [G escape-list bytes]) by the restatement, on the expanded tables"""
    n, M = len(idx), len(tables)
    return GR.encode(tables[np.arange(n) % M], idx, [n], G)
