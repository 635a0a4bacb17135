"""numpy restatement of the moving average FusedAdam(ema_decay=...) keeps (lic_adam_run_ema), written from the text of
include/lic.h, not from the kernel:

    d_t = min(d, (1 + t) / (10 + t)) with warm-up, d without;  ema_weight = 1 - d_t          (double, on the host)
    w   = float32(ema_weight)                                                                 (one rounding)
    e   = e + w * (p_new - e)        three fp32 operations, each rounded on its own: subtract, multiply, add

`t` is the 1-based step count the bias corrections use.  numpy does not fuse a multiply with an add, so the three
statements below are the three roundings; the kernel must give these bits.  A skipped step (skip_nonfinite and a norm
that is not finite) leaves e as it leaves p, m and v."""
import math

import numpy as np

import clip_ref

F = np.float32


def ema_weight(t, d, warmup=True):
    """the weight of the new parameter at step t (1-based), a Python double"""
    d = float(d)
    if warmup:
        d = min(d, (1.0 + t) / (10.0 + t))
    return 1.0 - d


def ema_update(e, p_new, w):
    """e + w * (p_new - e) with three fp32 roundings; returns a new array"""
    e, p_new = np.asarray(e), np.asarray(p_new)
    assert e.dtype == np.float32 and p_new.dtype == np.float32
    w = F(w)
    with np.errstate(all="ignore"):
        diff = (p_new - e).astype(np.float32)
        scaled = (w * diff).astype(np.float32)
        return (e + scaled).astype(np.float32)


def ema_step(params, grads, ms, vs, emas, step, lr, decay, warmup=True, max_norm=math.inf, skip_nonfinite=False, **hyper):
    """clip_ref.clipped_step over lists of fp32 arrays, in place, then the average of every tensor, in place as well.
    Returns (norm, coefficient, skipped)."""
    norm, coef, skipped = clip_ref.clipped_step(params, grads, ms, vs, step, lr, max_norm=max_norm,
                                                skip_nonfinite=skip_nonfinite, **hyper)
    if skipped:
        return norm, coef, True
    w = ema_weight(step, decay, warmup)
    for e, p in zip(emas, params):
        e[...] = ema_update(e, p, w)
    return norm, coef, False
