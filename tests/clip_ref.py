"""numpy restatement of the clipped Adam step of FusedAdam(max_grad_norm=..., skip_nonfinite=...): the norm and
coefficient of lic_grad_norm_finish and the update of lic_adam_run_scaled, written from include/lic.h and the header
comment of csrc/lic_optim.hip, not from the kernels.

    norm  = float32(sqrt(float64 sum of g^2 over every tensor))            (exact inputs: any summation order)
    coef  = min(float32(max_norm) / (norm + float32(1e-6)), 1) in fp32;    exactly 1 for max_norm = +inf
    g     = float32(g * coef)                                              (one rounding)
    g'    = g + weight_decay * p;  m += (1 - beta1) * (g' - m);  v = beta2 * v + (1 - beta2) * g' * g'
    p    -= (lr / bias_correction1) * m / (sqrt(v) / sqrt(bias_correction2) + eps)

The scalars 1 - beta, lr / bias_correction1 and sqrt(bias_correction2) are formed in double and rounded once, as
torch does; everything per element is fp32.  The kernels fuse some multiply-adds, numpy does not: the Adam part agrees
with them to rounding, not bit for bit (the norm and the coefficient do agree bit for bit)."""
import math

import numpy as np

F = np.float32


def grad_norm(grads):
    """fp32 global L2 norm: double sum of squares (math.fsum: correctly rounded whatever the order), double sqrt,
    one rounding"""
    total = math.fsum(math.fsum((g.astype(np.float64).ravel() ** 2).tolist()) for g in grads)
    return F(math.sqrt(total))


def coefficient(norm, max_norm):
    if math.isinf(max_norm) and max_norm > 0:
        return F(1.0)
    with np.errstate(all="ignore"):
        return np.minimum(F(max_norm) / (F(norm) + F(1e-6)), F(1.0))   # (np.minimum keeps a NaN, as torch.clamp does)


def adam_update(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """one tensor, in place; `step` is the 1-based count of this update"""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    lerp_w, step_size, bc2_sqrt = F(1.0 - beta1), F(lr / bc1), F(math.sqrt(bc2))
    b2, omb2, ep, wd = F(beta2), F(1.0 - beta2), F(eps), F(weight_decay)
    with np.errstate(all="ignore"):
        if weight_decay != 0.0:
            g = g + wd * p
        m += lerp_w * (g - m)
        v *= b2
        v += (omb2 * g) * g
        p -= step_size * (m / (np.sqrt(v) / bc2_sqrt + ep))


def clipped_step(params, grads, ms, vs, step, lr, max_norm=math.inf, skip_nonfinite=False, **hyper):
    """the whole step over lists of fp32 arrays, in place.  Returns (norm, coefficient, skipped)."""
    assert all(a.dtype == np.float32 for a in list(params) + list(grads) + list(ms) + list(vs))
    norm = grad_norm(grads)
    coef = coefficient(norm, max_norm)
    if skip_nonfinite and not np.isfinite(norm):
        return norm, coef, True
    for p, g, m, v in zip(params, grads, ms, vs):
        with np.errstate(all="ignore"):
            scaled = (g * coef).astype(np.float32)
        adam_update(p, scaled, m, v, step, lr, **hyper)
    return norm, coef, False
