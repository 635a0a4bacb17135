"""Images of any size through models that need multiples of 64: pad, run, crop back.

`model(x)` keeps refusing other sizes (phi / psi shapes must agree, Models.py:73, 283-284); `padded_forward` is
the explicit way round it, for evaluation on test sets whose images are whatever size they are."""
from __future__ import annotations

import torch

from . import functional as F_


@torch.no_grad()
def padded_forward(model, x: torch.Tensor, mode: str = "replicate", align: str = "topleft", training: bool = False,
                   quality=None):
    """Pads x [B,3,H,W] to the next multiples of 64 (`functional.pad_to_multiple`), runs `model(x_pad, training)`
    and returns its out-dict with `x_hat` replaced by the dense crop back to [B,3,H,W]; adds `padded_hw` = (Hp, Wp)
    and `window` = (top, left, H, W).  The likelihoods stay those of the padded latents -- they are what a
    decoder needs -- so `rd_loss(out, x, lambda)` with the ORIGINAL x reports bits per original pixel and the
    distortion over the original image without any change to the loss: `functional._RdLossFn` takes its pixel
    count (`x.shape[2] * x.shape[3]`) and its element count from the `x` it is given and only sums the
    log-likelihood tensors, whatever their shape.  Works for JointAutoregressiveHierarchical,
    HierarchicalMixtureResidual and ScalableImageCoding; `quality` goes to a rate-level model.  Inference only: no gradient flows through the pad or
    the crop."""
    if x.dim() != 4:
        raise ValueError("expected a [B,C,H,W] tensor")
    H, W = x.shape[2], x.shape[3]
    Hp, Wp, top, left = F_.pad_geometry(H, W, 64, align)
    x_pad = F_.pad_to_multiple(x, 64, mode, align)
    kw = {} if quality is None else {"quality": quality}
    out = dict(model(x_pad, training=training, **kw))
    out["x_hat"] = F_.crop_window(out["x_hat"], top, left, H, W)
    out["padded_hw"] = (Hp, Wp)
    out["window"] = (top, left, H, W)
    return out
