"""What the moving average of the weights costs per optimizer step on config 2's parameter set
(JointAutoregressiveHierarchical(192, 1), random gradients), in one process, alternating, medians:
  (a) FusedAdam.step()                                                  -- no average
  (b) FusedAdam.step() + torch._foreach_lerp_(emas, params, w)          -- what a user had to write before
  (c) FusedAdam.step() + torch._foreach_mul_(emas, d) + torch._foreach_add_(emas, params, alpha=w)   -- the older recipe
  (d) FusedAdam(ema_decay=0.999).step()                                 -- lic_adam_run_ema
For each: `device`, the time between two events around the call on an idle queue with cold caches (a 512 MB fill in
front, as at the end of a backward pass) -- for (b) and (c) this includes the gaps between their launches -- and
`host`, the wall time of the call itself (launches only; the queue is empty when it starts).  The bandwidth lines
divide the bytes the algorithm needs (28 per element for (a): p, g, m, v read, p, m, v written; 36 for (d): e read and
written as well) by the device time, which holds one launch and its launch latency.
    python tools/bench_ema.py [--reps 30] [--M 192]
"""
import json

import torch
from bench_optim import measure, nic, setup   # (the same command line, parameter set and measuring loop)

DECAY = 0.999


def main():
    args, base, grads = setup("bench_ema.py")

    def variant(**kw):
        params = [torch.nn.Parameter(p.clone()) for p in base]
        return params, nic.FusedAdam(params, lr=1e-4, **kw)

    pa, oa = variant()
    pb, ob = variant()
    pc, oc = variant()
    pd, od = variant(ema_decay=DECAY, ema_warmup=False)
    eb, ec = [p.detach().clone() for p in pb], [p.detach().clone() for p in pc]
    w = 1.0 - DECAY

    def step_b():
        ob.step()
        with torch.no_grad():
            torch._foreach_lerp_(eb, [p.detach() for p in pb], w)

    def step_c():
        oc.step()
        with torch.no_grad():
            torch._foreach_mul_(ec, DECAY)
            torch._foreach_add_(ec, [p.detach() for p in pc], alpha=w)

    variants = (("a: FusedAdam", pa, oa.step), ("b: FusedAdam + _foreach_lerp_", pb, step_b),
                ("c: FusedAdam + _foreach_mul_/_add_", pc, step_c), ("d: FusedAdam(ema_decay=0.999)", pd, od.step))
    med, rows = measure(variants, grads, args, 38)
    assert od.fused_steps == oa.fused_steps == args.warmup + args.reps
    elements = sum(p.numel() for p in base)
    out = {"tensors": len(base), "elements": elements, "reps": args.reps, **rows}
    for k, nbytes in (("a", 28), ("d", 36)):
        out[f"{k}_TB_per_s"] = round(elements * nbytes / med[k][0] / 1e6, 3)
        print(f"({k}) {nbytes} bytes per element over the device time: {out[f'{k}_TB_per_s']:.3f} TB/s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
