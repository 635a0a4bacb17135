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
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import neural_image_compression_amd as nic  # noqa: E402

DECAY = 0.999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--M", type=int, default=192)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ema.py measures on an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = nic.JointAutoregressiveHierarchical(args.M, 1).to(dev)
    base = [p.detach() for p in model.parameters()]
    g = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, device=dev, generator=g) * 1e-2 for p in base]

    def variant(**kw):
        params = [torch.nn.Parameter(p.clone()) for p in base]
        return params, nic.FusedAdam(params, lr=1e-4, **kw)

    pa, oa = variant()
    pb, ob = variant()
    pc, oc = variant()
    pd, od = variant(ema_decay=DECAY, ema_warmup=False)
    eb, ec = [p.detach().clone() for p in pb], [p.detach().clone() for p in pc]
    w = 1.0 - DECAY

    def step_a():
        oa.step()

    def step_b():
        ob.step()
        with torch.no_grad():
            torch._foreach_lerp_(eb, [p.detach() for p in pb], w)

    def step_c():
        oc.step()
        with torch.no_grad():
            torch._foreach_mul_(ec, DECAY)
            torch._foreach_add_(ec, [p.detach() for p in pc], alpha=w)

    def step_d():
        od.step()

    variants = (("a: FusedAdam", pa, step_a), ("b: FusedAdam + _foreach_lerp_", pb, step_b),
                ("c: FusedAdam + _foreach_mul_/_add_", pc, step_c), ("d: FusedAdam(ema_decay=0.999)", pd, step_d))
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    times = {name: ([], []) for name, _, _ in variants}
    for rep in range(args.warmup + args.reps):
        for name, params, fn in variants:
            for p, gr in zip(params, grads):      # fresh gradient tensors, as after a backward pass
                p.grad = gr.clone()
            flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[name][0].append(e0.elapsed_time(e1) * 1e3)
                times[name][1].append((t1 - t0) * 1e6)
    assert od.fused_steps == oa.fused_steps == args.warmup + args.reps
    elements = sum(p.numel() for p in base)
    out = {"tensors": len(base), "elements": elements, "reps": args.reps}
    med = {}
    for name, _, _ in variants:
        d, h = times[name]
        med[name[0]] = (statistics.median(d), statistics.median(h))
        out[name[0]] = {"device_us": round(med[name[0]][0], 1), "device_us_min_max": [round(min(d), 1), round(max(d), 1)],
                        "host_us": round(med[name[0]][1], 1), "host_us_min_max": [round(min(h), 1), round(max(h), 1)]}
        print(f"{name:38s} device {med[name[0]][0]:8.1f} us   host {med[name[0]][1]:8.1f} us")
    for k in ("b", "c", "d"):
        out[f"{k}_minus_a"] = {"device_us": round(med[k][0] - med["a"][0], 1), "host_us": round(med[k][1] - med["a"][1], 1)}
        print(f"({k}) - (a): device {med[k][0] - med['a'][0]:+8.1f} us   host {med[k][1] - med['a'][1]:+8.1f} us")
    for k, nbytes in (("a", 28), ("d", 36)):
        out[f"{k}_TB_per_s"] = round(elements * nbytes / med[k][0] / 1e6, 3)
        print(f"({k}) {nbytes} bytes per element over the device time: {out[f'{k}_TB_per_s']:.3f} TB/s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
