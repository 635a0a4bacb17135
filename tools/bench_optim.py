"""What gradient clipping costs per optimizer step on config 2's parameter set (JointAutoregressiveHierarchical(192, 1),
random gradients), three ways in one process, alternating, medians:
  (a) FusedAdam.step()                                          -- no clipping
  (b) torch.nn.utils.clip_grad_norm_(params, 1.0) + FusedAdam.step()   -- what a user had to write before
  (c) FusedAdam(max_grad_norm=1.0).step()                       -- lic_grad_norm_partial / _finish + lic_adam_run_scaled
For each: `device`, the time between two events around the call on an idle queue with cold caches (a 512 MB fill in
front, as at the end of a backward pass) -- for (b) this includes the gaps between its launches -- and `host`, the wall
time of the call itself (launches only; the queue is empty when it starts).
    python tools/bench_optim.py [--reps 30] [--M 192]
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


def setup(tool):
    """the command line both optimizer benchmarks take, config 2's parameters and one random gradient per tensor"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--M", type=int, default=192)
    args = ap.parse_args()
    assert torch.cuda.is_available(), f"{tool} measures on an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = nic.JointAutoregressiveHierarchical(args.M, 1).to(dev)
    base = [p.detach() for p in model.parameters()]
    g = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, device=dev, generator=g) * 1e-2 for p in base]
    return args, base, grads


def measure(variants, grads, args, width):
    """The measuring loop of bench_optim.py and bench_ema.py.  variants: ("x: name", parameters, step function), the
    first one "a"; they alternate, args.reps repetitions after args.warmup.  Prints one line per variant and each
    variant's difference to (a); returns (letter -> (median device us, median host us), the rows of the JSON line)."""
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=grads[0].device)
    times = {name: ([], []) for name, _, _ in variants}
    for rep in range(args.warmup + args.reps):
        for name, params, fn in variants:
            for p, gr in zip(params, grads):      # fresh gradient tensors, as after a backward pass (some scale in place)
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
    med, rows = {}, {}
    for name, _, _ in variants:
        d, h = times[name]
        med[name[0]] = (statistics.median(d), statistics.median(h))
        rows[name[0]] = {"device_us": round(med[name[0]][0], 1), "device_us_min_max": [round(min(d), 1), round(max(d), 1)],
                         "host_us": round(med[name[0]][1], 1), "host_us_min_max": [round(min(h), 1), round(max(h), 1)]}
        print(f"{name:{width}s} device {med[name[0]][0]:8.1f} us   host {med[name[0]][1]:8.1f} us")
    for k in list(med)[1:]:
        rows[f"{k}_minus_a"] = {"device_us": round(med[k][0] - med["a"][0], 1), "host_us": round(med[k][1] - med["a"][1], 1)}
        print(f"({k}) - (a): device {med[k][0] - med['a'][0]:+8.1f} us   host {med[k][1] - med['a'][1]:+8.1f} us")
    return med, rows


def main():
    args, base, grads = setup("bench_optim.py")

    def variant(clip):
        params = [torch.nn.Parameter(p.clone()) for p in base]
        opt = nic.FusedAdam(params, lr=1e-4, max_grad_norm=1.0 if clip else None)
        return params, opt

    pa, oa = variant(False)
    pb, ob = variant(False)
    pc, oc = variant(True)

    def step_b():
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        ob.step()

    variants = (("a: FusedAdam", pa, oa.step), ("b: clip_grad_norm_ + FusedAdam", pb, step_b),
                ("c: FusedAdam(max_grad_norm=1)", pc, oc.step))
    _, rows = measure(variants, grads, args, 34)
    elements = sum(p.numel() for p in base)
    print(json.dumps({"tensors": len(base), "gradient_MB": round(elements * 4 / 1e6, 1), "reps": args.reps,
                      "grad_norm": float(oc.grad_norm()), **rows}))


if __name__ == "__main__":
    main()
