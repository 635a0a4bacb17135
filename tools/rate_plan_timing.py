#!/usr/bin/env python3
"""Rate levels under launch plans: the training step of a rate-level model, three ways, alternating in one
process on one GPU --
  a  eager, one float quality and one float lambda per step (the step of Trainer(rate_points=...));
  b  eager, qualities and lambdas per image as device tensors (`device_quality=True`, a lambda tensor in rd_loss);
  c  the recorded step (plan.StepPlan) fed with new per-image qualities and lambdas every step.
Config 3's shape: JointAutoregressiveHierarchical(128, 3, rate_levels=4), bf16, 32 x 3 x 256 x 256, FusedAdam.  Every
variant has its own model and optimizer from the same seed and draws a new rate point (a) or B of them (b, c) per step.
Timing: a host clock around `steps` steps that end in a device synchronise, `rounds` times per variant, the variants taking
turns inside a round; images/s is reported as the median over the rounds with the lowest and the highest beside it.
Launches per step: forward + loss + backward captured once (as the plan captures it) and counted by lic_plan_info; the
noise draw, the uploads and the optimizer's launch are outside that count for every variant.

usage: python tools/rate_plan_timing.py [--variants abc] [--steps 25] [--rounds 5] [--warmup 10] [--json PATH]
(`--variants a` also runs on a tree without the device-quality path.)"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import neural_image_compression_amd as nic  # noqa: E402
from neural_image_compression_amd import _lib as L  # noqa: E402

M, K, LEVELS, B, H, W = 128, 3, 4, 32, 256, 256
POINTS = [(0.0, 0.0018), (1.0, 0.0035), (2.0, 0.0067), (3.0, 0.013), (0.5, 0.0025), (2.5, 0.0095)]


def build(dev):
    torch.manual_seed(0)
    model = nic.JointAutoregressiveHierarchical(M, K, rate_levels=LEVELS).to(dev)
    with torch.no_grad():
        for i, name in enumerate(model.GAIN_TABLES):   # gains off 1, so that the rate points differ
            getattr(model, name).uniform_(-0.5, 0.5, generator=torch.Generator(device=dev).manual_seed(10 + i))
    model.set_precision("bf16")
    return model, nic.FusedAdam(model.parameters(), lr=1e-4)


def count_launches(model, body, dev):
    """kernels / memsets / memcpys of one captured `body()` (forward + loss + backward into empty gradients, as a step
    behind zero_grad(set_to_none=True)), by the library's own reader"""
    lib = L.load()
    cap = torch.cuda.Stream(device=dev)
    cap.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(cap):
        body()
    torch.cuda.current_stream(dev).wait_stream(cap)
    torch.cuda.synchronize(dev)
    for p in model.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=cap):
        body()
    plan = C.c_void_p()
    rc = lib.lic_plan_create(C.c_void_p(graph.raw_cuda_graph()), C.byref(plan))
    if rc != 0:
        raise L.LicError(f"lic_plan_create: {rc} ({lib.lic_plan_last_error().decode()})")
    info = (C.c_int64 * 7)()
    L.check(lib.lic_plan_info(plan, info), "lic_plan_info")
    lib.lic_plan_destroy(plan)
    return {"kernels": info[1], "memsets": info[2], "memcpys": info[3]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rate_plan_timing needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1234)
    x = torch.rand(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    rng = {v: random.Random(7) for v in "abc"}
    steps, bodies, info = {}, {}, {}

    if "a" in args.variants:
        ma, oa = build(dev)

        def body_a(q=1.5, lam=0.005):
            res = nic.rd_loss(ma(x, quality=q), x, lam, sync=False)
            res["loss"].backward()
            return res

        def step_a():
            oa.zero_grad(set_to_none=True)
            body_a(*rng["a"].choice(POINTS))
            oa.step()
        steps["a"], bodies["a"] = step_a, (ma, body_a)

    if "b" in args.variants:
        mb, ob = build(dev)
        up = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
        fixed = (up([p[0] for p in POINTS[:1] * B]), up([p[1] for p in POINTS[:1] * B]))

        def body_b(q=None, lam=None):
            q, lam = (fixed[0] if q is None else q), (fixed[1] if lam is None else lam)
            res = nic.rd_loss(mb(x, quality=q, device_quality=True), x, lam, sync=False)
            res["loss"].backward()
            return res

        def step_b():
            pairs = [rng["b"].choice(POINTS) for _ in range(B)]
            ob.zero_grad(set_to_none=True)
            body_b(up([p[0] for p in pairs]), up([p[1] for p in pairs]))
            ob.step()
        steps["b"], bodies["b"] = step_b, (mb, body_b)

    if "c" in args.variants:
        from neural_image_compression_amd.plan import StepPlan
        mc, oc = build(dev)
        first = [POINTS[0]] * B
        plan = StepPlan(mc, nic.rd_loss, torch.tensor([p[1] for p in first], device=dev), x,
                        quality=torch.tensor([p[0] for p in first], device=dev))
        info["c"] = {k: plan.info[k] for k in ("kernels", "memsets", "memcpys")}

        def step_c():
            pairs = [rng["c"].choice(POINTS) for _ in range(B)]
            plan.step(x, quality=[p[0] for p in pairs], lam=[p[1] for p in pairs])
            oc.step()
        steps["c"] = step_c

    for v, fn in steps.items():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    rates, enqueue = {v: [] for v in steps}, {v: [] for v in steps}
    for _ in range(args.rounds):
        for v, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            rates[v].append(B * args.steps / (time.perf_counter() - t0))
            enqueue[v].append((t1 - t0) / args.steps * 1e3)
    result = {"config": f"JAH({M},{K},rate_levels={LEVELS}) bf16 {B}x3x{H}x{W} FusedAdam", "steps_per_round": args.steps,
              "rounds": args.rounds, "variants": {}}
    for v in steps:
        result["variants"][v] = {"images_per_s": round(statistics.median(rates[v]), 1), "lowest": round(min(rates[v]), 1),
                                 "highest": round(max(rates[v]), 1),
                                 # the host's share: the time until the last launch of the window was enqueued
                                 "host_enqueue_ms_per_step": round(statistics.median(enqueue[v]), 3),
                                 "ms_per_step": round(B / statistics.median(rates[v]) * 1e3, 3)}
        print(f"{v}: {result['variants'][v]}", flush=True)
    # launches per step, last: a capture that fails must not disturb the timings above
    for v, (model, body) in bodies.items():
        try:
            info[v] = count_launches(model, body, dev)
        except Exception as e:   # noqa: BLE001 -- reported, not hidden: the number is then "not measured"
            info[v] = {"not measured": f"{type(e).__name__}: {e}"}
    for v in steps:
        result["variants"][v]["launches_per_step"] = info.get(v)
    print(json.dumps(result), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
