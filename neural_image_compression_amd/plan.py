"""StepPlan: the training step (Trainer.py:78-85: forward, rd_loss, backward) captured once and replayed by
liblic_hip.so's launch plan (include/lic.h, lic_plan_*) -- the same kernels on the same two streams as the eager
step, with no Python between the launches.

Why: the bf16 configurations are host-paced.  One step is ~180 launches; the Python around them (autograd nodes,
allocations, ctypes marshalling) costs ~3.1 ms of a 3.8 ms step, the launches themselves 0.7 ms, the GPU work ~3 ms.
A HIP graph would remove the host cost, but this ROCm replays a graph with more than one branch node by node from
the host (10 ms per step) and a single-branch graph loses the decoder / latent-side overlap.  So torch captures the
step only as a RECORD (private memory pool: fixed addresses); lic_plan_create turns the record into two launch
sequences with one event per cross-stream edge, and every replay is one C call.

What stays outside the plan, in eager Python: the uniform noise of the quantiser (one generator launch into a fixed
buffer: the draw is the reference's, z first -- Models.py:57-58 -- and advances torch's generator exactly as the
eager step does, so eager and planned steps produce the same bits from the same seed) and the optimizer
(FusedAdam: one launch; its bias corrections are host arithmetic).

Limits: one process, one GPU (the gradient all-reduce of parallel.py runs from autograd hooks, which a replay does
not execute: use the eager step for data-parallel training); fixed batch shape; training mode."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import torch

from . import _lib as L
from . import functional as F_
from .functional import _stream


def _read_dag(lib, plan):
    sizes = (C.c_int64 * 2)()
    L.check(lib.lic_plan_dag(plan, 0, 0, sizes, None, None, None, None, None), "lic_plan_dag")
    n, ne = sizes[0], sizes[1]
    ptr, idx = (C.c_int32 * (n + 1))(), (C.c_int32 * max(ne, 1))()
    kind, flags, us = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_double * n)()
    L.check(lib.lic_plan_dag(plan, n, ne, sizes, ptr, idx, kind, flags, us), "lic_plan_dag")
    return {"preds": [list(idx[ptr[k]:ptr[k + 1]]) for k in range(n)],
            "kind": [("kernel", "memset", "memcpy", "empty")[k] for k in kind],
            "wide": [bool(f & 1) for f in flags], "filler": [bool(f & 2) for f in flags], "us": list(us)}


def _read_commands(lib, plan, n_sides):
    n = C.c_int64(0)
    L.check(lib.lic_plan_commands(plan, n_sides, 0, C.byref(n), None), "lic_plan_commands")
    buf = (C.c_int32 * (3 * n.value))()
    L.check(lib.lic_plan_commands(plan, n_sides, n.value, C.byref(n), buf), "lic_plan_commands")
    flat = list(buf)
    return list(zip(flat[0::3], flat[1::3], flat[2::3]))


class _ReadBack:
    """what the plan holds, as data (include/lic.h: lic_plan_dag, lic_plan_commands)"""

    def dag(self):
        """the captured operations in capture order: {'preds': [[...]], 'kind', 'wide', 'filler', 'us'}, one entry each"""
        return _read_dag(self._lib, self._plan)

    def commands(self, n_sides: int):
        """the HIP calls one replay makes with `n_sides` distinct side streams: [(kind, stream, argument)], kind
        0 = wait for an event, 1 = launch of an operation, 2 = record of an event"""
        return _read_commands(self._lib, self._plan, n_sides)


class _RatePoint:
    """The per-image values a recorded step reads from device memory -- the qualities and / or the lambdas of a rate-level
    model -- as rows of one resident [rows][B] tensor.  The capture bakes the tensor's address in, not its
    contents: `set` puts new values there in front of a replay, through one pinned staging tensor and ONE non-blocking
    copy (not part of the record, no host synchronisation).  The staging tensor has two halves used in turn, each behind
    the event of the copy that last read it: the host may run ahead of the device by a step without touching values
    still on their way."""

    def __init__(self, dev, batch: int, **initial):
        self.names = [k for k, v in initial.items() if v is not None]
        for k in self.names:
            v = initial[k]
            if not (torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (batch,)):
                raise L.LicError(f"`{k}` of a plan must be a CUDA float32 tensor [{batch}]")
        self.resident = torch.stack([initial[k].detach() for k in self.names]) if self.names else None
        if self.names:
            self.host = self.resident.cpu()                          # the values in place, for the arguments `set` omits
            self.stage = torch.empty((2,) + tuple(self.host.shape), dtype=torch.float32).pin_memory()
            self.events, self.turn = [None, None], 0

    def row(self, name):
        """the resident [B] tensor of `name`, or None when the plan holds it as a constant"""
        return self.resident[self.names.index(name)] if name in self.names else None

    def set(self, **values):
        """new values (host sequences or CPU tensors of B floats) for the rows named; None keeps what is there"""
        given = {k: v for k, v in values.items() if v is not None}
        if not given:
            return
        for k, v in given.items():
            if k not in self.names:
                raise L.LicError(f"this plan was captured without a resident `{k}`: it cannot change between replays")
            if torch.is_tensor(v) and v.is_cuda:
                raise L.LicError(f"`{k}` goes through a pinned host tensor: pass host values, or write the plan's resident "
                                 "tensor yourself")
            self.host[self.names.index(k)].copy_(torch.as_tensor(v, dtype=torch.float32).reshape(-1))
        slot, self.turn = self.turn, self.turn ^ 1
        if self.events[slot] is not None:
            self.events[slot].synchronize()   # (the copy of two calls ago: long done unless the host is far ahead)
        self.stage[slot].copy_(self.host)
        self.resident.copy_(self.stage[slot], non_blocking=True)
        self.events[slot] = torch.cuda.Event()
        self.events[slot].record()


class StepPlan(_ReadBack):
    def __init__(self, model, loss_fn: Callable, lambda_val, example: torch.Tensor, warmup: int = 2,
                 side_stream: Optional[torch.cuda.Stream] = None, tune: bool = False, quality=None):
        """`loss_fn(model_out, x, lambda_val, sync=False)` -> dict with 'loss' (loss.rd_loss); `example`: a batch
        of the shape every later batch will have.  Runs `warmup` eager steps WITHOUT an optimizer step (they fill
        the caches: packed-weight plan, gradient buffers, allocator), then captures one.
        A rate-level model: `quality` and `lambda_val` as CUDA float32 [B] tensors.  The plan keeps resident copies
        (`self.quality`, `self.lam`), records `model(x, quality=self.quality, device_quality=True)` and
        `loss_fn(out, x, self.lam, sync=False)`, and `step(x, quality=, lam=)` then serves any rate points, one per
        image.  (A float `lambda_val` is baked into the record as ever.)"""
        if not example.is_cuda:
            raise L.LicError("StepPlan needs a CUDA batch (there is no CPU fallback)")
        if torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size() > 1:
            raise L.LicError("StepPlan replays one GPU's step; data-parallel training uses the eager step "
                             "(the gradient all-reduce runs from autograd hooks)")
        self.model, self.loss_fn = model, loss_fn
        self.x = example.clone(memory_format=torch.preserve_format)
        self._plan = C.c_void_p()
        self._lib = L.load()
        dev = example.device
        self._rate = _RatePoint(dev, example.shape[0], quality=quality, lam=lambda_val if torch.is_tensor(lambda_val) else None)
        self.quality = self._rate.row("quality")
        self.lam = self._rate.row("lam") if torch.is_tensor(lambda_val) else lambda_val
        self._model_kw = {} if quality is None else {"quality": self.quality, "device_quality": True}
        self._one = torch.ones((), device=dev, dtype=torch.float32)
        gen_state = torch.cuda.get_rng_state(dev)   # (the probe and the warm-up draw noise: restored below)
        with torch.no_grad():
            probe = model.analysis_hyperprior(self.x, training=True, **self._model_kw) \
                if hasattr(model, "analysis_hyperprior") else model(self.x)
        y, z = probe["y"], probe["z"]
        Bn, Mc, hy, wy = y.shape
        _, Mz, hz, wz = z.shape
        nz, ny = Bn * hz * wz * Mz, Bn * hy * wy * Mc
        # one buffer, z's noise first: the layout (NHWC per latent) and the draw order of models.analysis_hyperprior
        self.u = torch.empty(nz + ny, device=dev, dtype=y.dtype)
        self.noise = (self.u[:nz].view(Bn, hz, wz, Mz).permute(0, 3, 1, 2),
                      self.u[nz:].view(Bn, hy, wy, Mc).permute(0, 3, 1, 2))
        del probe, y, z
        # the second stream: the model's own (high priority: the decoder chain it carries is the critical path of the
        # overlapped region -- the plan's second stream inherits the capture's fork, so it carries that chain too)
        if side_stream is None and hasattr(model, "side_stream"):
            side_stream = model.side_stream()
        self.side = side_stream if side_stream is not None else torch.cuda.Stream(device=dev)
        self.side2 = torch.cuda.Stream(device=dev)
        self._sides = (C.c_void_p * 2)(self.side.cuda_stream, self.side2.cuda_stream)
        cap = torch.cuda.Stream(device=dev)
        cap.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(cap):
            for _ in range(max(warmup, 1)):
                self._eager_body()
        torch.cuda.current_stream(dev).wait_stream(cap)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph(keep_graph=True)
        self._zero_grads()
        # launches the eager step SKIPS when nothing changed must be in the record: the warm-up took no optimizer
        # step, so the per-step weight preparation (prep.StepPrep.run) would see unchanged version counters
        prep = getattr(model, "_step_prep", None)
        if prep is not None:
            prep.invalidate()
        with torch.cuda.graph(self.graph, stream=cap):
            self.out, self.results = self._body()
        torch.cuda.set_rng_state(gen_state, dev)   # (building the plan leaves torch's generator where it found it)
        rc = self._lib.lic_plan_create(C.c_void_p(self.graph.raw_cuda_graph()), C.byref(self._plan))
        if rc != 0:
            why = self._lib.lic_plan_last_error().decode()
            self._plan = C.c_void_p()
            raise L.LicError(f"lic_plan_create failed: {L._STATUS.get(rc, rc)} ({why})")
        self.tuning = None
        if tune:
            # time every operation, list-schedule onto the two streams, keep whichever schedule measures faster
            # (a few dozen replays of the captured step: same inputs, same outputs)
            r = (C.c_double * 4)()
            rc = self._lib.lic_plan_tune(self._plan, _stream(), self._sides, 2, r)
            if rc != 0:
                raise L.LicError(f"lic_plan_tune failed: {L._STATUS.get(rc, rc)} ({self._lib.lic_plan_last_error().decode()})")
            torch.cuda.synchronize(dev)
            self.tuning = {"sum_of_operations_us": round(r[0], 1), "capture_order_us": round(r[1], 1),
                           "tuned_us": round(r[2], 1), "tuned_kept": bool(r[3])}
        info = (C.c_int64 * 7)()
        L.check(self._lib.lic_plan_info(self._plan, info), "lic_plan_info")
        self.info = dict(zip(("nodes", "kernels", "memsets", "memcpys", "on_side_stream", "events", "tuned"), list(info)))
        self.replays = 0
        self.streams = 3   # 1: everything on the caller's stream, 2: one side stream (A/B, debugging)
        self._params = list(model.parameters())
        self._grads = [p.grad for p in self._params]   # the captured step's gradient tensors: every replay rewrites them

    def _zero_grads(self):
        for p in self.model.parameters():
            p.grad = None
        for e in F_.GRAD_VIEWS.values():   # (bucket slots of a one-rank reducer may go out again)
            e[2] = False

    def _body(self):
        # (recorded steps launch the decoder's and the latent side's pending reductions as soon as dL/dy is complete, on the
        # second stream: functional.flush_point -- worth ~1 % replayed, harmful eager)
        F_.PLAN_RECORDING = True
        try:
            out = self.model(self.x, noise=self.noise, **self._model_kw)
            res = self.loss_fn(out, self.x, self.lam, sync=False)
            res["loss"].backward(self._one)   # (a resident 1.0: `backward()` alone launches a fill for it every step)
        finally:
            F_.PLAN_RECORDING = False
        return out, res

    def _eager_body(self):
        self._zero_grads()
        self.u.uniform_()
        return self._body()

    def step(self, x: torch.Tensor, quality=None, lam=None):
        """forward + loss + backward of `x` (same shape as the example): gradients land in `p.grad` of every
        parameter (the tensors of the captured step: same addresses every time); returns (model_out, results), the
        captured step's output tensors, rewritten by every call.  `quality`, `lam` (a plan captured with resident ones):
        B host values each for this and the following steps; omitted, the previous values stay."""
        if x.shape != self.x.shape:
            raise L.LicError(f"StepPlan was captured for batches of shape {tuple(self.x.shape)}, got {tuple(x.shape)}")
        if x.data_ptr() != self.x.data_ptr():
            self.x.copy_(x, non_blocking=True)
        self._rate.set(quality=quality, lam=lam)
        for p, g in zip(self._params, self._grads):   # (an optimizer.zero_grad(set_to_none=True) in between)
            if p.grad is not g:
                p.grad = g
        self.u.uniform_()
        rc = self._lib.lic_plan_replay(self._plan, _stream(), self._sides, self.streams - 1)
        if rc != 0:
            raise L.LicError(f"lic_plan_replay failed: {L._STATUS.get(rc, rc)} ({self._lib.lic_plan_last_error().decode()})")
        self.replays += 1
        return self.out, self.results

    def close(self):
        if self._plan:
            self._lib.lic_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ForwardPlan(_ReadBack):
    """The analysis + hyperprior forward (models.analysis_hyperprior: the scope BASELINE's north star quotes its roofline
    on; also what a serving process runs before the entropy coder) captured once under no_grad and replayed by the
    library -- StepPlan without the backward pass.  `training`: with the quantiser's uniform noise (drawn per call into a
    fixed buffer, the reference's order) or with rounding.  `quality` (a rate-level model): a CUDA float32 [B] tensor; the
    plan keeps a resident copy (`self.quality`) which the record reads, and `plan(x, quality=...)` serves any qualities."""

    def __init__(self, model, example: torch.Tensor, training: bool = True, warmup: int = 2, quality=None):
        if not example.is_cuda:
            raise L.LicError("ForwardPlan needs a CUDA batch (there is no CPU fallback)")
        self.model, self.training = model, training
        self._lib = L.load()
        self._plan = C.c_void_p()
        self.x = example.clone(memory_format=torch.preserve_format)
        dev = example.device
        self._rate = _RatePoint(dev, example.shape[0], quality=quality)
        self.quality = self._rate.row("quality")
        kw = {} if quality is None else {"quality": self.quality, "device_quality": True}
        gen_state = torch.cuda.get_rng_state(dev)
        with torch.no_grad():
            probe = model.analysis_hyperprior(self.x, training=training, **kw)
        y, z = probe["y"], probe["z"]
        Bn, Mc, hy, wy = y.shape
        _, Mz, hz, wz = z.shape
        nz, ny = Bn * hz * wz * Mz, Bn * hy * wy * Mc
        self.u = torch.empty(nz + ny, device=dev, dtype=y.dtype)
        self.noise = (self.u[:nz].view(Bn, hz, wz, Mz).permute(0, 3, 1, 2),
                      self.u[nz:].view(Bn, hy, wy, Mc).permute(0, 3, 1, 2)) if training else None
        del probe, y, z
        self.side = model.side_stream() if hasattr(model, "side_stream") else torch.cuda.Stream(device=dev)
        self._sides = (C.c_void_p * 1)(self.side.cuda_stream)
        cap = torch.cuda.Stream(device=dev)
        cap.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(cap), torch.no_grad():
            for _ in range(max(warmup, 1)):
                self.u.uniform_()
                model.analysis_hyperprior(self.x, training=training, noise=self.noise, **kw)
        torch.cuda.current_stream(dev).wait_stream(cap)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.no_grad(), torch.cuda.graph(self.graph, stream=cap):
            self.out = model.analysis_hyperprior(self.x, training=training, noise=self.noise, **kw)
        torch.cuda.set_rng_state(gen_state, dev)
        rc = self._lib.lic_plan_create(C.c_void_p(self.graph.raw_cuda_graph()), C.byref(self._plan))
        if rc != 0:
            why = self._lib.lic_plan_last_error().decode()
            self._plan = C.c_void_p()
            raise L.LicError(f"lic_plan_create failed: {L._STATUS.get(rc, rc)} ({why})")
        info = (C.c_int64 * 7)()
        L.check(self._lib.lic_plan_info(self._plan, info), "lic_plan_info")
        self.info = dict(zip(("nodes", "kernels", "memsets", "memcpys", "on_side_stream", "events", "tuned"), list(info)))

    def __call__(self, x: torch.Tensor, quality=None):
        if x.shape != self.x.shape:
            raise L.LicError(f"ForwardPlan was captured for batches of shape {tuple(self.x.shape)}, got {tuple(x.shape)}")
        if x.data_ptr() != self.x.data_ptr():
            self.x.copy_(x, non_blocking=True)
        self._rate.set(quality=quality)
        if self.training:
            self.u.uniform_()
        rc = self._lib.lic_plan_replay(self._plan, _stream(), self._sides, 1)
        if rc != 0:
            raise L.LicError(f"lic_plan_replay failed: {L._STATUS.get(rc, rc)} ({self._lib.lic_plan_last_error().decode()})")
        return self.out

    def close(self):
        if self._plan:
            self._lib.lic_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
