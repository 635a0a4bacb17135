"""Reductions left pending until the end of a backward pass (lic_reduce_batch, include/lic.h).

The bf16 layers' weight-gradient slab reductions and second-stage column sums are 5-15 us launches, ~40 per step:
their first stages run at once (the `_partial` entry points fill an L.ReduceJob), the jobs wait in the queue below and
one batched launch finishes them all when autograd's backward pass ends.  The fp32 layers never queue anything: they
call the immediate entry points only.

The queue, its switch and the bf16 reduction helpers that feed it live here; functional.py re-exports the public
names.  The knobs this module reads (GRAD_VIEWS, PLAN_RECORDING) stay attributes of `functional`, read at call time.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import functional as F_   # (imports this module back: its names are used at call time only)

DEFER_REDUCTIONS = True   # False: every reduction right away, launch by launch (the tests compare the two)
_PENDING_JOBS = []   # L.ReduceJob of the running backward pass
_PENDING_KEEP = []   # tensors they name: partial sums, operands, parameters
_PENDING_SEEN = set()   # id() of the parameters whose gradients are pending
_PENDING_LATE = []   # tensors of an EARLY flush on another stream: released at the end of the pass


def flush_reductions(early_on=None):
    """launch every pending reduction (one lic_reduce_batch).  Autograd calls this at the end of a backward pass, on the
    caller's stream, after that stream has been made to wait for every stream gradients were produced on.
    `early_on` (a stream; flush_point's backward): launch what is pending so far on THAT stream, after everything queued
    on the current one -- the batched reduction holds no LDS and few registers, so unlike the weight-gradient launches it
    does run beside the data-gradient chain that continues on the current stream.  The tensors it reads were allocated on
    their producers' streams: they are kept until the end of the pass, where the engine orders the caller's stream behind
    every stream of the pass."""
    if _PENDING_JOBS:
        n = len(_PENDING_JOBS)
        arr = (L.ReduceJob * n)(*_PENDING_JOBS)
        del _PENDING_JOBS[:]
        try:
            if early_on is not None:
                early_on.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(early_on):
                    L.check(L.load().lic_reduce_batch(arr, n, F_._stream()), "lic_reduce_batch")
                _PENDING_LATE.extend(_PENDING_KEEP)
            else:
                L.check(L.load().lic_reduce_batch(arr, n, F_._stream()), "lic_reduce_batch")
        finally:
            del _PENDING_KEEP[:]
    if early_on is None:
        del _PENDING_LATE[:]
        _PENDING_SEEN.clear()


class _FlushPointFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, stream):
        ctx.stream = stream
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        if _PENDING_JOBS and ctx.stream is not None:
            flush_reductions(early_on=ctx.stream)
        return g, None


def flush_point(t: torch.Tensor, stream):
    """identity; in the backward pass, when the gradient of `t` is complete, the reductions pending so far (those of
    everything downstream of `t`) are launched on `stream` while the pass continues upstream of `t` on its own stream"""
    if not (F_.PLAN_RECORDING and DEFER_REDUCTIONS and t.requires_grad and torch.is_grad_enabled() and
            stream is not None) or F_.GRAD_VIEWS:
        return t
    return _FlushPointFn.apply(t, stream)


_WILL_EXECUTE = getattr(torch._C, "_will_engine_execute_node", None)
_GRADIENT_EDGE = getattr(torch.autograd.graph, "get_gradient_edge", None)


def _gradient_kept(p) -> bool:
    """Will the running backward pass hand the gradient of leaf `p` to its AccumulateGrad node, which keeps the tensor
    alive until the pending reduction has written it?  Not in a pass restricted to other inputs
    (torch.autograd.grad(y, [x]), backward(inputs=[x])): ctx.needs_input_grad still asks for the gradient, the engine
    drops the returned tensor at once, and a reduction left pending would write into memory the allocator has handed to
    someone else by then.  Nor where the gradient is captured for the caller (torch.autograd.grad(y, [p]): the engine
    refuses the question for a captured leaf) or outside a backward pass: those reduce at once as well.  The engine's
    answer comes from torch._C._will_engine_execute_node (private; checked against torch 2.10): where a build lacks it,
    nothing is deferred."""
    if _WILL_EXECUTE is None or _GRADIENT_EDGE is None:
        return False
    try:
        return bool(_WILL_EXECUTE(_GRADIENT_EDGE(p).node))
    except RuntimeError:
        return False


def can_defer(*params) -> bool:
    """May the reductions behind the gradients of `params` wait for the end of this backward pass?  Only if nothing
    reads such a gradient earlier: no data-parallel bucket hooks (they fire per gradient), the parameter has no
    gradient yet (autograd would ADD to it on arrival) and has not been met before in this pass (two uses of one
    parameter are summed when the second arrives: everything pending is flushed first), and we are inside a backward
    pass of the autograd engine (the flush is its final callback).  The pending job names the gradient tensor's memory
    but holds no reference to the tensor: autograd adopts a returned gradient as `.grad` only while nobody else holds it
    (otherwise it would COPY it -- before the reduction has run).  `params` must name EVERY leaf whose reduction the
    caller leaves pending under this answer (a layer's bias beside its weight): one of them dropped by a pass restricted
    to the others is enough to refuse."""
    if not DEFER_REDUCTIONS or F_.GRAD_VIEWS:
        return False
    ps = [p for p in params if p is not None]
    if not ps:
        return False
    if not all(p.is_leaf for p in ps):   # a derived weight: its gradient is READ by the next backward node
        return False
    if not all(_gradient_kept(p) for p in ps):
        return False
    if any(p.grad is not None or id(p) in _PENDING_SEEN for p in ps):
        flush_reductions()
        return False
    try:
        torch.autograd.Variable._execution_engine.queue_callback(flush_reductions)
    except RuntimeError:
        return False
    _PENDING_SEEN.update(id(p) for p in ps)
    return True


def defer(job, *keep):
    """queue `job` for the pass's batched reduction; `keep`: the tensors it names (None entries are skipped), held until
    it has run -- never the gradient tensor it writes (see can_defer)"""
    _PENDING_JOBS.append(job)
    _PENDING_KEEP.extend(t for t in keep if t is not None)


def _reparam_epilogue(job, param_c, bound):
    """`job`'s sums go through the backward of the GDN re-parametrisation of `param_c` (the caller keeps `param_c`)"""
    job.epilogue, job.param, job.bound = L.REDUCE_EPI_REPARAM, param_c.data_ptr(), bound


def _defer_sums(job, reparam, *keep):
    """defer `job`; `reparam` = (parameter, bound) or None: with the re-parametrisation's backward behind its sums"""
    if reparam is None:
        defer(job, *keep)
    else:
        _reparam_epilogue(job, *reparam)
        defer(job, reparam[0], *keep)


# ------------------------------------------------------------------------------------------
# the bf16 layers' column sums: allocate, run the first stage (`dfr`: leave the second to the queue), hand the job over
# ------------------------------------------------------------------------------------------
def _colsum_bf16(t2d, P, Cc, dfr=False, reparam=None):
    """column sums of a bf16 [P][Cc] matrix; `dfr`: stage 2 joins the backward pass's batched reduction; `reparam` =
    (parameter, bound): followed by the GDN re-parametrisation's backward (deferred mode only)"""
    lib = L.load()
    nbytes = lib.lic_colsum_bf16_workspace_bytes(P, Cc)
    ws = torch.empty((nbytes + 3) // 4, device=t2d.device, dtype=torch.float32)
    out = torch.empty((Cc,), device=t2d.device, dtype=torch.float32)
    if dfr:
        job = L.ReduceJob()
        L.check(lib.lic_colsum_bf16_partial(F_._ptr(t2d), Cc, P, Cc, 1.0, F_._ptr(out), F_._ptr(ws), nbytes, C.byref(job),
                                            F_._stream()), "lic_colsum_bf16_partial")
        _defer_sums(job, reparam, ws, t2d)
    else:
        L.check(lib.lic_colsum_bf16(F_._ptr(t2d), Cc, P, Cc, 1.0, F_._ptr(out), F_._ptr(ws), nbytes, F_._stream()),
                "lic_colsum_bf16")
    return out


def _rows_sum(part, dfr=False, reparam=None):
    """column sums of a small fp32 [rows][C] matrix of partial sums (the per-workgroup rows lic_gdn_bwd_bf16 leaves):
    one COLUMNS job, pending (`dfr`, optionally with the re-parametrisation's backward) or run right away as a one-job
    lic_reduce_batch -- the same kernel, so that deferring changes no bit"""
    rows, Cc = part.shape
    out = torch.empty((Cc,), device=part.device, dtype=torch.float32)
    job = L.ReduceJob()
    job.src, job.dst, job.kind, job.splitk, job.Cn, job.scale = part.data_ptr(), out.data_ptr(), L.REDUCE_COLUMNS, rows, Cc, 1.0
    if dfr:
        _defer_sums(job, reparam, part)
    else:
        L.check(L.load().lic_reduce_batch(C.byref(job), 1, F_._stream()), "lic_reduce_batch")
    return out


def _colsum2_bf16(a2d, b2d, P, Cc, dfr=False, reparam_a=None):
    """column sums of two bf16 [P][Cc] matrices in one launch pair (`dfr` / `reparam_a`: as _colsum_bf16, the
    re-parametrisation applies to the first matrix's sums)"""
    lib = L.load()
    nbytes = 2 * lib.lic_colsum_bf16_workspace_bytes(P, Cc)
    ws = torch.empty((nbytes + 3) // 4, device=a2d.device, dtype=torch.float32)
    out = torch.empty((2, Cc), device=a2d.device, dtype=torch.float32)
    if dfr:
        jobs = (L.ReduceJob * 2)()
        L.check(lib.lic_colsum2_bf16_partial(F_._ptr(a2d), F_._ptr(b2d), Cc, P, Cc, 1.0, F_._ptr(out[0]), F_._ptr(out[1]),
                                             F_._ptr(ws), nbytes, jobs, F_._stream()), "lic_colsum2_bf16_partial")
        _defer_sums(L.ReduceJob.from_buffer_copy(jobs[0]), reparam_a, ws, a2d, b2d)
        defer(L.ReduceJob.from_buffer_copy(jobs[1]))
    else:
        L.check(lib.lic_colsum2_bf16(F_._ptr(a2d), F_._ptr(b2d), Cc, P, Cc, 1.0, F_._ptr(out[0]), F_._ptr(out[1]),
                                     F_._ptr(ws), nbytes, F_._stream()), "lic_colsum2_bf16")
    return out[0], out[1]


def _leaky_bwd_colsum_bf16(y, dy, slope, P, Cc, dfr=False):
    """(dy through the LeakyReLU's backward, its column sums): _leaky_bwd_bf16 + _colsum_bf16 in one pass, the same bits"""
    lib = L.load()
    dx = torch.empty_like(y)
    nbytes = lib.lic_colsum_bf16_workspace_bytes(P, Cc)
    ws = torch.empty((nbytes + 3) // 4, device=y.device, dtype=torch.float32)
    out = torch.empty((Cc,), device=y.device, dtype=torch.float32)
    job = L.ReduceJob() if dfr else None
    L.check(lib.lic_leaky_bwd_colsum_bf16(F_._ptr(y), F_._ptr(dy), F_._ptr(dx), P, Cc, slope, F_._ptr(out), F_._ptr(ws), nbytes,
                                          C.byref(job) if dfr else None, F_._stream()), "lic_leaky_bwd_colsum_bf16")
    if dfr:
        defer(job, ws)
    return dx, out
