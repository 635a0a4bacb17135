"""`FusedAdam`: torch.optim.Adam whose `step()` is ONE kernel launch (`lic_adam_run`, include/lic.h) over every
parameter instead of nine multi-tensor launches.

A subclass of torch.optim.Adam: same constructor, same `state_dict()` (`step`, `exp_avg`, `exp_avg_sq` per
parameter, created by torch's own `_init_group`), so checkpoints move freely between the two -- the reference's
`Trainer` takes whatever optimizer it is given (Trainer.py:11-16) and the notebook builds `torch.optim.Adam`
(Main.ipynb).  The arithmetic is torch's non-amsgrad Adam with L2 weight decay, bias corrections computed on
the host from the step count (torch's default, non-capturable path); anything else -- amsgrad, maximize,
capturable / differentiable, non-fp32 or CPU parameters, parameters without gradients, step counts that differ
between parameters -- falls through to torch's implementation for that call.

`FusedAdam(..., max_grad_norm=m, skip_nonfinite=True)` adds what `torch.nn.utils.clip_grad_norm_(params, m)` in
front of `step()` does, and a guard against a non-finite step, without the foreach launches and the ~240 host-side
calls of that recipe: `lic_grad_norm_partial` per group and one `lic_grad_norm_finish` leave the global L2 norm, the
clipping coefficient and a not-finite flag in 4 dwords of device memory, and `lic_adam_run_scaled` reads them there
-- the host never waits for the norm.  `grad_norm()` is the last step's norm (a device scalar), `skipped_steps()`
the number of steps the guard dropped.  ONE deviation from GradScaler-style skipping: a skipped fused step leaves
parameters and moments untouched but still advances the step count, because the bias corrections are computed on
the host from that count and the host does not know the flag.  (The fallback path reads the norm back anyway and
skips before torch's step, so there the count stays.)  `grad_norm(parameters)` is the norm alone, for any optimizer.

`FusedAdam(..., ema_decay=d, ema_warmup=True)` keeps the exponential moving average of the weights these models are
evaluated and shipped with, in `state[p]["ema"]`, inside the same launch (`lic_adam_run_ema`: the parameter is in
registers when its average moves -- no foreach launches, no second read of every parameter):
    e += w * (p_new - e),  w = 1 - d_t,  d_t = min(d, (1 + t) / (10 + t)) with warm-up, d without
with t the 1-based step count the bias corrections use, w formed in double on the host and rounded to fp32 once, and
three fp32 roundings per element.  The torch path applies the same three operations after torch's step and gives the
same bits for the same p.  `swap_ema()` exchanges weights and averages (`lic_swap_run`) and bumps the version
counter of every tensor it wrote, so whatever is derived from the parameters (prep.StepPrep, functional.PREPARED,
the masked context weight, the bf16 packs) is derived again; `with opt.ema_weights():` swaps in and back,
`ema_state_dict(model)` is the model's state dict under the averages.  `step()` refuses to run while swapped.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import struct
from typing import NamedTuple

import torch

from . import _lib as L
from . import functional as F_


class JobTable(NamedTuple):
    """one lic_adam_plan partition on the device, and what it was built for"""
    key: object         # the addresses and lengths the table holds: built again when they differ
    dev: torch.Tensor   # the lic_adam_job array; behind it the averages' addresses, where the table has any
    njobs: int
    blocks: int
    gptrs: object       # ctypes array of njobs gradient addresses, filled per launch (None: no gradients travel)

    def ema_ptr(self):
        """the device table of the averages' addresses (lic_adam_run_ema, lic_swap_run: 8-byte aligned)"""
        return self.dev.data_ptr() + self.njobs * C.sizeof(L.AdamJob)


def _upload_jobs(jobs, dev, emas=()):
    """(p, m, v, n) address tuples -> (their lic_adam_job array, partitioned by lic_adam_plan, on `dev`; its block
    count).  `emas`: one address per job, uploaded behind the array in the same copy (JobTable.ema_ptr)"""
    arr = (L.AdamJob * len(jobs))()
    for j, job in zip(arr, jobs):
        j.p, j.m, j.v, j.n = job
    blocks = L.load().lic_adam_plan(arr, len(jobs))
    if blocks <= 0:
        raise L.LicError(f"lic_adam_plan failed: {blocks}")
    raw = bytearray(bytes(arr) + struct.pack(f"{len(emas)}q", *emas))
    return torch.frombuffer(raw, dtype=torch.uint8).to(dev), int(blocks)


def _launch_norm(lib, tabs, partials, max_norm, count_skip, state):
    """lic_grad_norm_partial over the gradients each table's `gptrs` point at, one lic_grad_norm_finish over all"""
    stream, at = F_._stream(), 0
    for tab in tabs:
        L.check(lib.lic_grad_norm_partial(C.c_void_p(tab.dev.data_ptr()), tab.njobs, tab.blocks, tab.gptrs,
                                          C.c_void_p(partials.data_ptr() + 8 * at), stream), "lic_grad_norm_partial")
        at += tab.blocks
    L.check(lib.lic_grad_norm_finish(C.c_void_p(partials.data_ptr()), at, max_norm, count_skip,
                                     C.c_void_p(state.data_ptr()), stream), "lic_grad_norm_finish")


def clip_gradients(parameters, max_norm, skip_nonfinite):
    """torch's clipping, where the kernels do not do it: torch.nn.utils.clip_grad_norm_ over the parameters that have
    a gradient (max_norm None: the norm alone).  Returns (norm, skip): skip says that skip_nonfinite is on and the
    norm is not finite -- reading that back is the one synchronisation, made only when skip_nonfinite is on."""
    params = [p for p in parameters if p.grad is not None]
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(params, float(max_norm))
    else:
        norm = torch.nn.utils.get_total_norm([p.grad for p in params])
    return norm, bool(skip_nonfinite) and not bool(torch.isfinite(norm))


def _hyper(group):
    """what a cached plan was made for besides the tensors: a change of any of these plans the step again"""
    return (group["lr"], group["betas"], group["eps"], group["weight_decay"], group["amsgrad"], group.get("maximize"),
            group.get("capturable"), group.get("differentiable"))


class _GroupPlan:
    """one parameter group's part of a planned step"""
    __slots__ = ("group", "plist", "params", "hyper", "table", "bumped", "steps", "ema")

    def __init__(self, group, params, table, bumped, steps, ema):
        self.group, self.plist, self.params, self.hyper = group, group["params"], params, _hyper(group)
        self.table, self.bumped, self.steps = table, bumped, steps   # bumped: the tensors a launch writes
        self.ema = ema      # address of the device table of averages, None without


class FusedAdam(torch.optim.Adam):
    MAX_TENSORS = 448   # per parameter group (include/lic.h: lic_adam_run)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=True, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        # global-norm clipping over ALL groups (torch.nn.utils.clip_grad_norm_'s max_norm) / leave the step out when
        # the norm is not finite.  Attributes of the optimizer, not of param_groups: the state dict stays torch's
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be >= 0, got {max_grad_norm}")
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        # the moving average of the weights: state[p]["ema"], part of the state dict only when it is on
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        self.ema_decay, self.ema_warmup = (None if ema_decay is None else float(ema_decay)), bool(ema_warmup)
        self.swapped = False      # True while the averages are the live weights (swap_ema)
        self._swap_tabs = {}      # group index -> JobTable of swap_ema() (with the averages' addresses, no gradients)
        self._clip_state = None   # 4 dwords on the device: norm, coefficient, not-finite flag, skipped steps (lic.h)
        self._partials = None     # one double per block of every group (lic_grad_norm_partial), allocated per plan
        self._last_norm = None    # what grad_norm() returns
        self._skipped_host = 0    # steps skipped on the fallback path
        self._tables = {}   # group index -> JobTable of step(), kept while its key holds
        self._fast = None   # the last planned step (a _GroupPlan per group), re-used while nothing it depends on changed
        self._t0, self._lazy = 0.0, 0   # step count the plan started from / fast steps not yet written to the state
        self.fused_steps = 0

    def _eligible(self, group, params, grads):
        if group["amsgrad"] or group.get("maximize") or group.get("capturable") or group.get("differentiable"):
            return False
        if isinstance(group["lr"], torch.Tensor) or not params or len(params) > self.MAX_TENSORS:
            return False   # (lic_adam_run's kernel-argument block holds MAX_TENSORS gradient addresses)
        dev = params[0].device
        for p, g in zip(params, grads):
            if p.device != dev or not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or \
                    g.is_sparse or not p.is_contiguous() or not g.is_contiguous():
                return False
        return dev.index == torch.cuda.current_device()

    def _clipping(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _clip_prologue(self, lib, tabs):
        """the norm of the gradients `tabs` (one job table per group) point at -> self._clip_state, no read-back"""
        dev = tabs[0].dev.device
        total = sum(t.blocks for t in tabs)
        if self._clip_state is None or self._clip_state.device != dev:
            self._skipped_host = self.skipped_steps()
            self._clip_state = torch.zeros(4, dtype=torch.float32, device=dev)
        if self._partials is None or self._partials.numel() != total or self._partials.device != dev:
            self._partials = torch.empty(total, dtype=torch.float64, device=dev)
        max_norm = float("inf") if self.max_grad_norm is None else float(self.max_grad_norm)
        _launch_norm(lib, tabs, self._partials, max_norm, int(self.skip_nonfinite), self._clip_state)
        self._last_norm = self._clip_state[0]

    def _launch(self, lib, plan, t, clip):
        """the update of one group at the 1-based step count t: lic_adam_run, or the entry that adds what is on"""
        group, tab = plan.group, plan.table
        beta1, beta2 = group["betas"]
        args = [C.c_void_p(tab.dev.data_ptr()), tab.njobs, tab.blocks, tab.gptrs, float(group["lr"]), float(beta1),
                float(beta2), float(group["eps"]), float(group["weight_decay"]), 1.0 - beta1 ** t, 1.0 - beta2 ** t]
        state = C.c_void_p(self._clip_state.data_ptr()) if clip else None
        if plan.ema is not None:
            name = "lic_adam_run_ema"
            args += [C.c_void_p(plan.ema), self._ema_weight(t), state, int(self.skip_nonfinite)]
        elif clip:
            name = "lic_adam_run_scaled"
            args += [state, int(self.skip_nonfinite)]
        else:
            name = "lic_adam_run"
        L.check(getattr(lib, name)(*args, F_._stream()), name)

    def _ema_weight(self, t):
        """w of e += w * (p - e) at the 1-based step count t, in double (lic.h: lic_adam_run_ema rounds it once)"""
        d = self.ema_decay
        if self.ema_warmup:
            d = min(d, (1.0 + t) / (10.0 + t))
        return 1.0 - d

    def _ema_buffers(self, params):
        """state[p]["ema"] of every parameter, created as a copy of p where the state has none yet (a new state, or
        one loaded from a state dict without averages)"""
        out = []
        for p in params:
            st = self.state[p]
            if "ema" not in st:
                st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
            out.append(st["ema"])
        return out

    def grad_norm(self):
        """global L2 norm of the gradients of the last step(): a 0-dim tensor on the parameters' device (a view of the
        kernels' state after a fused step: reading it is the caller's synchronisation, this call makes none)"""
        if not self._clipping():
            raise RuntimeError("gradient clipping is off: construct FusedAdam with max_grad_norm= and / or "
                               "skip_nonfinite=True to have the norm computed")
        if self._last_norm is None:
            raise RuntimeError("grad_norm() is the norm of the last step(): no step has been taken yet")
        return self._last_norm

    def skipped_steps(self):
        """number of steps skip_nonfinite dropped so far (one read-back of 4 bytes)"""
        n = self._skipped_host
        if self._clip_state is not None:
            n += int(self._clip_state.view(torch.int32)[3])
        return n

    @torch.no_grad()
    def step(self, closure=None):
        if self.swapped:
            raise RuntimeError("step() while the averaged weights are swapped in: call swap_ema() first (or leave the "
                               "ema_weights() context)")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # Fast path (the host side of the step is what bounds the bf16 configurations: planning a launch through
        # torch's `_init_group` and re-deriving the job-table key cost 0.5 ms of a 4.4 ms step): once a step has
        # been planned, the next one only checks that the groups' parameter lists and hyper-parameters are the very
        # objects / values it planned for and that every gradient is there, then gathers the gradient addresses.
        plans = self._fast
        if plans is not None and self._plan_holds(plans):
            self._run(plans, self._t0 + self._lazy + 1.0)
            # the per-parameter `step` tensors of the state (CPU scalars, one per parameter: bumping them is ~240
            # small ATen calls per step) are brought up to date lazily: _flush_steps() before anything reads them
            self._lazy += 1
        else:
            plans = self._plan()
            if plans is None:
                return self._fallback(loss)
            self._run(plans, None)
            # (the job tables hold the parameter / moment addresses: valid while these very tensors are the state.
            # _plan() took whole groups only and made the tables' keys from these tensors a moment ago, so what is
            # left to ask before the plan is kept is that all groups share one step count)
            if len({float(pl.steps[0]) for pl in plans}) == 1:
                self._fast = plans
                self._t0, self._lazy = float(plans[0].steps[0]), 0
        self.fused_steps += 1
        return loss

    def _plan_holds(self, plans):
        """is every group what `plans` was made for, and every gradient there"""
        if len(plans) != len(self.param_groups):
            return False
        for plan, g in zip(plans, self.param_groups):
            if g is not plan.group or g["params"] is not plan.plist or len(plan.plist) != len(plan.params) or \
                    _hyper(g) != plan.hyper:
                return False
            for p, k in zip(plan.params, plan.table.key):
                gr = p.grad
                if gr is None or gr.dtype != torch.float32 or not gr.is_contiguous() or p.data_ptr() != k[0]:
                    return False   # (a missing gradient, or parameter storage that moved: plan again)
        return True

    def _plan(self):
        """a _GroupPlan per group from the state as it is now, the job tables built or re-used; None when any group
        has to take torch's path.  Whatever was cached is flushed and dropped first."""
        self._flush_steps()
        self._fast = None
        found = []
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps = [], [], [], [], [], []
            self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps)
            emas = self._ema_buffers(params) if self.ema_decay is not None else None
            if len(params) != len([p for p in group["params"]]) or not self._eligible(group, params, grads) or \
                    not all(m.is_contiguous() and v.is_contiguous() for m, v in zip(exp_avgs, exp_avg_sqs)) or \
                    len({float(s) for s in steps}) != 1:
                return None
            if emas is not None and not all(e.is_contiguous() and e.dtype == torch.float32 and e.device == p.device
                                            for p, e in zip(params, emas)):
                return None
            found.append((group, params, exp_avgs, exp_avg_sqs, steps, emas))
        plans = []
        for gi, (group, params, exp_avgs, exp_avg_sqs, steps, emas) in enumerate(found):
            key = tuple((p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, m, v in zip(params, exp_avgs, exp_avg_sqs))
            if emas is not None:    # (the averages' addresses are part of what the plan was made for)
                key = tuple(k + (e.data_ptr(),) for k, e in zip(key, emas))
            tab = self._tables.get(gi)
            if tab is None or tab.key != key:
                dev_tab, blocks = _upload_jobs([k[:4] for k in key], params[0].device,
                                               () if emas is None else [k[4] for k in key])
                tab = self._tables[gi] = JobTable(key, dev_tab, len(params), blocks, (C.c_void_p * len(params))())
            # the kernel writes through raw pointers: autograd (and prep.StepPrep, which re-derives the packed
            # weights when a parameter's version moves) is told that the parameters and moments changed
            written = params + exp_avgs + exp_avg_sqs + (emas or [])
            ema = None if emas is None else tab.ema_ptr()
            plans.append(_GroupPlan(group, list(params), tab, written, list(steps), ema))
        return plans

    def _run(self, plans, t):
        """the launches of one step.  t: the 1-based step count all groups share (the cached plan), or None: each
        group's own, from its `step` tensors, which are then incremented behind its launch"""
        lib = L.load()
        clip = self._clipping()
        for plan in plans:
            gptrs = plan.table.gptrs
            for i, p in enumerate(plan.params):    # gradients are fresh tensors every step: their addresses go along
                gptrs[i] = p.grad.data_ptr()       # as kernel arguments (copied at launch)
        if clip:    # (the norm is global: every group's partial sums before the first update)
            self._clip_prologue(lib, [plan.table for plan in plans])
        for plan in plans:
            self._launch(lib, plan, float(plan.steps[0]) + 1.0 if t is None else t, clip)
            if t is None:
                for s in plan.steps:     # (only once the launch went out: a refused launch leaves the state untouched)
                    s += 1
            torch.autograd.graph.increment_version(plan.bumped)

    def _flush_steps(self):
        """apply the step counts the fast path has not yet written into the state's `step` tensors"""
        n, fast = getattr(self, "_lazy", 0), self._fast
        if n and fast is not None:
            for plan in fast:
                for s in plan.steps:
                    s += n
            self._t0 += n
        self._lazy = 0

    def state_dict(self):
        self._flush_steps()
        return super().state_dict()

    def zero_grad(self, set_to_none: bool = True):
        # (torch's zero_grad walks every group through a profiler scope and foreach bookkeeping: 0.1 ms for 59 tensors)
        if set_to_none and self._fast is not None:
            for plan in self._fast:
                for p in plan.params:
                    p.grad = None
            return
        return super().zero_grad(set_to_none)

    def load_state_dict(self, state_dict):
        self._flush_steps()
        self._fast = None          # (new state tensors: plan again)
        self._tables, self._swap_tabs = {}, {}
        return super().load_state_dict(state_dict)

    def add_param_group(self, param_group):
        if getattr(self, "_fast", None) is not None:
            self._flush_steps()
        self._fast = None
        return super().add_param_group(param_group)

    def _fallback(self, loss):
        """torch's own update for this call (state was initialised by the same `_init_group`)"""
        self._flush_steps()
        self._fast = None
        if self._clipping():
            self._last_norm, skip = clip_gradients([p for group in self.param_groups for p in group["params"]],
                                                   self.max_grad_norm, self.skip_nonfinite)
            if skip:
                self._skipped_host += 1
                return loss    # (the averages stay as they are, like everything else)
        if self.ema_decay is None:
            super().step()
            return loss
        # torch creates a parameter's state only where it finds none at all: the copies the averages start from
        # are taken before the step and entered behind it
        start = {p: p.detach().clone(memory_format=torch.contiguous_format) for group in self.param_groups
                 for p in group["params"] if p.grad is not None and "ema" not in self.state.get(p, {})}
        stepped = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        super().step()
        by_count = collections.defaultdict(list)
        for p in stepped:
            st = self.state[p]
            if "ema" not in st:
                st["ema"] = start[p]
            by_count[float(st["step"])].append(p)
        for t, ps in by_count.items():
            # lic_adam_run_ema's three roundings: p - e, w * (...), e + (...), w rounded to fp32 once
            w = struct.unpack("f", struct.pack("f", self._ema_weight(t)))[0]
            es = [self.state[p]["ema"] for p in ps]
            diff = torch._foreach_sub([p.detach() for p in ps], es)
            torch._foreach_mul_(diff, w)
            torch._foreach_add_(es, diff)
        return loss

    # -- the averaged weights ------------------------------------------------------------------------------------
    def _swap_fused(self, pairs):
        if len(pairs) > self.MAX_TENSORS:
            return False
        dev = pairs[0][0].device
        for p, e in pairs:
            if p.device != dev or not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or \
                    e.device != dev or e.dtype != torch.float32 or not e.is_contiguous() or p.numel() == 0:
                return False
        return dev.index == torch.cuda.current_device()

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every parameter with its average, bit for bit: one `lic_swap_run` per group that a fused step can
        take, torch copies otherwise.  Every tensor written gets its version counter bumped, so step preparation and
        every cache keyed on a parameter's version derive their buffers again on the next forward -- nothing for the
        caller to remember.  `swapped` says which side is live."""
        if self.ema_decay is None:
            raise RuntimeError("the moving average is off: construct FusedAdam with ema_decay=")
        written = []
        for gi, group in enumerate(self.param_groups):
            pairs = [(p, self.state[p]["ema"]) for p in group["params"] if "ema" in self.state.get(p, {})]
            if not pairs:
                continue
            if self._swap_fused(pairs):
                lib = L.load()
                key = tuple((p.data_ptr(), e.data_ptr(), p.numel()) for p, e in pairs)
                tab = self._swap_tabs.get(gi)
                if tab is None or tab.key != key:
                    # (only p and n are read: lic_adam_plan wants m / v non-null)
                    dev_tab, blocks = _upload_jobs([(p, p, p, n) for p, _, n in key], pairs[0][0].device,
                                                   [e for _, e, _ in key])
                    tab = self._swap_tabs[gi] = JobTable(key, dev_tab, len(pairs), blocks, None)
                L.check(lib.lic_swap_run(C.c_void_p(tab.dev.data_ptr()), tab.njobs, tab.blocks,
                                         C.c_void_p(tab.ema_ptr()), F_._stream()), "lic_swap_run")
                for p, e in pairs:      # (written through raw pointers: tell autograd and everything keyed on versions)
                    written += [p, e]
            else:
                for p, e in pairs:      # (in-place ops on a detached view bump the parameter's own counter)
                    keep = p.detach().clone()
                    p.detach().copy_(e)
                    e.copy_(keep)
        if written:
            torch.autograd.graph.increment_version(written)
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights():` -- the averaged weights are the live ones inside (validation, coding), the trained
        ones again behind it, whatever happens inside"""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    @torch.no_grad()
    def ema_state_dict(self, model):
        """`model.state_dict()` with every averaged parameter replaced by its average (copies; buffers and parameters
        without an average as they are).  The model is not touched."""
        if self.ema_decay is None:
            raise RuntimeError("the moving average is off: construct FusedAdam with ema_decay=")
        out = collections.OrderedDict((k, v.detach().clone()) for k, v in model.state_dict().items())
        if not self.swapped:    # (while swapped the model already holds the averages)
            for name, p in model.named_parameters(remove_duplicate=False):
                e = self.state.get(p, {}).get("ema")
                if e is not None and name in out:
                    out[name] = e.detach().clone().view_as(out[name])
        return out


_norm_tables = {}   # (device, tensor lengths) -> [(device job table, njobs, blocks)] of grad_norm()


def grad_norm(parameters):
    """Global L2 norm of the gradients of `parameters` (fp32 CUDA tensors on the current device, contiguous gradients;
    parameters without a gradient are left out, as torch.nn.utils.clip_grad_norm_ does): the two launches FusedAdam's
    clipping takes, for logging the norm under any optimizer.  Returns a 0-dim device tensor, no synchronisation."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        raise ValueError("grad_norm: no parameter has a gradient")
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.device != dev or g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or \
                g.numel() == 0:
            raise ValueError("grad_norm: gradients must be non-empty contiguous fp32 CUDA tensors on one device")
    if dev.index != torch.cuda.current_device():
        raise ValueError("grad_norm: the gradients are not on the current device")
    lib = L.load()
    key = (dev.index, tuple(g.numel() for g in grads))
    tabs = _norm_tables.get(key)
    if tabs is None:
        tabs = []
        for at in range(0, len(grads), FusedAdam.MAX_TENSORS):    # (one kernel-argument block per launch)
            # only the lengths are read: lic_adam_plan wants the pointers non-null
            jobs = [(g.data_ptr(),) * 3 + (g.numel(),) for g in grads[at:at + FusedAdam.MAX_TENSORS]]
            dev_tab, blocks = _upload_jobs(jobs, dev)
            tabs.append(JobTable(key, dev_tab, len(jobs), blocks, None))
        if len(_norm_tables) >= 8:
            _norm_tables.clear()
        _norm_tables[key] = tabs
    partials = torch.empty(sum(t.blocks for t in tabs), dtype=torch.float64, device=dev)
    state = torch.zeros(4, dtype=torch.float32, device=dev)
    launches, at = [], 0
    for tab in tabs:
        launches.append(tab._replace(gptrs=(C.c_void_p * tab.njobs)(*[g.data_ptr() for g in grads[at:at + tab.njobs]])))
        at += tab.njobs
    _launch_norm(lib, launches, partials, float("inf"), 0, state)
    return state[0]
