"""Training-loop counterpart of the reference's Trainer (Trainer.py:10-165) with data
parallelism added (the reference is single-device).

Reproduced contract: constructor signature (Trainer.py:11-13), step order zero_grad -> forward ->
rd_loss -> backward -> optimizer.step (:81-86), `_next_batch` wrap-around (:133-138), scheduler
modes 'plateau' / 'cosine' (:32-40, :94-99), interval defaults max_steps/200, /25, /200 (:27-29),
checkpoint dict keys model/optimizer/step/scheduler and `max_steps += step` on resume (:52-71),
scalar tags `losses/<key>` for every float of the loss dict (:140-143) and the three validation
tags (:162-164, including the reference's "validation_pnsr" spelling).
The reference's histogram logging (:167-217) ships whole latent tensors to the host every
`log_interval`; here `_log_histograms` / `_log_channel_activity` / `_log_entropy_params` emit the
same tags from device-side summaries (`data.tensor_stats` -> `lic_tensor_stats`: count, mean, std,
min, max and a 64-bin histogram; 6 doubles + 64 counters cross PCIe per tag).  Image / figure logging
(:219-345) is not reproduced.  Scalars go to a TensorBoard SummaryWriter when tensorboard is
installed, otherwise to <log_dir>/scalars.jsonl (summaries as JSON objects).
Added to the reference's contract as trailing keyword arguments: `clip_max_norm` (global-norm gradient clipping, the
`torch.nn.utils.clip_grad_norm_(model.parameters(), clip_max_norm)` of the usual recipe for these models) and
`skip_nonfinite` (a step whose gradient norm is not finite is left out); `train/grad_norm` and
`train/skipped_steps` are logged every `log_interval`; `ema_eval` (with a FusedAdam(ema_decay=...)): validation runs on
the moving average of the weights, swapped in for its duration.  Whenever the optimizer averages, the checkpoint
holds the averaged model under one more key, `ema_state_dict`, which loaders of the reference's format ignore; the
averages themselves travel in the optimizer's state dict.
`rate_points=[(q, lambda), ...]` trains a rate-level model (models: rate_levels): every step draws one pair
from a host generator seeded with `rate_seed`, runs the model at quality q and the loss at that lambda; the generator's
state travels in the checkpoint (key `rate_rng`), and validation runs once per pair, logged under `val/q<i>/...`.
`rate_per_image=True` draws one pair per IMAGE from the same generator (`draw_rate_points`), so a batch holds rate points
side by side; qualities and lambdas go to the device as [B] tensors, the model runs with `device_quality=True` and the
loss with its per-image lambda, and `step_plan=True` is allowed: the recorded step reads both from device memory.
"""
from __future__ import annotations

import json
import os
import random
from typing import Optional

import torch
import torch.distributed as dist
from torch.optim.lr_scheduler import CosineAnnealingLR, ReduceLROnPlateau

from .optim import FusedAdam, clip_gradients
from .parallel import GradientAllReducer, all_reduce_mean_scalars, broadcast_parameters


class _JsonlWriter:
    def __init__(self, log_dir, purge_step=0):
        os.makedirs(log_dir, exist_ok=True)
        self.f = open(os.path.join(log_dir, "scalars.jsonl"), "a")

    def add_scalar(self, tag, value, step):
        self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")

    def add_summary(self, tag, summary, step):
        self.f.write(json.dumps({"tag": tag, "summary": summary, "step": int(step)}) + "\n")

    def close(self):
        self.f.close()


def _make_writer(log_dir, purge_step):
    try:
        from torch.utils.tensorboard import SummaryWriter  # noqa: WPS433
        return SummaryWriter(log_dir, purge_step=purge_step)
    except Exception:
        return _JsonlWriter(log_dir, purge_step)


def _interval(explicit, max_steps, fraction):
    """the reference's default cadence: max_steps / fraction steps (Trainer.py:27-29)"""
    return explicit if explicit else int(max_steps / fraction)


def _build_scheduler(kind, optimizer, max_steps):
    """'plateau' -> ReduceLROnPlateau(min, patience 100, factor 0.5); 'cosine' -> CosineAnnealingLR(T_max =
    max_steps, eta_min 1e-5); anything else -> none (Trainer.py:32-40).  Returns (scheduler, steps_on_val_loss)."""
    if kind == "plateau":
        return ReduceLROnPlateau(optimizer, mode="min", patience=100, factor=0.5), True
    if kind == "cosine":
        return CosineAnnealingLR(optimizer, T_max=max_steps, eta_min=1e-5), False
    return None, False


def draw_rate_points(rng: random.Random, rate_points, batch: int):
    """the (quality, lambda) pairs of one batch under `rate_per_image`: one `rng.choice` per image, in image order"""
    return [rng.choice(rate_points) for _ in range(batch)]


class Trainer:
    def __init__(self, model, optimizer, train_loader, val_loader=None, rd_loss=None, lambda_val=0.005,
                 scheduler=None, max_steps=10000, resume=False, log_interval=None, img_interval=None,
                 val_interval=None, log_dir="runs/experiment", checkpoint_path="./checkpoints/checkpoint.pth",
                 device="cuda", distributed: Optional[bool] = None, writer=None, step_plan: bool = False,
                 clip_max_norm: Optional[float] = None, skip_nonfinite: bool = False, ema_eval: bool = False,
                 rate_points=None, rate_seed: int = 0, rate_per_image: bool = False):
        if rd_loss is None:
            raise ValueError("You must provide a rate-distortion loss function (`rd_loss`)")
        self.rate_points = None if rate_points is None else [(float(q), float(lam)) for q, lam in rate_points]
        self.rate_per_image = bool(rate_per_image)
        if self.rate_per_image and self.rate_points is None:
            raise ValueError("rate_per_image=True needs rate_points")
        if self.rate_points is not None:
            if not self.rate_points:
                raise ValueError("rate_points must hold at least one (quality, lambda) pair")
            if step_plan and not self.rate_per_image:
                raise ValueError("rate_points with step_plan=True: the recorded step bakes one lambda and one quality in; "
                                 "a rate-level model trains with the eager step, or with rate_per_image=True")
            if getattr(model, "rate_levels", None) is None:
                raise ValueError("rate_points need a model with rate_levels")
            for q, _ in self.rate_points:
                model.check_quality(q)
        # (the same seed on every rank of a data-parallel run: all ranks draw the same pair)
        self._rate_rng = random.Random(rate_seed)
        self.last_rate_point = None
        self.device = device
        self.model = model.to(device)
        self.optimizer, self.rd_loss, self.lambda_val = optimizer, rd_loss, lambda_val
        self.train_loader, self.val_loader = train_loader, val_loader
        self.train_iter = iter(train_loader)
        self.step, self.max_steps = 0, max_steps
        self.log_interval = _interval(log_interval, max_steps, 200)
        self.img_interval = _interval(img_interval, max_steps, 25)
        self.val_interval = _interval(val_interval, max_steps, 200)
        self.log_statistics = True  # latent / likelihood summaries every log_interval (Trainer.py:88-92)
        self.scheduler, self.use_plateau = _build_scheduler(scheduler, optimizer, max_steps)
        self.resume, self.checkpoint_path = resume, checkpoint_path
        self.ema_eval = bool(ema_eval)
        if resume and checkpoint_path is not None and os.path.exists(checkpoint_path):
            self.load_checkpoint()
        # data parallel: one process per GPU; gradients all-reduced (mean) once per step
        self.distributed = dist.is_initialized() if distributed is None else distributed
        self.rank = dist.get_rank() if self.distributed else 0
        self.reducer = None
        if self.distributed and dist.get_world_size() > 1:
            if step_plan:   # (refused before the reducer registers its bucket slots: they would outlive this object)
                raise ValueError("step_plan replays one GPU's step; data-parallel training uses the eager step")
            broadcast_parameters(self.model)
            if hasattr(self.model, "overlap_branches") and dist.get_backend() != "nccl":
                self.model.overlap_branches = False  # ranks time-sharing one GPU (gloo rehearsals) stall with it
            two = hasattr(self.model, "decoder") and getattr(self.model, "overlap_branches", False) and \
                next(self.model.parameters()).is_cuda
            self.reducer = GradientAllReducer(
                self.model.parameters(),
                stream_groups=[list(self.model.decoder.parameters())] if hasattr(self.model, "decoder") else None,
                group_streams=[self.model.side_stream()] if two else None)
        self.writer = writer if writer is not None else (_make_writer(log_dir, self.step) if self.rank == 0 else None)
        # step_plan=True: forward + loss + backward are captured on the first batch and replayed by the library's
        # launch plan (plan.StepPlan: same kernels and streams, no Python between launches -- the host-paced bf16
        # configurations gain ~10 %).  One GPU, `rd_loss` must accept sync=False (loss.rd_loss does); a batch of
        # another shape (the last one of an epoch) takes the eager step.
        self.step_plan = bool(step_plan)
        self._plan = None
        # gradient clipping / non-finite guard: a FusedAdam does both inside its own launches (optim.py: no read-back,
        # no extra pass over the gradients); any other optimizer gets torch's clip_grad_norm_ in front of its step.
        # Either way after the reducer, so every rank clips the same averaged gradient; the optimizer step is outside
        # the step plan, so step_plan=True needs nothing of its own.
        self.clip_max_norm, self.skip_nonfinite = clip_max_norm, bool(skip_nonfinite)
        self._clip = clip_max_norm is not None or self.skip_nonfinite
        self._fused_clip = self._clip and isinstance(optimizer, FusedAdam)
        if self._fused_clip:
            optimizer.max_grad_norm, optimizer.skip_nonfinite = clip_max_norm, self.skip_nonfinite
        self._grad_norm, self._skipped = None, 0   # (of the torch path)

    # -- checkpointing: the reference's file format (Trainer.py:52-71) ---------------------------
    def _checkpoint_state(self):
        sched = None if self.scheduler is None else self.scheduler.state_dict()
        state = {"model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(), "step": self.step,
                 "scheduler": sched}
        if self._averages():
            state["ema_state_dict"] = self.optimizer.ema_state_dict(self.model)
        if self.rate_points is not None:
            version, words, gauss = self._rate_rng.getstate()
            state["rate_rng"] = {"version": version, "words": list(words), "gauss": gauss}
        return state

    def _averages(self):
        """does the optimizer keep a moving average of the weights (optim.FusedAdam(ema_decay=...))"""
        return getattr(self.optimizer, "ema_decay", None) is not None and hasattr(self.optimizer, "ema_weights")

    def save_checkpoint(self):
        if self.rank != 0:   # replicas are identical: one writer
            return
        folder = os.path.dirname(self.checkpoint_path)
        if folder:
            os.makedirs(folder, exist_ok=True)
        torch.save(self._checkpoint_state(), self.checkpoint_path)
        print(f"[trainer] step {self.step}: checkpoint written to {self.checkpoint_path}")

    def load_checkpoint(self):
        state = torch.load(self.checkpoint_path, map_location=self.device)
        self.model.load_state_dict(state["model"])
        self.optimizer.load_state_dict(state["optimizer"])
        if self.scheduler is not None and state["scheduler"] is not None:
            self.scheduler.load_state_dict(state["scheduler"])
        if self.rate_points is not None and state.get("rate_rng") is not None:
            rng = state["rate_rng"]
            self._rate_rng.setstate((rng["version"], tuple(rng["words"]), rng["gauss"]))
        self.step = state["step"]
        self.max_steps += self.step   # `max_steps` counts the steps of THIS run (Trainer.py:70)
        print(f"[trainer] resumed from {self.checkpoint_path} at step {self.step}")

    # -- the step (Trainer.py:78-86) -------------------------------------------------------------
    def _optimizer_step(self):
        if self._clip and not self._fused_clip:
            self._grad_norm, skip = clip_gradients([p for g in self.optimizer.param_groups for p in g["params"]],
                                                   self.clip_max_norm, self.skip_nonfinite)
            if skip:
                self._skipped += 1
                return
        self.optimizer.step()

    def _log_clipping(self):
        """train/grad_norm (and train/skipped_steps) of the step just taken: the only steps that read them back"""
        if not self._clip or self.writer is None or not self.log_interval or self.step % self.log_interval != 0:
            return
        norm = self.optimizer.grad_norm() if self._fused_clip else self._grad_norm
        self.writer.add_scalar("train/grad_norm", float(norm), self.step)
        if self.skip_nonfinite:
            skipped = self.optimizer.skipped_steps() if self._fused_clip else self._skipped
            self.writer.add_scalar("train/skipped_steps", skipped, self.step)

    def _planned_step(self, imgs, pairs=None):
        from .loss import _KEYS
        from .plan import StepPlan
        rate = {} if pairs is None else {"quality": [q for q, _ in pairs], "lam": [lam for _, lam in pairs]}
        if self._plan is None:
            if pairs is None:
                self._plan = StepPlan(self.model, self.rd_loss, self.lambda_val, imgs)
            else:
                up = lambda v: torch.tensor(v, dtype=torch.float32, device=imgs.device)
                self._plan = StepPlan(self.model, self.rd_loss, up(rate["lam"]), imgs, quality=up(rate["quality"]))
        if imgs.shape != self._plan.x.shape:
            return None
        model_out, res = self._plan.step(imgs, **rate)
        self._optimizer_step()
        results = dict(res)
        buf = results.pop('_buffer', None)
        if buf is not None:   # the plain numbers the eager rd_loss returns, from one device-to-host copy
            host = buf[:len(_KEYS)].tolist()
            for i, k in enumerate(_KEYS[1:], start=1):
                results[k] = host[i]
        return model_out, results

    def train_step(self, imgs):
        imgs = imgs.to(self.device)
        pairs = None
        if self.rate_per_image:
            pairs = self.last_rate_point = draw_rate_points(self._rate_rng, self.rate_points, imgs.shape[0])
        if self.step_plan and imgs.is_cuda:
            done = self._planned_step(imgs, pairs)
            if done is not None:
                return done
        self.optimizer.zero_grad()
        if pairs is not None:
            q = torch.tensor([q for q, _ in pairs], dtype=torch.float32, device=imgs.device)
            lam = torch.tensor([lam for _, lam in pairs], dtype=torch.float32, device=imgs.device)
            model_out = self.model(imgs, quality=q, device_quality=True)
            results = self.rd_loss(model_out, imgs, lam)
        elif self.rate_points is not None:
            q, lam = self.last_rate_point = self._rate_rng.choice(self.rate_points)
            model_out = self.model(imgs, quality=q)
            results = self.rd_loss(model_out, imgs, lam)
        else:
            model_out = self.model(imgs)
            results = self.rd_loss(model_out, imgs, self.lambda_val)
        results['loss'].backward()
        if self.reducer is not None:
            self.reducer.finish()
        self._optimizer_step()
        return model_out, results

    def train(self):
        while self.step < self.max_steps:
            imgs = self._next_batch()
            model_out, results = self.train_step(imgs)
            self._log_scalars(results)
            self._log_clipping()
            if self.writer is not None and self.log_interval and self.step % self.log_interval == 0 and \
                    self.log_statistics and self._has_device_outputs(model_out):
                self._log_histograms(model_out)
                self._log_channel_activity(model_out, 'y')
                self._log_channel_activity(model_out, 'z')
                self._log_entropy_params(model_out)
            if self.val_loader is not None and self.val_interval and self.step % self.val_interval == 0:
                val_loss = self._validate()
                if self.use_plateau:
                    self.scheduler.step(val_loss)
            if self.scheduler is not None and not self.use_plateau:
                self.scheduler.step()
            if self.scheduler is not None and self.writer is not None:
                self.writer.add_scalar("train/learning_rate", self.optimizer.param_groups[0]['lr'], self.step)
            self.step += 1
        if self.writer is not None:
            self.writer.close()
        if self.checkpoint_path is not None:
            self.save_checkpoint()

    def _next_batch(self):
        """next training batch; the loader is restarted when it runs out (Trainer.py:133-138)"""
        batch = next(self.train_iter, None)
        if batch is None:
            self.train_iter = iter(self.train_loader)
            batch = next(self.train_iter)
        return batch

    def _log_scalars(self, results):
        """every plain number of the loss dict under losses/<key> (Trainer.py:140-143)"""
        if self.writer is None:
            return
        for key, value in results.items():
            if isinstance(value, (float, int)):
                self.writer.add_scalar("losses/" + key, value, self.step)

    # ---- Trainer.py:167-217 from device-side summaries --------------------------------------
    @staticmethod
    def _has_device_outputs(model_out):
        keys = ("y", "y_in", "z", "z_in", "logp_y", "logp_z", "p_y", "p_z")
        return all(k in model_out and torch.is_tensor(model_out[k]) and model_out[k].is_cuda for k in keys)

    def _summary(self, tag, t):
        from .data import tensor_stats
        st = tensor_stats(t)
        if hasattr(self.writer, "add_summary"):
            self.writer.add_summary(tag, st, self.step)
        else:  # a TensorBoard writer: the scalar moments
            for k in ("mean", "std", "min", "max"):
                self.writer.add_scalar(f"{tag}/{k}", st[k], self.step)
        return st

    def _log_histograms(self, model_out):
        ln2 = 0.6931471805599453
        for tag, key in (("latents/y", "y"), ("latents/y_hat", "y_in"), ("latents/z", "z"), ("latents/z_hat", "z_in"),
                         ("probability/logp_y", "logp_y"), ("probability/logp_z", "logp_z"),
                         ("probability/p_y", "p_y"), ("probability/p_z", "p_z")):
            st = self._summary(tag, model_out[key])
            if key in ("logp_y", "logp_z", "p_y", "p_z"):
                self.writer.add_scalar(f"probability/{key}_mean", st["mean"], self.step)
            if key in ("logp_y", "logp_z"):
                self.writer.add_scalar(f"entropy/entropy_{key[-1]}_mean", -st["mean"] / ln2, self.step)
        for n in ("y", "z"):
            logp = model_out["logp_" + n].detach()
            self._summary(f"entropy/{n}", -logp / ln2)
            self._summary(f"entropy/{n}_per_component", -logp.sum(dim=(2, 3)) / ln2)

    def _log_channel_activity(self, model_out, tensor_name='y'):
        logp = model_out['logp_' + tensor_name].detach()
        avg_bits_per_c = (-logp / 0.6931471805599453).mean(dim=(0, 2, 3))
        self.writer.add_scalar(f"activity/{tensor_name}_dead_channels_by_entropy",
                               float((avg_bits_per_c < 1e-4).float().sum()), self.step)

    def _log_entropy_params(self, model_out):
        if 'mu' in model_out and 'sigma' in model_out:
            self._summary("entropy_params/mu", model_out['mu'])
            self._summary("entropy_params/sigma", model_out['sigma'])
        if 'weights' in model_out:
            for k in ("weights", "mus", "sigmas"):
                self._summary(f"entropy_params/{k}", model_out[k])
            used = (model_out['weights'].detach() > 1e-4).float().sum(dim=1).mean()
            self.writer.add_scalar("entropy_params/used_components_mean", float(used), self.step)

    def validate(self):
        """one validation pass (as `train()` runs every `val_interval`): on the averaged weights when `ema_eval` is set
        and the optimizer averages, with the trained weights back in place behind it"""
        return self._validate()

    def _validate(self):
        """mean loss / bpp / PSNR over the validation loader in eval mode (Trainer.py:145-165); under data
        parallelism the three means are averaged over the ranks"""
        if self.ema_eval and self._averages() and not self.optimizer.swapped:
            with self.optimizer.ema_weights():
                return self._validate()
        if self.rate_points is not None:
            # once per pair, each under its own tags; the scheduler sees the mean of the pairs' losses
            losses = [self._validate_at(f"val/q{i}/", {"quality": q}, lam) for i, (q, lam) in enumerate(self.rate_points)]
            return sum(losses) / len(losses)
        return self._validate_at("validation/", {}, self.lambda_val)

    def _validate_at(self, prefix, model_kw, lam):
        sums = [0.0, 0.0, 0.0]
        self.model.eval()
        with torch.no_grad():
            for imgs in self.val_loader:
                imgs = imgs.to(self.device)
                res = self.rd_loss(self.model(imgs, training=False, **model_kw), imgs, lam)
                for i, v in enumerate((res["loss"], res["bpp_total"], res["psnr"])):
                    sums[i] += float(v)
        self.model.train()
        means = [v / len(self.val_loader) for v in sums]
        if self.distributed:
            # every rank validates its own shard of the images: average the three numbers over the ranks, so that
            # ReduceLROnPlateau sees the SAME value everywhere and the replicated parameters cannot drift apart
            means = all_reduce_mean_scalars(means, self.device)
        if self.writer is not None:
            # (tag spelling as in the reference, Trainer.py:162-164)
            for tag, v in zip(("validation_loss", "validation_bpp", "validation_pnsr"), means):
                self.writer.add_scalar(prefix + tag, v, self.step)
        return means[0]
