"""Evaluation-loop counterpart of the reference's CompressionEvaluator (Evaluator.py:17-92,
235-242): per-batch bpp_total / bpp_y / bpp_z from rd_loss, MSE(255), PSNR(RGB) on
x_hat.clamp(0,1), luma PSNR with BT.601 weights, and the result-file format.

Differences, stated: MS-SSIM (third-party `pytorch_msssim` in the reference, absent offline) is
computed on the device by `functional.ms_ssim` / `lic_msssim`, which follows that package's
published 0.2.1 algorithm (parity unpinned).  The reference's aggregation reports
`BPP` = mean(bpp_y) (Evaluator.py:81 uses bpp_y_values); this class reproduces that under 'BPP'
for drop-in compatibility and adds the intended value as 'BPP(total)'.
`load_checkpoint_weights(model, path)` puts the averaged weights of a checkpoint into the model to be
evaluated when the checkpoint has them, the trained ones otherwise.
"""
from __future__ import annotations

import math
import os

import torch


_LUMA = (0.299, 0.587, 0.114)   # BT.601 weights the reference uses for its luma metrics (Evaluator.py:27-30)


def _psnr_unit_range(mse: float) -> float:
    return float("inf") if mse <= 0 else -10.0 * math.log10(mse)


def load_checkpoint_weights(model, checkpoint, ema: bool = True, map_location=None):
    """Load the weights a checkpoint of `trainer.Trainer` (or of the reference's Trainer) holds into `model`: the moving
    average of the weights (`ema_state_dict`, written when the optimizer keeps one) when `ema` is set and the checkpoint
    has it, else the trained weights (`model`).  `checkpoint`: a path or the loaded dict.  Returns the key it used."""
    if not isinstance(checkpoint, dict):
        checkpoint = torch.load(checkpoint, map_location=map_location)
    key = "ema_state_dict" if ema and checkpoint.get("ema_state_dict") is not None else "model"
    model.load_state_dict(checkpoint[key])
    return key


class _RunningMeans:
    """arithmetic means of named per-batch values, in first-seen key order"""

    def __init__(self):
        self._sum, self._n = {}, {}

    def add(self, **values):
        for name, v in values.items():
            self._sum[name] = self._sum.get(name, 0.0) + float(v)
            self._n[name] = self._n.get(name, 0) + 1

    def means(self):
        return {name: self._sum[name] / self._n[name] for name in self._sum}


class _Evaluator:
    """what the two evaluators share: the distortion metrics of a batch and the result file"""

    def __init__(self, model, dataloader, device, lambda_val, save_dir):
        self.model, self.dataloader, self.device, self.lambda_val = model, dataloader, device, lambda_val
        self.save_dir = save_dir
        os.makedirs(self.save_dir, exist_ok=True)
        from .functional import ms_ssim
        self._ms_ssim = ms_ssim

    @staticmethod
    def rgb_to_luma(x):
        """[B,3,H,W] in [0,1] -> [B,H,W] luma"""
        wr, wg, wb = _LUMA
        return wr * x[:, 0] + wg * x[:, 1] + wb * x[:, 2]

    def compute_metrics(self, orig, recon):
        """The five distortion numbers of one batch (Evaluator.py:32-53).  Both mean-squared errors come
        back in ONE device-to-host copy (the reference calls .item() four times)."""
        y_o, y_r = self.rgb_to_luma(orig).unsqueeze(1), self.rgb_to_luma(recon).unsqueeze(1)
        mse_rgb, mse_y = torch.stack([((orig - recon) ** 2).mean(), ((y_o - y_r) ** 2).mean()]).tolist()
        return {
            "MSE(255)": mse_rgb * 255.0 ** 2,
            "PSNR(RGB)": _psnr_unit_range(mse_rgb),
            "MS-SSIM(RGB)": float(self._ms_ssim(recon, orig, data_range=1.0, size_average=True)),
            "PSNR(Y)": _psnr_unit_range(mse_y),
            "MS-SSIM(Y)": float(self._ms_ssim(y_r, y_o, data_range=1.0, size_average=True)),
        }

    def save_results(self, metrics, nb_steps, caption=""):
        """the reference's result-file name and line format (Evaluator.py:235-242, 486-493)"""
        lines = [f"Lambda: {self.lambda_val}", f"Trained for: {nb_steps} steps"]
        lines += [f"{name}: {value:.6f}" for name, value in metrics.items()]
        path = os.path.join(self.save_dir, f"eval_results_{self.lambda_val}_lambda_{caption}.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"Results saved to {path}")
        return path


class CompressionEvaluator(_Evaluator):
    """Constructor and method signatures are the reference's (Evaluator.py:18, 32, 55, 235)."""

    def __init__(self, model, dataloader, device, lambda_val, save_dir="./eval_results"):
        super().__init__(model, dataloader, device, lambda_val, save_dir)

    def evaluate(self, rd_loss_fn, coded: bool = False, pad_mode=None):
        """`coded=True` (not in the reference, which has no entropy coder) also writes every batch through
        `codec.ContextCodec` and reports the size of the actual bitstream as 'BPP(coded)' next to the
        estimated -log2 p rates.
        `pad_mode` ('replicate', 'reflect' or 'zeros'; None = the path above, unchanged): every batch goes through
        `padded_forward`, so the loader may yield images of any size -- batches of one image each, of differing
        sizes, are the expected case.  Rates and distortions are per ORIGINAL pixel; 'BPP(coded)' is the size of
        the self-describing `ContextCodec.compress_image` byte string, header included."""
        if pad_mode is not None:
            return self._evaluate_padded(rd_loss_fn, coded, pad_mode)
        codec = None
        if coded:
            from .codec import ContextCodec
            codec = ContextCodec(self.model)
        distortion, rate = _RunningMeans(), _RunningMeans()
        first_inputs, first_recons = [], []
        self.model.eval()
        with torch.no_grad():
            for batch in self.dataloader:
                batch = batch.to(self.device)
                out = self.model(batch, training=False)
                rd = rd_loss_fn(out, batch, self.lambda_val)
                x_hat = out["x_hat"].clamp(0, 1)
                distortion.add(**self.compute_metrics(batch, x_hat))
                rate.add(y=rd["bpp_y"], z=rd["bpp_z"], total=rd["bpp_total"])
                if codec is not None:
                    rate.add(coded=codec.compress(batch)["bpp_coded"])
                first_inputs.append(batch[0].cpu())
                first_recons.append(x_hat[0].cpu())
        return self._report(distortion, rate), first_inputs, first_recons

    def _evaluate_padded(self, rd_loss_fn, coded, pad_mode):
        from .anysize import padded_forward
        codec = None
        if coded:
            from .codec import ContextCodec
            codec = ContextCodec(self.model)
        distortion, rate = _RunningMeans(), _RunningMeans()
        first_inputs, first_recons = [], []
        self.model.eval()
        with torch.no_grad():
            for batch in self.dataloader:
                batch = batch.to(self.device)
                out = padded_forward(self.model, batch, mode=pad_mode, training=False)
                rd = rd_loss_fn(out, batch, self.lambda_val)
                x_hat = out["x_hat"].clamp(0, 1)
                distortion.add(**self.compute_metrics(batch, x_hat))
                rate.add(y=rd["bpp_y"], z=rd["bpp_z"], total=rd["bpp_total"])
                if codec is not None:
                    npix = batch.shape[0] * batch.shape[2] * batch.shape[3]
                    rate.add(coded=8.0 * len(codec.compress_image(batch, mode=pad_mode)) / npix)
                first_inputs.append(batch[0].cpu())
                first_recons.append(x_hat[0].cpu())
        return self._report(distortion, rate), first_inputs, first_recons

    @staticmethod
    def _report(distortion, rate):
        report, r = distortion.means(), rate.means()
        # 'BPP' is what the reference's aggregation computes -- the mean of bpp_y (Evaluator.py:78,81) -- kept
        # under that name for drop-in result files; the intended total is reported beside it
        report["BPP"] = r["y"]
        report["BPP(y)"] = r["y"]
        report["BPP(z)"] = r["z"]
        report["BPP(total)"] = r["total"]
        if "coded" in r:
            report["BPP(coded)"] = r["coded"]
        print("\n--- Evaluation Results ---")
        print("\n".join(f"{name}: {value:.6f}" for name, value in report.items()))
        return report


class VisionCompressionEvaluator(_Evaluator):
    """The reference's evaluator of `ScalableImageCoding` (Evaluator.py:245-328, 486-493): constructor, `evaluate`,
    `save_results` and the report keys are its own.  Its aggregation reports 'BPP' = mean(bpp_y) (Evaluator.py:313 takes
    bpp_y_values), reproduced here under that name as `CompressionEvaluator` reproduces line 81; the intended value is
    added as 'BPP(total)'.  `coded=True` (not in the reference, which has no coder) writes every batch through
    `codec.ScalableCodec` and reports the size of the LICBITS6 container as 'BPP(coded)' and of its base prefix -- what
    a vision client downloads -- as 'BPP(coded base)'."""

    def __init__(self, model, dataloader, device, lambda_val, gamma, save_dir="./eval_results"):
        super().__init__(model, dataloader, device, lambda_val, save_dir)
        self.gamma = gamma

    def evaluate(self, vision_rd_loss, coded: bool = False):
        codec = None
        if coded:
            from .codec import ScalableCodec
            codec = ScalableCodec(self.model)
        distortion, rate = _RunningMeans(), _RunningMeans()
        first_inputs, first_recons = [], []
        self.model.eval()
        with torch.no_grad():
            for batch in self.dataloader:
                batch = batch.to(self.device)
                out = self.model(batch, training=False)
                rd = vision_rd_loss(out, batch, self.lambda_val, self.gamma)
                x_hat = out["x_hat"].clamp(0, 1)
                distortion.add(**self.compute_metrics(batch, x_hat))
                rate.add(y=rd["bpp_y"], y1=rd["bpp_y1"], y2=rd["bpp_y2"], z=rd["bpp_z"], total=rd["bpp_total"])
                if codec is not None:
                    r = codec.compress(batch)
                    rate.add(coded=r["bpp_coded"], coded_base=r["bpp_coded_base"])
                first_inputs.append(batch[0].cpu())
                first_recons.append(x_hat[0].cpu())
        report, r = distortion.means(), rate.means()
        report["BPP"] = r["y"]                      # the reference's quirk (class docstring)
        for key, name in (("y", "BPP(y)"), ("y1", "BPP(y1)"), ("y2", "BPP(y2)"), ("z", "BPP(z)"), ("total", "BPP(total)"),
                          ("coded", "BPP(coded)"), ("coded_base", "BPP(coded base)")):
            if key in r:
                report[name] = r[key]
        print("\n--- Evaluation Results ---")
        print("\n".join(f"{name}: {value:.6f}" for name, value in report.items()))
        return report, first_inputs, first_recons
