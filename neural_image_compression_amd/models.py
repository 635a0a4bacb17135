"""Model classes with the reference's names and forward contract (reference: Models.py:10-338).
`ScalableImageCoding` (Models.py:208-338) cannot execute upstream; it is provided with the
three one-line repairs that let it run, listed in its docstring."""
from __future__ import annotations


import numpy as np
import torch
import torch.nn as nn

from . import functional as F_
from .components import (Decoder3x3, Decoder5x5, Encoder3x3, Encoder5x5, HyperDecoder3x3, HyperDecoder5x5,
                         HyperEncoder3x3, HyperEncoder5x5, LatentSpaceTransform)
from .entropy import (ContextModel, EntropyParameters, FactorizedEntropyBottleneck, GaussianConditional,
                      GaussianMixtureConditional)


class _HyperpriorContextModel(nn.Module):
    _stacks = None  # (Encoder, Decoder, HyperEncoder, HyperDecoder)
    context = "raster"

    def __init__(self, latent_channels: int = 192, K: int = 1, context: str = "raster", rate_levels: int = None):
        """`rate_levels` = Q >= 2: a variable-rate model (gain units) with Q trained quality levels;
        `forward(x, quality=q)` then takes any real q in [0, Q-1].  None: no gain units, no parameters of theirs.
        `context`: "raster" (the reference's type-A masked convolution over y_in) or "checkerboard" (He et al. 2021,
        DESIGN 8(f).2: phi = masked_conv(anchor(y_in)) with the checkerboard mask; anchors -- latent pixels with i + j
        even -- get phi = bias and are coded from the hyperprior alone, the others from the anchors around them, so a
        codec decodes in two steps).  Same modules and state-dict keys either way."""
        super().__init__()
        if not isinstance(latent_channels, int) or latent_channels < 1:
            raise ValueError(f"latent_channels must be int >= 1, got {latent_channels}")
        if not isinstance(K, int) or K < 1:
            raise ValueError(f"K must be int >= 1, got {K}")
        if context not in ("raster", "checkerboard"):
            raise ValueError(f"context must be 'raster' or 'checkerboard', got {context!r}")
        self.context = context
        self.M = latent_channels
        self.K = K
        self.H = latent_channels
        self.distribution = 'Mean-Scale Gaussian' if K == 1 else 'Mixture of Gaussians'
        self.conditional = GaussianConditional() if K == 1 else GaussianMixtureConditional()
        Enc, Dec, HEnc, HDec = self._stacks
        self.encoder = Enc(latent_channels=self.M)
        self.decoder = Dec(latent_channels=self.M)
        self.hyper_encoder = HEnc(latent_channels=self.M)
        self.hyper_decoder = HDec(latent_channels=self.M)
        self.factorized_entropy_model = FactorizedEntropyBottleneck(self.M)
        self.context_model = ContextModel(latent_channels=self.M,
                                          mask_type="checkerboard" if context == "checkerboard" else "A")
        self.entropy_parameters = EntropyParameters(latent_channels=self.M, hyper_latent_channels=self.H,
                                                    K=self.K)
        if rate_levels is not None and (not isinstance(rate_levels, int) or isinstance(rate_levels, bool)
                                        or rate_levels < 2):
            raise ValueError(f"rate_levels must be None or an int >= 2, got {rate_levels!r}")
        self.rate_levels = rate_levels
        if rate_levels is not None:
            # log of the gain in front of each quantiser and of the inverse gain behind it, one row per level
            for name in self.GAIN_TABLES:
                setattr(self, name, nn.Parameter(torch.zeros(rate_levels, self.M)))

    def check_quality(self, quality, batch: int = None, device_quality: bool = False):
        """`quality` as the model takes it: None for a plain model; a float (the whole batch) or a [B] tensor, every
        value in [0, Q-1], for a rate-level model.  -> None, or a host list of 1 or B floats.  ValueError otherwise.
        `device_quality`: the qualities stay on the device -- a CUDA float32 [B] tensor, of which only shape and dtype are
        checked here; the values are never read back and the kernel clamps them to [0, Q-1].  -> the
        tensor."""
        if self.rate_levels is None:
            if quality is not None or device_quality:
                raise ValueError("this model has no rate levels (rate_levels=None): it takes no `quality`")
            return None
        if quality is None:
            raise ValueError(f"a model with rate_levels={self.rate_levels} needs `quality` in [0, {self.rate_levels - 1}]")
        if device_quality:
            if not (torch.is_tensor(quality) and quality.is_cuda and quality.dtype == torch.float32 and quality.dim() == 1
                    and quality.is_contiguous() and (batch is None or quality.shape[0] == batch)):
                raise ValueError("device_quality=True takes `quality` as a contiguous CUDA float32 tensor [B]")
            return quality.detach()
        if torch.is_tensor(quality):
            if quality.dim() != 1 or (batch is not None and quality.shape[0] != batch):
                raise ValueError(f"`quality` must be a float or a tensor [B], got shape {tuple(quality.shape)}")
            qs = [float(v) for v in quality.tolist()]
        else:
            qs = [float(quality)]
        for q in qs:
            if not 0.0 <= q <= self.rate_levels - 1:   # (a NaN fails both comparisons)
                raise ValueError(f"quality {q} outside [0, {self.rate_levels - 1}]")
        return qs

    GAIN_TABLES = ("log_gain_y", "log_inv_gain_y", "log_gain_z", "log_inv_gain_z")

    def gain_rows(self, qs, *tables):
        """the rows [len(qs)][M] of each of `tables` ([Q][M] log gains) at the qualities `qs` (check_quality's list):
        geometric interpolation between the neighbouring levels, exp((1 - l) * log_g[i] + l * log_g[i + 1]) with
        i = floor(q) clamped to Q-2 and l = q - i, both weights float32.  Plain torch ops, the same handful for any number
        of tables (they are stacked), and for one quality nothing but slices: autograd carries the rows' gradients back
        to the tables.  One quality and a constant list give the same bits.
        `qs` as a device tensor (check_quality with `device_quality`): one launch, functional.gain_rows_device."""
        if torch.is_tensor(qs):
            return F_.gain_rows_device(qs, *tables)
        T = tables[0].unsqueeze(0) if len(tables) == 1 else torch.stack(tables)           # [k][Q][M]
        idx = [min(int(q), self.rate_levels - 2) for q in qs]
        lf = [np.float32(q - i) for q, i in zip(qs, idx)]
        if len(qs) == 1:
            i, l = idx[0], lf[0]
            rows = torch.exp(float(np.float32(1) - l) * T[:, i:i + 1] + float(l) * T[:, i + 1:i + 2])
        else:
            it = torch.tensor(idx, device=T.device, dtype=torch.long)
            lt = torch.tensor(lf, device=T.device, dtype=T.dtype).unsqueeze(1)
            rows = torch.exp((1.0 - lt) * T[:, it] + lt * T[:, it + 1])
        return rows.unbind(0)

    def _gains(self, qs):
        """all four rows of one forward, by table name, from one pass of `gain_rows`"""
        return dict(zip(self.GAIN_TABLES, self.gain_rows(qs, *(getattr(self, n) for n in self.GAIN_TABLES))))

    def hyper_synthesis(self, z_in: torch.Tensor, quality=None, _gains=None, device_quality=False, **kw):
        """psi = hyper_decoder(z_in * inverse gain of z at `quality`); the bare module call for a plain model"""
        qs = self.check_quality(quality, z_in.shape[0], device_quality)
        if qs is None:
            return self.hyper_decoder(z_in, **kw)
        inv = _gains["log_inv_gain_z"] if _gains is not None else self.gain_rows(qs, self.log_inv_gain_z)[0]
        lat16 = z_in.is_cuda and self.hyper_decoder.precision == "bf16"
        return self.hyper_decoder(F_.channel_scale(z_in, inv, cast_out=lat16), **kw)

    def synthesis(self, y_in: torch.Tensor, quality=None, _gains=None, device_quality=False):
        """x_hat = decoder(y_in * inverse gain of y at `quality`); the bare module call for a plain model"""
        qs = self.check_quality(quality, y_in.shape[0], device_quality)
        if qs is None:
            return self.decoder(y_in)
        inv = _gains["log_inv_gain_y"] if _gains is not None else self.gain_rows(qs, self.log_inv_gain_y)[0]
        dec16 = y_in.is_cuda and self.decoder.precision == "bf16"
        return self.decoder(F_.channel_scale(y_in, inv, cast_out=dec16))

    def set_precision(self, precision: str = "fp32", latent: str = None):
        """"fp32" (default, the reference's arithmetic) or "bf16": bf16 activation storage and bf16 MFMA with
        fp32 accumulation (BASELINE config 3; not in the reference) in the analysis / synthesis
        stacks and -- `latent`, default = `precision` -- in the hyper encoder / decoder, the context model and
        the entropy-parameter MLP.  The latents y, z, the raw entropy parameters, quantisation, every
        likelihood and the loss stay fp32; parameters and their gradients are always fp32."""
        latent = precision if latent is None else latent
        for v in (precision, latent):
            if v not in ("fp32", "bf16"):
                raise ValueError(f"precision must be 'fp32' or 'bf16', got {v!r}")
        self.encoder.precision = self.decoder.precision = precision
        for m in (self.hyper_encoder, self.hyper_decoder, self.context_model, self.entropy_parameters):
            m.precision = latent
        self.hyper_decoder.out_f32 = latent != "bf16"   # psi feeds the bf16 MLP directly
        return self

    def analysis_hyperprior(self, x: torch.Tensor, training: bool = True, noise=None, with_packed_params=False,
                            _fork=None, quality=None, _gains=None, device_quality=False):
        """Everything of `forward` except the synthesis transform (Models.py:49-97): the scope the
        north star quotes its roofline target on.  Returns the out-dict without 'x_hat'
        (`with_packed_params`: plus '_act', the activated entropy parameters as the one packed tensor
        the likelihood / coder-table kernels read).  `_fork(y_in)` is called as soon as y_in exists.
        A rate-level model (`quality`): y and z are scaled by their gains in the quantisation launches --
        'y' and 'z' of the out-dict are the gained latents, which is what the hyper-encoder reads -- and z_in by its
        inverse gain in front of the hyper-decoder; the context model, the entropy parameters and both likelihoods see
        y_in / z_in as ever.  `device_quality`: `quality` is a CUDA float32 [B] tensor that stays on the device."""
        qs = self.check_quality(quality, x.shape[0], device_quality)
        if qs is not None and _gains is None:
            _gains = self._gains(qs)        # (`forward` hands in the rows it made: one pass of torch ops per step)
        if x.shape[2] % 64 or x.shape[3] % 64:
            raise RuntimeError("H and W must be multiples of 64 (phi/psi shapes must agree, Models.py:73)")
        if self.use_step_prep and x.is_cuda:
            self.step_prep().run()   # one launch: every packed weight / GDN re-parametrisation of this step
        F_.AUX_STREAM = self.side_stream() if (x.is_cuda and self.overlap_branches) else None
        try:
            y = self.encoder(x)
        finally:
            F_.AUX_STREAM = None
        if x.is_cuda and self.overlap_branches:
            # backward: once dL/dy is complete the decoder's and the latent side's pending reductions start on the second
            # stream, beside the encoder's backward chain (functional.flush_point)
            y = F_.flush_point(y, self.side_stream())
        # bf16-storage consumers of y (hyper-encoder), y_in (decoder, context model) and z_in (hyper-decoder): their bf16
        # copies come out of the quantisation launches instead of one cast launch per consumer
        lat16 = x.is_cuda and self.hyper_encoder.precision == "bf16"
        dec16 = x.is_cuda and self.decoder.precision == "bf16"
        if training:
            if noise is None:
                # the reference draws rand_like(z) then rand_like(y) (Models.py:57-58); z's shape is known
                # before z is, and drawing both here lets the decoder branch start right after the encoder
                # (one generator launch for both; each tensor is laid out NHWC like the latent it perturbs, so the
                # quantisation kernel reads it in place -- an NCHW u_z cost a layout-copy launch per step)
                Bn, Mc, hy, wy = y.shape
                hz, wz = (hy + 3) // 4, (wy + 3) // 4
                nz, ny = Bn * hz * wz * Mc, Bn * hy * wy * Mc
                u = torch.rand(nz + ny, device=y.device, dtype=y.dtype)
                uz = u[:nz].view(Bn, hz, wz, Mc).permute(0, 3, 1, 2)
                uy = u[nz:].view(Bn, hy, wy, Mc).permute(0, 3, 1, 2)
            else:
                uz, uy = noise
        else:
            uz = uy = None
        if qs is not None:
            # (y_in's bf16 copy serves the context model alone: the decoder reads the inverse-gained y_in)
            if self.context == "checkerboard":
                y, y_in, y_ctx = F_.gain_quantize(y, uy, _gains["log_gain_y"], training, anchor=True, cast_in=lat16,
                                                  cast_out=lat16)
            else:
                y, y_in = F_.gain_quantize(y, uy, _gains["log_gain_y"], training, cast_in=lat16, cast_out=lat16)
                y_ctx = y_in
        elif self.context == "checkerboard":
            # the context model convolves anchor(y_in); decoder and likelihood keep y_in (one launch writes both)
            y_in, y_ctx = F_.quantize_anchor(y, uy, training, cast_in=lat16, cast_out=dec16 or lat16)
        else:
            y_in = y_ctx = F_.quantize(y, uy, training, cast_in=lat16, cast_out=dec16 or lat16)
        if _fork is not None:
            _fork(y_in)
        z = self.hyper_encoder(y)
        if qs is not None:
            z, z_in = F_.gain_quantize(z, uz, _gains["log_gain_z"], training)
        else:
            z_in = F_.quantize(z, uz, True, cast_out=lat16) if training else F_.quantize(z, None, False, cast_out=lat16)
        pz_side = None
        if _fork is not None and x.is_cuda and self.overlap_branches and F_.PLAN_RECORDING:
            # the factorised likelihood of z_in depends on nothing else of the latent side: it goes behind the decoder on the
            # second stream (forward: into the stretch where that stream idles while this one finishes the entropy
            # parameters; backward: autograd runs its backward there too, off the longer of the two backward chains).
            # Recorded steps only (plan.StepPlan): +0.6 % replayed at config 3, -1 % for the eager fp32 step of config 2
            main_s, side_s = torch.cuda.current_stream(), self.side_stream()
            side_s.wait_stream(main_s)
            with torch.cuda.stream(side_s):
                pz_side = self.factorized_entropy_model.likelihood_and_log(z_in)
            z_in.record_stream(side_s)
            for t in pz_side:
                t.record_stream(main_s)   # (forward() joins the streams before anything reads them)
        both = (self.context_model.precision, self.hyper_decoder.precision)
        if x.is_cuda and (both == ("fp32", "fp32") or (both == ("bf16", "bf16") and not self.hyper_decoder.out_f32)):
            # Models.py:73 `torch.cat([phi, psi], dim=1)` without the copy: the context conv and the hyper
            # decoder's last conv write the two channel ranges of one NHWC buffer (phi first; fp32, or bf16 when
            # both producers hand bf16 features to the bf16 entropy-parameter MLP)
            Bn, _, hh, ww = y_in.shape
            c_phi = self.context_model.masked.out_channels
            c_psi = self.hyper_decoder.net[-1].out_channels
            comb = torch.empty((Bn, hh, ww, c_phi + c_psi), device=x.device,
                               dtype=torch.float32 if both[0] == "fp32" else torch.bfloat16)
            psi = self.hyper_synthesis(z_in, quality, _gains, device_quality, out=comb[..., c_phi:])
            phi = self.context_model(y_ctx, out=comb[..., :c_phi])
            combined = F_.join_channels(phi, psi, comb)
        else:
            psi = self.hyper_synthesis(z_in, quality, _gains, device_quality)
            phi = self.context_model(y_ctx)
            combined = torch.cat([phi, psi], dim=1)  # (bf16 features: a 6 MB layout copy, phi first)
        act = self.entropy_parameters.packed(combined)
        if self.K == 1:
            mu, sigma = self.entropy_parameters.split(act)
            params = {"mu": mu, "sigma": sigma}
        else:
            weights, mus, sigmas = self.entropy_parameters.split(act)
            params = {"weights": weights, "mus": mus, "sigmas": sigmas}
        p_z, logp_z = pz_side if pz_side is not None else self.factorized_entropy_model.likelihood_and_log(z_in)
        p_y, logp_y = self.conditional.packed_likelihood_and_log(y_in, act, self.K)
        out = {'y': y, 'y_in': y_in, 'z': z, 'z_in': z_in, 'p_z': p_z, 'logp_z': logp_z,
               'p_y': p_y, 'logp_y': logp_y, 'training': training}
        out.update(params)
        if with_packed_params:
            out['_act'] = act
        if qs is not None:
            out['quality'] = quality
        return out

    # The synthesis transform depends only on y_in; the hyper / context / likelihood branch only on
    # (y, y_in): independent until rd_loss.  With `overlap_branches` the decoder runs on a second HIP
    # stream beside the latent-side branch (many small launches that cannot fill 256 CUs by
    # themselves), in forward and -- autograd replays each op on its forward stream -- in backward.
    overlap_branches = True
    # all parameter-derived buffers refreshed by one launch per optimizer step (prep.StepPrep); False: the layers
    # derive them per call
    use_step_prep = True

    def __getstate__(self):
        # the step preparation holds weak references and device job tables of THIS object: a pickled / deep-copied
        # model builds its own on first use
        st = dict(self.__dict__)
        st.pop("_step_prep", None)
        st.pop("_side_stream", None)
        return st

    def step_prep(self):
        if getattr(self, "_step_prep", None) is None:
            from .prep import StepPrep
            self._step_prep = StepPrep(self)
        return self._step_prep

    def side_stream(self):
        """the second HIP stream of `overlap_branches` (created on first use)"""
        if getattr(self, "_side_stream", None) is None:
            # High priority: the decoder chain is the critical path of the overlapped region, the latent-side
            # launches on the main stream fill what it leaves (+0.6 % step, and the big decoder launches keep
            # ~5 % more of their stand-alone speed).
            self._side_stream = torch.cuda.Stream(priority=-1)
        return self._side_stream

    def forward(self, x: torch.Tensor, training: bool = True, noise=None, quality=None, device_quality: bool = False):
        """`noise` (test hook, not in the reference): (u_z, u_y) uniform [0,1) tensors used instead
        of torch.rand_like, in the reference's draw order (z first, Models.py:57-58).  `quality`: required by a
        rate-level model, a float for the whole batch or a tensor [B], in [0, rate_levels - 1].  `device_quality`: `quality`
        is a CUDA float32 [B] tensor that is never read back -- no host sync, legal inside a recorded step; the gain rows
        come from one launch, which clamps each value to [0, rate_levels - 1]."""
        qs = self.check_quality(quality, x.shape[0], device_quality)
        gains = None if qs is None else self._gains(qs)
        if not (self.overlap_branches and x.is_cuda):
            out = self.analysis_hyperprior(x, training, noise, quality=quality, _gains=gains, device_quality=device_quality)
            return {'x_hat': self.synthesis(out['y_in'], quality, gains, device_quality), **out}
        main = torch.cuda.current_stream()
        side = self.side_stream()
        box = {}

        def fork(y_in):
            side.wait_stream(main)
            with torch.cuda.stream(side):
                box['x_hat'] = self.synthesis(y_in, quality, gains, device_quality)
            y_in.record_stream(side)

        out = self.analysis_hyperprior(x, training, noise, _fork=fork, quality=quality, _gains=gains,
                                       device_quality=device_quality)
        main.wait_stream(side)
        box['x_hat'].record_stream(main)
        return {'x_hat': box['x_hat'], **out}


class JointAutoregressiveHierarchical(_HyperpriorContextModel):
    """5x5 conv/GDN stacks (Models.py:10-106)."""
    _stacks = (Encoder5x5, Decoder5x5, HyperEncoder5x5, HyperDecoder5x5)


class HierarchicalMixtureResidual(_HyperpriorContextModel):
    """3x3 residual stacks (Models.py:109-205)."""
    _stacks = (Encoder3x3, Decoder3x3, HyperEncoder3x3, HyperDecoder3x3)


class ScalableImageCoding(nn.Module):
    """Models.py:208-338: the 5x5 model whose latent y is split into a base part y1 (`base_channels`) and an
    enhancement part y2, each with its own masked context model and entropy-parameter MLP over the shared hyper
    features, plus a `LatentSpaceTransform` of y1 (`F_tilde`, the features a frozen vision backbone is matched
    against by `vision_rd_loss`).  Same constructor, attributes, state-dict keys and out-dict keys as the reference.
    The reference's forward cannot run; the repairs made here, and nothing else:
      * `self.factorized_entropy_model(z_in, debug)` (Models.py:302) passes a positional argument the entropy
        model does not take -> called without it;
      * in mixture mode the second parameter dict overwrites the first (`params1 = {...weights2...}`,
        Models.py:298-299) -> it is `params2`;
      * `LatentSpaceTransform` keeps its channel count (components.LatentSpaceTransform)."""

    def __init__(self, latent_channels: int = 192, base_channels: int = 128, K: int = 1):
        super().__init__()
        if not isinstance(latent_channels, int) or latent_channels < 1:
            raise ValueError(f"latent_channels must be int >= 1, got {latent_channels}")
        if not isinstance(K, int) or K < 1:
            raise ValueError(f"K must be int >= 1, got {K}")
        if not isinstance(base_channels, int) or not 0 < base_channels < latent_channels:
            raise ValueError(f"base_channels must be an int in (0, latent_channels), got {base_channels}")
        self.M, self.M1, self.M2 = latent_channels, base_channels, latent_channels - base_channels
        self.H, self.K = latent_channels, K
        self.distribution = 'Mean-Scale Gaussian' if K == 1 else 'Mixture of Gaussians'
        self.conditional = GaussianConditional() if K == 1 else GaussianMixtureConditional()
        self.encoder = Encoder5x5(latent_channels=self.M)
        self.decoder = Decoder5x5(latent_channels=self.M)
        self.hyper_encoder = HyperEncoder5x5(latent_channels=self.M)
        self.hyper_decoder = HyperDecoder5x5(latent_channels=self.M)
        self.factorized_entropy_model = FactorizedEntropyBottleneck(self.M)
        self.context_model_1 = ContextModel(latent_channels=self.M1)
        self.context_model_2 = ContextModel(latent_channels=self.M2)
        self.entropy_parameters_1 = EntropyParameters(latent_channels=self.M1, hyper_latent_channels=self.H, K=self.K)
        self.entropy_parameters_2 = EntropyParameters(latent_channels=self.M2, hyper_latent_channels=self.H, K=self.K)
        self.LST = LatentSpaceTransform(latent_channels=self.M1, upsampling_factors=[2, 1, 1, 1])

    use_step_prep = _HyperpriorContextModel.use_step_prep
    step_prep = _HyperpriorContextModel.step_prep

    def forward(self, x: torch.Tensor, training: bool = True, debug=False, noise=None):
        """`noise` (test hook, not in the reference): (u_z, u_y) used instead of torch.rand_like, z first."""
        if x.shape[2] % 64 or x.shape[3] % 64:
            raise RuntimeError("H and W must be multiples of 64 (phi/psi shapes must agree, Models.py:283-284)")
        if self.use_step_prep and x.is_cuda:
            self.step_prep().run()
        y = self.encoder(x)
        z = self.hyper_encoder(y)
        if training:
            uz, uy = noise if noise is not None else (torch.rand_like(z), torch.rand_like(y))
            z_in, y_in = F_.quantize(z, uz, True), F_.quantize(y, uy, True)
        else:
            z_in, y_in = F_.quantize(z, None, False), F_.quantize(y, None, False)
        y1, y2 = torch.split(y_in, [self.M1, self.M2], dim=1)
        psi = self.hyper_decoder(z_in)
        out = {'y': y, 'y_in': y_in, 'y1': y1, 'y2': y2, 'z': z, 'z_in': z_in, 'training': training}
        params = {}
        for tag, yk, ctx, ep in (("1", y1, self.context_model_1, self.entropy_parameters_1),
                                 ("2", y2, self.context_model_2, self.entropy_parameters_2)):
            act = ep.packed(torch.cat([ctx(yk), psi], dim=1))
            names = ("mu", "sigma") if self.K == 1 else ("weights", "mus", "sigmas")
            params.update({n + tag: v for n, v in zip(names, ep.split(act))})
            out['p_y' + tag], out['logp_y' + tag] = self.conditional.packed_likelihood_and_log(yk, act, self.K)
        out['p_z'], out['logp_z'] = self.factorized_entropy_model.likelihood_and_log(z_in)
        out['x_hat'] = self.decoder(y_in)
        out['F_tilde'] = self.LST(y1)
        out.update(params)
        return out
