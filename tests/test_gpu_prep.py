"""lic_prep_run (one launch per optimizer step for every parameter-derived buffer) against the stand-alone
entry points it replaces: the buffers must be bit-identical, the model's outputs and gradients must not
change by a single bit, it must relaunch exactly when the parameters changed, and the context model's
weight must end up masked in place (ContextModels.py:19).  Every published buffer is also held to tests/prep_ref.py,
the numpy statement of the layouts applied to the parameter itself, and the rebuild rules of prep.StepPrep (a replaced
parameter storage, invalidate(), a precision switch) are run."""
import numpy as np
import pytest
import torch

import prep_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import functional as F_
    return nic, F_, torch.device("cuda:0")


def _step(nic, model, x, noise):
    model.zero_grad(set_to_none=True)
    out = model(x, noise=noise)
    res = nic.rd_loss(out, x, 0.01, sync=False)
    res["loss"].backward()
    torch.cuda.synchronize()
    return [out[k].detach().clone() for k in ("x_hat", "y", "z", "logp_y", "logp_z")] + [res["loss"].detach().clone()] + \
           [p.grad.detach().clone() for p in model.parameters()]


def _model(nic, cls, M, K, dev):
    """cls: "jah", "hmr", or "jah_cb" = the joint model with the checkerboard context"""
    if cls == "jah_cb":
        return nic.JointAutoregressiveHierarchical(M, K, context="checkerboard").to(dev)
    return (nic.JointAutoregressiveHierarchical if cls == "jah" else nic.HierarchicalMixtureResidual)(M, K).to(dev)


def _reference_bits(model, p, kind):
    """bit patterns of the buffer `kind` of parameter `p` by tests/prep_ref.py (the layouts of include/lic.h applied to
    the parameter: no packing kernel involved), or None for a kind this function does not know"""
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    from neural_image_compression_amd.layers import ConvTranspose2d, GDN
    owner = next(m for m in model.modules() if any(q is p for q in m.parameters(recurse=False)))
    w = p.detach().cpu().numpy()
    prec, name = kind.split(".", 1) if "." in kind else ("", kind)
    if isinstance(owner, GDN):
        is_beta = p is owner.beta
        bound = (owner.beta_reparam if is_beta else owner.gamma_reparam).bound_value
        ped = owner.beta_reparam.pedestal_value
        # the fp32 values by lic_gdn_reparam, each of them one of the two correct roundings of max(v, bound)^2 - pedestal
        g = torch.empty_like(p.detach())
        L.check(L.load().lic_gdn_reparam(p.data_ptr(), g.data_ptr(), p.numel(), bound, ped, F_._stream()), "reparam")
        torch.cuda.synchronize()
        g = g.cpu().numpy()
        fused, unfused = R.reparam_candidates(w, bound, ped)
        assert (((R.f32_bits(g) == R.f32_bits(fused)) | (R.f32_bits(g) == R.f32_bits(unfused)))).all()
        if name == "beta_e":
            return R.f32_bits(g)
        # gamma_eff[i][j]: gT is the B operand [k = j][n = i], g is [k = i][n = j]; the "p" kinds in the kperm K order
        vals = {"gdn_gT": g.T, "gdn_gTp": g.T, "gdn_g": g, "gdn_gp": g}.get(name)
        if vals is None:
            return None
        rk = R.PACK_BF16_KPERM if name.endswith("p") else (R.PACK_BF16 if prec == "bf16" else R.PACK_F32)
        assert prec == "bf16" or not name.endswith("p")
        return R.pack(rk, np.ascontiguousarray(vals)[None])
    tr = isinstance(owner, ConvTranspose2d)
    d0, d1, kh, kw = w.shape
    t = w.reshape(d0, d1, kh * kw)
    rk = R.PACK_BF16 if prec == "bf16" else R.PACK_F32
    if name in ("stem16", "head_dx16"):
        return R.pack(R.PACK_BF16, R.stem_logical(w))
    if name == "stem":        # [taps*Cin][Cout], row cin*tap + c
        return R.pack(rk, np.ascontiguousarray(t.transpose(2, 1, 0).reshape(1, kh * kw * d1, d0)))
    if name == "head":        # [Cin][taps*Cout], column cout*tap + c
        return R.pack(rk, np.ascontiguousarray(t.transpose(0, 2, 1).reshape(1, d0, kh * kw * d1)))
    if name == "head_dx":     # its transpose
        return R.pack(rk, np.ascontiguousarray(t.transpose(2, 1, 0).reshape(1, kh * kw * d1, d0)))
    if name in ("fwd", "dgrad"):
        # [tap][k][n]: forward contracts over the layer's input channels, dgrad over its output channels
        cin_first = t.transpose(2, 0, 1) if tr else t.transpose(2, 1, 0)       # [tap][Cin][Cout]
        return R.pack(rk, np.ascontiguousarray(cin_first if name == "fwd" else cin_first.transpose(0, 2, 1)))
    return None


@pytest.mark.parametrize("cls,M,K,precision", [("jah", 64, 3, "fp32"), ("jah", 64, 1, "bf16"), ("hmr", 32, 1, "fp32"),
                                                ("jah", 192, 1, "fp32"), ("jah", 40, 1, "fp32"), ("hmr", 24, 1, "fp32"),
                                                ("jah_cb", 64, 1, "fp32")])
# (no bf16 row at M = 40: lic_igemm_bf16 refuses that channel count with LIC_ERR_UNSUPPORTED, prepared or not)
def test_step_prep_is_bitwise_neutral_and_tracks_versions(env, cls, M, K, precision):
    nic, F_, dev = env
    torch.manual_seed(3)
    model = _model(nic, cls, M, K, dev)
    if precision == "bf16":
        model.set_precision("bf16")
    with torch.no_grad():   # GDN parameters on both sides of their lower bounds
        for m in model.modules():
            if type(m).__name__ == "GDN":
                m.gamma.add_(0.05 * torch.rand_like(m.gamma) - 0.02)
                m.beta.mul_(torch.rand_like(m.beta) * 1.5)
    B, H = 2, 128
    x = torch.rand(B, 3, H, H, device=dev).contiguous(memory_format=torch.channels_last)
    noise = (torch.rand(B, M, H // 64, H // 64, device=dev), torch.rand(B, M, H // 16, H // 16, device=dev))
    w_ctx = model.context_model.masked.weight
    model.use_step_prep = False
    ref = _step(nic, model, x, noise)
    masked_ref = w_ctx.detach().clone()
    with torch.no_grad():   # un-mask the weight again so that the prepared path has to mask it itself
        w_ctx.add_(1.0 - model.context_model.masked.mask)
    model.use_step_prep = True
    prep = model.step_prep()
    got = _step(nic, model, x, noise)
    assert prep.launches == 1
    assert torch.equal(w_ctx, masked_ref), "lic_prep_run must mask the context weight in place"
    for a, b in zip(ref, got):
        assert torch.equal(a, b), "step preparation changed a result"
    # every published buffer equals what the stand-alone packing entry points produce
    n_checked = 0
    for p, kind, buf in prep._entries:
        assert F_.prepared(p, kind) is buf
        if kind.endswith(".fwd") or kind.endswith(".dgrad"):
            entry = F_.PREPARED.pop((id(p), kind))
            tr = any(p is m.weight for m in model.modules() if type(m).__name__ == "ConvTranspose2d")
            if kind.startswith("f32"):
                alone = F_._pack_conv_weight(p.detach(), tr, kind.endswith("dgrad"))
            else:
                from neural_image_compression_amd import functional_bf16 as FB_
                alone = FB_._pack_conv_weight_bf16(p.detach(), tr, kind.endswith("dgrad"))
            F_.PREPARED[(id(p), kind)] = entry
            assert alone.data_ptr() != buf.data_ptr() and torch.equal(alone.view(torch.uint8), buf.view(torch.uint8)), kind
            n_checked += 1
    assert n_checked >= 20
    # ... and what the layouts of include/lic.h say about the parameter itself (tests/prep_ref.py: not another kernel)
    kinds = set()
    for p, kind, buf in prep._entries:
        if kind == "masked":
            assert buf is w_ctx
            continue
        want = _reference_bits(model, p, kind)
        assert want is not None, f"no reference for the kind {kind}"
        got = buf.detach().cpu().contiguous().view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32).numpy()
        got = got.view(np.uint16 if buf.dtype == torch.bfloat16 else np.uint32).reshape(-1)
        assert got.shape == want.shape and np.array_equal(got, want), (kind, tuple(p.shape))
        kinds.add(kind)
    if precision == "bf16":
        need = {"f32.beta_e", "bf16.gdn_gT", "bf16.gdn_gTp", "bf16.gdn_g", "bf16.gdn_gp", "bf16.stem", "bf16.head",
                "bf16.head_dx", "bf16.fwd", "bf16.dgrad"} | ({"bf16.stem16", "bf16.head_dx16"} if M == 64 else set())
    elif cls == "hmr":
        need = {"f32.fwd", "f32.dgrad"}
    else:
        need = {"f32.beta_e", "f32.gdn_gT", "f32.gdn_g", "f32.stem", "f32.head", "f32.head_dx", "f32.fwd", "f32.dgrad"}
    assert need <= kinds, need - kinds
    # same parameters -> no relaunch; after an optimizer step -> exactly one more
    _step(nic, model, x, noise)
    assert prep.launches == 1
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.step()
    got2 = _step(nic, model, x, noise)
    assert prep.launches == 2
    model.use_step_prep = False
    F_.PREPARED.clear()
    ref2 = _step(nic, model, x, noise)
    for a, b in zip(ref2, got2):
        assert torch.equal(a, b), "step preparation changed a result after an optimizer step"
    assert not torch.equal(ref[0], ref2[0])


def test_prepared_buffers_die_with_the_model(env):
    nic, F_, dev = env
    import gc
    model = nic.JointAutoregressiveHierarchical(64, 1).to(dev)
    x = torch.rand(1, 3, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        model(x, training=False)
    keys = list(model.step_prep()._keys)
    assert keys and all(k in F_.PREPARED for k in keys)
    del model
    gc.collect()
    assert not any(k in F_.PREPARED for k in keys)


# ---------------------------------------------------------------------------------------------
# prep.StepPrep's rebuild rules
# ---------------------------------------------------------------------------------------------
def _small(env, M=24, seed=5):
    nic, F_, dev = env
    torch.manual_seed(seed)
    model = nic.JointAutoregressiveHierarchical(M, 1).to(dev)
    x = torch.rand(1, 3, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
    noise = (torch.rand(1, M, 1, 1, device=dev), torch.rand(1, M, 4, 4, device=dev))
    return model, x, noise


def _unprepared(nic, F_, model, x, noise):
    """the step with every buffer derived on the fly by the stand-alone entry points"""
    model.use_step_prep = False
    saved = dict(F_.PREPARED)
    F_.PREPARED.clear()
    try:
        return _step(nic, model, x, noise)
    finally:
        F_.PREPARED.update(saved)
        model.use_step_prep = True


def _equal(a, b, what):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert torch.equal(u, v), what


def test_replaced_parameter_storage_rebuilds_the_table(env):
    nic, F_, dev = env
    model, x, noise = _small(env)
    prep = model.step_prep()
    first = _step(nic, model, x, noise)
    assert prep.launches == 1
    table = prep._jobs_dev
    convs = [m for m in model.modules() if type(m).__name__ == "Conv2d" and m.weight.shape[1] >= 4]
    gdns = [m for m in model.modules() if type(m).__name__ == "GDN"]
    w, gamma = convs[0].weight, gdns[0].gamma
    old = (w.data_ptr(), gamma.data_ptr())
    keep = [w.data, gamma.data]                    # the old storages stay allocated: the new ones are elsewhere
    w.data = w.data.clone().mul_(1.25)             # new storage AND new values: a stale pointer reads the old ones
    gamma.data = gamma.data.clone().add_(0.01)
    assert w.data_ptr() != old[0] and gamma.data_ptr() != old[1]
    got = _step(nic, model, x, noise)
    assert prep._jobs_dev is not table, "the job table holds pointers into the replaced storage"
    assert prep.launches == 2
    _equal(_unprepared(nic, F_, model, x, noise), got, "after p.data = ...: prepared and unprepared steps differ")
    assert not torch.equal(first[0], got[0])
    del keep


def test_data_writes_need_invalidate(env):
    nic, F_, dev = env
    model, x, noise = _small(env, seed=6)
    prep = model.step_prep()
    _step(nic, model, x, noise)
    assert prep.launches == 1
    conv = next(m for m in model.modules() if type(m).__name__ == "Conv2d" and m.weight.shape[1] >= 4)
    w = conv.weight
    buf = F_.prepared(w, "f32.fwd")
    assert buf is not None
    before = buf.clone()
    version = w._version
    w.data.mul_(0.5)                                # does not bump the parameter's version counter
    assert w._version == version
    _step(nic, model, x, noise)
    assert prep.launches == 1, "a write through .data is invisible to the version counters"
    assert F_.prepared(w, "f32.fwd") is buf and torch.equal(buf, before), "the buffers stay stale until invalidate()"
    prep.invalidate()
    got = _step(nic, model, x, noise)
    assert prep.launches == 2, "invalidate(): exactly one more launch"
    _step(nic, model, x, noise)
    assert prep.launches == 2
    fresh = F_.prepared(w, "f32.fwd")
    want = _reference_bits(model, w, "f32.fwd")
    assert np.array_equal(fresh.cpu().view(torch.int32).numpy().view(np.uint32).reshape(-1), want)
    assert not torch.equal(fresh, before)
    _equal(_unprepared(nic, F_, model, x, noise), got, "after invalidate(): prepared and unprepared steps differ")


def test_precision_switch_rebuilds_with_the_bf16_kinds(env):
    nic, F_, dev = env
    model, x, noise = _small(env, M=64, seed=7)
    prep = model.step_prep()
    _step(nic, model, x, noise)
    assert prep.launches == 1 and not any(k.startswith("bf16.") for _, k, _ in prep._entries)
    table = prep._jobs_dev
    model.set_precision("bf16")
    got = _step(nic, model, x, noise)
    assert prep._jobs_dev is not table and prep.launches == 2
    kinds = {k for _, k, _ in prep._entries}
    assert {"bf16.fwd", "bf16.dgrad", "bf16.gdn_gT", "bf16.gdn_gTp", "bf16.gdn_g", "bf16.gdn_gp", "bf16.stem", "bf16.head",
            "bf16.head_dx", "bf16.stem16", "bf16.head_dx16", "f32.beta_e"} <= kinds, kinds
    for p, kind, buf in prep._entries:
        assert F_.prepared(p, kind) is buf
    _equal(_unprepared(nic, F_, model, x, noise), got, "bf16: prepared and unprepared steps differ")
