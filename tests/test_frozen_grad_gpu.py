"""GPU: the input gradient of the frozen encoder in HIP (`MixingStyleEncoder.input_grad_backend = "hip"`: `_HipFrozenTrunk` ->
`mst_encoder_forward_frozen`, `mst_encoder_frozen_backward_apply`, `mst_encoder_train_conv2_dgrad`, `mst_encoder_conv1_dgrad`; head
`_HipHead`).

Yardsticks (tests/frozen_ref.py, validated on the host by tests/test_frozen_grad_cpu.py): the PyTorch modules with the same
parameters on the host (`encoder_backend="torch"`) in float64 and in fp32.  A max-pool gradient is discontinuous at ties, so

* DECISIONS: the HIP path's arg-max per pooling window may differ from the float64 tree's only where float64 itself has a
  near-tie: gap below tau = 4 x max |z_fp32 - z_float64| of that layer (2: both candidates move; 2: the project's allowance over
  the reference's own fp32 error).  At most 2 + 1e-4 x windows differ per layer.
* ARITHMETIC: with the HIP path's decisions pinned, the float64 restatement of the backward pass is the reference; the HIP
  gradient's max |d| / max |ref| stays within 2 x that of the same restatement evaluated in fp32 on the host.

Inputs: cases.pcm_batch (integer-built, the same bits on every machine) through the model's own stage A."""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

import cases
import frozen_ref as fr
import parity
from test_encoder_gpu import close

pytestmark = pytest.mark.gpu


def as_stems(x):
    return {s: x[:, 2 * i:2 * i + 2] for i, s in enumerate(cases.STEMS)}


@functools.lru_cache(maxsize=None)
def gpu_model(cfgname):
    from mst_amd.model import MixingStyleEncoder
    cfg = fr.CASES[cfgname]
    m = MixingStyleEncoder(channels=8, feature_dim=64, encoder_backend="hip", **cfg).cuda().eval()
    for q in m.parameters():
        q.requires_grad_(False)
    m.input_grad_backend = "hip"
    m._loaded_seed = None
    return m


def model_with(cfgname, seed):
    """THE module of this configuration holding make_state_dict(cfg, seed): a second seed is loaded into the same module, so the
    handle behind `hip_encoder()` is refreshed on the device, not rebuilt."""
    m = gpu_model(cfgname)
    if m._loaded_seed != seed:
        full = dict(m.state_dict())
        full.update(cases.make_state_dict(fr.CASES[cfgname], seed))
        m.load_state_dict(full, strict=True)
        m._loaded_seed = seed
    return m


def hip_gradient(model, lm, feats, R):
    leaf = lm.clone().requires_grad_(True)
    emb = model.forward_from_logmel(leaf, feats)
    (emb * R).sum().backward()
    return emb.detach(), leaf.grad


@functools.lru_cache(maxsize=None)
def case(cfgname, B, frames, seed=42):
    """Everything one (configuration, shape) needs, computed once and never modified."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = fr.CASES[cfgname]
    model = model_with(cfgname, seed)
    x = cases.pcm_batch(B, fr.clip_samples(cfg, frames))
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(as_stems(x.cuda()))
    assert lm.shape == (B, 8, cfg["n_mels"], frames)
    feats, R = fr.side_inputs(B, cfg["embed_dim"])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    twin64, twin32 = fr.torch_twin(cfg, sd, torch.float64), fr.torch_twin(cfg, sd, torch.float32)
    t64, t32 = fr.tree(twin64, lm.cpu(), feats), fr.tree(twin32, lm.cpu(), feats)
    enc = model.hip_encoder()
    emb_f, taps, ws = enc.forward_frozen(lm, feats.cuda())
    ones1, ones2 = torch.ones_like(taps["pool1"]), torch.ones_like(taps["pool_in"])
    m1 = (enc.frozen_backward_apply(1, ones1, B, frames, ws) != 0).transpose(0, 1).cpu()   # (B, ns, 32, R, Fr)
    m2 = (enc.frozen_backward_apply(2, ones2, B, frames, ws) != 0).transpose(0, 1).cpu()   # (B, ns, 64, H1, W1)
    emb, grad = hip_gradient(model, lm, feats.cuda(), R.cuda())
    torch.cuda.synchronize()
    return dict(cfg=cfg, lm=lm, feats=feats, R=R, twin64=twin64, twin32=twin32, t64=t64, t32=t32, emb_frozen=emb_f.cpu(),
                pool1=taps["pool1"].cpu(), pool_in=taps["pool_in"].cpu(), m1=m1, m2=m2, emb=emb.cpu(), grad=grad.cpu())


def arithmetic_check(c, B, frames, label):
    """Test 3 for a computed case; returns (hip error, fp32 restatement's error), both max |d| / max |ref| against float64."""
    cfg, t64, t32 = c["cfg"], c["t64"], c["t32"]
    ref = fr.pinned_gradient(c["twin64"], cfg, c["pool_in"], t64["A1"], t64["A2"], c["m1"], c["m2"], c["R"], frames)
    r32 = fr.pinned_gradient(c["twin32"], cfg, c["pool_in"], t32["A1"], t32["A2"], c["m1"], c["m2"], c["R"], frames)
    e_ref, e_hip = fr.normwise(r32, ref), fr.normwise(c["grad"], ref)
    parity.record(f"frozen grad {label} d logmel [fp32 restatement vs f64]", r32, ref)
    parity.record(f"frozen grad {label} d logmel [hip vs f64]", c["grad"], ref)
    parity.note(f"frozen grad {label} 2x rule", e_ref=e_ref, e_hip=e_hip, ratio=e_hip / e_ref)
    print(f"frozen grad {label}: fp32 restatement {e_ref:.3e}, hip {e_hip:.3e}, ratio {e_hip / e_ref:.2f}")
    assert float(ref.abs().max()) > 0 and torch.isfinite(c["grad"]).all()
    ns = fr.geometry(cfg)[0]
    covered = (ns - 1) * cfg["overlap"] + cfg["split_size"]
    assert torch.count_nonzero(c["grad"][:, :, covered:]) == 0   # mel rows no sub-band covers: exactly 0
    assert e_hip <= 2.0 * e_ref, f"{label}: hip {e_hip:.3e} > 2 x fp32 restatement {e_ref:.3e}"
    return e_hip, e_ref


# ---- 1. forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,B,frames", fr.SHAPES)
def test_forward_frozen_matches_float64_and_the_eval_forward(cfgname, B, frames):
    c = case(cfgname, B, frames)
    t64 = c["t64"]
    close(c["pool1"], t64["pool1"], 1e-4)
    close(c["pool_in"], t64["pool_in"], 1e-4)
    close(c["emb_frozen"], t64["emb"], 1e-4)
    close(c["emb"], t64["emb"], 1e-4)   # the autograd path (head: _HipHead)
    with torch.no_grad():
        plain = model_with(cfgname, 42).hip_encoder().forward(c["lm"], c["feats"].cuda()).cpu()
    close(c["emb_frozen"], plain, 1e-4)   # other kernels: the same bar, not the same bits


# ---- 2. decisions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,B,frames", fr.SHAPES)
def test_max_pool_decisions_differ_from_float64_only_at_near_ties(cfgname, B, frames):
    c = case(cfgname, B, frames)
    for layer, k in zip((1, 2), fr.pool_shapes(c["cfg"])):
        z64, z32, hip = c["t64"][f"z{layer}"], c["t32"][f"z{layer}"], c[f"m{layer}"]
        assert hip.shape == z64.shape
        tau = 4.0 * float((z32.double() - z64).abs().max())
        ref = fr.decisions(z64, *k)
        per_window = fr.windows(hip, *k).sum(-1)
        assert int(per_window.max()) <= 1   # one-hot, and nothing outside the pooled region
        assert not hip[..., per_window.shape[-2] * k[0]:, :].any() and not hip[..., per_window.shape[-1] * k[1]:].any()
        differ = (fr.windows(hip, *k) != fr.windows(ref, *k)).any(-1)
        gap = (fr.picked_value(z64, hip, *k) - fr.picked_value(z64, ref, *k)).abs()   # (a side that picks nothing counts as 0)
        n, nd = differ.numel(), int(differ.sum())
        worst = float(gap[differ].max()) if nd else 0.0
        share, _ = fr.near_tie_share(z64, *k, tau)
        fp32_differs = int((fr.windows(fr.decisions(z32, *k), *k) != fr.windows(ref, *k)).any(-1).sum())
        parity.note(f"frozen grad {cfgname} ({B}, {frames}) layer {layer} decisions", windows=n, hip_differs=nd, torch_fp32_differs=fp32_differs,
                    tau=tau, worst_gap=worst, near_tie_share=share)
        print(f"{cfgname} ({B}, {frames}) layer {layer}: {n} windows, hip differs in {nd} (torch fp32: {fp32_differs}), tau {tau:.3e}, "
              f"worst gap {worst:.3e}, near-tie share {share:.3e}")
        assert share <= 1e-3
        assert nd <= 2 + 1e-4 * n
        assert worst < tau, f"layer {layer}: a differing window has a float64 gap of {worst:.3e} >= tau {tau:.3e}"


# ---- 3. arithmetic with the decisions pinned ------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,B,frames", fr.SHAPES)
def test_gradient_with_pinned_decisions_two_times_rule(cfgname, B, frames):
    """Measured ratios hip / fp32 restatement: see DESIGN 3.10."""
    arithmetic_check(case(cfgname, B, frames), B, frames, f"{cfgname} ({B}, {frames})")


# ---- 4. the conv1 input-gradient kernel alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname", ["default", "baseline_sh"])
@pytest.mark.parametrize("B,frames", [(3, 20), (3, 41), (2, 431)])
def test_conv1_input_gradient_kernel(cfgname, B, frames):
    cfg = fr.CASES[cfgname]
    model = model_with(cfgname, 42)
    enc = model.hip_encoder()
    ns, split, ov, M = fr.geometry(cfg)[0], cfg["split_size"], cfg["overlap"], cfg["n_mels"]
    dy1 = torch.randn(ns, B, 32, split, frames, generator=cases._g(31))
    got = enc.conv1_dgrad(dy1.cuda(), B, frames).cpu()
    assert got.shape == (B, 8, M, frames)
    ref = torch.zeros(B, 8, M, frames, dtype=torch.float64)
    for i in range(ns):
        w = model.audio_encoder.subnet_cnns[i].conv1.weight.detach().cpu().double()
        ref[:, :, i * ov:i * ov + split] += torch.nn.grad.conv2d_input((B, 8, split, frames), w, dy1[i].double(), padding=3)
    for i in (0, ns // 2, ns - 1):   # a band's rows hold its neighbours' overlap too
        close(got[:, :, i * ov:i * ov + split], ref[:, :, i * ov:i * ov + split], 1e-5)
    close(got, ref, 1e-5)
    covered = (ns - 1) * ov + split
    assert torch.count_nonzero(got[:, :, covered:]) == 0
    again = enc.conv1_dgrad(dy1.cuda(), B, frames).cpu()
    assert torch.equal(got, again)
    alone = enc.conv1_dgrad(dy1[:, 1:2].contiguous().cuda(), 1, frames).cpu()
    assert torch.equal(alone[0], got[1])


# ---- 5. bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,B,frames", [("default", 2, 83), ("baseline_sh", 3, 122)])
def test_gradient_bits(cfgname, B, frames):
    c = case(cfgname, B, frames)
    model = model_with(cfgname, 42)
    lm, feats, R = c["lm"], c["feats"].cuda(), c["R"].cuda()
    emb, grad = hip_gradient(model, lm, feats, R)
    assert torch.equal(grad.cpu(), c["grad"]) and torch.equal(emb.cpu(), c["emb"])          # the same call twice
    b = B - 1
    _, alone = hip_gradient(model, lm[b:b + 1], feats[b:b + 1], R[b:b + 1])
    assert torch.equal(alone[0].cpu(), c["grad"][b])                                       # a clip does not see its neighbours
    leaf = lm.clone().requires_grad_(True)
    loss = (model.forward_from_logmel(leaf, feats) * R).sum()
    loss.backward(retain_graph=True)
    assert torch.equal(leaf.grad.cpu(), c["grad"])
    loss.backward()
    assert torch.equal(leaf.grad.cpu(), 2 * c["grad"])                                     # the saved activations were left intact
    la, lb = lm.clone().requires_grad_(True), lm[:1].clone().requires_grad_(True)          # two forwards alive at once
    ea = model.forward_from_logmel(la, feats)
    eb = model.forward_from_logmel(lb, feats[:1])
    (eb * R[:1]).sum().backward()
    (ea * R).sum().backward()
    assert torch.equal(la.grad.cpu(), c["grad"])
    _, solo = hip_gradient(model, lm[:1], feats[:1], R[:1])
    assert torch.equal(lb.grad, solo)


def test_end_to_end_is_trunk_cotangent_through_stage_a():
    """tests/test_style_term_gpu.py::test_composition_is_trunk_cotangent_through_stage_a with the trunk in HIP."""
    import test_style_term_gpu as st
    from mst_amd.mixing_utils import deferred_features
    model = st.make_encoder("hip").cuda()
    model.input_grad_backend = "hip"
    x, target, _ = st.make_inputs()
    x, target = x.cuda(), target.cuda()
    pre = model.audio_encoder.mel_preprocessor
    deferred = deferred_features(64).expand(st.B, 64).cuda()
    with torch.no_grad():
        lm, feats = pre.plan(0).forward_stems(st.as_stems(x), True, True)
    leaf = lm.clone().requires_grad_(True)
    emb_leaf = model.forward_from_logmel(leaf, feats)
    st.style_loss(emb_leaf, target).backward()
    g = leaf.grad
    assert g is not None and float(g.abs().max()) > 0
    xa = x.clone().requires_grad_(True)
    pre(st.as_stems(xa)).backward(g)
    xe = x.clone().requires_grad_(True)
    emb = model(st.as_stems(xe), deferred)
    assert emb.requires_grad
    st.style_loss(emb, target).backward()
    assert torch.equal(emb.detach(), emb_leaf.detach())
    assert xe.grad is not None and float(xe.grad.abs().max()) > 0
    assert torch.equal(xe.grad, xa.grad)


# ---- 6. refresh -------------------------------------------------------------------------------------------------------------
def test_another_state_dict_in_the_same_module():
    model = model_with("default", 42)
    enc = model.hip_encoder()
    try:
        c = case("default", 2, 45, 43)
        assert model.hip_encoder() is enc   # refreshed on the device (mst_encoder_update_params), not rebuilt
        arithmetic_check(c, 2, 45, "default (2, 45) seed 43")
        assert not torch.equal(c["grad"], case("default", 2, 45)["grad"])
    finally:
        model_with("default", 42)


# ---- 7. public behaviour ------------------------------------------------------------------------------------------------------
def test_default_switch_keeps_the_refusal():
    import test_style_term_gpu as st
    model = st.make_encoder("hip").cuda()
    assert model.input_grad_backend == "none"
    x, _, feats = st.make_inputs()
    xg = x.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match='encoder_backend="torch"'):
        model(st.as_stems(xg), feats.cuda())


def test_refusals_name_the_reason():
    import test_style_term_gpu as st
    from mst_amd.model import MixingStyleEncoder
    x, _, feats = st.make_inputs()
    x, feats = x.cuda(), feats.cuda()

    def fresh(**kw):
        torch.manual_seed(1)
        m = MixingStyleEncoder(embed_dim=64, feature_dim=64, encoder_backend="hip", **kw).cuda().eval()
        for q in m.parameters():
            q.requires_grad_(False)
        m.input_grad_backend = "hip"
        return m

    def stems():
        return st.as_stems(x.clone().requires_grad_(True))
    m = fresh()
    m.audio_encoder.subnet_cnns[0].conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"require grad.*freeze"):
        m(stems(), feats)
    m = fresh()
    with pytest.raises(RuntimeError, match="mixing_features requires grad"):
        m(stems(), feats.clone().requires_grad_(True))
    m = fresh().train()
    with pytest.raises(RuntimeError, match="training mode"):
        m(stems(), feats)
    m = fresh()
    lm = torch.randn(2, 8, 128, 40, device="cuda")
    with pytest.raises(RuntimeError, match="non-fp32"):
        m.forward_from_logmel(lm.double().requires_grad_(True), feats)
    with pytest.raises(RuntimeError, match="non-CUDA"):
        m.forward_from_logmel(lm.cpu().requires_grad_(True), feats)
    with pytest.raises(RuntimeError, match="19 frames < 20"):
        m.forward_from_logmel(lm[..., :19].clone().requires_grad_(True), feats)
    with pytest.raises(RuntimeError, match="19 frames < 20"):
        m(st.as_stems(x[..., :18 * 256 + 7].clone().requires_grad_(True)), feats)
    m.conv1_precision = "f16x3"
    with pytest.raises(RuntimeError, match="conv1_precision='f16x3'"):
        m.forward_from_logmel(lm.clone().requires_grad_(True), feats)
    m.conv1_precision = "fp32"
    m.small_nets_backend = "torch"
    with pytest.raises(RuntimeError, match="attention head"):
        m.forward_from_logmel(lm.clone().requires_grad_(True), feats)
    m = fresh(n_mels=64, split_size=32, overlap=16)
    with pytest.raises(RuntimeError, match="split_size=32"):
        m.forward_from_logmel(torch.randn(2, 8, 64, 40, device="cuda").requires_grad_(True), feats)
    m = fresh()
    m.input_grad_backend = "cuda"
    with pytest.raises(ValueError, match="input_grad_backend"):
        m.forward_from_logmel(lm.clone().requires_grad_(True), feats)


def test_gradient_step_decreases_the_style_loss():
    """tests/test_style_term_gpu.py::test_gradient_step_decreases_the_style_loss with trunk and head in HIP."""
    import test_style_term_gpu as st
    model = st.make_encoder("hip").cuda()
    model.input_grad_backend = "hip"
    x, target, feats = st.make_inputs()
    x, target, feats = x.cuda(), target.cuda(), feats.cuda()
    xg = x.clone().requires_grad_(True)
    loss = st.style_loss(model(st.as_stems(xg), feats), target)
    loss.backward()
    grad = xg.grad
    eta = 1e-3 * loss.item() / float((grad.double() ** 2).sum())
    with torch.no_grad():
        after = st.style_loss(model(st.as_stems(x - eta * grad), feats), target)
    predicted, realised = 1e-3 * loss.item(), loss.item() - after.item()
    print(f"style loss {loss.item():.6f} -> {after.item():.6f}: predicted decrease {predicted:.3e}, realised {realised:.3e}")
    assert after.item() < loss.item()
    assert realised >= 0.5 * predicted


def test_example_trains_with_the_hip_style_encoder():
    sys.path.insert(0, os.path.join(cases.ROOT, "examples"))
    import train_tcn_mixer
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        train_tcn_mixer.main(["--steps", "3", "--seconds", "0.5", "--batch-size", "2", "--style-weight", "1", "--style-encoder", "hip"])
    lines = [l for l in out.getvalue().splitlines() if l.startswith("step")]
    losses = [float(l.split("loss")[1].split()[0]) for l in lines]
    assert len(losses) == 3 and all(np.isfinite(l) and abs(l) < 1e6 for l in losses)
    assert all("style" in l for l in lines)
