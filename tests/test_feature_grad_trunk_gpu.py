"""GPU: the gradient through the mixing features behind the frozen encoder -- `mst_encoder_frozen_film_grad` (csrc/encoder.hip),
`mst_film_input_grad` (csrc/head.hip) and the public switch `MixingStyleEncoder.feature_grad_backend = "hip"` end to end.

Yardsticks: the PyTorch modules with the same parameters on the host in float64 and fp32 (tests/frozen_ref.py).  As in
tests/test_frozen_grad_gpu.py the max-pool decisions are pinned to the HIP path's (a pooling gradient is discontinuous at ties),
and the HIP result's max |d| / max |ref| against the float64 restatement stays within 2 x that of the same restatement
evaluated in fp32 on the host."""
import functools

import pytest
import torch
import torch.nn.functional as F

import cases
import feature_grad_ref as fg
import frozen_ref as fr
import parity
from test_frozen_grad_gpu import case, model_with

pytestmark = pytest.mark.gpu


def film_tensor(twin, feats):
    """(B, ns * 192) in the film head's order, per band [gamma1(32) beta1(32) gamma2(64) beta2(64)], with history."""
    film = twin.film_encoder(feats)
    ns = len(twin.audio_encoder.subnet_cnns)
    return torch.cat([torch.cat([film[f"gamma1_{i}"], film[f"beta1_{i}"], film[f"gamma2_{i}"], film[f"beta2_{i}"]], dim=1)
                      for i in range(ns)], dim=1)


def bn_outputs(twin, logmel, feats):
    """u1 (B, ns, 32, R, Fr), u2 (B, ns, 64, H1, W1): BN_eval(conv + bias) of both layers of the twin's forward."""
    dt = twin.film_encoder.film_head.weight.dtype
    u, hooks = {}, []
    for i, c in enumerate(twin.audio_encoder.subnet_cnns):
        hooks.append(c.bn1.register_forward_hook(lambda m, a, out, i=i: u.__setitem__((1, i), out.detach())))
        hooks.append(c.bn2.register_forward_hook(lambda m, a, out, i=i: u.__setitem__((2, i), out.detach())))
    with torch.no_grad():
        twin.forward_from_logmel(logmel.detach().to(dt), feats.to(dt))
    for h in hooks:
        h.remove()
    ns = len(twin.audio_encoder.subnet_cnns)
    return torch.stack([u[(1, i)] for i in range(ns)], 1), torch.stack([u[(2, i)] for i in range(ns)], 1)


def pinned_film_gradient(twin, c, frames):
    """d film (B, ns * 192) of (emb * R).sum() in the twin's dtype with the max-pool decisions of the HIP path:
    head autograd at the HIP pool_in -> df2 = mask2 up(d pool_in), dgamma2 = sum df2 u2, dbeta2 = sum df2 -> dy2 = A2 df2 ->
    conv2d_input -> df1 = mask1 up(d pool1), dgamma1 = sum df1 u1, dbeta1 = sum df1.  Also returns d pool_in."""
    cfg = c["cfg"]
    dt = twin.film_encoder.film_head.weight.dtype
    ns, sub, H1 = fr.geometry(cfg)
    split = cfg["split_size"]
    t = c["t64"] if dt == torch.float64 else c["t32"]
    B, W1 = c["pool_in"].shape[0], frames // 5
    u1, u2 = bn_outputs(twin, c["lm"].cpu(), c["feats"])
    p = c["pool_in"].detach().to(dt).clone().requires_grad_(True)
    with torch.enable_grad():
        emb = twin.audio_encoder.attention_pooling(p)
        dpool_in, = torch.autograd.grad((emb * c["R"].to(dt)).sum(), p)
    FD, W2 = H1 // 4, W1 // 4
    up2 = torch.zeros(B, ns, 64, H1, W1, dtype=dt)
    up2[..., :4 * FD, :4 * W2] = dpool_in.reshape(B, ns, 64, FD, W2).repeat_interleave(4, -2).repeat_interleave(4, -1)
    df2 = c["m2"].to(dt) * up2
    dy2 = t["A2"].to(dt)[..., None, None] * df2
    out = torch.zeros(B, ns, 192, dtype=dt)
    out[:, :, 64:128], out[:, :, 128:192] = (df2 * u2).sum(dim=(-2, -1)), df2.sum(dim=(-2, -1))
    for i, cn in enumerate(twin.audio_encoder.subnet_cnns):
        dp1 = torch.nn.grad.conv2d_input((B, 32, H1, W1), cn.conv2.weight, dy2[:, i], padding=3)
        up1 = torch.zeros(B, 32, split, frames, dtype=dt)
        up1[..., :sub * H1, :5 * W1] = dp1.repeat_interleave(sub, -2).repeat_interleave(5, -1)
        df1 = c["m1"][:, i].to(dt) * up1
        out[:, i, 0:32], out[:, i, 32:64] = (df1 * u1[:, i]).sum(dim=(-2, -1)), df1.sum(dim=(-2, -1))
    return out.reshape(B, ns * 192), dpool_in


def film_input_gradient(twin, feats, dfilm):
    """d feats of <dfilm, film(feats)> through the twin's FiLM MLP (eval mode) in its dtype."""
    dt = twin.film_encoder.film_head.weight.dtype
    f = feats.detach().to(dt).clone().requires_grad_(True)
    with torch.enable_grad():
        g, = torch.autograd.grad((film_tensor(twin, f) * dfilm.to(dt)).sum(), f)
    return g


# ---- 4. the two kernels against the float64 tree, decisions pinned --------------------------------------------------------
@pytest.mark.parametrize("cfgname,B,frames", fr.SHAPES)
def test_film_gradient_and_film_input_gradient_two_times_rule(cfgname, B, frames):
    """Measured ratios hip / fp32 restatement: see DESIGN 3.13."""
    from mst_amd.model import _film_input_grad
    c = case(cfgname, B, frames)
    model = model_with(cfgname, 42)
    enc = model.hip_encoder()
    ref, dpool64 = pinned_film_gradient(c["twin64"], c, frames)
    r32, _ = pinned_film_gradient(c["twin32"], c, frames)
    lm, feats = c["lm"], c["feats"].cuda()
    _, taps, ws = enc.forward_frozen(lm, feats, head=False)
    dpool = dpool64.float().cuda()
    dfilm = torch.full((B, enc.n_sub * 192), float("nan"), device="cuda")
    dy2 = enc.frozen_backward_apply(2, dpool, B, frames, ws)
    enc.frozen_film_grad(2, dpool, dfilm, B, frames, ws)
    assert torch.isnan(dfilm.view(B, -1, 192)[:, :, :64]).all() and torch.isfinite(dfilm.view(B, -1, 192)[:, :, 64:]).all()   # its own slots only
    dp1 = enc.conv2_dgrad(dy2, B, frames)
    enc.frozen_film_grad(1, dp1, dfilm, B, frames, ws)
    torch.cuda.synchronize()
    got = dfilm.cpu()
    assert torch.isfinite(got).all()
    label = f"{cfgname} ({B}, {frames})"
    bad = []
    for name, sl in (("gamma1", slice(0, 32)), ("beta1", slice(32, 64)), ("gamma2", slice(64, 128)), ("beta2", slice(128, 192))):
        pick = lambda z: z.reshape(B, -1, 192)[:, :, sl]
        e_ref, e_hip = fr.normwise(pick(r32), pick(ref)), fr.normwise(pick(got), pick(ref))
        parity.record(f"film grad {label} d{name} [hip vs f64]", pick(got), pick(ref))
        parity.note(f"film grad {label} d{name} 2x rule", e_ref=e_ref, e_hip=e_hip, ratio=e_hip / e_ref)
        print(f"film grad {label} d{name}: fp32 restatement {e_ref:.3e}, hip {e_hip:.3e}, ratio {e_hip / e_ref:.2f}")
        assert float(pick(ref).abs().max()) > 0
        if not e_hip <= 2.0 * e_ref:
            bad.append((name, e_hip, e_ref))
    assert not bad, f"{label}: hip beyond 2 x the fp32 restatement: {bad}"
    # twice: the same bits
    again = torch.empty_like(dfilm)
    enc.frozen_film_grad(2, dpool, again, B, frames, ws)
    enc.frozen_film_grad(1, dp1, again, B, frames, ws)
    assert torch.equal(again.cpu(), got)
    # FiLM MLP: the same cotangent (the HIP dfilm) through the three evaluations
    fe = model.film_encoder
    film_w = [q.detach() for q in (fe.feature_mlp[0].weight, fe.feature_mlp[0].bias, fe.feature_mlp[3].weight, fe.feature_mlp[3].bias,
                                    fe.film_head.weight, fe.film_head.bias)]
    dfe = _film_input_grad(feats.contiguous(), dfilm, film_w).cpu()
    f64, f32 = film_input_gradient(c["twin64"], c["feats"], got), film_input_gradient(c["twin32"], c["feats"], got)
    e_ref, e_hip = fr.normwise(f32, f64), fr.normwise(dfe, f64)
    parity.record(f"film input grad {label} [hip vs f64]", dfe, f64)
    parity.note(f"film input grad {label} 2x rule", e_ref=e_ref, e_hip=e_hip, ratio=e_hip / e_ref)
    print(f"film input grad {label}: fp32 restatement {e_ref:.3e}, hip {e_hip:.3e}, ratio {e_hip / e_ref:.2f}")
    assert float(f64.abs().max()) > 0 and e_hip <= 2.0 * e_ref
    assert torch.equal(_film_input_grad(feats.contiguous(), dfilm, film_w).cpu(), dfe)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
def style_loss(emb, target):
    return (1.0 - (F.normalize(emb, dim=1) * F.normalize(target, dim=1)).sum(dim=1)).mean()


def as_stems(x):
    return {s: x[:, 2 * i:2 * i + 2] for i, s in enumerate(cases.STEMS)}


def e2e_inputs(cfg, frames, B=2):
    T = fr.clip_samples(cfg, frames)
    g = cases._g(9900 + frames)
    x = torch.randn(B, 8, T, generator=g) * torch.tensor(fg.AMPS).repeat_interleave(2)[None, :, None]
    target = F.normalize(torch.randn(B, cfg["embed_dim"], generator=g), dim=1)
    return x, target


def host_tree_gradient(twin, cfg, x, target, dead):
    """The stems' gradient of 1 - cos through the twin on the host in its dtype, log-mel and the 24 live features both
    differentiable (the other 40 entries: the constants `dead`)."""
    dt = twin.film_encoder.film_head.weight.dtype
    from oracle import mel as omel
    xx = x.detach().to(dt).requires_grad_(True)
    kw = dict(n_fft=cfg["n_fft"], hop=cfg["hop_length"], n_mels=cfg["n_mels"])
    lm = omel.logmel(xx, **kw)
    live = torch.zeros(64, dtype=torch.bool)
    live[fg.LIVE] = True
    feats = torch.where(live[None, :], fg.features(xx, kw["n_fft"], kw["hop"], kw["n_mels"]), dead.to(dt))
    emb = twin.forward_from_logmel(lm, feats)
    g, = torch.autograd.grad(style_loss(emb, target.to(dt)), xx)
    return g


@functools.lru_cache(maxsize=None)
def e2e(cfgname, frames):
    from mst_amd.mixing_utils import deferred_features
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = fr.CASES[cfgname]
    model = model_with(cfgname, 42)
    x, target = e2e_inputs(cfg, frames)
    B = x.shape[0]
    deferred = deferred_features(64).expand(B, 64).cuda()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    twin64, twin32 = fr.torch_twin(cfg, sd, torch.float64), fr.torch_twin(cfg, sd, torch.float32)
    torch_model = fr.torch_twin(cfg, sd, torch.float32).cuda()

    def run(m, switch):
        old = m.feature_grad_backend
        m.feature_grad_backend = switch
        try:
            xg = x.cuda().requires_grad_(True)
            emb = m(as_stems(xg), deferred)
            style_loss(emb, target.cuda()).backward()
            torch.cuda.synchronize()
            return emb.detach().cpu(), xg.grad.cpu()
        finally:
            m.feature_grad_backend = old
    out = {"hip": run(model, "hip"), "hip_none": run(model, "none"), "torch": run(torch_model, "hip"), "torch_none": run(torch_model, "none")}
    out["hip_again"] = run(model, "hip")
    with torch.no_grad():
        dead = model.audio_encoder.mel_preprocessor.plan(0).forward_stems(as_stems(x.cuda()), False, True)[1].cpu()
    out["g64"] = host_tree_gradient(twin64, cfg, x, target, dead)
    out["g32"] = host_tree_gradient(twin32, cfg, x, target, dead)
    return out


@pytest.mark.parametrize("cfgname", ["default", "baseline_sh"])
@pytest.mark.parametrize("frames", [24, 45])
@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_end_to_end_style_gradient(cfgname, frames, backend):
    r = e2e(cfgname, frames)
    (emb, got), (emb0, const) = r[backend], r[backend + "_none"]
    g64, g32 = r["g64"], r["g32"]
    assert torch.isfinite(got).all() and torch.equal(emb, emb0)   # the switch does not touch the forward
    e_ref, e = fg.dist(g32.numpy(), g64.numpy()), fg.dist(got.numpy(), g64.numpy())
    moved = fg.dist(got.numpy(), const.numpy())
    label = f"{cfgname} {frames} frames {backend}"
    parity.record(f"style grad with features {label} [host fp32 vs f64]", g32, g64)
    parity.record(f"style grad with features {label} [under test vs f64]", got, g64)
    parity.note(f"style grad with features {label}", e_ref=e_ref, e=e, feature_path_share=moved)
    print(f"style grad with features {label}: host fp32 {e_ref:.3e}, under test {e:.3e}; distance from the gradient with constant "
          f"features {moved:.3e}")
    assert e <= 2.0 * e_ref
    assert moved > 2.0 * e_ref   # the feature path is in the gradient: this fails without the feature
    assert fg.dist(const.numpy(), g64.numpy()) > 2.0 * e_ref
    if backend == "hip":
        assert torch.equal(r["hip_again"][1], got)


def test_switch_off_keeps_todays_behaviour():
    from mst_amd.mixing_utils import deferred_features
    cfg = fr.CASES["default"]
    model = model_with("default", 42)
    assert model.feature_grad_backend == "none"
    x, _ = e2e_inputs(cfg, 24)
    xg = x.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="mixing_features requires grad"):
        model(as_stems(xg), torch.zeros(2, 64, device="cuda").requires_grad_(True))
    pre = model.audio_encoder.mel_preprocessor
    lm, feats = pre.forward_with_grad(as_stems(xg), pre.plan(0), True)
    assert lm.grad_fn is not None and feats.grad_fn is None and not feats.requires_grad
    model.feature_grad_backend = "cuda"
    try:
        with pytest.raises(ValueError, match="feature_grad_backend"):
            model(as_stems(xg), deferred_features(64).expand(2, 64).cuda())
    finally:
        model.feature_grad_backend = "none"


def test_features_with_history_from_the_caller():
    """Features the caller extracted with `grad_backend="hip"` keep their history through the frozen HIP trunk: the same
    gradient as the deferred rows filled from the encoder's own launch, up to the separate adjoint passes' rounding."""
    from mst_amd.mixing_utils import MixingFeatureExtractor
    cfg = fr.CASES["default"]
    model = model_with("default", 42)
    x, target = e2e_inputs(cfg, 24)
    ext = MixingFeatureExtractor(44100, cfg["n_fft"], cfg["hop_length"], cfg["n_mels"])
    ext.grad_backend = "hip"
    model.feature_grad_backend = "hip"
    try:
        xg = x.cuda().requires_grad_(True)
        feats = ext.extract_all_features(as_stems(xg))
        assert feats.grad_fn is not None
        style_loss(model(as_stems(xg), feats), target.cuda()).backward()
        torch.cuda.synchronize()
    finally:
        model.feature_grad_backend = "none"
    fused = e2e("default", 24)["hip"][1]
    assert fg.dist(xg.grad.cpu().numpy(), fused.numpy()) <= 2e-6   # (eps32 * log2(n_fft) * 3 transforms: test_feature_grad_gpu.py)


@pytest.mark.parametrize("style_encoder", ["hip", "torch"])
def test_example_trains_with_differentiated_features(style_encoder):
    import contextlib
    import io
    import os
    import sys
    sys.path.insert(0, os.path.join(cases.ROOT, "examples"))
    import train_tcn_mixer

    def run(*extra):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            train_tcn_mixer.main(["--steps", "3", "--seconds", "0.5", "--batch-size", "2", "--style-weight", "1", "--style-encoder",
                                  style_encoder, *extra])
        lines = [l for l in out.getvalue().splitlines() if l.startswith("step")]
        return lines, [float(l.split("loss")[1].split()[0]) for l in lines]
    lines, grad = run("--style-features", "grad")
    _, const = run("--style-features", "const")
    _, default = run()
    assert len(grad) == 3 and all(l == l and abs(l) < 1e6 for l in grad) and all("style" in l for l in lines)
    if style_encoder == "hip":       # (every kernel of this step has a fixed summation order; the library trunk need not)
        assert const == default      # the default is the loop as it was
        assert grad[0] == const[0]   # the same first forward
    assert grad[1:] != const[1:]     # another gradient


def test_refusals_name_the_reason():
    from mst_amd.mixing_utils import deferred_features
    from mst_amd.model import MixingStyleEncoder
    cfg = fr.CASES["default"]
    x, _ = e2e_inputs(cfg, 24)
    deferred = deferred_features(64).expand(2, 64).cuda()
    torch.manual_seed(1)
    m = MixingStyleEncoder(embed_dim=64, feature_dim=64, encoder_backend="torch").cuda()
    for q in m.parameters():
        q.requires_grad_(False)
    m.feature_grad_backend = "hip"
    with pytest.raises(RuntimeError, match=r"training mode.*model\.eval\(\)"):
        m.train()(as_stems(x.cuda().requires_grad_(True)), deferred)
    m.eval()
    with pytest.raises(RuntimeError, match="float64"):
        m(as_stems(x.cuda().double().requires_grad_(True)), deferred)
    with pytest.raises(RuntimeError, match=r"T > n_fft/2 = 512"):
        m(as_stems(x[..., :512].cuda().requires_grad_(True)), deferred)
    torch.manual_seed(1)
    d = MixingStyleEncoder(embed_dim=64, feature_dim=180, encoder_backend="torch").cuda().eval()
    for q in d.parameters():
        q.requires_grad_(False)
    d.feature_grad_backend = "hip"
    from mst_amd.mixing_utils import deferred_features as dfz
    with pytest.raises(RuntimeError, match="use_detailed_spectral"):
        d(as_stems(x.cuda().requires_grad_(True)), dfz(180).expand(2, 180).cuda())
    h = MixingStyleEncoder(embed_dim=64, feature_dim=64, encoder_backend="hip").cuda().eval()
    for q in h.parameters():
        q.requires_grad_(False)
    h.feature_grad_backend = "hip"   # input_grad_backend stays "none": the HIP trunk has no such path
    lm = torch.randn(2, 8, 128, 40, device="cuda")
    with pytest.raises(RuntimeError, match="input_grad_backend"):
        h.forward_from_logmel(lm, torch.zeros(2, 64, device="cuda").requires_grad_(True))
