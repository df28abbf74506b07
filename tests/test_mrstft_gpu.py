"""GPU: MultiResolutionSTFTLoss(backend="hip") -- `mst_mrstft_forward/backward` -- against float64.

The float64 yardstick and the reference's own fp32 result are backend="torch" on the host CPUs (tests/test_mrstft_cpu.py
pins that restatement to the reference's fixture); every quantity is compared on WHOLE gradients.

What the gradient is held to (measured with the reference before the kernels existed):
  * the loss and its six components are well-conditioned: 1e-4 relative, the project's bar;
  * the spectral-convergence gradient is smooth: cases_tcn.TwoTimesRule, every element;
  * the log-magnitude gradient at the reference's floor of 1e-5 is NOT (bins with xm of 1e-6 .. 1e-3 carry weights up to
    1e5 x a typical bin's, their phase is rounding noise, sign() flips where xm ~ ym): the reference's own fp32 gradient is
    5e-4 .. 3e-3 (l2) from float64, and a second honest fp32 evaluation lay at 0.36x .. 2.9x of that.  So: the l2 distance
    pooled over all cases at most 4x the reference's, and per case at most 10x that case's reference value."""
import functools

import numpy as np
import pytest
import torch

import cases  # noqa: F401
import cases_mrstft as cm
import cases_tcn as ct
import parity
from mst_amd.loss import MultiResolutionSTFTLoss

pytestmark = pytest.mark.gpu


def _cap_threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def torch_eval(x, y, dtype, term="full", **kw):
    """loss, (n, 2) components, whole gradient: backend="torch" on the host CPUs."""
    _cap_threads()
    scw, lw = cm.TERMS[term]
    m = MultiResolutionSTFTLoss(backend="torch", sc_weight=scw, log_weight=lw, **kw)
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    loss = m(xx, y.cpu().to(dtype))
    loss.backward()
    return loss.item(), m.components(xx.detach(), y.cpu().to(dtype)).double().numpy(), xx.grad.double().numpy()


def torch_eval_terms(x, y, dtype):
    """torch_eval for all three terms from ONE forward graph (the contract size: the STFTs are the cost)."""
    _cap_threads()
    m = MultiResolutionSTFTLoss(backend="torch")
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    terms = m._terms_torch(xx, y.cpu().to(dtype))
    n = len(terms)
    sc, lg = sum(t[0] for t in terms) / n, sum(t[1] for t in terms) / n
    total = 0.0
    for a, b in terms:
        total = total + (a + b)
    total = total / n
    comp = torch.stack([torch.stack(t) for t in terms]).detach().double().numpy()
    out = {}
    for name, val in (("full", total), ("sc", sc), ("log", lg)):
        g, = torch.autograd.grad(val, xx, retain_graph=name != "log")
        out[name] = (val.item(), comp, g.double().numpy())
    return out


def hip_eval(x, y, term="full", **kw):
    scw, lw = cm.TERMS[term]
    m = MultiResolutionSTFTLoss(sc_weight=scw, log_weight=lw, **kw)
    xg = x.detach().cuda().requires_grad_(True)
    yg = y.cuda()
    loss = m(xg, yg)
    loss.backward()
    comp = m.components(xg.detach(), yg)
    torch.cuda.synchronize()
    return loss.item(), comp.cpu().double().numpy(), xg.grad.cpu().double().numpy()


@functools.lru_cache(maxsize=None)
def reference(case, term):
    """(fp32, float64) results of backend="torch" for a case of cases_mrstft: computed once, shared, never modified."""
    x, y = cm.inputs(case)
    return torch_eval(x, y, torch.float32, term), torch_eval(x, y, torch.float64, term)


@functools.lru_cache(maxsize=None)
def kernels(case, term):
    x, y = cm.inputs(case)
    return hip_eval(x, y, term)


def rel(a, b):
    return abs(a - b) / abs(b)


def check_loss_bar(name, got, ref32, ref64):
    """Bar 1: total and every component within 1e-4 relative of float64; the reference's own fp32 distance next to it."""
    (l, c, _), (l32, c32, _), (l64, c64, _) = got, ref32, ref64
    e = max(rel(l, l64), float((np.abs(c - c64) / np.abs(c64)).max()))
    e32 = max(rel(l32, l64), float((np.abs(c32 - c64) / np.abs(c64)).max()))
    parity.note(f"mrstft {name} loss+components", hip_vs_f64=e, ref_fp32_vs_f64=e32)
    print(f"mrstft {name}: loss and components: under test {e:.3e}, reference fp32 {e32:.3e}")
    assert np.isfinite(l) and np.isfinite(c).all()
    assert e <= 1e-4, (name, e, l, l64, c, c64)


def check_sc_bar(name, g, g32, g64):
    """Bar 2: the spectral-convergence gradient, every element, under the rule of the TCN tests."""
    rule = ct.TwoTimesRule(f"mrstft {name}")
    rule.add("grad sc", g, g32, g64)
    rule.check()


def dist(g, g64):
    return cm.l2(g - g64)


@pytest.mark.parametrize("case", cm.case_ids())
def test_loss_and_components(case):
    ref32, ref64 = reference(case, "full")
    check_loss_bar(case, kernels(case, "full"), ref32, ref64)
    for term in ("sc", "log"):   # the weighted totals
        l, l64 = kernels(case, term)[0], reference(case, term)[1][0]
        assert rel(l, l64) <= 1e-4, (term, l, l64)


@pytest.mark.parametrize("case", cm.case_ids())
def test_spectral_convergence_gradient_every_element(case):
    ref32, ref64 = reference(case, "sc")
    g = kernels(case, "sc")[2]
    assert g.shape == ref64[2].shape and np.isfinite(g).all()
    check_sc_bar(case, g, ref32[2], ref64[2])


@pytest.mark.parametrize("term", ["log", "full"])
def test_log_and_full_gradient_pooled_l2(term):
    num_k = num_r = den = 0.0
    worst = 0.0
    for case in cm.case_ids():
        ref32, ref64 = reference(case, term)
        g, g32, g64 = kernels(case, term)[2], ref32[2], ref64[2]
        assert np.isfinite(g).all()
        dk, dr, n = dist(g, g64), dist(g32, g64), cm.l2(g64)
        parity.record(f"mrstft {case} grad {term} [ref fp32 vs f64]", g32, g64)
        parity.record(f"mrstft {case} grad {term} [hip vs f64]", g, g64)
        print(f"mrstft {case} grad {term}: l2 distance from float64: under test {dk / n:.3e}, reference fp32 {dr / n:.3e}, "
              f"ratio {dk / dr:.2f}")
        worst = max(worst, dk / dr)
        num_k, num_r, den = num_k + dk * dk, num_r + dr * dr, den + n * n
    pooled_k, pooled_r = np.sqrt(num_k / den), np.sqrt(num_r / den)
    parity.note(f"mrstft grad {term} pooled l2", hip=pooled_k, ref_fp32=pooled_r, ratio=pooled_k / pooled_r, worst_case_ratio=worst)
    print(f"mrstft grad {term}: pooled under test {pooled_k:.3e}, reference fp32 {pooled_r:.3e}, ratio {pooled_k / pooled_r:.2f}, "
          f"worst per-case ratio {worst:.2f}")
    assert pooled_k <= 4 * pooled_r
    assert worst <= 10


# ---- singular points, exact

def _run(x, y, **kw):
    m = MultiResolutionSTFTLoss(**kw)
    xg = x.cuda().requires_grad_(True)
    loss = m(xg, y.cuda())
    loss.backward()
    return loss.detach().cpu(), xg.grad.cpu()


def test_silent_rows_in_both_have_exactly_zero_gradient():
    x, y = cm.make_xy(2, 6000, "near")
    x[:, 2:4] = 0
    y[:, 2:4] = 0
    loss, g = _run(x, y)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    assert (g[:, 2:4] == 0).all()
    assert g[:, :2].abs().sum() > 0 and g[:, 4:].abs().sum() > 0
    check_loss_bar("silent rows 2-3", hip_eval(x, y), torch_eval(x, y, torch.float32), torch_eval(x, y, torch.float64))


def test_identical_inputs_give_exactly_zero():
    _, y = cm.make_xy(2, 6000, "near")
    loss, g = _run(y.clone(), y)
    assert loss.item() == 0.0
    assert (g == 0).all() and not torch.isnan(g).any()


def test_silent_rows_in_the_target_only():
    x, y = cm.make_xy(2, 6000, "near")
    y[:, 2:4] = 0
    loss, g = _run(x, y)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    check_loss_bar("target rows 2-3 silent", hip_eval(x, y), torch_eval(x, y, torch.float32), torch_eval(x, y, torch.float64))


# ---- autograd contract

def test_backward_scales_with_the_incoming_gradient_on_the_device():
    x, y = cm.make_xy(2, 6000, "near")
    m = MultiResolutionSTFTLoss()
    xg, yg = x.cuda().requires_grad_(True), y.cuda()
    m(xg, yg).backward()
    g1 = xg.grad.clone()
    xg.grad = None
    (3.5 * m(xg, yg)).backward()
    g35 = xg.grad.clone()
    ulp = torch.maximum((3.5 * g1).abs(), g35.abs()) * 2.0 ** -23
    assert ((g35 - 3.5 * g1).abs() <= ulp).all()
    assert g1.abs().sum() > 0


def test_bit_reproducible_and_second_backward_on_a_fresh_graph():
    x, y = cm.inputs("t44100_near")
    m = MultiResolutionSTFTLoss()
    yg = y.cuda()
    runs = []
    for _ in range(3):
        xg = x.cuda().requires_grad_(True)
        loss = m(xg, yg)
        loss.backward()
        runs.append((loss.detach().clone(), xg.grad.clone()))
    for loss, g in runs[1:]:
        assert torch.equal(loss, runs[0][0])
        assert torch.equal(g, runs[0][1])


def test_forward_only_without_requires_grad():
    x, y = cm.make_xy(2, 6000, "near")
    xg = x.cuda()
    loss = MultiResolutionSTFTLoss()(xg, y.cuda())
    assert not loss.requires_grad and loss.grad_fn is None and xg.grad is None
    with torch.no_grad():
        l2 = MultiResolutionSTFTLoss()(x.cuda().requires_grad_(True), y.cuda())
    assert torch.equal(loss, l2)


def test_2d_input_equals_3d_bit_for_bit():
    x, y = cm.inputs("2d4096_near")
    l2d, g2d = _run(x, y)
    l3d, g3d = _run(x[None], y[None])
    assert l2d.dim() == 0 and g2d.shape == x.shape and g3d.shape == (1,) + tuple(x.shape)
    assert torch.equal(l2d, l3d) and torch.equal(g2d, g3d[0])


# ---- resolutions

@pytest.mark.parametrize("name,kw", [
    ("single 512/128", dict(fft_sizes=[512], hop_sizes=[128], win_sizes=[512])),
    ("hop n/2", dict(fft_sizes=[1024, 2048, 512], hop_sizes=[512, 1024, 256], win_sizes=[1024, 2048, 512])),
    ("hop n/8", dict(fft_sizes=[1024, 2048, 512], hop_sizes=[128, 256, 64], win_sizes=[1024, 2048, 512])),
    ("four", dict(fft_sizes=[2048, 1024, 512, 1024], hop_sizes=[512, 128, 256, 512], win_sizes=[2048, 1024, 512, 1024])),
])
def test_resolution_lists(name, kw):
    x, y = cm.make_xy(2, 6000, "far")
    check_loss_bar(name, hip_eval(x, y, **kw), torch_eval(x, y, torch.float32, **kw), torch_eval(x, y, torch.float64, **kw))
    check_sc_bar(name, hip_eval(x, y, "sc", **kw)[2], torch_eval(x, y, torch.float32, "sc", **kw)[2],
                 torch_eval(x, y, torch.float64, "sc", **kw)[2])


# ---- contract size

def test_contract_size():
    """2 x 8 x 441 000 (10 s clips), "near": bars 1 and 2 and the per-case limit of bar 3, against backend="torch" in fp32 and
    float64 on the host."""
    x, y = cm.make_xy(2, 441000, "near")
    r32, r64 = torch_eval_terms(x, y, torch.float32), torch_eval_terms(x, y, torch.float64)
    ref = {t: (r32[t], r64[t]) for t in cm.TERMS}
    got = {t: hip_eval(x, y, t) for t in cm.TERMS}
    check_loss_bar("2x8x441000", got["full"], *ref["full"])
    check_sc_bar("2x8x441000", got["sc"][2], ref["sc"][0][2], ref["sc"][1][2])
    for t in ("log", "full"):
        g, g32, g64 = got[t][2], ref[t][0][2], ref[t][1][2]
        dk, dr = dist(g, g64), dist(g32, g64)
        parity.note(f"mrstft 2x8x441000 grad {t} l2", hip=dk / cm.l2(g64), ref_fp32=dr / cm.l2(g64), ratio=dk / dr)
        print(f"mrstft 2x8x441000 grad {t}: under test {dk / cm.l2(g64):.3e}, reference fp32 {dr / cm.l2(g64):.3e}, ratio {dk / dr:.2f}")
        assert np.isfinite(g).all() and dk <= 10 * dr


# ---- the call the trainer makes

def test_cycle_loss_through_the_mixer():
    """loss(tcn(x), x).backward() with TCNMixer(backend="torch") on the GPU: parameter gradients with the HIP loss within 10x
    the torch loss's own fp32 distance from float64, norm-wise per parameter tensor."""
    from mst_amd import tcn_mixer as tm
    c = ct.CASES["st_default"]
    x = cases.pcm_batch(1, 20000).cuda()

    def grads(dtype, backend):
        tcn = tm.TCNMixer(**ct.mixer_kwargs(c))
        tcn.load_state_dict(ct.make_tcn_state_dict(c), strict=True)
        tcn = tcn.to(device="cuda", dtype=dtype).eval()
        gen = tm.TCNFiLMGenerator(embed_dim=ct.EMBED, num_blocks=c["nb"], hidden_channels=c["H"])
        gen.load_state_dict(ct.make_film_state_dict(ct.EMBED, c), strict=True)
        gen = gen.to(device="cuda", dtype=dtype).eval()
        tcn.backend = gen.backend = "torch"
        with torch.no_grad():
            film = gen(ct.embeddings(1, ct.EMBED).cuda().to(dtype))
        loss = MultiResolutionSTFTLoss(backend=backend)(tcn(x.to(dtype), film_params=film), x.to(dtype))
        loss.backward()
        return loss.item(), {k: p.grad.double().cpu() for k, p in tcn.named_parameters()}

    lh, gh = grads(torch.float32, "hip")
    l32, g32 = grads(torch.float32, "torch")
    l64, g64 = grads(torch.float64, "torch")
    assert rel(lh, l64) <= 1e-4
    worst = 0.0
    for k, ref in g64.items():
        assert torch.isfinite(gh[k]).all(), k
        dk, dr = (gh[k] - ref).norm().item(), (g32[k] - ref).norm().item()
        worst = max(worst, dk / dr)
        assert dk <= 10 * dr, (k, dk / ref.norm().item(), dr / ref.norm().item())
    parity.note("mrstft through TCNMixer: parameter gradients", worst_ratio_to_torch_fp32=worst, loss_rel=rel(lh, l64))


def test_example_cycle_flag():
    """examples/style_transfer.py --cycle: the distance input -> target style -> input style, finite and positive."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("style_transfer_example", os.path.join(cases.ROOT, "examples", "style_transfer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--seconds", "1", "--cycle"])
    assert np.isfinite(out["cycle_loss"]) and out["cycle_loss"] > 0
    assert "cycle_loss" not in mod.main(["--seconds", "1"])
