"""GPU: the style term of the style-transfer trainer end to end -- 1 - cos(encoder(stems), target) through a frozen
MixingStyleEncoder in eval mode, gradient to the WAVEFORM: stage A forward and backward in HIP (`_LogMelHip`), the conv trunk on
PyTorch-ROCm autograd (`encoder_backend="torch"`)."""
import contextlib
import io
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import cases
from mst_amd.mixing_utils import deferred_features
from mst_amd.model import MixingStyleEncoder

pytestmark = pytest.mark.gpu

B, T, EMBED = 2, 16384 + 300, 64


def make_encoder(backend="torch"):
    torch.manual_seed(4711)
    model = MixingStyleEncoder(embed_dim=EMBED, feature_dim=64, encoder_backend=backend).eval()
    for q in model.parameters():
        q.requires_grad_(False)
    return model


def make_inputs():
    g = cases._g(4713)   # (seeds 4712 and 4715 sit on max-pool kinks: the float64 pipeline itself realises < 0.5 there)
    x = 0.1 * torch.randn(B, 8, T, generator=g)
    target = F.normalize(torch.randn(B, EMBED, generator=g), dim=1)
    feats = torch.rand(B, 64, generator=g) * 2 - 1   # real (not deferred) mixing features: used as given
    return x, target, feats


def style_loss(emb, target):
    return (1.0 - (F.normalize(emb, dim=1) * F.normalize(target, dim=1)).sum(dim=1)).mean()


def as_stems(x):
    return {s: x[:, 2 * i:2 * i + 2] for i, s in enumerate(cases.STEMS)}


@pytest.fixture(scope="module")
def deterministic_convs():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def test_composition_is_trunk_cotangent_through_stage_a(deterministic_convs):
    model = make_encoder().cuda()
    x, target, _ = make_inputs()
    x, target = x.cuda(), target.cuda()
    pre = model.audio_encoder.mel_preprocessor
    deferred = deferred_features(64).expand(B, 64).cuda()
    # the trunk alone, from the HIP forward's log-mel as a leaf
    with torch.no_grad():
        lm, feats = pre.plan(0).forward_stems(as_stems(x), True, True)
    leaf = lm.clone().requires_grad_(True)
    emb_leaf = model.forward_from_logmel(leaf, feats)
    style_loss(emb_leaf, target).backward()
    g = leaf.grad
    assert g is not None and float(g.abs().max()) > 0
    # stage A backward applied to that cotangent directly
    xa = x.clone().requires_grad_(True)
    pre(as_stems(xa)).backward(g)
    # end to end
    xe = x.clone().requires_grad_(True)
    emb = model(as_stems(xe), deferred)
    assert emb.requires_grad
    style_loss(emb, target).backward()
    assert torch.equal(emb.detach(), emb_leaf.detach())
    assert xe.grad is not None and float(xe.grad.abs().max()) > 0
    assert torch.equal(xe.grad, xa.grad)


def test_gradient_step_decreases_the_style_loss():
    """First order: eta with a predicted decrease eta ||grad||^2 of 1e-3 of the loss; the realised decrease is at least half of it
    (the float64 pipeline -- oracle.mel.logmel and the same modules in double on the host -- realises 0.79 of the prediction
    at this seed and eta)."""
    model = make_encoder().cuda()
    x, target, feats = make_inputs()
    x, target, feats = x.cuda(), target.cuda(), feats.cuda()
    xg = x.clone().requires_grad_(True)
    loss = style_loss(model(as_stems(xg), feats), target)
    loss.backward()
    grad = xg.grad
    eta = 1e-3 * loss.item() / float((grad.double() ** 2).sum())
    with torch.no_grad():
        after = style_loss(model(as_stems(x - eta * grad), feats), target)
    predicted, realised = 1e-3 * loss.item(), loss.item() - after.item()
    print(f"style loss {loss.item():.6f} -> {after.item():.6f}: predicted decrease {predicted:.3e}, realised {realised:.3e}")
    assert after.item() < loss.item()
    assert realised >= 0.5 * predicted


def test_hip_backend_raises_and_names_torch():
    model = make_encoder("hip").cuda()
    x, _, feats = make_inputs()
    xg = x.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match='encoder_backend="torch"'):
        model(as_stems(xg), feats.cuda())
    with torch.no_grad():   # grad mode off: the eval path, as before
        assert model(as_stems(xg), feats.cuda()).shape == (B, EMBED)


def _run_example(*extra):
    sys.path.insert(0, os.path.join(cases.ROOT, "examples"))
    import train_tcn_mixer
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        train_tcn_mixer.main(["--steps", "3", "--seconds", "0.5", "--batch-size", "2", *extra])
    lines = [l for l in out.getvalue().splitlines() if l.startswith("step")]
    return lines, [float(l.split("loss")[1].split()[0]) for l in lines]


def test_example_with_and_without_the_style_term():
    lines1, with_style = _run_example("--style-weight", "1")
    lines0, without = _run_example("--style-weight", "0")
    default_lines, default = _run_example()
    assert len(with_style) == len(without) == 3
    assert all(l == l and abs(l) < 1e6 for l in with_style + without)
    assert all("style" in l for l in lines1) and not any("style" in l for l in lines0)
    assert with_style != without
    assert lines0 == default_lines and without == default   # weight 0 is the loop without the term, print for print
