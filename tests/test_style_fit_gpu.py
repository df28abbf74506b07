"""GPU: the per-pair fit `mst_amd.tcn_mixer.optimize_tcn_style_transfer` -- one clip of 17 640 samples, a small mixer and a small
frozen encoder, 4 steps.  `sync="step"` (the reference's per-step read-back and host-side best tracking) is the yardstick of
`sync="deferred"` (history and best output kept on the device by mst_keep_best): the same kernels, so the same bits."""
import contextlib
import copy
import io
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import cases
from mst_amd.model import MixingStyleEncoder
from mst_amd.synth import synth_batch
from mst_amd.tcn_mixer import STEM_ORDER, TCNMixer, optimize_tcn_style_transfer

pytestmark = pytest.mark.gpu

T, EMBED, STEPS = 17640, 64, 4


def make_encoder(feature_grad=False):
    torch.manual_seed(4711)
    enc = MixingStyleEncoder(n_fft=1024, hop_length=256, n_mels=128, embed_dim=EMBED, feature_dim=64, encoder_backend="hip").cuda().eval()
    for q in enc.parameters():
        q.requires_grad_(False)
    enc.input_grad_backend = "hip"
    if feature_grad:
        enc.feature_grad_backend = "hip"
    return enc


def make_tcn():
    torch.manual_seed(4712)
    return TCNMixer(hidden_channels=8, num_blocks=3, kernel_size=5, use_film=False)


def make_pair():
    x = synth_batch(1, T)[0]
    stems = {s: x[2 * i:2 * i + 2] for i, s in enumerate(STEM_ORDER)}
    target = F.normalize(torch.randn(EMBED, generator=cases._g(4714)), dim=0)
    return stems, target


def fit(tcn, steps=STEPS, enc=None, **kw):
    stems, target = make_pair()
    return optimize_tcn_style_transfer(tcn, stems, target, enc or make_encoder(), None, torch.device("cuda", 0), num_steps=steps,
                                       lr=0.01, verbose=False, **kw)


@pytest.fixture(scope="module")
def runs():
    """The deferred and the per-step run from identical mixers; computed once."""
    base = make_tcn()
    out = {}
    for sync in ("deferred", "step"):
        tcn = copy.deepcopy(base)
        out[sync] = (fit(tcn, sync=sync), tcn)
    return out


def test_deferred_equals_per_step(runs):
    (d, tcn_d), (s, tcn_s) = runs["deferred"], runs["step"]
    assert set(d) == set(s) == {"processed_stems", "processed_mixture", "distances", "final_distance", "converged"}
    assert len(d["distances"]) == STEPS and all(isinstance(v, float) and v == v for v in d["distances"])
    print("distances:", d["distances"])
    assert d["distances"] == s["distances"]
    assert d["final_distance"] == s["final_distance"] == min(d["distances"]) and d["converged"] == s["converged"]
    for k in STEM_ORDER:
        assert d["processed_stems"][k].shape == (2, T) and not d["processed_stems"][k].is_cuda
        assert torch.equal(d["processed_stems"][k], s["processed_stems"][k])
    assert torch.equal(d["processed_mixture"], s["processed_mixture"])
    sd_d, sd_s = tcn_d.state_dict(), tcn_s.state_dict()
    assert all(torch.equal(sd_d[k], sd_s[k]) for k in sd_d)
    assert not all(torch.equal(v.cpu(), make_tcn().state_dict()[k]) for k, v in sd_d.items())   # (the fit moved them)
    assert len(set(d["distances"])) > 1


def test_best_output_is_the_first_minimum_and_the_mixture_is_the_sum(runs):
    out, _ = runs["deferred"]
    k = out["distances"].index(min(out["distances"]))
    # a fifth, separate forward of the parameters as they were BEFORE update k: a fit of k steps leaves exactly those behind
    tcn = make_tcn()
    if k > 0:
        assert fit(tcn, steps=k)["distances"] == out["distances"][:k]
    tcn = tcn.cuda().train()
    tcn.backend = "hip-train"
    stems, _ = make_pair()
    x = torch.cat([stems[s] for s in STEM_ORDER], dim=0).unsqueeze(0).cuda()
    with torch.no_grad():
        y = tcn(x)[0].cpu()
    for i, s in enumerate(STEM_ORDER):
        assert torch.equal(out["processed_stems"][s], y[2 * i:2 * i + 2]), (s, k)
    assert torch.equal(out["processed_mixture"], sum(out["processed_stems"][s] for s in STEM_ORDER))


def test_feature_gradient_and_sgd():
    out = fit(make_tcn(), enc=make_encoder(feature_grad=True), optimizer="sgd")
    assert len(out["distances"]) == STEPS and all(v == v and 0.0 <= v <= 2.0 for v in out["distances"])
    assert out["final_distance"] == min(out["distances"])
    out = fit(make_tcn(), steps=2, optimizer="adamw")
    assert len(out["distances"]) == 2 and out["final_distance"] == min(out["distances"])


def _example(name):
    sys.path.insert(0, os.path.join(cases.ROOT, "examples"))
    return __import__(name)


def test_fit_example_runs():
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = _example("fit_style_pair").main(["--steps", "3"])
    assert len(res["distances"]) == 3 and "distance to the target" in out.getvalue()


def test_training_example_with_the_hip_optimiser_repeats_itself():
    def run():
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            _example("train_tcn_mixer").main(["--optimizer", "hip", "--steps", "3", "--seconds", "0.4"])
        lines = [l for l in out.getvalue().splitlines() if l.startswith("step")]
        return lines, [float(l.split("loss")[1].split()[0]) for l in lines]
    lines1, losses1 = run()
    lines2, _ = run()
    assert len(losses1) == 3 and all(l == l and abs(l) < 1e6 for l in losses1)
    assert lines1 == lines2
