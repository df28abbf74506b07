"""CPU: the float64 restatement of the mixing features' gradient (tests/feature_grad_ref.py) against the fixture the
reference's own MixingFeatureExtractor wrote under autograd (tests/golden/feature_grad.npz), and the ABI of the new entry
points."""
import os

import numpy as np
import pytest
import torch

import cases
import feature_grad_ref as fr

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_grad.npz"))
ISSUE_LIVE = [0, 1, 2, 3, 6, 15, 16, 17, 18, 21, 30, 31, 32, 33, 34, 35, 36, 37, 40, 49, 50, 51, 52, 55]


def test_live_set_is_the_24_of_the_reference():
    assert fr.LIVE == ISSUE_LIVE == GOLD["live"].tolist()
    from mst_amd.mixing_utils import LIVE_FEATURES
    assert list(LIVE_FEATURES) == ISSUE_LIVE
    # the restatement's own Jacobian: exactly these rows are non-zero
    x, _ = fr.inputs("t700")
    xx = x.double().requires_grad_(True)
    f = fr.features(xx, 1024, 256, 128)
    live = []
    for k in range(64):
        gk, = torch.autograd.grad(f[0, k], xx, retain_graph=True, allow_unused=True)
        if gk is not None and bool((gk != 0).any()):
            live.append(k)
    assert live == ISSUE_LIVE


@pytest.mark.parametrize("case", list(fr.CASES))
def test_inputs_are_the_fixtures(case):
    x, g = fr.inputs(case)
    assert np.array_equal(np.array(cases.checksum(x)), GOLD[f"{case}.in_checksum"])
    assert np.array_equal(g.numpy(), GOLD[f"{case}.cotangent"])
    _, _, _, T, B, peak = fr.CASES[case]
    if peak is not None:
        b, r, t = peak
        assert int(x[b, r].abs().argmax()) == t and t in (0, T - 1)


@pytest.mark.parametrize("case", ["t700", "w1500-peaklast", "hop8"])
def test_restatement_fp32_gradient_matches_the_golden(case):
    n_fft, hop, n_mels, _, _, _ = fr.CASES[case]
    x, g = fr.inputs(case)
    for grp in list(fr.GROUPS) + ["all"]:
        gc = fr.group_cotangent(g, grp)
        f32, g32 = fr.gradient(x, gc, n_fft, hop, n_mels, torch.float32)
        _, g64 = fr.gradient(x, gc, n_fft, hop, n_mels, torch.float64)
        ref = GOLD[f"{case}.{grp}.grad"]
        idx = GOLD[f"{case}.{grp}.idx"]
        # two fp32 evaluations of one function: both lie within their own error of float64
        e_gold = float(GOLD[f"{case}.{grp}.e_ref"])
        assert fr.dist(g32.numpy(), g64.numpy()) <= 4 * e_gold + 1e-7, (case, grp)
        scale = np.abs(g64.numpy()).max()
        assert np.abs(g32.numpy().ravel()[idx] - ref).max() <= 2e-5 * scale, (case, grp)
        assert np.abs(g64.numpy().ravel()[idx] - ref).max() <= 2e-5 * scale, (case, grp)
        live = fr.LIVE
        assert np.abs(f32.numpy()[:, live] - GOLD[f"{case}.features"][:, live]).max() <= 1e-4
    if case == "t700":
        assert np.array_equal(x.numpy(), GOLD["t700.x"])
        _, g64 = fr.gradient(x, g, n_fft, hop, n_mels)
        assert fr.dist(GOLD["t700.all.grad_full"], g64.numpy()) == pytest.approx(float(GOLD["t700.all.e_ref"]), rel=1e-6)


def test_crest_spike_sits_on_the_first_maximum():
    for case in ("t6000-peak0", "w1500-peaklast"):
        n_fft, hop, n_mels, T, _, (b, r, t) = fr.CASES[case]
        x, g = fr.inputs(case)
        _, g64 = fr.gradient(x, fr.group_cotangent(g, "crest"), n_fft, hop, n_mels)
        assert int(g64[b, r].abs().argmax()) == t


def test_clamp_and_nan_masks():
    """A clamped feature passes no gradient; a silent channel clamps its crest (log10(0) = -inf -> -100) and gives NaN in the
    reference's rms (sqrt'(0) 0), which the restatement reproduces unless the stem's own terms are taken out."""
    x, g = fr.inputs("t700")
    big = x.clone()
    big[:, 0:2] *= 6000.0            # vocals rms ~ 120 > 100: clamped
    f, gx = fr.gradient(big, fr.group_cotangent(g, "rms"), 1024, 256, 128)
    assert f[0, 49] == 100.0 and f[0, 50] == 100.0
    assert not gx[0, 0:2].any() and gx[0, 2:4].any()
    sil = x.clone()
    sil[:, 4:6] = 0.0                # drums silent
    f, gx = fr.gradient(sil, g, 1024, 256, 128)
    assert f[0, 17] == -100.0 and f[0, 18] == -100.0 and f[0, 15] == 0.0
    assert torch.isnan(gx[0, 4:6]).all()
    f2, gx2 = fr.gradient(sil, g, 1024, 256, 128, without_stems=(2,))
    assert torch.isfinite(gx2).all() and torch.equal(f2, f)
    nan_in = x.clone()
    nan_in[0, 0, 5] = float("nan")
    f3 = fr.features(nan_in.double(), 1024, 256, 128)
    assert f3[0, 49] == 0.0 and torch.isfinite(f3).all()   # NaN -> 0, as _flatten_features


def test_abi_of_the_new_entry_points():
    from mst_amd import _lib
    for name in ("mst_melfeat_backward", "mst_melfeat_backward_workspace_bytes", "mst_encoder_frozen_film_grad",
                 "mst_film_input_grad", "mst_film_input_grad_workspace_bytes"):
        assert name in _lib.SYMBOLS
    L = _lib.lib()
    assert L.mst_melfeat_backward_workspace_bytes(2, 4097, 1024, 256, 128) >= 2 * (2 * 8 * 128 * 17 * 4)
    assert L.mst_melfeat_backward_workspace_bytes(2, 512, 1024, 256, 128) == 0    # T <= n_fft / 2
    assert L.mst_melfeat_backward_workspace_bytes(2, 4097, 512, 128, 128) == 0    # n_fft
