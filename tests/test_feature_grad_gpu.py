"""GPU: the gradient of the mixing features to the waveform, `mst_melfeat_backward` (csrc/mrstft.hip), alone and fused with the
log-mel cotangent, and its public switch `MixingFeatureExtractor.grad_backend = "hip"`.

Yardstick: the float64 restatement of the 24 live features (tests/feature_grad_ref.py, validated on the host against the
reference's own autograd by tests/test_feature_grad_cpu.py).  Tolerance, per cotangent group: ||d - ref64|| / ||ref64|| is at
most 2 x the same distance of the REFERENCE's fp32 gradient (tests/golden/feature_grad.npz `<case>.<group>.e_ref`).
Inputs: Gaussian stems with the per-stem amplitudes 0.02 / 0.01 / 0.015 / 0.005 (the masking sigmoids stay unsaturated)."""
import functools
import os

import numpy as np
import pytest
import torch

import cases
import feature_grad_ref as fr
import parity
from oracle import mel as omel

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_grad.npz"))
ALL_GROUPS = list(fr.GROUPS) + ["all"]


@functools.lru_cache(maxsize=None)
def extractor(n_fft, hop, n_mels):
    from mst_amd.mixing_utils import MixingFeatureExtractor
    return MixingFeatureExtractor(44100, n_fft, hop, n_mels)


def stems_of(x, grad=True):
    return {s: x[:, 2 * i:2 * i + 2].contiguous().cuda().requires_grad_(grad) for i, s in enumerate(cases.STEMS)}


def hip_backward(case, x, g, g_logmel=None, feats=None, keep_workspace=False):
    """`mst_melfeat_backward` on x (B, 8, T) CPU with the cotangent g (B, 64); feats default: the forward's own."""
    from mst_amd.mixing_utils import melfeat_backward
    n_fft, hop, n_mels = fr.CASES[case][:3]
    ext = extractor(n_fft, hop, n_mels)
    xc = x.cuda().contiguous()
    if feats is None:
        feats = forward_feats(ext, xc)
    out = melfeat_backward(xc, g.cuda(), feats, None if g_logmel is None else g_logmel.cuda(), n_fft, hop, n_mels,
                           ext._grad_tables(xc.device), keep_workspace)
    torch.cuda.synchronize()
    return out


def forward_feats(ext, xc):
    with torch.no_grad():
        return ext.extract_all_features({s: xc[:, 2 * i:2 * i + 2] for i, s in enumerate(cases.STEMS)})


@functools.lru_cache(maxsize=None)
def ref64(case, group):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    n_fft, hop, n_mels = fr.CASES[case][:3]
    x, g = fr.inputs(case)
    return fr.gradient(x, fr.group_cotangent(g, group), n_fft, hop, n_mels)[1]


@functools.lru_cache(maxsize=None)
def hip_result(case, group):
    x, g = fr.inputs(case)
    return hip_backward(case, x, fr.group_cotangent(g, group)).cpu()


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(fr.CASES))
def test_gradient_per_group_two_times_rule(case):
    """Measured distances: see DESIGN 3.13."""
    x, _ = fr.inputs(case)
    assert np.array_equal(np.array(cases.checksum(x)), GOLD[f"{case}.in_checksum"])
    bad = []
    for grp in ALL_GROUPS:
        got, ref = hip_result(case, grp), ref64(case, grp)
        assert got.shape == x.shape and torch.isfinite(got).all()
        e, e_ref = fr.dist(got.numpy(), ref.numpy()), float(GOLD[f"{case}.{grp}.e_ref"])
        parity.record(f"feature grad {case} {grp} [hip vs f64]", got, ref)
        parity.note(f"feature grad {case} {grp} 2x rule", e_ref=e_ref, e_hip=e, ratio=e / e_ref)
        print(f"feature grad {case} {grp}: reference fp32 {e_ref:.3e}, hip {e:.3e}, ratio {e / e_ref:.2f}")
        idx = GOLD[f"{case}.{grp}.idx"]   # the reference's own fp32 values at the sampled positions: the same function
        assert np.abs(got.numpy().ravel()[idx] - GOLD[f"{case}.{grp}.grad"]).max() <= 1e-4 * np.abs(ref.numpy()).max()
        if not e <= 2.0 * e_ref:
            bad.append((grp, e, e_ref))
    assert not bad, f"{case}: beyond 2 x the reference's fp32 distance: {bad}"


@pytest.mark.parametrize("case", ["t700", "w1500-peaklast"])
def test_entries_outside_the_live_set_change_nothing(case):
    x, g = fr.inputs(case)
    live_only = torch.zeros_like(g)
    live_only[:, fr.LIVE] = g[:, fr.LIVE]
    assert torch.equal(hip_backward(case, x, live_only).cpu(), hip_result(case, "all"))
    dead_only = g - live_only
    assert torch.count_nonzero(hip_backward(case, x, dead_only)) == 0


@pytest.mark.parametrize("case", list(fr.CASES))
def test_crest_spike_lands_on_the_float64_index(case):
    got, ref = hip_result(case, "crest"), ref64(case, "crest")
    x, _ = fr.inputs(case)
    assert torch.equal(got.abs().argmax(dim=-1), ref.abs().argmax(dim=-1))
    assert torch.equal(got.abs().argmax(dim=-1), x.abs().argmax(dim=-1))
    peak = fr.CASES[case][5]
    if peak is not None:
        b, r, t = peak
        assert int(got[b, r].abs().argmax()) == t
        assert torch.sign(got[b, r, t]) == torch.sign(ref[b, r, t])


@pytest.mark.parametrize("case", list(fr.CASES))
def test_masking_decisions_differ_from_float64_only_at_near_ties(case):
    """The kernel's arg-max over the other stems is taken on ITS mel power (the workspace keeps it): S = channel mean."""
    n_fft, hop, n_mels, T, B, _ = fr.CASES[case]
    x, g = fr.inputs(case)
    _, ws = hip_backward(case, x, fr.group_cotangent(g, "masking"), keep_workspace=True)
    F = 1 + T // hop
    P = ws[:B * 8 * n_mels * F * 4].view(torch.float32).reshape(B, 4, 2, n_mels, F).cpu()
    S32 = (P[:, :, 0] + P[:, :, 1]) * 0.5
    S64 = fr.stem_means(x.double(), n_fft, hop, n_mels)
    assert float((S32.double() - S64).abs().max()) <= 1e-5 * float(S64.max())
    a32, _ = fr.masking_decisions(S32)
    a64, gap = fr.masking_decisions(S64)
    differ = a32 != a64
    tau = 4.0 * float((S32.double() - S64).abs().max())
    n, nd = differ.numel(), int(differ.sum())
    worst = float(gap[differ].max()) if nd else 0.0
    parity.note(f"feature grad {case} masking decisions", bins=n, hip_differs=nd, tau=tau, worst_gap=worst)
    print(f"{case}: {n} arg-max decisions, hip differs in {nd}, tau {tau:.3e}, worst float64 gap {worst:.3e}")
    assert worst < tau
    assert nd <= 1e-3 * n
    feats = forward_feats(extractor(n_fft, hop, n_mels), x.cuda()).cpu()
    assert 0.2 < float(feats[:, 30:34].min()) and float(feats[:, 30:34].max()) < 0.9   # unsaturated: the test checks something


# ---- 2. fused with the log-mel cotangent ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logmel_cotangent(case):
    """g_L = g0 (mel + 1e-10) / (mel + c), c = 1e-2 mean(mel): a well-conditioned cotangent (tests/test_logmel_grad_gpu.py)."""
    n_fft, hop, n_mels = fr.CASES[case][:3]
    x, _ = fr.inputs(case)
    mel = omel.mel_power(x.double(), n_fft=n_fft, hop=hop, n_mels=n_mels)
    g0 = torch.randn(mel.shape, generator=cases._g(7800 + list(fr.CASES).index(case)))
    return (g0.double() * (mel + 1e-10) / (mel + 1e-2 * mel.mean())).float()


def logmel_backward_alone(case, x, gl):
    from mst_amd.model import MelSpectrogramPreprocessor
    n_fft, hop, n_mels = fr.CASES[case][:3]
    st = stems_of(x)
    MelSpectrogramPreprocessor(44100, n_fft, hop, n_mels)(st).backward(gl.cuda())
    torch.cuda.synchronize()
    return torch.cat([st[s].grad for s in cases.STEMS], dim=1).cpu()


@pytest.mark.parametrize("case", ["t4097", "w1500-peaklast", "hop8", "hop2"])
def test_fused_pass_is_the_sum_of_the_two_passes(case):
    """One adjoint pass with w = g_L / (mel + 1e-10) + g_P against the two separate calls.  The two evaluations differ by
    fp32 rounding of three length-n transforms each: eps32 * log2(2048) * 3 = 2e-6 norm-wise bounds their distance."""
    x, g = fr.inputs(case)
    gl = logmel_cotangent(case)
    feat_part, lm_part = hip_result(case, "all"), logmel_backward_alone(case, x, gl)
    fused = hip_backward(case, x, g, gl).cpu()
    d = fr.dist(fused.numpy(), (feat_part.double() + lm_part.double()).numpy())
    print(f"fused {case}: distance from the sum of the two passes {d:.3e}; |feature part| / |log-mel part| = "
          f"{float(feat_part.norm() / lm_part.norm()):.3e}")
    assert d <= 2e-6
    assert fr.dist(fused.numpy(), lm_part.numpy()) > 1e-3 and fr.dist(fused.numpy(), feat_part.numpy()) > 1e-3   # both parts are in it
    assert torch.equal(fused, hip_backward(case, x, g, gl).cpu())   # twice: the same bits


@pytest.mark.parametrize("case", ["t4097", "w1500-peaklast"])
def test_clip_alone_is_bit_equal_to_clip_in_batch(case):
    x, g = fr.inputs(case)
    gl = logmel_cotangent(case)
    assert x.shape[0] == 3
    both_f, both = hip_backward(case, x, g, gl).cpu(), hip_result(case, "all")
    assert torch.equal(both, hip_backward(case, x, g).cpu())
    for b in (0, 2):
        assert torch.equal(hip_backward(case, x[b:b + 1], g[b:b + 1]).cpu()[0], both[b])
        assert torch.equal(hip_backward(case, x[b:b + 1], g[b:b + 1], gl[b:b + 1]).cpu()[0], both_f[b])


# ---- 3. masks -------------------------------------------------------------------------------------------------------------
def test_a_clamped_feature_passes_no_gradient():
    case = "t700"
    x, g = fr.inputs(case)
    big = x.clone()
    big[:, 0:2] *= 6000.0   # vocals rms ~ 120: clamped to 100
    feats = forward_feats(extractor(1024, 256, 128), big.cuda()).cpu()
    assert feats[0, 49] == 100.0 and feats[0, 50] == 100.0
    got = hip_backward(case, big, fr.group_cotangent(g, "rms")).cpu()
    assert torch.count_nonzero(got[:, 0:2]) == 0 and torch.count_nonzero(got[:, 2:4]) > 0
    ref = fr.gradient(big, fr.group_cotangent(g, "rms"), 1024, 256, 128)[1]
    assert fr.dist(got.numpy(), ref.numpy()) <= 2.0 * float(GOLD[f"{case}.rms.e_ref"])


@pytest.mark.parametrize("case", ["t700", "hop2"])
def test_a_silent_stem_gives_finite_gradients(case):
    """The reference: NaN on the silent rows (sqrt'(0) 0).  Here: exact zeros from the silent stem's own rms / crest / loudness
    terms; the other stems as the float64 restatement with that stem's terms taken out, within 2 x the same restatement's fp32
    distance (the reference itself has no finite gradient to measure)."""
    n_fft, hop, n_mels = fr.CASES[case][:3]
    x, g = fr.inputs(case)
    sil = x.clone()
    sil[:, 4:6] = 0.0   # drums
    for grp in ("rms", "crest"):
        got = hip_backward(case, sil, fr.group_cotangent(g, grp)).cpu()
        assert torch.isfinite(got).all() and torch.count_nonzero(got[:, 4:6]) == 0 and torch.count_nonzero(got[:, 0:4]) > 0
    got = hip_backward(case, sil, g).cpu()
    assert torch.isfinite(got).all()
    _, r64 = fr.gradient(sil, g, n_fft, hop, n_mels, torch.float64, without_stems=(2,))
    _, r32 = fr.gradient(sil, g, n_fft, hop, n_mels, torch.float32, without_stems=(2,))
    others = [0, 1, 2, 3, 6, 7]
    e, e_ref = fr.dist(got[:, others].numpy(), r64[:, others].numpy()), fr.dist(r32[:, others].numpy(), r64[:, others].numpy())
    print(f"silent drums {case}: fp32 restatement {e_ref:.3e}, hip {e:.3e}")
    assert e <= 2.0 * e_ref
    # the silent rows keep the one term that is finite in the reference too: the mixture's loudness
    assert fr.dist(got[:, 4:6].numpy(), r64[:, 4:6].numpy()) <= 2.0 * max(fr.dist(r32[:, 4:6].numpy(), r64[:, 4:6].numpy()), 6e-8)


# ---- the public switch ----------------------------------------------------------------------------------------------------
def test_extractor_grad_backend():
    from mst_amd.mixing_utils import MixingFeatureExtractor
    case = "t4097"
    x, g = fr.inputs(case)
    ext = MixingFeatureExtractor()
    assert ext.grad_backend == "none"
    st = stems_of(x)
    plain = ext.extract_all_features(st)
    assert plain.grad_fn is None and not plain.requires_grad          # today's behaviour
    ext.grad_backend = "hip"
    f = ext.extract_all_features(st)
    assert f.grad_fn is not None and torch.equal(f.detach(), plain)
    f.backward(g.cuda())
    got = torch.cat([st[s].grad for s in cases.STEMS], dim=1).cpu()
    assert torch.equal(got, hip_result(case, "all"))
    one = {s: x[1, 2 * i:2 * i + 2].contiguous().cuda().requires_grad_(True) for i, s in enumerate(cases.STEMS)}   # (2, T): the reference's call
    f1 = ext.extract_all_features(one)
    assert f1.shape == (64,) and f1.grad_fn is not None
    f1.backward(g[1].cuda())
    assert torch.equal(torch.cat([one[s].grad for s in cases.STEMS], dim=0).cpu(), got[1])
    with torch.no_grad():
        assert ext.extract_all_features(st).grad_fn is None
    assert ext.extract_all_features(stems_of(x, grad=False)).grad_fn is None
    ext.grad_backend = "cuda"
    with pytest.raises(ValueError, match="grad_backend"):
        ext.extract_all_features(st)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason():
    from mst_amd import _lib
    from mst_amd.mixing_utils import MixingFeatureExtractor
    x, g = fr.inputs("t4097")

    def ext(**kw):
        e = MixingFeatureExtractor(**kw)
        e.grad_backend = "hip"
        return e
    with pytest.raises(RuntimeError, match="use_detailed_spectral"):
        ext(use_detailed_spectral=True).extract_all_features(stems_of(x))
    with pytest.raises(RuntimeError, match="CUDA"):
        ext().extract_all_features({s: q.detach().cpu().requires_grad_(True) for s, q in stems_of(x).items()})
    with pytest.raises(RuntimeError, match="float64"):
        ext().extract_all_features({s: q.detach().double().requires_grad_(True) for s, q in stems_of(x).items()})
    with pytest.raises(RuntimeError, match=r"T > n_fft/2 = 512"):
        ext().extract_all_features(stems_of(x[..., :512]))
    with pytest.raises(RuntimeError, match="hop_length=64"):
        ext(hop_length=64).extract_all_features(stems_of(x))
    # the entry point itself
    feats180 = torch.zeros(3, 180, device="cuda")
    with pytest.raises(_lib.MstError, match="detailed-spectral"):
        hip_backward("t4097", x, torch.zeros(3, 180), feats=feats180)
