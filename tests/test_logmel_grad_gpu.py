"""GPU: the waveform gradient of the log-mel front end (`MelSpectrogramPreprocessor` under autograd -> `mst_logmel_backward`).

Yardstick: `oracle.mel.logmel` under float64 autograd on the host; "the reference's own arithmetic" is the same function under
fp32 autograd.  Tolerance: cases_tcn.TwoTimesRule on the WHOLE gradient (element-wise with the 1 %-of-max floor within
2 x the reference's own worst, norm-wise within 1e-4).

The raw derivative 1 / (mel + 1e-10) is ill-conditioned on single-bin mel filters (the reference's own fp32 gradient lies
between 6e-7 and 1.3e-4 norm-wise from float64 depending on the seed), so the cotangent is g = g0 (mel + 1e-10) / (mel + c)
with g0 ~ N(0, 1) and c = 1e-2 mean(mel) from the float64 reference, rounded to fp32 once; the identical g goes to all
three evaluations (the backward is linear in g: any g is a legitimate test).  Each case asserts as a precondition that its
e_ref is below 1e-4, so an ill-conditioned draw cannot widen the allowance unnoticed."""
import functools

import numpy as np
import pytest
import torch

import cases
import cases_tcn as ct
from mst_amd.model import MelSpectrogramPreprocessor
from oracle import mel as omel

pytestmark = pytest.mark.gpu

B = 2
# name -> n_fft, hop, n_mels, T, noise std
CASES = {
    "min": (1024, 256, 128, 513, 0.3),        # shortest legal clip: both reflections overlap nearly the whole signal; 3 frames
    "odd": (1024, 256, 128, 2085, 0.3),       # T no multiple of hop, 9 frames
    "span": (1024, 256, 128, 20000, 0.3),     # crosses the 64-chunk workgroup boundary: halo frames, ring wrap
    "quiet": (1024, 256, 128, 2085, 1e-3),    # log-mel around -5 .. -23: where exp(-logmel) of a saved output would be least exact
    "2048": (2048, 512, 80, 40000, 0.3),      # the decimation step; crosses the span boundary at this hop
    "2048-min": (2048, 512, 256, 1025, 0.3),  # shortest clip, widest filterbank
}


def _cap_threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x (B, 8, T) fp32 with clip 1 channel 3 all zeros, g (B, 8, n_mels, F) fp32, gradients of the oracle in fp32 and float64):
    computed once, shared, never modified."""
    _cap_threads()
    n_fft, hop, n_mels, T, std = CASES[case]
    seed = 9100 + list(CASES).index(case)
    x = std * torch.randn(B, 8, T, generator=cases._g(seed))
    x[1, 3] = 0.0
    kw = dict(n_fft=n_fft, hop=hop, n_mels=n_mels)
    x64 = x.double().requires_grad_(True)
    mel64 = omel.mel_power(x64, **kw)
    c = float(np.float32(1e-2 * mel64.detach().mean().item()))
    g0 = torch.randn(mel64.shape, generator=cases._g(seed + 50))
    g = (g0.double() * (mel64.detach() + 1e-10) / (mel64.detach() + c)).float()
    g64, = torch.autograd.grad(torch.log(mel64 + 1e-10), x64, g.double())
    x32 = x.clone().requires_grad_(True)
    g32, = torch.autograd.grad(omel.logmel(x32, **kw), x32, g)
    return x, g, g32.numpy(), g64.numpy()


def pre_for(case):
    n_fft, hop, n_mels, _, _ = CASES[case]
    return MelSpectrogramPreprocessor(44100, n_fft, hop, n_mels)


def stems_of(x, grad=cases.STEMS):
    """{stem: (B, 2, T) CUDA leaf}; the stems named in `grad` require grad."""
    return {s: x[:, 2 * i:2 * i + 2].contiguous().cuda().requires_grad_(s in grad) for i, s in enumerate(cases.STEMS)}


def hip_grad(pre, x, g, grad=cases.STEMS):
    """-> (log-mel (B, 8, M, F) CPU, {stem: gradient CPU or None})"""
    st = stems_of(x, grad)
    lm = pre(st)
    assert lm.grad_fn is not None and lm.requires_grad
    lm.backward(g.cuda())
    torch.cuda.synchronize()
    return lm.detach().cpu(), {s: (None if q.grad is None else q.grad.cpu()) for s, q in st.items()}


def cat(grads):
    return torch.cat([grads[s] for s in cases.STEMS], dim=1)


@functools.lru_cache(maxsize=None)
def hip_result(case):
    x, g, _, _ = inputs(case)
    lm, grads = hip_grad(pre_for(case), x, g)
    return lm, cat(grads)


@pytest.mark.parametrize("case", list(CASES))
def test_gradient_two_times_rule(case):
    x, g, g32, g64 = inputs(case)
    _, got = hip_result(case)
    assert got.shape == x.shape and torch.isfinite(got).all()
    rule = ct.TwoTimesRule(f"logmel-grad {case}")
    rule.add("grad_x", got.numpy(), g32, g64)
    e_ref = rule.rows[0][1]
    print(f"logmel-grad {case}: e_ref {e_ref:.3e}, under test {rule.rows[0][2]:.3e}, normwise ref "
          f"{ct.max_rel(g32, g64)[1]:.3e} under test {rule.rows[0][3]:.3e}")
    assert e_ref < 1e-4, f"{case}: ill-conditioned draw, the reference's own fp32 error is {e_ref:.3e}"
    rule.check()


@pytest.mark.parametrize("case", list(CASES))
def test_silent_channel_gets_exactly_zero(case):
    _, _, g32, g64 = inputs(case)
    _, got = hip_result(case)
    assert not g64[1, 3].any() and not g32[1, 3].any()   # (the reference gives exactly 0 there)
    assert torch.count_nonzero(got[1, 3]) == 0
    assert torch.count_nonzero(got[1, 2]) > 0


@pytest.mark.parametrize("case", ["min", "span", "2048"])
def test_backward_twice_is_bit_equal(case):
    x, g, _, _ = inputs(case)
    _, first = hip_result(case)
    _, again = hip_grad(pre_for(case), x, g)
    assert torch.equal(first, cat(again))


@pytest.mark.parametrize("case", ["odd", "span", "2048-min"])
def test_clip_alone_is_bit_equal_to_clip_in_batch(case):
    x, g, _, _ = inputs(case)
    _, both = hip_result(case)
    _, alone = hip_grad(pre_for(case), x[:1], g[:1])
    assert torch.equal(cat(alone), both[:1])


def touched(n_fft, hop, T, f):
    """Samples of the clip that frame f reads, through the reflect padding."""
    t = torch.arange(f * hop - n_fft // 2, f * hop + n_fft // 2)
    t = torch.where(t < 0, -t, torch.where(t >= T, 2 * (T - 1) - t, t))
    mask = torch.zeros(T, dtype=torch.bool)
    mask[t] = True
    return mask


@pytest.mark.parametrize("case,frame", [("span", 0), ("span", 61), ("span", 64), ("span", 78), ("odd", 3), ("2048", 63), ("2048", 78)])
def test_one_frame_cotangent_stays_inside_its_frame(case, frame):
    n_fft, hop, _, T, _ = CASES[case]
    x, g, _, _ = inputs(case)
    assert frame < g.shape[-1]
    g1 = torch.zeros_like(g)
    g1[..., frame] = g[..., frame]
    _, grads = hip_grad(pre_for(case), x, g1)
    got, mask = cat(grads), touched(n_fft, hop, T, frame)
    assert torch.count_nonzero(got[..., ~mask]) == 0
    assert torch.count_nonzero(got[0, 0, mask]) > mask.sum() // 2


def test_only_vocals_requires_grad():
    x, g, _, _ = inputs("odd")
    _, full = hip_result("odd")
    _, grads = hip_grad(pre_for("odd"), x, g, grad=("vocals",))
    assert grads["bass"] is None and grads["drums"] is None and grads["other"] is None
    assert torch.equal(grads["vocals"], full[:, 0:2])


@pytest.mark.parametrize("case", ["odd", "2048-min"])
def test_forward_value_is_the_no_grad_forward(case):
    x, _, _, _ = inputs(case)
    lm, _ = hip_result(case)
    pre = pre_for(case)
    plain = pre(stems_of(x, grad=()))
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(plain.cpu(), lm)
    with torch.no_grad():   # stems that require grad, grad mode off: today's path
        off = pre(stems_of(x))
    assert off.grad_fn is None and torch.equal(off.cpu(), lm)


def test_forward_matches_the_oracle():
    x, _, _, _ = inputs("odd")
    lm, _ = hip_result("odd")
    ref = omel.logmel(x.double(), n_fft=1024, hop=256, n_mels=128)
    live = torch.ones(B, 8, dtype=torch.bool)
    live[1, 3] = False
    assert (lm[live].double() - ref[live]).abs().max() < 1e-3


def test_refusals_name_the_reason():
    x = 0.1 * torch.randn(1, 8, 4096, generator=cases._g(1))
    with pytest.raises(RuntimeError, match="hop_length=64"):
        MelSpectrogramPreprocessor(44100, 1024, 64, 128)(stems_of(x))
    with pytest.raises(RuntimeError, match=r"T > n_fft/2 = 512"):
        MelSpectrogramPreprocessor()(stems_of(x[..., :512]))
    with pytest.raises(RuntimeError, match="float64"):
        MelSpectrogramPreprocessor()({s: q.detach().double().requires_grad_(True) for s, q in stems_of(x).items()})


def test_wider_filterbank_is_refused_not_truncated():
    pre = MelSpectrogramPreprocessor()
    fb = pre.mel_transform.mel_scale.fb
    fb[100] = 0
    fb[100, 40:43] = torch.tensor([0.25, 0.5, 0.125])
    x = 0.1 * torch.randn(1, 8, 4096, generator=cases._g(2))
    lm = pre(stems_of(x))
    with pytest.raises(RuntimeError, match="widest band has 3"):
        lm.backward(torch.ones_like(lm))
