"""The gradient of the mixing features to the stems: a torch restatement of the 24 features that carry one in the reference
(src/mixing_utils.py), with the reference's detach pattern, in any dtype (float64 = the yardstick of the GPU tests), and the
cases / inputs / cotangents the tests and the fixture generator (tests/golden/make_feature_grad_golden.py) share.

Layout of the 64 basic features (keys sorted: bass, drums, masking, other, vocals): per stem block o in {0 bass, 15 drums,
34 other, 49 vocals}: rms L/R (o, o+1), crest L/R (o+2, o+3), loudness twice (o+4, o+5; through `.item()`: no gradient),
rel_loudness (o+6), spectral x5 and stereo x3 (rebuilt with torch.tensor([...]): no gradient); masking 30..33 in the order
vocals, bass, drums, other."""
import functools

import numpy as np
import torch

import cases
from oracle import mel as omel

STEM_OFF = {"vocals": 49, "bass": 0, "drums": 15, "other": 34}
OFFS = [STEM_OFF[s] for s in cases.STEMS]          # in row order v, b, d, o
GROUPS = {
    "rms": sorted(o + k for o in OFFS for k in (0, 1)),
    "crest": sorted(o + k for o in OFFS for k in (2, 3)),
    "rel_loudness": sorted(o + 6 for o in OFFS),
    "masking": [30, 31, 32, 33],
}
LIVE = sorted(i for g in GROUPS.values() for i in g)
AMPS = (0.02, 0.01, 0.015, 0.005)                  # per stem v, b, d, o: the masking sigmoids stay away from saturation

# name -> n_fft, hop, n_mels, T, B, peak ((clip, row, sample) forced to be the row's peak, or None)
CASES = {
    "t700": (1024, 256, 128, 700, 1, None),
    "t4097": (1024, 256, 128, 4097, 3, None),
    "t6000-peak0": (1024, 256, 128, 6000, 1, (0, 3, 0)),
    "w1500-peaklast": (2048, 512, 80, 1500, 3, (1, 6, 1499)),
    "w11003": (2048, 512, 80, 11003, 1, None),
    "hop8": (1024, 128, 128, 4097, 1, None),
    "hop2": (2048, 1024, 80, 1500, 1, None),
}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x (B, 8, T) fp32, g (B, 64) fp32 cotangent ~ N(0, 1)): computed once, shared, never modified."""
    _, _, _, T, B, peak = CASES[case]
    seed = 7700 + list(CASES).index(case)
    x = torch.randn(B, 8, T, generator=cases._g(seed)) * torch.tensor(AMPS).repeat_interleave(2)[None, :, None]
    if peak is not None:
        b, r, t = peak
        x[b, r, t] = -1.5 * x[b, r].abs().max()
    g = torch.randn(B, 64, generator=cases._g(seed + 50))
    return x, g


def group_cotangent(g, group):
    """`g` on the entries of one group (or "all": every one of the 64), zero elsewhere."""
    if group == "all":
        return g.clone()
    out = torch.zeros_like(g)
    out[:, GROUPS[group]] = g[:, GROUPS[group]]
    return out


def _loudness(a):
    rms = torch.sqrt(torch.mean(a ** 2, dim=(-2, -1)))
    return -0.691 + 10 * torch.log10(rms ** 2 + 1e-10)


def stem_means(x, n_fft, hop, n_mels):
    """S (B, 4, n_mels, F): the channel mean of each stem's mel power."""
    mel = omel.mel_power(x, n_fft=n_fft, hop=hop, n_mels=n_mels)
    return mel.reshape(x.shape[0], 4, 2, *mel.shape[-2:]).mean(dim=2)


def masking_decisions(S):
    """arg-max over the other stems (B, 4, n_mels, F) (first maximum in stem order without self, as torch.stack(...).max(0)
    picks) and the gap between the largest and the second largest of the others."""
    args, gaps = [], []
    for i in range(4):
        others = [k for k in range(4) if k != i]
        st = torch.stack([S[:, k] for k in others])
        top = st.topk(2, dim=0).values
        args.append(torch.tensor(others)[st.max(dim=0)[1]])
        gaps.append(top[0] - top[1])
    return torch.stack(args, dim=1), torch.stack(gaps, dim=1)


def features(x, n_fft=1024, hop=256, n_mels=128, without_stems=()):
    """x (B, 8, T) -> (B, 64): the live features with history, zeros elsewhere, clamped and NaN-replaced as
    `_flatten_features` does.  without_stems: stem indices (row order) whose own rms / crest / loudness terms are constants
    (what the kernel computes for a silent stem, where the reference's sqrt'(0) gives NaN)."""
    B = x.shape[0]
    f = [None] * 64
    mix = ((x[:, 0:2] + x[:, 2:4]) + x[:, 4:6]) + x[:, 6:8]
    l_mix = _loudness(mix)
    for i, o in enumerate(OFFS):
        a = x[:, 2 * i:2 * i + 2]
        if i in without_stems:
            a = a.detach()
        rms = torch.sqrt(torch.mean(a ** 2, dim=-1))
        peak = torch.max(torch.abs(a), dim=-1)[0]
        crest = 20 * torch.log10(peak / (rms + 1e-8))
        if i in without_stems:   # (a constant: no NaN from sqrt'(0) 0)
            rms, crest = rms.detach(), crest.detach()
        f[o], f[o + 1], f[o + 2], f[o + 3] = rms[:, 0], rms[:, 1], crest[:, 0], crest[:, 1]
        f[o + 6] = _loudness(a) - l_mix
    S = stem_means(x, n_fft, hop, n_mels)
    for i in range(4):
        others = torch.stack([S[:, k] for k in range(4) if k != i])
        f[30 + i] = torch.sigmoid((0.0 - (S[:, i] - others.max(dim=0)[0])) / 1.0).mean(dim=(-2, -1))
    zero = torch.zeros(B, dtype=x.dtype)
    out = torch.stack([zero if q is None else q for q in f], dim=1)
    out = torch.clamp(out, min=-100.0, max=100.0)
    return torch.where(torch.isnan(out), torch.zeros_like(out), out)


def gradient(x, g, n_fft, hop, n_mels, dtype=torch.float64, without_stems=()):
    """d <g, features(x)> / dx in `dtype` -> (features (B, 64), gradient (B, 8, T)), both detached."""
    xx = x.detach().to(dtype).requires_grad_(True)
    f = features(xx, n_fft, hop, n_mels, without_stems)
    gx, = torch.autograd.grad(f, xx, g.to(dtype))
    return f.detach(), gx.detach()


def dist(a, ref):
    """||a - ref|| / ||ref|| in float64."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))
