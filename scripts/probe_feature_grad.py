"""Gradient through the mixing features: HIP-event times on the workload of the style step (8 clips x 10 s, both real
configurations), alternating the sides in one process so that they see the same machine state.

    python scripts/probe_feature_grad.py [--out profiles/feature_grad_probe.json] [--repeats 5] [--window 0.5] [--stage-a-only]

Per configuration:
  * stage A alone: `mst_melfeat_backward` (the 24 live features' gradient to the stems) against PyTorch-ROCm autograd of a
    plain torch restatement of the same features (torch.stft, the same window and filterbank), backward only; and the
    fused call (log-mel cotangent + feature cotangent, one adjoint pass) against the log-mel backward alone;
  * the frozen style step 1 - cos(encoder(stems), target), forward + backward to the stems, with the feature path
    (`feature_grad_backend="hip"`) and without, on `encoder_backend="hip"` (+ `input_grad_backend="hip"`) and `"torch"`.
Median and range over the repeats of a >= `window` s timed loop each."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mst_amd.mixing_utils import LIVE_FEATURES, STEMS, MixingFeatureExtractor, deferred_features, melfeat_backward  # noqa: E402
from mst_amd.model import MelSpectrogramPreprocessor, MixingStyleEncoder  # noqa: E402
from mst_amd.synth import synth_batch  # noqa: E402

CONFIGS = [dict(n_fft=1024, hop_length=256, n_mels=128, split_size=20, overlap=10, embed_dim=768),
           dict(n_fft=2048, hop_length=512, n_mels=80, split_size=16, overlap=8, embed_dim=512)]
B, T = 8, 441000
OFFS = (49, 0, 15, 34)   # feature blocks of the rows' stems v, b, d, o


def timed(fn, window):
    """ms per call over a loop of >= window seconds (HIP events), after one call to size the loop."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(2, int(window * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def torch_live_features(x, window, fb, n_fft, hop):
    """(B, 8, T) -> (B, 64): the 24 live features with history (zeros elsewhere), plain torch ops."""
    Bn = x.shape[0]
    f = [None] * 64

    def loud(a):
        return -0.691 + 10 * torch.log10(torch.sqrt(torch.mean(a ** 2, dim=(-2, -1))) ** 2 + 1e-10)
    mix = ((x[:, 0:2] + x[:, 2:4]) + x[:, 4:6]) + x[:, 6:8]
    l_mix = loud(mix)
    for i, o in enumerate(OFFS):
        a = x[:, 2 * i:2 * i + 2]
        rms = torch.sqrt(torch.mean(a ** 2, dim=-1))
        crest = 20 * torch.log10(torch.max(torch.abs(a), dim=-1)[0] / (rms + 1e-8))
        f[o], f[o + 1], f[o + 2], f[o + 3], f[o + 6] = rms[:, 0], rms[:, 1], crest[:, 0], crest[:, 1], loud(a) - l_mix
    X = torch.stft(x.reshape(-1, x.shape[-1]), n_fft, hop, n_fft, window, center=True, pad_mode="reflect", normalized=False,
                   onesided=True, return_complex=True)
    mel = torch.matmul(X.abs().pow(2.0).transpose(-1, -2), fb).transpose(-1, -2)
    S = mel.reshape(Bn, 4, 2, *mel.shape[-2:]).mean(dim=2)
    for i in range(4):
        others = torch.stack([S[:, k] for k in range(4) if k != i]).max(dim=0)[0]
        f[30 + i] = torch.sigmoid(others - S[:, i]).mean(dim=(-2, -1))
    zero = torch.zeros(Bn, device=x.device)
    return torch.clamp(torch.stack([zero if q is None else q for q in f], dim=1), -100.0, 100.0)


def stats(v):
    s = sorted(v)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1], repeats_ms=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_grad_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--stage-a-only", action="store_true", help="stage A alone, one call each (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_feature_grad.py measures on the GPU; there is none here")
    rows = []
    x0 = synth_batch(B, T).cuda()
    gen = torch.Generator().manual_seed(1)
    for cfg in CONFIGS:
        n_fft, hop, n_mels = cfg["n_fft"], cfg["hop_length"], cfg["n_mels"]
        row = dict(B=B, T=T, n_fft=n_fft, hop=hop, n_mels=n_mels)
        ext = MixingFeatureExtractor(44100, n_fft, hop, n_mels)
        pre = MelSpectrogramPreprocessor(44100, n_fft, hop, n_mels).cuda()
        tabs = ext._grad_tables(x0.device)
        as_stems = lambda t: {s: t[:, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}  # noqa: E731
        with torch.no_grad():
            feats = ext.extract_all_features(as_stems(x0))
            lm = pre(as_stems(x0))
        g = torch.zeros(B, 64)
        g[:, list(LIVE_FEATURES)] = torch.randn(B, len(LIVE_FEATURES), generator=gen)
        g = g.cuda()
        gl = (torch.randn(lm.shape, generator=gen).cuda() * torch.exp(lm).clamp(max=1.0)).contiguous()
        x = x0.clone().requires_grad_(True)
        f_torch = torch_live_features(x, tabs[0], pre.mel_transform.mel_scale.fb, n_fft, hop)
        lm_hip = pre(as_stems(x))
        sides = {
            "melfeat_backward_hip": lambda: melfeat_backward(x0, g, feats, None, n_fft, hop, n_mels, tabs),
            "melfeat_backward_torch_autograd": lambda: torch.autograd.grad(f_torch, x, g, retain_graph=True)[0],
            "fused_logmel_and_features_hip": lambda: melfeat_backward(x0, g, feats, gl, n_fft, hop, n_mels, tabs),
            "logmel_backward_alone_hip": lambda: torch.autograd.grad(lm_hip, x, gl, retain_graph=True)[0],
        }
        got = {k: fn() for k, fn in sides.items()}   # warm-up of every side
        torch.cuda.synchronize()
        row["max_diff_over_max_grad_hip_vs_torch"] = float((got["melfeat_backward_hip"] - got["melfeat_backward_torch_autograd"]).abs().max()
                                                           / got["melfeat_backward_torch_autograd"].abs().max())
        del got
        if a.stage_a_only:
            continue
        t = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k, fn in sides.items():
                t[k].append(timed(fn, a.window))
        row["stage_a"] = {k: stats(v) for k, v in t.items()}
        row["stage_a"]["torch_over_hip"] = row["stage_a"]["melfeat_backward_torch_autograd"]["median_ms"] / \
            row["stage_a"]["melfeat_backward_hip"]["median_ms"]
        del f_torch, lm_hip, sides
        torch.cuda.empty_cache()
        # the frozen style step
        deferred = deferred_features(64).expand(B, 64).cuda()
        target = F.normalize(torch.randn(B, cfg["embed_dim"], generator=gen), dim=1).cuda()
        step_t = {}
        steps = {}
        for backend in ("hip", "torch"):
            torch.manual_seed(0)
            m = MixingStyleEncoder(feature_dim=64, encoder_backend=backend, **cfg).cuda().eval()
            for q in m.parameters():
                q.requires_grad_(False)
            if backend == "hip":
                m.input_grad_backend = "hip"
            for switch in ("none", "hip"):
                def step(m=m, switch=switch):
                    m.feature_grad_backend = switch
                    xg = x0.detach().requires_grad_(True)
                    emb = m(as_stems(xg), deferred)
                    (1.0 - (F.normalize(emb, dim=1) * target).sum(dim=1)).mean().backward()
                    return xg.grad
                steps[f"{backend}_features_{'grad' if switch == 'hip' else 'const'}"] = step
        for k, fn in steps.items():
            fn()
            step_t[k] = []
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for k, fn in steps.items():
                step_t[k].append(timed(fn, a.window))
        row["style_step_fwd_bwd"] = {k: stats(v) for k, v in step_t.items()}
        for backend in ("hip", "torch"):
            s = row["style_step_fwd_bwd"]
            s[f"{backend}_feature_path_cost_ms"] = s[f"{backend}_features_grad"]["median_ms"] - s[f"{backend}_features_const"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del steps
        torch.cuda.empty_cache()
    if a.stage_a_only:
        return
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"), configs=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
