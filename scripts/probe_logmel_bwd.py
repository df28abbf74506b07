"""Log-mel front end, gradient to the waveform: HIP-event time of the HIP backward (`mst_logmel_backward`, csrc/mrstft.hip,
reached through `MelSpectrogramPreprocessor` under autograd) against PyTorch-ROCm autograd of a `torch.stft`-based log-mel with
the same window and filterbank, alternating in one process so both see the same machine state.

    python scripts/probe_logmel_bwd.py [--out profiles/logmel_bwd_probe.json] [--repeats 3] [--window 0.5]

Per configuration (8 clips x 8 channels x 441 000 samples): ms of the backward alone (the forward graph is built once and
kept; median and spread over repeats of a >= `window` s timed loop) for both sides, the ratio, the forward times for scale,
and the largest difference of the two gradients relative to the largest gradient element."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mst_amd.mixing_utils import STEMS  # noqa: E402
from mst_amd.model import MelSpectrogramPreprocessor  # noqa: E402
from mst_amd.synth import synth_batch  # noqa: E402

CONFIGS = [(1024, 256, 128), (2048, 512, 80)]
B, T = 8, 441000


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


def torch_logmel(x, window, fb, n_fft, hop):
    """(B, 8, T) -> (B, 8, n_mels, frames): torch.stft (center / reflect, one-sided), |X|^2, mel matmul, log(. + 1e-10)."""
    X = torch.stft(x.reshape(-1, x.shape[-1]), n_fft, hop, n_fft, window, center=True, pad_mode="reflect", normalized=False,
                   onesided=True, return_complex=True)
    mel = torch.matmul(X.abs().pow(2.0).transpose(-1, -2), fb).transpose(-1, -2)
    return torch.log(mel + 1e-10).reshape(x.shape[0], x.shape[1], fb.shape[1], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logmel_bwd_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    x0 = synth_batch(B, T).cuda()
    for n_fft, hop, n_mels in CONFIGS:
        pre = MelSpectrogramPreprocessor(44100, n_fft, hop, n_mels).cuda()
        window, fb = pre.mel_transform.spectrogram.window, pre.mel_transform.mel_scale.fb
        x = x0.clone().requires_grad_(True)
        stems = {s: x[:, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}
        lm_hip = pre(stems)
        lm_torch = torch_logmel(x, window, fb, n_fft, hop)
        g = torch.randn(lm_hip.shape, generator=torch.Generator().manual_seed(1)).cuda() * torch.exp(lm_hip.detach()).clamp(max=1.0)
        sides = {"hip": lambda: torch.autograd.grad(lm_hip, x, g, retain_graph=True)[0],
                 "torch": lambda: torch.autograd.grad(lm_torch, x, g, retain_graph=True)[0]}
        fwd = {"hip": lambda: pre({s: q.detach() for s, q in stems.items()}),
               "torch": lambda: torch_logmel(x.detach(), window, fb, n_fft, hop)}
        grads = {k: f() for k, f in sides.items()}   # warm-up of both
        torch.cuda.synchronize()
        diff = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        del grads
        t = {(k, w): [] for k in sides for w in ("bwd", "fwd")}
        for _ in range(a.repeats):
            for k in sides:
                t[k, "bwd"].append(timed(sides[k], a.window))
                t[k, "fwd"].append(timed(fwd[k], a.window))
        row = dict(B=B, C=8, T=T, n_fft=n_fft, hop=hop, n_mels=n_mels, frames=lm_hip.shape[-1], max_diff_over_max_grad=diff)
        for (k, w), v in t.items():
            row[f"{k}_{w}_ms"] = med(v)
            row[f"{k}_{w}_ms_repeats"] = v
            row[f"{k}_{w}_spread"] = (max(v) - min(v)) / med(v)
        row["torch_over_hip_bwd"] = row["torch_bwd_ms"] / row["hip_bwd_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del lm_hip, lm_torch, x, stems, g, sides, fwd
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"), configs=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
