"""Frozen encoder, gradient to the log-mel: HIP-event time of forward + backward of `emb.sum()` through the hand-written path
(`input_grad_backend = "hip"`: `_HipFrozenTrunk` + `_HipHead`) against the same module on PyTorch-ROCm / MIOpen autograd
(`encoder_backend = "torch"`) on the same log-mel, alternating in one process so both see the same machine state.

    python scripts/probe_frozen_grad.py [--out profiles/frozen_grad_probe.json] [--repeats 3] [--window 0.5]

Per configuration (8 clips x 10 s, the style trainer's batch): ms of forward + backward for both sides (median and spread over
repeats of a >= `window` s timed loop), the ratio, the per-section times of one HIP backward (`_HipFrozenTrunk.last_timing`),
the largest difference of the two gradients relative to the largest gradient element (max-pool ties included: the two
sides may pick different arg-maxima in a few windows), and the conv1 input-gradient section's rate as the share of the
157.3 TF/s fp32 matrix peak that its EXECUTED MFMAs (padding half of the N-tile included; counted from the shapes) reach."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mst_amd.model as mm  # noqa: E402
from mst_amd.mixing_utils import STEMS  # noqa: E402
from mst_amd.synth import synth_batch  # noqa: E402

CONFIGS = {
    "default": dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=128, split_size=20, overlap=10, embed_dim=768),
    "baseline_sh": dict(sample_rate=44100, n_fft=2048, hop_length=512, n_mels=80, split_size=16, overlap=8, embed_dim=512),
}
B, T = 8, 441000
PEAK_FP32_MFMA = 157.3e12


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


def frozen(cfg, backend, state_dict=None):
    torch.manual_seed(0)
    m = mm.MixingStyleEncoder(channels=8, feature_dim=64, encoder_backend=backend, **cfg)
    if state_dict is not None:
        m.load_state_dict(state_dict)
    m = m.cuda().eval()
    for q in m.parameters():
        q.requires_grad_(False)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_grad_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    x = synth_batch(B, T).cuda()
    stems = {s: x[:, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}
    feats = 2.0 * torch.randn(B, 64, generator=torch.Generator().manual_seed(1)).cuda()
    for name, cfg in CONFIGS.items():
        hip = frozen(cfg, "hip")
        hip.input_grad_backend = "hip"
        ref = frozen(cfg, "torch", {k: v.cpu() for k, v in hip.state_dict().items()})
        with torch.no_grad():
            lm = hip.audio_encoder.mel_preprocessor(stems)
        frames = lm.shape[-1]

        def step(model):
            leaf = lm.detach().requires_grad_(True)
            model.forward_from_logmel(leaf, feats).sum().backward()
            return leaf.grad
        sides = {"hip": lambda: step(hip), "torch": lambda: step(ref)}
        grads = {k: f() for k, f in sides.items()}   # warm-up of both
        torch.cuda.synchronize()
        diff = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        del grads
        mm._TRAIN_TIMING = True   # backward passes with events between their sections: per-section median of five
        runs = []
        for _ in range(5):
            step(hip)
            runs.append(dict(mm._HipFrozenTrunk.last_timing))
        mm._TRAIN_TIMING = False
        sections = {k: med([r[k] for r in runs]) for k in runs[0]}
        t = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k in sides:
                t[k].append(timed(sides[k], a.window))
        ns, split = hip.audio_encoder.n_subbands, cfg["split_size"]
        tiles = B * ns * ((split + 1) // 2) * ((frames + 39) // 40)
        mfma_flop = tiles * 8 * 49 * 5 * (2 * 16 * 16 * 4)   # 8 chunks x 49 taps x 5 M-tiles x one 16x16x4 MFMA
        row = dict(config=name, B=B, T=T, frames=frames, max_diff_over_max_grad=diff, hip_backward_sections_ms=sections,
                   conv1_dgrad_executed_mfma_flop=mfma_flop,
                   conv1_dgrad_share_of_fp32_mfma_peak=mfma_flop / (sections["conv1_dgrad"] * 1e-3) / PEAK_FP32_MFMA)
        for k, v in t.items():
            row[f"{k}_fwd_bwd_ms"] = med(v)
            row[f"{k}_fwd_bwd_ms_repeats"] = v
            row[f"{k}_spread"] = (max(v) - min(v)) / med(v)
        row["torch_over_hip"] = row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del hip, ref, lm, sides
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"), configs=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
