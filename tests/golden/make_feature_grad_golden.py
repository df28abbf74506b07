"""Generate tests/golden/feature_grad.npz by running the REFERENCE's own MixingFeatureExtractor under autograd, on the host.

Usage (build container only; the reference checkout does not exist on the GPU box):
    python tests/golden/make_feature_grad_golden.py

Imports the reference's src/mixing_utils.py unmodified, as make_golden.py does (the stand-in `torchaudio` of
oracle/torchaudio_standin on sys.path).  Per case of tests/feature_grad_ref.py the fixture holds
    <case>.in_checksum                      the inputs are rebuilt from seeds by the tests and verified against this
    <case>.features   (B, 64)               the reference's forward values (fp32)
    <case>.cotangent  (B, 64)               the cotangent the gradients below were taken with (per group: its entries, zero elsewhere)
    <case>.<group>.e_ref                    || reference fp32 gradient - float64 restatement || / || float64 restatement ||
    <case>.<group>.idx, .grad               1024 seeded flat positions of the (B, 8, T) gradient and the reference's fp32 values there
    t700.<group>.grad_full (1, 8, 700)      the whole fp32 gradient of the smallest case, and t700.x its input
    live                                    the indices of the features with a non-zero Jacobian row (1024/256/128 and 2048/512/80)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "torchaudio_standin"))
sys.path.insert(0, "/root/reference/src")

import cases  # noqa: E402
import feature_grad_ref as fr  # noqa: E402
import mixing_utils as ref_mu  # noqa: E402  (reference)

torch.set_num_threads(8)
GROUPS = list(fr.GROUPS) + ["all"]


def ref_features(fe, xb):
    """xb (8, T) leaf -> the reference's feature vector with its history."""
    return fe.extract_all_features({s: xb[2 * i:2 * i + 2] for i, s in enumerate(cases.STEMS)})


def live_indices(n_fft, hop, n_mels):
    fe = ref_mu.MixingFeatureExtractor(44100, n_fft, hop, n_mels)
    x = (torch.randn(8, 3000, generator=cases._g(1)) * torch.tensor(fr.AMPS).repeat_interleave(2)[:, None]).requires_grad_(True)
    f = ref_features(fe, x)
    live = []
    for k in range(f.numel()):
        if f[k].grad_fn is None:
            continue
        gk, = torch.autograd.grad(f[k], x, retain_graph=True, allow_unused=True)
        if gk is not None and bool((gk != 0).any()):
            live.append(k)
    return live


def main():
    out = {}
    l1, l2 = live_indices(1024, 256, 128), live_indices(2048, 512, 80)
    assert l1 == l2, (l1, l2)
    out["live"] = np.array(l1, dtype=np.int64)
    for case, (n_fft, hop, n_mels, T, B, _) in fr.CASES.items():
        x, g = fr.inputs(case)
        fe = ref_mu.MixingFeatureExtractor(44100, n_fft, hop, n_mels)
        out[f"{case}.in_checksum"] = np.array(cases.checksum(x))
        out[f"{case}.cotangent"] = g.numpy()
        feats = []
        grads = {grp: [] for grp in GROUPS}
        for b in range(B):
            xb = x[b].clone().requires_grad_(True)
            f = ref_features(fe, xb)
            feats.append(f.detach())
            for grp in GROUPS:
                gb, = torch.autograd.grad(f, xb, fr.group_cotangent(g, grp)[b], retain_graph=True)
                grads[grp].append(gb)
        out[f"{case}.features"] = torch.stack(feats).numpy()
        for grp in GROUPS:
            g32 = torch.stack(grads[grp]).numpy()
            _, g64 = fr.gradient(x, fr.group_cotangent(g, grp), n_fft, hop, n_mels)
            out[f"{case}.{grp}.e_ref"] = np.array(fr.dist(g32, g64.numpy()))
            idx = cases.sample_idx(g32.size, 1024, seed=3)
            out[f"{case}.{grp}.idx"], out[f"{case}.{grp}.grad"] = idx, g32.ravel()[idx]
            if case == "t700":
                out[f"{case}.{grp}.grad_full"] = g32
            print(f"{case:16s} {grp:13s} e_ref {float(out[f'{case}.{grp}.e_ref']):.3e}")
        if case == "t700":
            out["t700.x"] = x.numpy()
    path = os.path.join(HERE, "feature_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
