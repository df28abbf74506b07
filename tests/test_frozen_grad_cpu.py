"""CPU: the yardsticks of tests/test_frozen_grad_gpu.py are themselves checked here (tests/frozen_ref.py).

* The float64 restatement of the backward pass with the float64 tree's OWN max-pool decisions pinned is float64 autograd of the
  tree to 1e-12 -- so a difference the GPU test finds is the code under test, not the restatement.
* The inputs of the GPU test are not full of max-pool near-ties: the share of windows whose two best candidates (or whose
  maximum and 0) are closer than tau = 4 * max |z_fp32 - z_float64| stays below 1e-3 for all six cases, so "every differing
  decision is a near-tie" is a narrow allowance.

The log-mel comes from the float64 oracle here (stage A runs on the GPU only), rounded to fp32 once."""
import functools

import pytest
import torch

import cases
import frozen_ref as fr
from oracle import mel as omel


@functools.lru_cache(maxsize=None)
def host_case(cfgname, B, frames):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = fr.CASES[cfgname]
    x = cases.pcm_batch(B, fr.clip_samples(cfg, frames))
    lm = omel.logmel(x.double(), n_fft=cfg["n_fft"], hop=cfg["hop_length"], n_mels=cfg["n_mels"]).float()
    assert lm.shape == (B, 8, cfg["n_mels"], frames)
    sd = cases.make_state_dict(cfg, 42)
    feats, R = fr.side_inputs(B, cfg["embed_dim"])
    t64 = fr.tree(fr.torch_twin(cfg, sd, torch.float64), lm, feats, want_grad_R=R)
    t32 = fr.tree(fr.torch_twin(cfg, sd, torch.float32), lm, feats)
    return cfg, sd, lm, feats, R, t64, t32


@pytest.mark.parametrize("cfgname", ["default", "baseline_sh"])
def test_pinned_restatement_is_float64_autograd(cfgname):
    B, frames = 2, 45
    cfg, sd, lm, feats, R, t64, _ = host_case(cfgname, B, frames)
    (k1, k2) = fr.pool_shapes(cfg)
    m1, m2 = fr.decisions(t64["z1"], *k1), fr.decisions(t64["z2"], *k2)
    twin = fr.torch_twin(cfg, sd, torch.float64)
    got = fr.pinned_gradient(twin, cfg, t64["pool_in"], t64["A1"], t64["A2"], m1, m2, R, frames)
    ref = t64["grad"]
    assert float(ref.abs().max()) > 0
    err = fr.normwise(got, ref)
    print(f"{cfgname}: restatement vs autograd, max |d| / max |ref| = {err:.3e}")
    assert err <= 1e-12
    ns = fr.geometry(cfg)[0]
    covered = (ns - 1) * cfg["overlap"] + cfg["split_size"]
    assert torch.count_nonzero(got[:, :, covered:]) == 0 and torch.count_nonzero(ref[:, :, covered:]) == 0


@pytest.mark.parametrize("cfgname,B,frames", fr.SHAPES)
def test_inputs_hold_few_near_ties(cfgname, B, frames):
    cfg, _, _, _, _, t64, t32 = host_case(cfgname, B, frames)
    for layer, k in zip((1, 2), fr.pool_shapes(cfg)):
        z64, z32 = t64[f"z{layer}"], t32[f"z{layer}"]
        tau = 4.0 * float((z32.double() - z64).abs().max())
        share, n = fr.near_tie_share(z64, *k, tau)
        flips = int((fr.decisions(z32, *k) != fr.decisions(z64, *k)).any(-1).any(-1).sum())
        print(f"{cfgname} ({B}, {frames}) layer {layer}: {n} windows, tau {tau:.3e}, near-tie share {share:.3e}, "
              f"fp32 tree differs from float64 in {flips} (band, channel) planes")
        assert share <= 1e-3
