"""GPU parity: HIP encoder (FiLM MLP, fused conv/BN/FiLM/ReLU/pool x2 on fp32 MFMA, attention pooling) through the
C ABI vs the CPU oracle and the goldens produced by the reference's own model code.

Tolerance (north_star: embeddings within 1e-4 rel fp32): |d| <= 1e-4 * max|ref| per tensor (+1e-4 rel elementwise).
"""
import os

import numpy as np
import pytest
import torch

import cases
import parity
from oracle import encoder as oenc
from oracle import mel as omel

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def build_model(cfg, backend="hip"):
    from mst_amd.model import MixingStyleEncoder
    m = MixingStyleEncoder(channels=8, feature_dim=64, encoder_backend=backend, **cfg)
    sd = cases.make_state_dict(cfg, seed=42)
    full = dict(m.state_dict())
    full.update(sd)
    m.load_state_dict(full, strict=True)
    return m.cuda().eval(), sd


def close(a, ref, tol=1e-4, name=None):
    import inspect
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    fr = inspect.stack()[1]
    parity.record(name or f"{fr.function}:{fr.lineno}", a, ref)
    np.testing.assert_allclose(a, ref, rtol=tol, atol=tol * scale)


def close_elementwise(a, ref, tol=1e-4, floor_frac=1e-2, max_miss=0, hard=None, name=None):
    """ELEMENT-wise bar (north_star: embeddings within 1e-4 rel): |d| <= tol * max(|ref|, floor_frac * max|ref|) for every
    element (the floor keeps elements that are ~0 next to O(1) neighbours -- ReLU outputs -- from dividing by nothing; it is
    the floor tests/parity.py reports with).  max_miss elements may exceed it, none by more than `hard`; the count is
    printed into the parity report either way."""
    import inspect
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    fr = inspect.stack()[1]
    row = parity.record((name or f"{fr.function}:{fr.lineno}") + " [element-wise]", a, ref, floor_frac=floor_frac)
    rel = np.abs(a - ref) / np.maximum(np.abs(ref), floor_frac * np.abs(ref).max())
    miss = int((rel > tol).sum())
    assert miss <= max_miss, f"{miss} of {rel.size} elements beyond {tol:g} (max {rel.max():.2e}); allowed {max_miss}"
    if hard is not None:
        assert rel.max() <= hard, f"worst element {rel.max():.2e} > {hard:g}"
    return row


def close_f16(a, ref, tol=1e-4, frac=5e-4, hard=5e-3, name=None):
    """Comparison of tensors that sit behind a STORED float16 value (the f16 training mode keeps its raw convolution outputs
    as float16): where the kernel's fp32 accumulation order and the oracle's differ in the last bit, a stored value lands on
    the neighbouring float16 (1e-3 of |y|, i.e. a few 1e-3 of the normalised activation).  At most `frac` of the elements
    may miss the 1e-4 tolerance for that reason, and none by more than `hard`."""
    import inspect
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    fr = inspect.stack()[1]
    parity.record(name or f"{fr.function}:{fr.lineno}", a, ref)
    d = np.abs(a - ref)
    miss = d > tol * np.abs(ref) + tol * scale
    assert miss.mean() <= frac, (int(miss.sum()), miss.size)
    np.testing.assert_allclose(a, ref, rtol=hard, atol=hard * scale)


@pytest.mark.parametrize("tag,cfg,T", [("default", cases.CFG_DEFAULT, 441000), ("cfg2", cases.CFG_BASELINE_SH, 441000),
                                        ("default_short", cases.CFG_DEFAULT, 66150),
                                        # "+chunked": conv1 on the chunked kernel (MST_CONV1_CHUNKED, read per launch):
                                        # conv_kernel<1, 2, 0> (20-mel sub-bands) and conv_kernel<1, 1, 0> (16-mel)
                                        ("default_short+chunked", cases.CFG_DEFAULT, 66150),
                                        ("cfg2+chunked", cases.CFG_BASELINE_SH, 441000)])
def test_encoder_vs_golden_and_oracle(tag, cfg, T, monkeypatch):
    tag, _, variant = tag.partition("+")
    if variant == "chunked":
        monkeypatch.setenv("MST_CONV1_CHUNKED", "1")
    g = np.load(os.path.join(G, "encoder.npz"))
    model, sd = build_model(cfg)
    x = torch.stack([cases.synth_clip(c, T) for c in (0, 1)], 0)
    feats = torch.from_numpy(g[f"{tag}.features"])
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        emb, taps = model.hip_encoder().forward(lm, feats.cuda(), taps=True)
    torch.cuda.synchronize()
    # stage-by-stage against the goldens (reference code outputs)
    close(taps["film"].cpu(), g[f"{tag}.film"], 1e-5)
    ns = cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"])
    p1 = taps["pool1"].cpu()
    for i in (0, ns // 2, ns - 1):
        assert tuple(p1[:, i].shape) == tuple(g[f"{tag}.pool1_{i}_shape"])
        idx = torch.from_numpy(g[f"{tag}.pool1_{i}_idx"])
        close(p1[:, i].flatten()[idx], g[f"{tag}.pool1_{i}_samples"])
    pin = taps["pool_in"].cpu()
    assert tuple(pin.shape) == tuple(g[f"{tag}.pool_in_shape"])
    close(pin.flatten()[torch.from_numpy(g[f"{tag}.pool_in_idx"])], g[f"{tag}.pool_in_samples"])
    close(pin.double().sum(-1), g[f"{tag}.pool_in_rowsum"])
    close(emb.cpu(), g[f"{tag}.embedding"])
    close_elementwise(emb.cpu(), g[f"{tag}.embedding"])   # every element within 1e-4 of the reference's own output
    # full tensors against the oracle on the same log-mel
    otaps = {}
    oemb = oenc.encoder_from_logmel(sd, lm.cpu(), feats, cfg["split_size"], cfg["overlap"], otaps)
    for i in range(ns):
        close(p1[:, i], otaps[f"pool1_{i}"])
    close(pin, otaps["pool_in"])
    close(emb.cpu(), oemb)
    close_elementwise(emb.cpu(), oemb)


def test_module_forward_matches_reference_call_contract():
    """MixingStyleEncoder(stems_dict, mixing_features) -> (B, 768), end to end in HIP, vs golden embeddings."""
    g = np.load(os.path.join(G, "encoder.npz"))
    model, _ = build_model(cases.CFG_DEFAULT)
    from mst_amd.mixing_utils import MixingFeatureExtractor
    x = torch.stack([cases.synth_clip(c, 441000) for c in (0, 1)], 0).cuda()
    stems = omel.tensor_to_stems_dict(x)
    feats = MixingFeatureExtractor().extract_all_features(stems)
    with torch.no_grad():
        emb = model(stems, feats)
    assert tuple(emb.shape) == (2, 768)
    close(emb.cpu(), g["default.embedding"], 2e-4)   # features come from the HIP extractor here, not the golden
    assert model.audio_encoder.n_subbands == 11 and model.audio_encoder.freq_dim == 2


def test_batch_independence_and_ragged_tail():
    """B not a multiple of the 8-wave set size, frames not a multiple of the pooling windows; each clip's
    embedding must not depend on its batch neighbours."""
    model, sd = build_model(cases.CFG_DEFAULT)
    T = 256 * 203 + 17    # 204 frames -> W1 = 40, W2 = 10 (partial column tiles in both convs)
    x = torch.stack([cases.synth_clip(c, T) for c in range(5)], 0)
    feats = torch.randn(5, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        e5 = model.hip_encoder().forward(lm, feats.cuda()).cpu()
        e1 = model.hip_encoder().forward(lm[3:4].contiguous(), feats[3:4].cuda()).cpu()
    assert torch.equal(e5[3], e1[0])
    close(e5, oenc.encoder_from_logmel(sd, lm.cpu(), feats))


def test_conv1_set_orders_and_ticketed_tiles_give_the_same_bits(monkeypatch):
    """conv1's eval forward hands its tiles to whichever wave asks next, inside segments whose extent depends on the order of the
    sets (`MST_CONV1_CLIP_GROUP`, `MST_CONV1_BAND_MAJOR`, read per launch): every order -- segments of one clip, of three, of the
    whole batch; a grid with more workgroups than sets (B = 1) -- must return the default order's embeddings bit for bit, in the
    channel-minor and in the reference log-mel layout."""
    from mst_amd import _lib
    model, _ = build_model(cases.CFG_DEFAULT)
    T = 256 * 260 + 5
    x = torch.stack([cases.synth_clip(c % 4, T) * (1.0 + 0.05 * c) for c in range(7)], 0).cuda()
    stems = omel.tensor_to_stems_dict(x)
    feats = torch.randn(7, 64, generator=torch.Generator().manual_seed(5)).cuda()
    plan = model.audio_encoder.mel_preprocessor.plan(0)
    enc = model.hip_encoder()
    with torch.no_grad():
        lm_ref = model.audio_encoder.mel_preprocessor(stems)
        lm_cm, _ = plan.forward_stems(stems, True, False, _lib.LOGMEL_CM32)
        for lm in (lm_cm, lm_ref):
            base = enc.forward(lm, feats).clone()
            for env in ({"MST_CONV1_CLIP_GROUP": "3"}, {"MST_CONV1_CLIP_GROUP": "7"}, {"MST_CONV1_BAND_MAJOR": "1"}):
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                got = enc.forward(lm, feats).clone()
                for k in env:
                    monkeypatch.delenv(k)
                assert torch.equal(got, base), env
        one = enc.forward(lm_ref[2:3].contiguous(), feats[2:3])
        assert torch.equal(one[0], enc.forward(lm_ref, feats)[2])


def test_torch_backend_agrees_and_train_mode_guard():
    model, _ = build_model(cases.CFG_DEFAULT)
    x = torch.stack([cases.synth_clip(c, 66150) for c in (0, 1)], 0).cuda()
    feats = torch.randn(2, 64, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x))
        a = model.forward_from_logmel(lm, feats)
        model.encoder_backend = "torch"
        b = model.forward_from_logmel(lm, feats)
        model.encoder_backend = "hip"
    close(a.cpu(), b.cpu())
    model.train()
    with torch.no_grad(), pytest.raises(RuntimeError):
        model.forward_from_logmel(lm, feats)
    model.train_backend = "torch"                   # explicit opt-in: grad enabled + train() on PyTorch-ROCm autograd
    out = model.forward_from_logmel(lm, feats)
    out.sum().backward()
    assert model.film_encoder.film_head.weight.grad is not None
    # the default backend never leaves the hand-written trunk silently: a call it cannot take (here: 40-mel sub-bands, first-pool
    # height 4) raises and names the reason, from forward_from_logmel and from forward alike; "hip-or-torch" is the explicit
    # warn-and-fall-back opt-in
    from mst_amd.model import MixingStyleEncoder
    m40 = MixingStyleEncoder(n_mels=128, split_size=40, overlap=20, feature_dim=64).cuda().train()
    assert m40.train_backend == "hip"
    with pytest.raises(RuntimeError, match="first-pool heights 1 and 2"):
        m40.forward_from_logmel(lm, feats)
    with pytest.raises(RuntimeError, match="first-pool heights 1 and 2"):
        m40(omel.tensor_to_stems_dict(x), feats)
    m40.train_backend = "hip-or-torch"
    with pytest.warns(RuntimeWarning, match="first-pool heights 1 and 2"):
        out = m40(omel.tensor_to_stems_dict(x), feats)
    assert torch.isfinite(out).all()
    m40.train_backend = "nonsense"
    with pytest.raises(ValueError):
        m40.forward_from_logmel(lm, feats)


def test_unsupported_geometry_fails_loudly():
    from mst_amd import _lib
    from mst_amd.model import MixingStyleEncoder
    m = MixingStyleEncoder(n_mels=128, split_size=100, overlap=20, feature_dim=64).cuda().eval()  # a band patch beyond one CU's LDS
    with pytest.raises(_lib.MstError, match="split_size"):
        m.hip_encoder()


@pytest.mark.parametrize("split,overlap", [(40, 20), (30, 10), (35, 31)])
def test_first_pool_heights_of_three_and_more(split, overlap):
    """The reference takes any split_size (src/model.py:111-117: sub = max(1, split_size // 10), MaxPool((sub, 5))); first-pool
    heights 1 and 2 run on the MFMA kernels, larger ones on conv1_generic_kernel (eval forward, reference layout).  Against the
    oracle on the same log-mel: pool1 of every band, pool_in, embeddings -- incl. split 35 (H1 = 11: MaxPool floors the last rows
    away twice), a ragged frame count and B = 3."""
    from mst_amd.model import MixingStyleEncoder
    torch.manual_seed(5)
    m = MixingStyleEncoder(n_mels=128, split_size=split, overlap=overlap, feature_dim=64, embed_dim=256).cuda().eval()
    with torch.no_grad():   # non-trivial BatchNorm statistics and FiLM gammas
        for c in m.audio_encoder.subnet_cnns:
            c.bn1.running_mean.normal_(0, 0.2), c.bn1.running_var.uniform_(0.5, 1.5)
            c.bn2.running_mean.normal_(0, 0.2), c.bn2.running_var.uniform_(0.5, 1.5)
    sub = split // 10
    assert sub >= 3 and m.audio_encoder.freq_dim == (split // sub) // 4
    T = 256 * 203 + 17
    x = torch.stack([cases.synth_clip(c, T) for c in range(3)], 0)
    feats = torch.randn(3, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        lm = m.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        emb, taps = m.hip_encoder().forward(lm, feats.cuda(), taps=True)
        e_mod = m(omel.tensor_to_stems_dict(x.cuda()), feats.cuda())     # the module's own call negotiates the reference layout
    assert torch.equal(e_mod, emb)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    otaps = {}
    oemb = oenc.encoder_from_logmel(sd, lm.cpu(), feats, split, overlap, otaps)
    for i in range(m.audio_encoder.n_subbands):
        close(taps["pool1"][:, i].cpu(), otaps[f"pool1_{i}"])
    close(taps["pool_in"].cpu(), otaps["pool_in"])
    close(emb.cpu(), oemb)
    close_elementwise(emb.cpu(), oemb)
    m.conv1_precision = "f16x3"   # the split-precision modes need the 2-row MFMA tiles and say so
    with pytest.raises(Exception, match="2-row conv1 tiles"):
        m.hip_encoder()


def test_config5_geometry_30s_256_mels():
    """BASELINE configs[4] shapes: 30 s clips (F = 5168), n_mels = 256 -> 24 sub-bands, attention input (B, 3072, 258)."""
    cfg = dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=256, split_size=20, overlap=10, embed_dim=768)
    model, sd = build_model(cfg)
    assert model.audio_encoder.n_subbands == 24
    T = 30 * 44100
    x = cases.synth_clip(2, T)[None]
    from mst_amd.mixing_utils import MixingFeatureExtractor
    from oracle import features as ofeat
    stems = omel.tensor_to_stems_dict(x.cuda())
    feats, lm = MixingFeatureExtractor(44100, 1024, 256, 256).features_and_logmel(stems)
    assert tuple(lm.shape) == (1, 8, 256, 5168)
    rf, rmel = ofeat.extract_all_features(x, 44100, 1024, 256, 256, return_mel=True)
    np.testing.assert_allclose(feats.cpu().numpy(), rf.numpy(), rtol=1e-4, atol=2e-4)
    from test_melfeat_gpu import check_logmel
    check_logmel(lm.cpu(), torch.log(rmel + 1e-10), x=x, cfg=(44100, 1024, 256, 256))
    with torch.no_grad():
        emb, taps = model.hip_encoder().forward(lm, feats, taps=True)
    assert tuple(taps["pool_in"].shape) == (1, 3072, 258)
    ref = oenc.encoder_from_logmel(sd, lm.cpu(), feats.cpu(), 20, 10)
    close(emb.cpu(), ref)


@pytest.mark.parametrize("mode", ["f16x3", "f16x3-all"])
@pytest.mark.parametrize("tag,T", [("default", 441000), ("default_short", 66150)])
def test_conv_f16x3_split_precision_meets_the_fp32_bar(tag, T, mode):
    """Opt-in conv1 on the f16 matrix cores (3-term split): same goldens, same 1e-4 tolerance as the exact path;
    also reports how far it is from the exact-fp32 kernel."""
    g = np.load(os.path.join(G, "encoder.npz"))
    cfg = cases.CFG_DEFAULT
    model, sd = build_model(cfg)
    x = torch.stack([cases.synth_clip(c, T) for c in (0, 1)], 0)
    feats = torch.from_numpy(g[f"{tag}.features"]).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        e32, t32 = model.hip_encoder().forward(lm, feats, taps=True)
        model.conv1_precision = mode
        e16, t16 = model.hip_encoder().forward(lm, feats, taps=True)
        model.conv1_precision = "fp32"
    ns = cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"])
    p1 = t16["pool1"].cpu()
    for i in (0, ns // 2, ns - 1):
        idx = torch.from_numpy(g[f"{tag}.pool1_{i}_idx"])
        close(p1[:, i].flatten()[idx], g[f"{tag}.pool1_{i}_samples"])
    close(t16["pool_in"].cpu().flatten()[torch.from_numpy(g[f"{tag}.pool_in_idx"])], g[f"{tag}.pool_in_samples"])
    close(e16.cpu(), g[f"{tag}.embedding"])
    d_pool = (t16["pool1"] - t32["pool1"]).abs().max().item() / t32["pool1"].abs().max().item()
    d_emb = (e16 - e32).abs().max().item() / e32.abs().max().item()
    d_pin = (t16["pool_in"] - t32["pool_in"]).abs().max().item() / t32["pool_in"].abs().max().item()
    print(f"{mode} vs exact fp32: pool1 {d_pool:.2e}, pool_in {d_pin:.2e}, embedding {d_emb:.2e} (relative to max)")
    assert d_pool < 2e-6 and d_pin < 1e-5 and d_emb < 1e-5


@pytest.mark.parametrize("mode", ["f16x3", "f16x3-all", "f16"])
def test_conv_f16_modes_on_16_mel_sub_bands(mode):
    """scripts/train_baseline.sh geometry (80 mels, 16/8 sub-bands, pool height 1): the split-precision modes sit on the
    exact-fp32 kernels' result, the plain f16 mode on the oracle evaluated with f16-rounded conv operands."""
    cfg = cases.CFG_BASELINE_SH
    model, sd = build_model(cfg)
    x = torch.stack([cases.synth_clip(c, 66150) for c in (0, 1)], 0)
    with torch.no_grad():
        stems = omel.tensor_to_stems_dict(x.cuda())
        from mst_amd.mixing_utils import MixingFeatureExtractor
        feats, lm = MixingFeatureExtractor(cfg["sample_rate"], cfg["n_fft"], cfg["hop_length"], cfg["n_mels"]).features_and_logmel(stems)
        e32, t32 = model.hip_encoder().forward(lm, feats, taps=True)
        model.conv1_precision = mode
        e16, t16 = model.hip_encoder().forward(lm, feats, taps=True)
        model.conv1_precision = "fp32"
    assert t16["pool1"].shape == t32["pool1"].shape and torch.isfinite(e16).all()
    if mode == "f16":
        want = oenc.encoder_from_logmel(sd, lm.cpu(), feats.cpu(), cfg["split_size"], cfg["overlap"], f16_operands=True)
        close(e16.cpu(), want)
        return
    d_pool = (t16["pool1"] - t32["pool1"]).abs().max().item() / t32["pool1"].abs().max().item()
    d_pin = (t16["pool_in"] - t32["pool_in"]).abs().max().item() / t32["pool_in"].abs().max().item()
    d_emb = (e16 - e32).abs().max().item() / e32.abs().max().item()
    print(f"{mode} vs exact fp32 (16-mel sub-bands): pool1 {d_pool:.2e}, pool_in {d_pin:.2e}, embedding {d_emb:.2e}")
    assert d_pool < 2e-6 and d_pin < 1e-5 and d_emb < 1e-5


@pytest.mark.parametrize("gain", [1.0, 3.0e3, 3.0e5, 1.0e-4])
def test_conv_f16x3_is_range_safe_for_any_activation_magnitude(gain):
    """The f16 split-precision modes scale conv2's f16 input per (clip, band) by a power of two derived on the device
    from a bound on conv1's output -- no host-side range check, nothing refused.  conv1's weights are multiplied by
    `gain`, which pushes the fp32 pooled activations far beyond the f16 range (gain 3e3: ~2e5 > 65504; 3e5: ~2e7) or
    down into f16's subnormals (1e-4): the f16x3-all result must stay within 1e-5 of the exact-fp32 kernels, element-wise
    relative to the tensor's max, and finite."""
    cfg = cases.CFG_DEFAULT
    from mst_amd.model import MixingStyleEncoder
    m = MixingStyleEncoder(channels=8, feature_dim=64, **cfg)
    sd = cases.make_state_dict(cfg, seed=42)
    for k in list(sd):
        if k.endswith("conv1.weight") or k.endswith("conv1.bias"):
            sd[k] = sd[k] * gain
        if k.endswith("bn1.running_mean"):   # keep BatchNorm(eval) from cancelling the gain: mean scales, variance does not
            sd[k] = sd[k] * gain
    full = dict(m.state_dict())
    full.update(sd)
    m.load_state_dict(full, strict=True)
    m = m.cuda().eval()
    g = np.load(os.path.join(G, "encoder.npz"))
    x = torch.stack([cases.synth_clip(c, 66150) for c in (0, 1)], 0)
    feats = torch.from_numpy(g["default_short.features"]).cuda()
    with torch.no_grad():
        lm = m.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        e32, t32 = m.hip_encoder().forward(lm, feats, taps=True)
        m.conv1_precision = "f16x3-all"
        e16, t16 = m.hip_encoder().forward(lm, feats, taps=True)
        m.conv1_precision = "f16"
        e1 = m.hip_encoder().forward(lm, feats)
    top = t32["pool1"].abs().max().item()
    print(f"gain {gain:g}: max fp32 pool1 = {top:.3g} (f16 max 65504)")
    if gain >= 3e3:
        assert top > 65504.0
    assert torch.isfinite(e16).all() and torch.isfinite(e1).all()
    parity.record(f"f16x3-all vs fp32 kernels, conv1 gain {gain:g}: pool_in", t16["pool_in"], t32["pool_in"])
    parity.record(f"f16x3-all vs fp32 kernels, conv1 gain {gain:g}: embedding", e16, e32)
    d_pin = (t16["pool_in"] - t32["pool_in"]).abs().max().item() / t32["pool_in"].abs().max().item()
    d_emb = (e16 - e32).abs().max().item() / e32.abs().max().item()
    # pool_in (the convolutions' own output) holds 1e-5 at every gain.  The embedding lies behind the attention softmax, whose logits
    # scale with the gain: at 3e3 and beyond the frame weights are nearly one-hot and two fp32 summation orders of the SAME
    # convolution (1e-6 apart in pool_in) already sit ~1e-5 apart there -- observed 0.9e-5 .. 1.2e-5 between builds that differ
    # only in the order of the taps; 3e-5 is that with a margin, not a looser convolution bound.
    assert d_pin < 1e-5 and d_emb < (1e-5 if gain < 3e3 else 3e-5), (d_pin, d_emb)


def test_conv_f16_amp_mode_matches_its_own_definition():
    """Opt-in "f16" mode (1-term f16 MFMA = the reference's --use_amp conv arithmetic): conv inputs and weights are
    rounded to float16, everything else is fp32.  Checked at 1e-4 against the oracle evaluated with exactly those
    roundings, and reported against the exact path (the mode itself is a ~1e-3 approximation of fp32)."""
    cfg = cases.CFG_DEFAULT
    model, sd = build_model(cfg)
    g = np.load(os.path.join(G, "encoder.npz"))
    x = torch.stack([cases.synth_clip(c, 66150) for c in (0, 1)], 0)
    feats = torch.from_numpy(g["default_short.features"])
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        e32 = model.hip_encoder().forward(lm, feats.cuda())
        model.conv1_precision = "f16"
        e16, t16 = model.hip_encoder().forward(lm, feats.cuda(), taps=True)
        model.conv1_precision = "fp32"
    taps = {}
    want = oenc.encoder_from_logmel(sd, lm.cpu(), feats, cfg["split_size"], cfg["overlap"], taps, f16_operands=True)
    ns = cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"])
    p1 = t16["pool1"].cpu()
    for i in (0, ns - 1):
        close(p1[:, i], taps[f"pool1_{i}"])
    close(t16["pool_in"].cpu(), taps["pool_in"])
    close(e16.cpu(), want)
    d = (e16 - e32).abs().max().item() / e32.abs().max().item()
    print(f"f16 (amp) vs exact fp32 embeddings: {d:.2e} of max")
    assert d < 2e-2


@pytest.mark.parametrize("T,B", [(66150, 3), (44100 * 2 + 1234, 2)])
def test_train_mode_forward_batch_statistics(T, B):
    """SURVEY 8 f1 (first half): `mst_encoder_forward_train` == the oracle with BatchNorm in training mode (statistics of
    the batch over (B, H, W), biased variance; dropout off): batch statistics, pool1, pool_in, embeddings."""
    cfg = cases.CFG_DEFAULT
    model, sd = build_model(cfg)
    x = torch.stack([cases.synth_clip(c, T) for c in range(B)], 0)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, 64, generator=g) * 3.0
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        emb, t = model.hip_encoder().forward_train(lm, feats.cuda())
        e_eval = model.hip_encoder().forward(lm, feats.cuda())
    torch.cuda.synchronize()
    taps = {}
    want = oenc.encoder_from_logmel(sd, lm.cpu(), feats, cfg["split_size"], cfg["overlap"], taps, bn_training=True)
    ns = cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"])
    for i in (0, ns // 2, ns - 1):
        for name, key in (("bn1", "bn1"), ("bn2", "bn2")):
            mean, var = taps[f"{name}_{i}"]
            got = t[key][i].cpu()
            close(got[:, 0], mean, 1e-4)
            close(1.0 / got[:, 1] ** 2 - 1e-5, var, 2e-4)
        close(t["pool1"][:, i].cpu(), taps[f"pool1_{i}"])
    close(t["pool_in"].cpu(), taps["pool_in"])
    close(emb.cpu(), want)
    assert (emb - e_eval).abs().max().item() > 1e-3 * e_eval.abs().max().item()   # it is NOT the eval forward


@pytest.mark.parametrize("cfgname,precision", [("default", "fp32"), ("default", "f16"), ("default", "f16x3"), ("baseline_sh", "fp32"),
                                               ("baseline_sh", "f16x3")])
def test_results_do_not_depend_on_workspace_contents(cfgname, precision):
    """Every slot of the activation workspace that a kernel reads must have been written by a kernel of the same step: with
    the workspace filled with 0xFF bytes (fp32 NaN, int64 -1) before each forward, the eval embeddings and a training
    step's loss and gradients are bit-identical to those of a run on whatever the allocator handed out.  (Found the hard
    way: conv2's raw-output slots right of the plane in the 2-row strip were read by the backward reduction as 0 * x.)"""
    from mst_amd import model as mm
    cfg = cases.CFG_BASELINE_SH if cfgname == "baseline_sh" else cases.CFG_DEFAULT
    B, T = 5, 44100 + 256 * 3   # default: 176 frames, W1 = 35 (partial 8-column tile in conv2), W2 = 8
    x = torch.stack([cases.synth_clip(c % 4, T) for c in range(B)], 0).cuda()
    g = torch.Generator().manual_seed(11)
    feats = (torch.randn(B, 64, generator=g) * 2.0).cuda()
    R = torch.randn(B, cfg["embed_dim"], generator=g).cuda()
    results = []
    try:
        for poison in (False, True):
            mm._POISON_WS = poison
            model, _ = build_model(cfg)
            with torch.no_grad():
                lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x))
                e_eval = model.forward_from_logmel(lm, feats).clone()
            model.train()
            model.train_backend, model.train_precision = "hip-strict", precision
            torch.manual_seed(3)   # Dropout masks
            loss = (model.forward_from_logmel(lm, feats) * R).sum()
            loss.backward()
            results.append((e_eval, loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}))
    finally:
        mm._POISON_WS = False
    (ea, la, ga), (eb, lb, gb) = results
    assert torch.isfinite(eb).all() and torch.equal(ea, eb)
    assert torch.isfinite(lb) and torch.equal(la, lb)
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, bad[:5]


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_f16_training_modes_at_config5_geometry(precision):
    """BASELINE configs[4] shapes (30 s clips -> 5168 frames, 256 mels -> 24 sub-bands; 130 conv1 tile columns, 1034 / 8 = 130
    conv2 tile columns with a partial last one) with a batch that is not a multiple of the 8-clip groups: the split-precision
    trunk must reproduce the fp32 trunk's loss and gradients at the fp32 kernels' own accuracy (both are ~1e-6 from float64
    on most tensors, see the gradient tests), the float16-operand trunk must stay within a few 1e-2 of them (its arithmetic
    is ~1e-2 from fp32) with finite values everywhere."""
    import copy
    cfg = dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=256, split_size=20, overlap=10, embed_dim=768)
    model, _ = build_model(cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    other = copy.deepcopy(model)
    model.train(), other.train()
    model.train_backend = other.train_backend = "hip-strict"
    model.train_precision, other.train_precision = "fp32", precision
    B, T = 3, 30 * 44100
    x = torch.stack([cases.synth_clip(c, T) for c in range(B)], 0).cuda()
    g = torch.Generator().manual_seed(12)
    feats = (torch.randn(B, 64, generator=g) * 2.0).cuda()
    R = torch.randn(B, cfg["embed_dim"], generator=g).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x))
    assert tuple(lm.shape) == (B, 8, 256, 5168)
    la = (model.forward_from_logmel(lm, feats) * R).sum()
    lb = (other.forward_from_logmel(lm, feats) * R).sum()
    la.backward(), lb.backward()
    # f16x3: two fp32-grade evaluations agree to ~1e-6 except where a near-tie max-pool decision differs (single sub-bands move by
    # up to a few 1e-3, as either does against float64 -- see the gradient tests)
    tol_loss, tol_med, tol_max = (1e-5, 1e-5, 2e-2) if precision == "f16x3" else (2e-2, 5e-2, 1.0)
    assert abs(la.item() - lb.item()) <= tol_loss * abs(la.item()), (la.item(), lb.item())
    errs = []
    for (n, pa), (_, pb) in zip(model.named_parameters(), other.named_parameters()):
        assert pb.grad is not None and torch.isfinite(pb.grad).all(), n
        den = pa.grad.abs().max().item()
        # conv biases in front of a batch-statistics BatchNorm and the softmax's additive bias have gradient 0 up to rounding
        if den > 1e-9 and not n.endswith(("conv1.bias", "conv2.bias", "attention.2.bias")):
            errs.append(((pa.grad - pb.grad).abs().max().item() / den, n))
    e = np.array([a for a, _ in errs])
    print(f"{precision} vs fp32 trunk at config5 geometry over {len(e)} tensors: median {np.median(e):.2e}, worst {max(errs)}")
    parity.note(f"{precision} training trunk vs fp32 trunk, config5 geometry (B=3, 30 s, 24 sub-bands), norm-wise per tensor",
                tensors=len(e), median=float(np.median(e)), p90=float(np.percentile(e, 90)), max=float(e.max()))
    assert np.median(e) < tol_med and e.max() < tol_max, max(errs)


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16"])
@pytest.mark.parametrize("B", [1, 9])
def test_training_at_the_minimum_clip_length(B, precision):
    """20 frames (the shortest clip the trunk accepts: W1 = 4, W2 = 1 -- single, partial tiles in every kernel) with a batch of 1
    (one ragged 8-clip group) and of 9 (a full group + a group of one): loss and gradients against float64 autograd of the
    torch modules (fp32 / f16x3: 1e-3 norm-wise per tensor -- tiny planes make single near-tie pooling decisions visible; f16:
    a sanity bound only -- float16 operands under batch statistics of a few hundred positions are 10-20 % away from fp32
    arithmetic here; its parity proper is the oracle test with the same roundings)."""
    import copy
    cfg = cases.CFG_DEFAULT
    model, _ = build_model(cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    ref64 = copy.deepcopy(model).double()
    model.train(), ref64.train()
    model.train_backend, ref64.train_backend, model.train_precision = "hip-strict", "torch", precision
    T = 19 * 256
    x = torch.stack([cases.synth_clip(c % 4, 44100)[:, 20000:20000 + T] * (1.0 + 0.2 * (c // 4)) for c in range(B)], 0).cuda()
    g = torch.Generator().manual_seed(21)
    feats = (torch.randn(B, 64, generator=g) * 2.0).cuda()
    R = torch.randn(B, cfg["embed_dim"], generator=g).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x))
    assert lm.shape[-1] == 20
    la = (model.forward_from_logmel(lm, feats) * R).sum()
    lc = (ref64.forward_from_logmel(lm.double(), feats.double()) * R.double()).sum()
    la.backward(), lc.backward()
    tol = 1e-3 if precision != "f16" else 0.5
    assert abs(la.item() - lc.item()) <= min(tol, 0.1) * abs(lc.item()) + 1e-6, (la.item(), lc.item())
    worst = (0.0, "")
    for (n, pa), (_, pc) in zip(model.named_parameters(), ref64.named_parameters()):
        assert pa.grad is not None and torch.isfinite(pa.grad).all(), n
        den = pc.grad.abs().max().item()
        if den < 1e-9 or n.endswith(("conv1.bias", "conv2.bias", "attention.2.bias")):
            continue
        worst = max(worst, ((pa.grad.double() - pc.grad).abs().max().item() / den, n))
    print(f"B={B}, 20 frames, {precision}: worst gradient error vs float64 autograd {worst[0]:.2e} ({worst[1]})")
    parity.note(f"training at 20 frames, B={B}, {precision}: worst norm-wise gradient error vs float64 autograd", worst=float(worst[0]))
    assert worst[0] < tol, worst


@pytest.mark.parametrize("B,T,n_mels,split,overlap", [(2, 7000, 40, 20, 10), (17, 30000, 128, 20, 10), (8, 12345, 64, 16, 8),
                                                      (3, 5200, 80, 16, 8)])
def test_split_precision_training_on_odd_shapes(B, T, n_mels, split, overlap):
    """Shapes off the beaten path -- 28 / 118 / 49 / 21 frames (partial and single tiles, W2 = 1), 3 / 11 / 7 / 9 sub-bands, both
    pooling geometries, batches of 2 / 17 / 8 / 3 (ragged and exact 8-clip groups): the f16x3 trunk (all f16 kernels, hi + lo)
    against the fp32 trunk -- finite everywhere, loss within 1e-5, gradients within 1e-2 norm-wise (near-tie pooling decisions on
    tiny planes, and the fp32 kernels' own cancellation error in the conv1 weight gradients of the low sub-bands -- up to 4e-3 from
    float64, see the gradient tests -- both show) with a median below 1e-5."""
    import copy
    cfg = dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=n_mels, split_size=split, overlap=overlap, embed_dim=256)
    model, _ = build_model(cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    other = copy.deepcopy(model)
    model.train(), other.train()
    model.train_backend = other.train_backend = "hip-strict"
    model.train_precision, other.train_precision = "fp32", "f16x3"
    x = torch.stack([cases.synth_clip(c % 4, 44100)[:, 3000:3000 + T] * (1.0 + 0.07 * c) for c in range(B)], 0).cuda()
    g = torch.Generator().manual_seed(31)
    feats = (torch.randn(B, 64, generator=g) * 2.0).cuda()
    R = torch.randn(B, cfg["embed_dim"], generator=g).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x))
    ea = model.forward_from_logmel(lm, feats)
    la = (ea * R).sum()
    lb = (other.forward_from_logmel(lm, feats) * R).sum()
    la.backward(), lb.backward()
    assert other._hip_train.train_mode == 2
    # the loss is a sum of B x 256 terms of either sign that cancel to ~1e-3 of their total magnitude: the bar is relative to that
    # magnitude (2e-7 of it, i.e. ~1e-4 .. 1e-5 of the loss itself)
    assert abs(la.item() - lb.item()) <= 2e-7 * (ea.detach() * R).abs().sum().item() + 1e-6, (la.item(), lb.item())
    errs = []
    for (n, pa), (_, pb) in zip(model.named_parameters(), other.named_parameters()):
        assert pb.grad is not None and torch.isfinite(pb.grad).all(), n
        den = pa.grad.abs().max().item()
        if den > 1e-9 and not n.endswith(("conv1.bias", "conv2.bias", "attention.2.bias")):
            errs.append(((pa.grad - pb.grad).abs().max().item() / den, n))
    e = np.array([a for a, _ in errs])
    print(f"B={B} T={T} mels={n_mels} split={split}: f16x3 vs fp32 trunk over {len(e)} tensors: median {np.median(e):.2e}, worst {max(errs)}")
    assert np.median(e) < 1e-5 and e.max() < 1e-2, max(errs)


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16"])
def test_cross_rank_batchnorm_statistics_two_shards(precision):
    """SURVEY C3 / DESIGN section 6: with `sync_bn` an N-rank training step computes what the single-process reference computes on
    the whole batch.  Two "ranks" are two encoders of this process with 3 clips each, driven in lockstep through the phases of
    `forward_train_steps` / `backward_apply_steps`; the test plays the all-reduce (integer SUM of the statistics words, MAX of
    the f16 modes' scale word).  Against one encoder on all 6 clips: pool_in of both shards (forward), d pool1, the FiLM
    gradients, and -- summed over the shards, as the trainer's gradient all-reduce does -- the BatchNorm and convolution
    weight gradients.  fp32-grade precisions: 2e-5; float16 operands: the shards' per-rank range scales differ from the
    single-process ones only by powers of two, results within 1e-3."""
    from mst_amd.model import HipEncoder
    cfg = cases.CFG_DEFAULT
    model, _ = build_model(cfg)
    B, T, h = 6, 44100, 2   # UNEQUAL shards (2 + 4 clips): the clip count travels with the sums, not as "world x local clips"
    x = torch.stack([cases.synth_clip(c % 4, T) * (1.0 + 0.1 * c) for c in range(B)], 0).cuda()
    g = torch.Generator().manual_seed(41)
    feats = (torch.randn(B, 64, generator=g) * 2.0).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x))
    Fr = lm.shape[-1]
    encs = [HipEncoder(model, "fp32") for _ in range(3)]   # [0]: all clips; [1], [2]: the shards
    params = _stacked_trunk_params(model)
    for e in encs:
        e.set_train_precision(precision)
        e.update_trunk_params(*params)

    def lockstep(gens):   # run generators side by side; after every yield combine the yielded views as the collective would
        outs = [None] * len(gens)
        while any(o is None for o in outs):
            ys = []
            for i, gen in enumerate(gens):
                try:
                    ys.append(next(gen))
                except StopIteration as done:
                    outs[i] = done.value
            if ys:
                assert len(ys) == len(gens) and len({k for k, _ in ys}) == 1
                views = [v for _, v in ys]
                tot = torch.stack(views).sum(0) if ys[0][0] == "sum" else torch.stack(views).max(0).values
                for v in views:
                    v.copy_(tot)
        return outs

    sl = [slice(0, B), slice(0, h), slice(h, B)]
    (_, t0), = lockstep([encs[0].forward_train_steps(lm, feats, head=False, world=0)])
    ts = lockstep([encs[i].forward_train_steps(lm[sl[i]].contiguous(), feats[sl[i]].contiguous(), head=False, world=2) for i in (1, 2)])
    tol = 2e-5 if precision != "f16" else 1e-3
    pin = torch.cat([ts[0][1]["pool_in"], ts[1][1]["pool_in"]], 0)
    close(pin.cpu(), t0["pool_in"].cpu(), tol)
    close(ts[0][1]["bn2"].cpu(), t0["bn2"].cpu(), tol)          # the shards normalise with the GLOBAL statistics
    # backward from a common d pool_in
    R = torch.randn(t0["pool_in"].shape, generator=g).cuda()
    dfilm = [torch.zeros(b, encs[0].n_sub * 192, device="cuda") for b in (B, h, B - h)]
    (dy2_0, dbn2_0), = lockstep([encs[0].backward_apply_steps(2, R, dfilm[0], B, Fr, world=0)])
    r2 = lockstep([encs[i].backward_apply_steps(2, R[sl[i]].contiguous(), dfilm[i], sl[i].stop - sl[i].start, Fr, world=2) for i in (1, 2)])
    dp1_0 = encs[0].conv2_dgrad(dy2_0, B, Fr)
    dp1 = [encs[i].conv2_dgrad(r2[i - 1][0], sl[i].stop - sl[i].start, Fr) for i in (1, 2)]
    if precision == "fp32":
        close(torch.cat(dp1, 0).cpu(), dp1_0.cpu(), tol)
    gw2_0 = encs[0].conv2_wgrad(t0["pool1"], B, Fr)
    gw2 = sum(encs[i].conv2_wgrad(ts[i - 1][1]["pool1"], sl[i].stop - sl[i].start, Fr) for i in (1, 2))
    (_, dbn1_0), = lockstep([encs[0].backward_apply_steps(1, dp1_0, dfilm[0], B, Fr, inplace=True, world=0)])
    r1 = lockstep([encs[i].backward_apply_steps(1, dp1[i - 1], dfilm[i], sl[i].stop - sl[i].start, Fr, inplace=True, world=2) for i in (1, 2)])
    gw1_0 = encs[0].conv1_wgrad(lm, B, Fr)
    gw1 = sum(encs[i].conv1_wgrad(lm[sl[i]].contiguous(), sl[i].stop - sl[i].start, Fr) for i in (1, 2))
    gtol = 1e-4 if precision != "f16" else 2e-2   # f16: a different scale exponent moves single float16 roundings
    close(torch.cat(dfilm[1:], 0).cpu(), dfilm[0].cpu(), gtol)
    close((r2[0][1] + r2[1][1]).cpu(), dbn2_0.cpu(), gtol)
    close((r1[0][1] + r1[1][1]).cpu(), dbn1_0.cpu(), gtol)
    close(gw2.cpu(), gw2_0.cpu(), gtol)
    close(gw1.cpu(), gw1_0.cpu(), gtol)
    # and without the exchange the shards do NOT reproduce the whole batch (per-rank statistics, the default)
    (_, tl), = lockstep([encs[1].forward_train_steps(lm[sl[1]].contiguous(), feats[sl[1]].contiguous(), head=False, world=0)])
    assert (tl["pool_in"] - t0["pool_in"][sl[1]]).abs().max().item() > 1e-3 * t0["pool_in"].abs().max().item()


def _stacked_trunk_params(model):
    cn = model.audio_encoder.subnet_cnns
    st = lambda f: torch.stack([f(c) for c in cn]).detach()  # noqa: E731
    return (st(lambda c: c.conv1.weight), st(lambda c: c.conv1.bias), st(lambda c: c.bn1.weight), st(lambda c: c.bn1.bias),
            st(lambda c: c.conv2.weight), st(lambda c: c.conv2.bias), st(lambda c: c.bn2.weight), st(lambda c: c.bn2.bias))


@pytest.mark.parametrize("T,B,gain", [(66150, 3, 1.0), (44100, 10, 3.0e3)])
def test_f16_train_forward_matches_the_oracle_with_f16_operands(T, B, gain):
    """f16-operand training forward (`mst_encoder_set_train_precision(enc, 1)`; BASELINE configs[4] / the reference's
    --use_amp convolutions): conv inputs and weights rounded to float16, fp32 accumulation, train-mode BatchNorm -- against
    the oracle evaluated with exactly those roundings; the weight fragments come from the per-step device rebuild.
    gain 3e3 multiplies conv1's weights: BatchNorm(batch statistics) removes it again, so the activations stay O(1), but the
    weights themselves (max ~1e2) and the bound that the per-band range scale is derived from grow with it."""
    from oracle.train_f16 import round_f16_ideal  # noqa: F401  (the oracle's f16_operands path is the eval-tested one)
    cfg = cases.CFG_DEFAULT
    model, sd = build_model(cfg)
    if gain != 1.0:
        with torch.no_grad():
            for c in model.audio_encoder.subnet_cnns:
                c.conv1.weight.mul_(gain), c.conv1.bias.mul_(gain)
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x = torch.stack([cases.synth_clip(c % 4, T) * (1.0 + 0.1 * (c // 4)) for c in range(B)], 0)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, 64, generator=g) * 3.0
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        enc = model.hip_encoder()
        e32, t32 = enc.forward_train(lm, feats.cuda())
        enc.set_train_precision(True)
        enc.update_trunk_params(*_stacked_trunk_params(model))
        emb, t = enc.forward_train(lm, feats.cuda())
        enc.set_train_precision(False)
    torch.cuda.synchronize()
    taps = {}
    want = oenc.encoder_from_logmel(sd, lm.cpu(), feats, cfg["split_size"], cfg["overlap"], taps, f16_operands=True, bn_training=True,
                                    f16_outputs=True)
    ns = cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"])
    for i in (0, ns // 2, ns - 1):
        for name in ("bn1", "bn2"):
            mean, var = taps[f"{name}_{i}"]
            got = t[name][i].cpu()
            close(got[:, 0], mean, 1e-4)
            close(1.0 / got[:, 1] ** 2 - 1e-5, var, 2e-4)
        close_f16(t["pool1"][:, i].cpu(), taps[f"pool1_{i}"])
    close_f16(t["pool_in"].cpu(), taps["pool_in"], frac=5e-3)   # second layer: flipped inputs and flipped stored outputs add up
    close(emb.cpu(), want, 2e-4)
    d = (emb - e32).abs().max().item() / e32.abs().max().item()
    print(f"f16-operand training forward vs exact fp32 training forward: embeddings {d:.2e} of max")
    assert 1e-6 < d < 2e-2   # it IS the f16 arithmetic, and it is close to fp32


@pytest.mark.parametrize("cfgname,loss_gain", [("default", 1.0), ("default", 1.0e-6), ("baseline_sh", 1.0)])
def test_f16_training_gradients_match_autograd_with_the_same_operand_roundings(cfgname, loss_gain):
    """`train_precision="f16"`: loss, every parameter gradient and the running statistics against float64 autograd of the
    same modules whose convolutions round BOTH operands of the forward product, of the input gradient and of the weight
    gradient to float16 precision and store their outputs as float16 (oracle/train_f16.py) -- the arithmetic contract of the
    mode (include/mst.h).
    The internal power-of-two loss scale makes the result independent of the magnitude of the upstream gradient: with
    loss_gain 1e-6 the unscaled d(conv output) values (~1e-9) would vanish in float16.
    Rounding to float16 makes the loss piecewise smooth: an evaluation that differs from float64 in the last fp32 bits
    crosses a few rounding boundaries and max-pool ties, and each crossing moves one sub-band's gradients by 1e-3..1e-2
    (batch of 10 one-second clips: a pooled plane has 16 entries per clip and channel).  That is a property of the
    arithmetic, not of the kernels: the SAME oracle evaluated by PyTorch in fp32 deviates from its float64 evaluation in
    the same way, largely in the same sub-bands.  Hence the criterion, relative to that fp32 evaluation: median error
    below 1e-4 (or 1.5 x PyTorch-fp32's median), at least half of the tensors within 2e-4, no more tensors beyond 1e-3 than PyTorch-fp32 has + 3, worst
    deviation at most 3 x PyTorch-fp32's worst (or 2e-2: which sub-band crosses a boundary, and how many of its 16 pooled
    entries per clip and channel move, differs between any two fp32 evaluations).  The exact-fp32 trunk is 1.7e-2 (median) away from this
    oracle, i.e. the test does tell f16 arithmetic from fp32 arithmetic.  Everything goes into the parity report."""
    import copy
    from oracle.train_f16 import convert_convs
    cfg = cases.CFG_BASELINE_SH if cfgname == "baseline_sh" else cases.CFG_DEFAULT   # baseline_sh: 16-mel sub-bands, MaxPool (1, 5)
    model, sd = build_model(cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    exact = copy.deepcopy(model)
    ref32 = convert_convs(copy.deepcopy(model))
    ref64 = convert_convs(copy.deepcopy(model).double())
    for m_ in (model, exact, ref32, ref64):
        m_.train()
    model.train_backend, exact.train_backend, ref32.train_backend, ref64.train_backend = "hip-strict", "hip-strict", "torch", "torch"
    model.train_precision, exact.train_precision = "f16", "fp32"
    B, T = 10, 44100    # two groups of 8 clips for the weight-gradient kernels, the second one ragged
    x = torch.stack([cases.synth_clip(c % 4, T) * (1.0 + 0.1 * (c // 4)) for c in range(B)], 0).cuda()
    stems = omel.tensor_to_stems_dict(x)
    g = torch.Generator().manual_seed(8)
    feats = (torch.randn(B, 64, generator=g) * 2.0).cuda()
    R = (torch.randn(B, cfg["embed_dim"], generator=g) * loss_gain).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(stems)
    la = (model.forward_from_logmel(lm, feats) * R).sum()
    lb = (exact.forward_from_logmel(lm, feats) * R).sum()
    lt = (ref32.forward_from_logmel(lm, feats) * R).sum()
    lc = (ref64.forward_from_logmel(lm.double(), feats.double()) * R.double()).sum()
    la.backward(), lb.backward(), lt.backward(), lc.backward()
    assert model._hip_train.train_f16 and not exact._hip_train.train_f16
    close(la.item(), lc.item(), 1e-4)
    errs = []
    grads = dict(model.named_parameters())
    for (n, pa), (_, pb), (_, pt), (_, pc) in zip(model.named_parameters(), exact.named_parameters(), ref32.named_parameters(),
                                                  ref64.named_parameters()):
        assert pa.grad is not None and torch.isfinite(pa.grad).all(), n
        den = pc.grad.abs().max().item()
        if "subnet_cnns" in n and n.endswith(("conv1.bias", "conv2.bias")):
            wmax = grads[n[:-4] + "weight"].grad.abs().max().item()
            assert pa.grad.abs().max().item() < 1e-3 * wmax, n
            continue
        if den < 1e-9 * loss_gain * max(1.0, pc.abs().max().item()):
            continue
        rel = lambda q: (q.grad.double() - pc.grad).abs().max().item() / den  # noqa: E731
        errs.append((n, rel(pa), rel(pb), rel(pt)))
    e16, far, t32 = (np.array([e[k] for e in errs]) for k in (1, 2, 3))
    out = [(n, f"{a:.1e}") for n, a, _, _ in errs if a >= 1e-3]
    print(f"f16 training [{cfgname}], loss gain {loss_gain:g}: gradient error vs the float64 oracle with f16 operand roundings over {len(errs)} "
          f"tensors: worst {e16.max():.2e}, median {np.median(e16):.2e}, within 2e-4: {int((e16 < 2e-4).sum())}, beyond 1e-3: {out}; "
          f"the same oracle in PyTorch fp32: worst {t32.max():.2e}, median {np.median(t32):.2e}, beyond 1e-3: {int((t32 >= 1e-3).sum())}; "
          f"exact-fp32 trunk vs the oracle (= how far f16 arithmetic is from fp32): median {np.median(far):.2e}, worst {far.max():.2e}")
    parity.note(f"f16 train gradients vs float64 autograd with f16 operand roundings [{cfgname}, loss gain {loss_gain:g}], norm-wise per tensor",
                tensors=len(errs), hip_max=float(e16.max()), hip_p90=float(np.percentile(e16, 90)), hip_median=float(np.median(e16)),
                hip_within_2e4=int((e16 < 2e-4).sum()), hip_beyond_1e3=len(out), torch_fp32_same_oracle_max=float(t32.max()),
                torch_fp32_same_oracle_beyond_1e3=int((t32 >= 1e-3).sum()), fp32_trunk_vs_f16_oracle_median=float(np.median(far)))
    assert np.median(e16) < max(1e-4, 1.5 * np.median(t32)) and (e16 < 2e-4).sum() >= 0.5 * len(errs), (np.median(e16), (e16 < 2e-4).sum())
    assert len(out) <= (t32 >= 1e-3).sum() + 3 and e16.max() <= max(3.0 * t32.max(), 2e-2), (out, e16.max(), t32.max())
    assert np.median(far) > 10.0 * np.median(e16)   # the oracle's roundings are the ones the kernels apply, not fp32's
    for (n, ba), (_, bc) in zip(model.named_buffers(), ref64.named_buffers()):
        if "running" in n:
            close(ba.cpu(), bc.cpu(), 1e-4)


def test_train_mode_backward_of_pool_relu_film_batchnorm():
    """`mst_encoder_train_backward_apply` (max-pool -> ReLU -> FiLM -> BatchNorm with batch statistics, both
    layers) against torch autograd through the oracle: gradient of the convolution outputs, of the FiLM parameters and
    of the BatchNorm weight / bias.  The convolution input gradient between the layers comes from autograd here."""
    cfg = cases.CFG_DEFAULT
    model, sd = build_model(cfg)
    B, T = 2, 66150
    x = torch.stack([cases.synth_clip(c, T) for c in range(B)], 0)
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(B, 64, generator=g) * 3.0
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
        enc = model.hip_encoder()
        emb, t = enc.forward_train(lm, feats.cuda())
    frames = lm.shape[-1]
    # oracle with autograd: leaf = FiLM parameters and the BN affine parameters
    sdg = {k: v.clone() for k, v in sd.items()}
    ns = cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"])
    for i in range(ns):
        for k in ("bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias", "conv1.weight", "conv2.weight"):
            sdg[f"audio_encoder.subnet_cnns.{i}.{k}"].requires_grad_(True)
    film = oenc.film_params(sd, feats).clone().requires_grad_(True)
    taps = {}
    lmc = lm.cpu()
    outs = [oenc.subband_cnn(sdg, i, lmc[:, :, i * 10:i * 10 + 20, :], film, 20, taps, bn_training=True) for i in range(ns)]
    cat = torch.cat(outs, dim=1)
    pool_in = cat.reshape(B, cat.shape[1] * cat.shape[2], cat.shape[3])
    for i in range(ns):
        taps[f"pool1_{i}"].retain_grad()
    R = torch.randn(pool_in.shape, generator=g)
    (pool_in * R).sum().backward()
    # native: layer 2 from d pool_in = R, layer 1 from autograd's d pool1
    dfilm = torch.zeros(B, ns * 192, device="cuda")
    dy2, dbn2 = enc.backward_apply(2, R.cuda(), dfilm, B, frames)
    dp1 = torch.stack([taps[f"pool1_{i}"].grad for i in range(ns)], 1).cuda()       # (B, ns, 32, 10, W1)
    dy1, dbn1 = enc.backward_apply(1, dp1, dfilm, B, frames)
    torch.cuda.synchronize()
    for i in (0, ns // 2, ns - 1):
        close(dy2[i].cpu(), taps[f"conv2_out_{i}"].grad, 2e-4)
        close(dy1[i].cpu(), taps[f"conv1_out_{i}"].grad, 2e-4)
        pfx = f"audio_encoder.subnet_cnns.{i}."
        close(dbn2[i, :, 0].cpu(), sdg[pfx + "bn2.weight"].grad, 2e-4)
        close(dbn2[i, :, 1].cpu(), sdg[pfx + "bn2.bias"].grad, 2e-4)
        close(dbn1[i, :, 0].cpu(), sdg[pfx + "bn1.weight"].grad, 2e-4)
        close(dbn1[i, :, 1].cpu(), sdg[pfx + "bn1.bias"].grad, 2e-4)
    close(dfilm.cpu(), film.grad, 2e-4)


@pytest.mark.parametrize("cfgname", ["default", "baseline_sh", "default-f16x3", "baseline_sh-f16x3"])
def test_hip_trunk_training_gradients_match_autograd_of_the_torch_modules(cfgname):
    """`train_backend="hip"` (conv trunk forward + backward in libmst.so) against PyTorch autograd of the same modules
    evaluated in FLOAT64: loss, every parameter gradient, running statistics.  Almost all gradients agree to ~2e-6.  Isolated
    larger deviations are fp32 effects that hit ANY fp32 implementation -- sums over 10^5 positions with heavy cancellation
    (conv1.weight of the lowest sub-band: x ~ -23, the log-mel silence floor, against sum(dy) = 0), near-tie max-pool arg-max
    decisions, fp32 BatchNorm reductions -- and PyTorch's own fp32 path shows more of them (on the reference's
    train_baseline.sh shapes it is 3.7e-2 off in one sub-band where the HIP trunk is at 2e-6), so the
    check is: every tensor within 5e-2, at least 95 % of them within 1e-4, and no more outliers than PyTorch fp32 has + 3.
    Dropout off (p = 0) for the comparison; with p = 0.3 the native forward must agree with the mask it is given."""
    import copy
    cfg = cases.CFG_BASELINE_SH if cfgname.startswith("baseline_sh") else cases.CFG_DEFAULT   # baseline_sh: the reference's scripts/train_baseline.sh
    model, sd = build_model(cfg)
    if cfgname.endswith("f16x3"):   # all convolution-shaped products on 3-term split-precision f16: held to the SAME bar as the fp32 kernels
        model.train_precision = "f16x3"
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    ref32 = copy.deepcopy(model)
    ref64 = copy.deepcopy(model).double()
    for m_ in (model, ref32, ref64):
        m_.train()
    model.train_backend, ref32.train_backend, ref64.train_backend = "hip", "torch", "torch"
    B, T = 4, 44100
    x = torch.stack([cases.synth_clip(c, T) for c in range(B)], 0).cuda()
    stems = omel.tensor_to_stems_dict(x)
    g = torch.Generator().manual_seed(8)
    feats = (torch.randn(B, 64, generator=g) * 2.0).cuda()
    R = torch.randn(B, cfg["embed_dim"], generator=g).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(stems)
    la = (model.forward_from_logmel(lm, feats) * R).sum()
    lb = (ref32.forward_from_logmel(lm, feats) * R).sum()
    lc = (ref64.forward_from_logmel(lm.double(), feats.double()) * R.double()).sum()
    la.backward(), lb.backward(), lc.backward()
    close(la.item(), lc.item(), 1e-5)
    worst_hip = worst_t32 = 0.0
    errs = []
    grads = dict(model.named_parameters())
    for (n, pa), (_, pb), (_, pc) in zip(model.named_parameters(), ref32.named_parameters(), ref64.named_parameters()):
        assert pa.grad is not None, n
        den = pc.grad.abs().max().item()
        if "subnet_cnns" in n and n.endswith(("conv1.bias", "conv2.bias")):
            # a bias in front of a batch-statistics BatchNorm has gradient exactly 0 (the mean is removed)
            wmax = grads[n[:-4] + "weight"].grad.abs().max().item()
            assert pa.grad.abs().max().item() < 1e-3 * wmax, n
            continue
        if den < 1e-9 * max(1.0, pc.abs().max().item()):   # e.g. attention.2.bias: softmax is shift-invariant
            continue
        d_hip = (pa.grad.double() - pc.grad).abs().max().item() / den
        d_t32 = (pb.grad.double() - pc.grad).abs().max().item() / den
        worst_hip, worst_t32 = max(worst_hip, d_hip), max(worst_t32, d_t32)
        errs.append((n, d_hip, d_t32))
    # Two fp32 effects produce isolated deviations from float64 autograd in ANY fp32 implementation (PyTorch's own fp32
    # path, evaluated next to ours, shows them too -- more of them and larger):
    #  (1) conditioning of the conv1 WEIGHT gradients: sum_p dy[p] x[p] over ~10^5 positions with x on the log-mel silence
    #      floor (-23.03, e.g. the synthetic vocals' silent first fifth) while sum_p dy[p] = 0 (batch-statistics BatchNorm
    #      removes the mean): the products cancel to ~1e-3 of their magnitude -> up to a few 1e-3 relative error;
    #  (2) near-tie max-pool decisions: where two candidates of a pooling window agree to fp32 rounding, fp32 and float64
    #      pick different winners and route the gradient differently; that perturbs ONE sub-band's tensors (and, through
    #      its FiLM gradient, the small FiLM MLP) by ~1e-3.  Which band is hit depends on the input's last bits.
    # Hence: every tensor within 1e-2, at least 80 % of them within 1e-4, no more outliers than PyTorch fp32 shows + 3, and
    # the worst deviation no larger than PyTorch fp32's worst or 5e-3.  The full distribution goes into the parity report.
    out_hip = [(n, f"{a:.1e}") for n, a, _ in errs if a >= 1e-4]
    out_t32 = [(n, f"{b:.1e}") for n, _, b in errs if b >= 1e-4]
    print(f"{cfgname}: parameter-gradient error vs float64 autograd over {len(errs)} tensors: hip trunk worst {worst_hip:.2e}, "
          f"outliers {out_hip}; PyTorch fp32 worst {worst_t32:.2e}, {len(out_t32)} outliers")
    hip_errs = np.array([a for _, a, _ in errs])
    parity.note(f"train gradients vs float64 autograd [{cfgname}], norm-wise per tensor", tensors=len(errs),
                hip_max=float(hip_errs.max()), hip_p90=float(np.percentile(hip_errs, 90)), hip_median=float(np.median(hip_errs)),
                hip_beyond_1e4=len(out_hip), torch_fp32_max=worst_t32, torch_fp32_beyond_1e4=len(out_t32))
    # (a near-tie max-pool decision that fp32 and float64 resolve differently moves one sub-band's tensors and the FiLM MLP behind
    # them by 1e-2 .. 4e-2 in ANY fp32 implementation -- PyTorch fp32 shows it on these very inputs; which side of the tie an
    # implementation lands on depends on the last bit of its FiLM parameters: hence a bound relative to PyTorch fp32 on the same
    # data, next to the fixed 1e-2)
    assert worst_hip < max(1e-2, 1.05 * worst_t32) and len(out_hip) <= 0.2 * len(errs) and len(out_hip) <= len(out_t32) + 3, out_hip
    assert worst_hip <= max(1.05 * worst_t32, 5e-3), (worst_hip, worst_t32)   # (5 %: the same near-tie flip, other roundings around it)
    for (n, ba), (_, bc) in zip(model.named_buffers(), ref64.named_buffers()):
        if "running" in n:
            close(ba.cpu(), bc.cpu(), 1e-4)
    # several forward passes may be alive at once (every pass owns its activation workspace): two forwards, then both backwards
    # in the "wrong" order, give twice the gradient of one pass; walking ONE graph twice works where the backward leaves the
    # activations intact (the f16 kernels) and is refused loudly where it does not (the fp32 kernels work in place)
    for prec, walks in (("fp32", 1), ("f16x3", 2)):
        model.train_precision = prec
        model.zero_grad()
        (model(stems, feats) * R).sum().backward()
        g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.zero_grad()
        o1 = (model(stems, feats) * R).sum()
        o2 = (model(stems, feats) * R).sum()
        o1.backward(retain_graph=True)
        o2.backward()
        if walks == 2:
            o1.backward()
        for n, p in model.named_parameters():
            den = g1[n].abs().max().item()
            if den > 1e-9:
                assert (p.grad - (1.0 + walks) * g1[n]).abs().max().item() <= 1e-5 * den * (1.0 + walks), (prec, n)
        if walks == 1:
            with pytest.raises(RuntimeError, match="second backward"):
                o1.backward()
    # ... and with DIFFERENT parameters in the passes that are alive together: forward A (P0), forward B (P1), backward A (the
    # fragments go back to P0), forward C (P2), backward B -- B's convolution input gradient and BatchNorm backward must run
    # on P1 (a pass counter that is written back by a backward would mistake C's fragments for B's)
    for prec in ("fp32", "f16x3"):
        model.train_precision = prec
        trunk = [q for c in model.audio_encoder.subnet_cnns for q in (c.conv2.weight, c.bn1.weight)]
        P0 = [q.detach().clone() for q in trunk]

        def put(k):   # trunk parameters only: their values reach the graph through torch.stack copies, nothing saved is modified
            with torch.no_grad():
                for q, q0 in zip(trunk, P0):
                    q.copy_(q0 * (1.0 + 0.07 * k) + 0.013 * k * (q0.dim() == 1))
        put(1)
        model.zero_grad()
        (model(stems, feats) * R).sum().backward()
        gB = {n: q.grad.clone() for n, q in model.named_parameters()}
        put(0)
        oA = (model(stems, feats) * R).sum()
        put(1)
        oB = (model(stems, feats) * R).sum()
        oA.backward()
        put(2)
        oC = (model(stems, feats) * R).sum()   # noqa: F841  (alive, never walked)
        model.zero_grad()
        oB.backward()
        for n, q in model.named_parameters():
            den = gB[n].abs().max().item()
            if den > 1e-9:
                assert (q.grad - gB[n]).abs().max().item() <= 1e-5 * den, (prec, n)
        put(0)
        del oC
    model.train_precision = "fp32"
    # dropout after the first pooling: every element is either dropped or scaled by 1 / (1 - p)
    enc = model._hip_train
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(stems)
        film = model.film_encoder.film_head(model.film_encoder.feature_mlp(feats))
        _, t0 = enc.forward_train(lm, film=film, head=False)
        mask = (torch.rand(t0["pool1"].shape, device="cuda") >= 0.3).to(torch.uint8)
        _, t1 = enc.forward_train(lm, film=film, head=False, drop1_mask=mask, drop1_p=0.3)
    assert torch.equal(t1["pool1"], torch.where(mask.bool(), t0["pool1"] * (1.0 / 0.7), torch.zeros_like(t0["pool1"])))


@pytest.mark.parametrize("cfgname", ["default", "baseline_sh"])
def test_conv2_input_gradient_with_dropout_mask(cfgname):
    """`mst_encoder_train_conv2_dgrad` (chunked fp32-MFMA conv on dy2 with transposed / flipped weights, Dropout keep-mask
    fused into the store) against the float64 input gradient of F.conv2d times the same mask."""
    cfg = cases.CFG_DEFAULT if cfgname == "default" else cases.CFG_BASELINE_SH
    model, sd = build_model(cfg)
    from mst_amd.model import HipEncoder
    enc = HipEncoder(model, "fp32")
    ns = cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"])
    B, frames = 3, 431
    H1, W1 = cfg["split_size"] // enc.sub, frames // 5
    g = torch.Generator().manual_seed(12)
    dy2 = torch.randn(ns, B, 64, H1, W1, generator=g)
    mask = (torch.rand(B, ns, 32, H1, W1, generator=g) >= 0.3).to(torch.uint8)
    got = enc.conv2_dgrad(dy2.cuda(), B, frames, mask.cuda(), 0.3).cpu()
    got_nomask = enc.conv2_dgrad(dy2.cuda(), B, frames).cpu()
    for i in (0, ns // 2, ns - 1):
        w = sd[f"audio_encoder.subnet_cnns.{i}.conv2.weight"].double()
        ref = torch.nn.grad.conv2d_input((B, 32, H1, W1), w, dy2[i].double(), padding=3)
        close(got_nomask[:, i], ref, 1e-5)
        close(got[:, i], ref * mask[:, i].double() / 0.7, 1e-5)


def test_song_a_real_music_end_to_end():
    """BASELINE configs[0] on the GPU: real music through stage A + HIP encoder vs the reference goldens (bs=2)."""
    from test_melfeat_gpu import check_feats, check_logmel
    g = np.load(os.path.join(G, "song_a.npz"))
    x = cases.song_a_clips()
    model, sd = build_model(cases.CFG_DEFAULT)
    from mst_amd.mixing_utils import MixingFeatureExtractor
    stems = omel.tensor_to_stems_dict(x.cuda())
    feats, lm = MixingFeatureExtractor().features_and_logmel(stems)
    check_feats(feats.cpu(), g["features"])
    check_logmel(lm.cpu(), omel.logmel(x), x=x)
    idx = torch.from_numpy(g["logmel_idx"])
    d = ((lm.cpu().flatten()[idx] - torch.from_numpy(g["logmel_samples"])).abs() /
         torch.from_numpy(g["logmel_samples"]).abs().clamp(min=1.0))
    print(f"song_A log-mel vs reference samples: max {d.max().item():.2e}, 99.9th pct {d.quantile(0.999).item():.2e}, "
          f"mean {d.mean().item():.2e}")
    with torch.no_grad():
        emb = model(stems, feats)
        model.conv1_precision = "f16x3-all"
        emb16 = model(stems, feats)
        model.conv1_precision = "fp32"
    close(emb.cpu(), g["embedding"], 2e-4)
    close(emb16.cpu(), g["embedding"], 2e-4)
    # Element-wise on real music the literal 1e-4 cannot be asked of ANY fp32 implementation: the log-mel of low-passed stems carries
    # fp32 FFT noise in its quiet bins (check_logmel) and a handful of embedding elements inherit it.  The allowance is derived from
    # the data, not a constant: the same encoder evaluated in FLOAT64 on the float64 log-mel of the same clips is the yardstick,
    # and the reference's own fp32 embedding (the golden) is measured against it first -- here 27 of 1536 elements are beyond 1e-4,
    # the worst by 2.8e-4.  The kernels may miss the float64 result on at most 1.25 x as many elements (+ 4) and by at most 2 x
    # as much as the reference's own arithmetic does.
    from test_melfeat_gpu import fft_noise_unit
    _, lm64 = fft_noise_unit(x)
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    e64 = oenc.encoder_from_logmel(sd64, lm64, torch.from_numpy(g["features"]).double(), cases.CFG_DEFAULT["split_size"],
                                   cases.CFG_DEFAULT["overlap"])
    floor = 1e-2 * e64.abs().amax(dim=1, keepdim=True)

    def vs64(e):
        rel = (e.double() - e64).abs() / torch.maximum(e64.abs(), floor)
        return int((rel > 1e-4).sum()), float(rel.max())
    miss_ref, worst_ref = vs64(torch.from_numpy(g["embedding"]))
    parity.note("song_A embedding: the reference's own fp32 output vs the float64 encoder", beyond_1e_4=miss_ref, worst=worst_ref,
                elements=int(e64.numel()))
    assert worst_ref < 1e-3, "the float64 yardstick and the reference golden disagree: fixture or oracle broken"
    for name, e in (("fp32 kernels", emb), ("f16x3-all", emb16)):
        miss, worst = vs64(e.cpu())
        parity.note(f"song_A embedding: {name} vs the float64 encoder", beyond_1e_4=miss, worst=worst,
                    allowed_beyond=int(1.25 * miss_ref + 4), allowed_worst=2.0 * max(worst_ref, 1e-4))
        parity.record(f"song_A embedding {name} vs reference [element-wise]", e.cpu(), g["embedding"])
        assert miss <= 1.25 * miss_ref + 4, f"{name}: {miss} elements beyond 1e-4 of the float64 result; the reference's own fp32: {miss_ref}"
        assert worst <= 2.0 * max(worst_ref, 1e-4), f"{name}: worst element {worst:.2e} vs the reference's own {worst_ref:.2e}"


def test_retrieval_validation_on_hip_path(tmp_path):
    """build_embedding_cache / compute_track_embedding (reference src/validation_utils.py:106-214) over
    track directories and PCM shards, 1 s query segments -> embeddings equal the oracle's on the same samples; the
    retrieval metric finds every track from a later, overlapping segment of itself."""
    import wave
    from mst_amd import ingest, validation_utils as vu
    from mst_amd.mixing_utils import MixingFeatureExtractor
    from oracle import features as ofeat
    model, sd = build_model(cases.CFG_DEFAULT)
    ext = MixingFeatureExtractor()
    sr, L = 44100, 60000

    class DS:
        track_dirs = []
    tracks = []
    for t in range(5):
        x = ingest.float_to_pcm16(cases.synth_clip(20 + t, L))        # int16 so that wav / shard / oracle agree exactly
        tracks.append(x.float() / 32768.0)
        if t < 3:                                                      # reference layout: 4 x {stem}.wav
            d = tmp_path / f"track{t}"
            d.mkdir()
            for i, s in enumerate(cases.STEMS):
                with wave.open(str(d / f"{s}.wav"), "wb") as w:
                    w.setnchannels(2); w.setsampwidth(2); w.setframerate(sr)
                    w.writeframes(x[2 * i:2 * i + 2].T.contiguous().numpy().astype("<i2").tobytes())
            DS.track_dirs.append(str(d))
        else:                                                          # PCM shard
            p = str(tmp_path / f"track{t}.pcm16")
            ingest.write_pcm_shard(p, x, sr)
            DS.track_dirs.append(p)
    DS.track_dirs.append(str(tmp_path / "missing_track"))              # reported and skipped, as in the reference
    cache = vu.build_embedding_cache(DS, list(range(6)), model, ext, None, "cuda", query_duration=1.0,
                                     batch_size=4, stem_ext=".wav")
    assert cache["track_indices"] == [0, 1, 2, 3, 4] and cache["embeddings"].shape == (5, 768)
    seg = torch.stack([t[:, :sr] for t in tracks], 0)
    rf = ofeat.extract_all_features(seg)
    want = oenc.encoder_forward(sd, seg, rf)
    close(cache["embeddings"], want, 2e-4)
    one = vu.compute_track_embedding(DS.track_dirs[1], 0.0, 1.0, model, ext, None, "cuda", stem_ext=".wav")
    close(one, want[1], 2e-4)
    st = vu.load_stems_segment(DS.track_dirs[4], 0.0, 1.0)
    e4 = vu.compute_embedding(st, rf[4], model, "cuda")
    close(e4, want[4], 2e-4)
    # queries: a shifted window of every track against the pool of first seconds
    q = torch.stack([vu.compute_track_embedding(DS.track_dirs[i], 0.05, 1.0, model, ext, None, "cuda", stem_ext=".wav")
                     for i in range(5)])
    m = vu.evaluate_retrieval_accuracy(q, cache["embeddings"], list(range(5)), cache["track_indices"], [1, 5])
    from oracle import retrieval as oret
    assert m == oret.evaluate_retrieval_accuracy(q, cache["embeddings"], list(range(5)), cache["track_indices"], (1, 5))
    # (no accuracy level is asserted: a random-init encoder does not separate synthetic tracks; the metric itself is
    #  pinned by the reference-generated fixture in test_data_dist_cpu.py, with top-1 0.6 < top-5 0.85)
    vu.save_cache(cache, str(tmp_path / "c" / "cache.pt"))
    assert torch.equal(vu.load_cache(str(tmp_path / "c" / "cache.pt"))["embeddings"], cache["embeddings"])


def test_embedding_cache_matches_the_reference_loop_fixture(tmp_path):
    """f3 against the REFERENCE: tests/golden/dataset.npz holds the cache that the reference's own
    validation_utils.build_embedding_cache + MixingFeatureExtractor + MixingStyleEncoder (CPU) built for the toy
    tracks of tests/cases.py (0.5 s queries; shorter tracks zero-padded; mono stems duplicated)."""
    from mst_amd import validation_utils as vu
    from mst_amd.data import FMABaselineDataset
    gd = np.load(os.path.join(G, "dataset.npz"))
    root = cases.write_toy_tracks(str(tmp_path))
    model, _ = build_model(cases.CFG_DEFAULT)
    ds = FMABaselineDataset(root, clip_duration=0.25)
    where = {os.path.basename(d): i for i, d in enumerate(ds.track_dirs)}
    names = gd["vu.cache_tracks"].tolist()
    cache = vu.build_embedding_cache(ds, [where[n] for n in names], model, ds.feature_extractor, None, "cuda",
                                     query_duration=0.5, batch_size=3)
    assert [os.path.basename(p) for p in cache["track_paths"]] == names
    close(cache["embeddings"], gd["vu.cache_embeddings"], 2e-4)
    one = vu.compute_track_embedding(ds.track_dirs[where["e_mono"]], 0.0, 0.5, model, ds.feature_extractor, None, "cuda")
    close(one, gd["vu.cache_embeddings"][names.index("e_mono")], 2e-4)
    # the Dataset with compute_features=True (main process, GPU) against the reference's in-worker CPU features
    dsf = FMABaselineDataset(root, clip_duration=0.25, num_segments=2, compute_features=True)
    np.random.seed(42)
    items = [dsf[where[n]] for n in sorted(cases.TOY_TRACKS)]
    got = torch.stack([f for it in items for f in it[1]])
    rf = torch.from_numpy(gd["fma2.features"])
    err = ((got - rf).abs() / (rf.abs() + 2.0)).max().item()
    print(f"dataset features vs reference fixture: scaled err {err:.2e}")
    assert err < 1e-4


def test_training_step_is_bit_deterministic():
    """The reference trainer asks for deterministic behaviour (src/train.py:22-31).  Every cross-workgroup reduction of the
    training path -- batch statistics, FiLM / BatchNorm gradient sums, both convolution weight gradients, the InfoNCE
    loss -- accumulates through order-independent integer accumulators (csrc/common.h DetAcc) or a fixed-order tree:
    two identical steps from the same state and seed give bit-identical loss and gradients."""
    import copy
    from mst_amd.loss import InfoNCELoss
    cfg = cases.CFG_DEFAULT
    base, _ = build_model(cfg)
    B, T = 6, 44100
    x = torch.stack([cases.synth_clip(c, T) for c in range(B)], 0).cuda()
    stems = omel.tensor_to_stems_dict(x)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(B, 64, generator=g).cuda()
    labels = (torch.arange(B) // 2).cuda()
    runs = []
    for _ in range(2):
        m = copy.deepcopy(base).train()
        m.train_backend = "hip-strict"
        torch.manual_seed(1234)                       # Dropout masks
        loss = InfoNCELoss(0.1)(m(stems, feats), labels)
        loss.backward()
        runs.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()},
                     {n: b.detach().clone() for n, b in m.named_buffers() if "running" in n}))
    (l0, g0, s0), (l1, g1, s1) = runs
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, f"{len(diff)} gradient tensors differ between two identical steps, e.g. {diff[:3]}"
    assert all(torch.equal(s0[n], s1[n]) for n in s0)


CFG_C5 = dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=256, split_size=20, overlap=10, embed_dim=768)   # BASELINE configs[4] shapes
TIE_GAP = 1e-6   # activations are O(1..20): two max-pool candidates closer than this differ by ~an fp32 ulp


@pytest.mark.parametrize("tag,precision", [("default", "fp32"), ("default", "f16x3"), ("c5", "fp32"), ("c5", "f16x3")])
def test_hip_training_step_matches_the_reference_training_fixture(tag, precision):
    """SURVEY 8 f1 pinned by the REFERENCE's own training arithmetic: tests/golden/train.npz was produced by the reference's
    MixingStyleEncoder.train() + InfoNCELoss + loss.backward() (src/train.py:246-262,292-296; src/model.py:118,125 batch
    statistics; Dropout p = 0), in fp32 and in float64, on integer-built PCM clips (bit-identical inputs on every machine).
    The whole product step -- stage A in HIP, the hand-written trunk forward / backward (fp32 MFMA, and the 3-term
    split-precision f16 kernels), the torch FiLM MLP / attention head, the HIP InfoNCE -- is held to the FLOAT64 fixture:
    loss 1e-5, train-mode embeddings and running statistics 1e-4, every parameter gradient 1e-4 of its tensor's max on 512
    sampled entries.  Two classes of tensors have a wider, data-derived bound, and the log names them:
      * a sub-band whose float64 activations hold a max-pool NEAR-TIE (fixture: smallest gap between the two largest candidates
        of a second-pooling window < 1e-6, i.e. an fp32 ulp of the activations): no fp32 evaluation can resolve which position
        wins, the window's gradient is routed to one or the other, and with ~100 windows per (band, channel) that moves the
        band's tensors by up to ~1e-2 (and the shared FiLM MLP behind its FiLM gradient by ~1e-3).  Measured: exactly the
        bands the fixture flags deviate, every other band sits at ~1e-5;
      * conv1 weight gradients, sums of dy * x over ~1e5 positions with x on the log-mel silence floor and sum(dy) = 0
        (cancellation to ~1e-3 of the terms): bound = 3x the deviation of the REFERENCE's own fp32 run from its float64 run; and
        1e-3 where the band's FIRST pooling holds a near-tie (one d(conv1 output) element lands on the neighbouring position)."""
    from mst_amd.loss import InfoNCELoss
    g = np.load(os.path.join(G, "train.npz"))
    cfg = cases.CFG_DEFAULT if tag == "default" else CFG_C5
    B, T = 4, 66150
    x = cases.pcm_batch(B, T)
    assert np.allclose(cases.checksum(x), g[f"{tag}.in_checksum"], rtol=1e-13)   # integer-built input (cases.pcm_clip): the fixture's samples
    stems = omel.tensor_to_stems_dict(x.cuda())
    feats = torch.from_numpy(g[f"{tag}.features"]).cuda()
    labels = torch.from_numpy(g[f"{tag}.labels"]).cuda()
    R = torch.randn(B, cfg["embed_dim"], generator=torch.Generator().manual_seed(77)).cuda()
    names = [str(n) for n in g[f"{tag}.param_names"]]
    gap1, gap2 = g[f"{tag}.pool1_min_gap"], g[f"{tag}.pool2_min_gap"]
    tie_bands = {i for i in range(len(gap2)) if gap2[i] < TIE_GAP}
    assert len(tie_bands) <= 2, "the fixture should leave most sub-bands free of near-ties"
    for lossname in ("infonce", "proj"):
        model, _ = build_model(cfg)
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        model.train()
        model.train_backend, model.train_precision = "hip-strict", precision
        assert [n for n, _ in model.named_parameters()] == names
        emb = model(stems, feats)
        loss = InfoNCELoss(0.1)(emb, labels) if lossname == "infonce" else (emb * R).sum()
        loss.backward()
        torch.cuda.synchronize()
        ref_loss = float(g[f"{tag}.f64.{lossname}.loss"])
        assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss.item(), ref_loss)
        if lossname == "infonce":
            close(emb.detach().cpu(), g[f"{tag}.f64.embedding"], 1e-4, name=f"train fixture [{tag} {precision}] embedding")
            worst_stat = 0.0
            for n, b in model.named_buffers():
                if "running" in n:   # one momentum update from the batch statistics (model.py:118,125 under train())
                    ref = g[f"{tag}.f64.buf.{n}"]
                    worst_stat = max(worst_stat, float(np.abs(b.cpu().double().numpy() - ref).max() / np.abs(ref).max()))
            parity.note(f"train fixture [{tag} {precision}] running statistics after the step, worst tensor (norm-wise)", err=worst_stat)
            assert worst_stat <= 1e-4
        rows, bad = [], []
        gscale = max(float(g[f"{tag}.f64.{lossname}.grad_norm.{n}"][1]) for n in names)   # largest gradient entry of any tensor
        for j, (n, q) in enumerate(model.named_parameters()):
            ref = g[f"{tag}.f64.{lossname}.grad_samples.{n}"]
            r32 = g[f"{tag}.f32.{lossname}.grad_samples.{n}"].astype(np.float64)
            gmax = float(g[f"{tag}.f64.{lossname}.grad_norm.{n}"][1])
            got = q.grad.detach().double().flatten().cpu()[cases.sample_idx(q.numel(), 512, 1000 + j)].numpy()
            if gmax <= 1e-9 * gscale:   # identically zero in exact arithmetic (conv biases in front of a batch-statistics BatchNorm,
                #                             the attention score bias under softmax): float64 leaves rounding dust, nothing to compare
                assert np.abs(got).max() <= 1e-6 * gscale, (n, np.abs(got).max(), gscale)
                continue
            e_hip, e_r32 = float(np.abs(got - ref).max() / gmax), float(np.abs(r32 - ref).max() / gmax)
            band = int(n.split("subnet_cnns.")[1].split(".")[0]) if "subnet_cnns." in n else None
            if band in tie_bands:
                limit, why = 3e-2, "near-tie band"
            elif n.startswith("film_encoder.") and tie_bands:
                limit, why = 5e-3, "FiLM MLP behind a near-tie band"
            elif n.endswith("conv1.weight"):
                limit, why = min(1e-2, max(1e-4, 3.0 * e_r32)), "conv1 weight (cancellation)"
                if gap1[band] < TIE_GAP:   # a first-pooling near-tie moves ONE d(conv1 output) element to the neighbouring position:
                    limit, why = max(limit, 1e-3), "conv1 weight, first-pooling near-tie in this band"   # 1 of ~2000 windows of a channel
            else:
                limit, why = 1e-4, ""
            rows.append((e_hip, e_r32, n, why))
            if e_hip > limit:
                bad.append((n, f"{e_hip:.1e} > {limit:.1e}", why))
        rows.sort(reverse=True)
        strict = np.array([r[0] for r in rows if not r[3]])
        parity.note(f"train fixture [{tag} {precision} {lossname}] gradients vs the reference in float64 (norm-wise per tensor)",
                    tensors=len(rows), held_to_1e4=len(strict), strict_max=float(strict.max()), strict_median=float(np.median(strict)),
                    near_tie_bands=str(sorted(tie_bands)), near_tie_gaps=str([float(f"{gap2[i]:.1e}") for i in sorted(tie_bands)]),
                    worst=rows[0][2], worst_err=rows[0][0], reference_fp32_there=rows[0][1])
        print(f"[{tag} {precision} {lossname}] near-tie bands {sorted(tie_bands)}; worst five: " +
              ", ".join(f"{n.split('audio_encoder.')[-1]} {a:.1e} (ref fp32 {b:.1e}{', ' + w if w else ''})" for a, b, n, w in rows[:5]))
        assert not bad, bad


def test_dropout_drawn_inside_the_pooling_epilogue():
    """Dropout after the first pooling (src/model.py:118, p = 0.3) drawn by the kernel: element o is kept iff
    philox2x32-10(seed, o) >= p * 2^32.  Checked: pool1 == where(mask, undropped / (1 - p), 0) bit for bit with the mask the kernel
    returns; the same seed gives the same mask and another seed a different one; the keep rate is 1 - p (87 k elements per clip:
    within 4 sigma); the draws of a clip's elements do not depend on the batch around it (a pure function of seed and element
    index); and the training step with dropout on is bit-deterministic under torch.manual_seed."""
    from mst_amd.model import HipEncoder
    cfg = cases.CFG_DEFAULT
    model, _ = build_model(cfg)
    B, T = 3, 44100
    x = torch.stack([cases.synth_clip(c, T) for c in range(B)], 0).cuda()
    stems = omel.tensor_to_stems_dict(x)
    feats = (torch.randn(B, 64, generator=torch.Generator().manual_seed(3)) * 2.0).cuda()
    enc = HipEncoder(model, "fp32")
    enc.update_trunk_params(*_stacked_trunk_params(model))
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(stems)
        film = model.film_encoder.film_head(model.film_encoder.feature_mlp(feats))
        _, t0 = enc.forward_train(lm, film=film, head=False)
        _, t1 = enc.forward_train(lm, film=film, head=False, drop1_p=0.3, drop1_seed=1234567)
        _, t2 = enc.forward_train(lm, film=film, head=False, drop1_p=0.3, drop1_seed=1234567)
        _, t3 = enc.forward_train(lm, film=film, head=False, drop1_p=0.3, drop1_seed=1234568)
        _, t4 = enc.forward_train(lm[:1].contiguous(), film=film[:1].contiguous(), head=False, drop1_p=0.3, drop1_seed=1234567)
    m1 = t1["drop1_mask"]
    assert m1.dtype == torch.uint8 and m1.shape == t0["pool1"].shape
    # NB the batch statistics of a 1-clip batch differ, the MASK of clip 0 must not
    assert torch.equal(t4["drop1_mask"][0], m1[0])
    assert torch.equal(t1["pool1"], torch.where(m1.bool(), t0["pool1"] * (1.0 / 0.7), torch.zeros_like(t0["pool1"])))
    assert torch.equal(m1, t2["drop1_mask"]) and torch.equal(t1["pool_in"], t2["pool_in"])
    assert not torch.equal(m1, t3["drop1_mask"])
    n = m1.numel()
    keep = m1.float().mean().item()
    assert abs(keep - 0.7) <= 4.0 * (0.7 * 0.3 / n) ** 0.5 + 1e-4, keep
    # neighbouring elements / channels / clips are uncorrelated at the level a dropout mask needs
    a = m1.float() - 0.7
    for sh, dim in ((1, 4), (1, 3), (1, 2), (1, 0)):
        c = (a * torch.roll(a, sh, dim)).mean().item() / 0.21
        assert abs(c) < 6.0 / n ** 0.5 + 2e-3, (dim, c)
    # end to end: the module's training step with dropout ON is reproducible under the torch seed
    model.train()
    model.train_backend = "hip-strict"
    outs = []
    for _ in range(2):
        torch.manual_seed(99)
        model.zero_grad()
        emb = model(stems, feats)
        emb.square().sum().backward()
        outs.append((emb.detach().clone(), model.audio_encoder.subnet_cnns[5].conv1.weight.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("precision", ["fp32", "f16", "f16x3"])
def test_non_finite_values_stay_visible_in_training(precision):
    """A NaN that enters the trunk (here: one NaN sample in a stem) must come out as non-finite embeddings and gradients, as it
    does under the reference's autocast step -- whose GradScaler then skips the optimizer step (src/train.py:251-262).  The
    float16 stores of the training kernels saturate FINITE values only; a clamp that maps NaN to -65504 would hand the trainer
    finite garbage instead."""
    model, _ = build_model(cases.CFG_DEFAULT)
    model.train()
    model.train_backend, model.train_precision = "hip-strict", precision
    B, T = 2, 44100
    x = torch.stack([cases.synth_clip(c, T) for c in range(B)], 0)
    x[1, 2, 20000] = float("nan")
    feats = (torch.randn(B, 64, generator=torch.Generator().manual_seed(3)) * 2.0).cuda()
    emb = model(omel.tensor_to_stems_dict(x.cuda()), feats)
    emb.sum().backward()
    torch.cuda.synchronize()
    assert not torch.isfinite(emb).all()
    g = torch.stack([c.conv1.weight.grad for c in model.audio_encoder.subnet_cnns])
    assert not torch.isfinite(g).all()
