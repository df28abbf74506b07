"""GPU parity of the small kernels around the convolutions -- FiLM MLP, attention scores, pooling + projection, the feature
finalise kernel and the InfoNCE forward -- at the sizes where THEY can go wrong (row counts below one M-tile, ragged across
tiles, clips that share a tile; band counts that are no multiple of anything; batches of one), not at the workload's size.

References come from oracle/ on the CPU (computed once per geometry and shared), tolerances are the existing ones:
  embeddings  every element within 1e-4 of max(|ref|, 1e-2 max|ref|)      (test_encoder_gpu.close_elementwise)
  film        |d| <= 1e-5 max|ref|                                         (test_encoder_gpu's bar for the FiLM tap)
  features    |d| <= 1e-4 |ref| + 2e-4                                     (test_melfeat_gpu.check_feats)
  loss        rtol 1e-5, atol 1e-6                                         (test_aug_loss_gpu)
"""
import functools

import numpy as np
import pytest
import torch

import cases
from oracle import encoder as oenc
from oracle import features as ofeat
from oracle import loss as oloss
from oracle import mel as omel
from test_encoder_gpu import G, close, close_elementwise
from test_melfeat_gpu import check_feats

pytestmark = pytest.mark.gpu

GEOM = {"default": cases.CFG_DEFAULT,          # 1024/256/128 mels, 20/10 sub-bands: 11 bands, C = 1408, E = 768
        "baseline_sh": cases.CFG_BASELINE_SH}  # 2048/512/80 mels, 16/8 sub-bands: 9 bands, C = 2304, E = 512
BMAX = 17


@functools.lru_cache(maxsize=None)
def _model(geom, feature_dim=64):
    from mst_amd.model import MixingStyleEncoder
    cfg = GEOM[geom]
    m = MixingStyleEncoder(channels=8, feature_dim=feature_dim, encoder_backend="hip", **cfg)
    sd = cases.make_state_dict(cfg, seed=42, feature_dim=feature_dim)
    full = dict(m.state_dict())
    full.update(sd)
    m.load_state_dict(full, strict=True)
    return m.cuda().eval(), sd


@functools.lru_cache(maxsize=None)
def _case(geom, frames, feature_dim=64):
    """17 clips of `frames` frames: the log-mel (device), the features, and the oracle's FiLM parameters and embeddings of all 17
    (eval mode: a clip's reference does not depend on the batch, so B = 1 and 3 read the first rows)."""
    model, sd = _model(geom, feature_dim)
    cfg = GEOM[geom]
    T = (frames - 1) * cfg["hop_length"]
    x = torch.stack([cases.synth_clip(c % 6, T + 4000)[:, 4000:] * (1.0 + 0.05 * (c // 6)) for c in range(BMAX)], 0)
    feats = torch.randn(BMAX, feature_dim, generator=torch.Generator().manual_seed(7)) * 2.0
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
    assert lm.shape[-1] == frames
    taps = {}
    oemb = oenc.encoder_from_logmel(sd, lm.cpu(), feats, cfg["split_size"], cfg["overlap"], taps)
    return model, lm, feats.cuda(), oemb, taps["film"]


@pytest.mark.parametrize("B", [1, 3, BMAX])
@pytest.mark.parametrize("frames", [20, 105, 345])   # W2 = 1, 5, 17: B * W2 below one 16-row M-tile, ragged, clips sharing tiles
@pytest.mark.parametrize("geom", ["default", "baseline_sh"])
def test_head_embeddings_vs_oracle(geom, frames, B):
    model, lm, feats, oemb, _ = _case(geom, frames)
    with torch.no_grad():
        emb = model.hip_encoder().forward(lm[:B].contiguous(), feats[:B].contiguous())
    assert tuple(emb.shape) == (B, GEOM[geom]["embed_dim"])
    close_elementwise(emb.cpu(), oemb[:B], name=f"small kernels: embeddings {geom} frames={frames} B={B}")


@pytest.mark.parametrize("geom", ["default", "baseline_sh"])
def test_head_is_batch_independent(geom):
    """Clips 0, 8 and 16 of a batch of 17 (first, middle of a clip tile, alone in the last tile) against the same clips run
    alone: the same bits -- no partition of K and no reduction order may depend on B or on the clip's place in the batch."""
    model, lm, feats, _, _ = _case(geom, 105)
    enc = model.hip_encoder()
    with torch.no_grad():
        e17, t17 = enc.forward(lm, feats, taps=True)
        e17, f17 = e17.clone(), t17["film"].clone()
        for c in (0, 8, 16):
            e1, t1 = enc.forward(lm[c:c + 1].contiguous(), feats[c:c + 1].contiguous(), taps=True)
            assert torch.equal(t1["film"][0], f17[c]), c
            assert torch.equal(e1[0], e17[c]), c


@pytest.mark.parametrize("B", [1, BMAX])
@pytest.mark.parametrize("feature_dim", [64, 180])
@pytest.mark.parametrize("geom", ["default", "baseline_sh"])   # 11 and 9 sub-bands
def test_film_vs_oracle(geom, feature_dim, B):
    """FiLM parameters against the oracle; the folded affine pairs (which no tap exposes) through the embeddings."""
    model, lm, feats, oemb, ofilm = _case(geom, 20, feature_dim)
    with torch.no_grad():
        emb, taps = model.hip_encoder().forward(lm[:B].contiguous(), feats[:B].contiguous(), taps=True)
    close(taps["film"].cpu(), ofilm[:B], 1e-5, name=f"small kernels: film {geom} Fd={feature_dim} B={B}")
    close_elementwise(emb.cpu(), oemb[:B], name=f"small kernels: embeddings behind film {geom} Fd={feature_dim} B={B}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("detailed", [False, True])
@pytest.mark.parametrize("T", [20 * 256, 30001])   # 21 frames; an odd length with a ragged last run of frames
def test_finalise_vs_oracle(T, detailed, B):
    from mst_amd.mixing_utils import MixingFeatureExtractor
    ext = MixingFeatureExtractor(use_detailed_spectral=True, n_spectral_bins=32) if detailed else MixingFeatureExtractor()
    x = torch.stack([cases.feature_case(n, T) for n in ("synth", "dc", "short_padded")[:B]], 0)
    f, _ = ext.features_and_logmel(omel.tensor_to_stems_dict(x.cuda()))
    assert f.shape[1] == (180 if detailed else 64)
    ref = ofeat.extract_all_features(x, detailed=detailed, n_bins=32)
    check_feats(f.cpu(), ref, name=f"features T={T} detailed={detailed} B={B}")
    f2, _ = ext.features_and_logmel(omel.tensor_to_stems_dict(x.cuda()))   # a second call in the same process: the same bits
    assert torch.equal(f, f2)


def _rows64(e, lab, row0, rows, tau):
    from mst_amd.loss import info_nce_rows
    s, c = info_nce_rows(e.double(), lab, row0, rows, tau)
    return s.item(), int(c.item())


@pytest.mark.parametrize("N,D", [(3, 768), (48, 768), (72, 768)])
def test_infonce_forward_vs_golden_and_oracle(N, D):
    from mst_amd.loss import InfoNCELoss, info_nce_rows_hip
    e = torch.randn(N, D, generator=torch.Generator().manual_seed(5))   # N = 48: the golden's own draw (seed 5, first)
    lab = torch.arange(N) % 24 if N == 48 else torch.arange(N) // 3 if N == 72 else torch.tensor([0, 0, 1])
    loss = InfoNCELoss(0.1)(e.cuda(), lab.cuda())
    close_loss = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6)   # noqa: E731
    close_loss(loss.item(), oloss.info_nce(e, lab, 0.1).item())
    if N == 48:
        close_loss(loss.item(), np.load(G + "/infonce.npz")["pairs48.loss"])
    s, c = info_nce_rows_hip(e.cuda(), lab.cuda(), 0, N, 0.1)
    want_s, want_c = _rows64(e, lab, 0, N, 0.1)
    assert int(c.item()) == want_c == (2 if N == 3 else N)
    close_loss(s.item(), want_s)
    s2, c2 = info_nce_rows_hip(e.cuda(), lab.cuda(), 0, N, 0.1)   # a second call: the same bits
    assert torch.equal(s, s2) and torch.equal(c, c2)


def test_infonce_forward_sharded_rows():
    """Rows 24..47 of N = 72 (one rank's share of a gathered batch), and the three shards together against the oracle's mean."""
    from mst_amd.loss import info_nce_rows_hip
    N = 72
    e = torch.randn(N, 768, generator=torch.Generator().manual_seed(6))
    lab = torch.arange(N) // 3
    parts = [info_nce_rows_hip(e.cuda(), lab.cuda(), r0, 24, 0.1) for r0 in (0, 24, 48)]
    want_s, want_c = _rows64(e, lab, 24, 24, 0.1)
    np.testing.assert_allclose(parts[1][0].item(), want_s, rtol=1e-5, atol=1e-6)
    assert int(parts[1][1].item()) == want_c == 24
    total = sum(p[0].item() for p in parts) / sum(p[1].item() for p in parts)
    np.testing.assert_allclose(total, oloss.info_nce(e, lab, 0.1).item(), rtol=1e-5, atol=1e-6)


def test_infonce_forward_without_positive_pairs_and_many_calls():
    """Every song once: no anchor has a positive, the count is 0 (and the module raises, as the reference does).  Then a long run
    of calls of alternating sizes: every one returns what the first of its size returned (no state survives a call)."""
    from mst_amd.loss import InfoNCELoss, info_nce_rows_hip
    e = torch.randn(12, 64, generator=torch.Generator().manual_seed(8)).cuda()
    s, c = info_nce_rows_hip(e, torch.arange(12).cuda(), 0, 12, 0.1)
    assert c.item() == 0 and s.item() == 0
    with pytest.raises(RuntimeError, match="No positive pairs"):
        InfoNCELoss(0.1)(e, torch.arange(12).cuda())
    labs = {12: (torch.arange(12) // 2).cuda(), 5: torch.tensor([0, 1, 0, 1, 2]).cuda()}
    first = {}
    for k in range(150):
        n = 12 if k % 3 else 5
        s, c = info_nce_rows_hip(e[:n].contiguous(), labs[n], 0, n, 0.1)
        got = (s.item(), c.item())
        assert first.setdefault(n, got) == got, (k, n)
    assert first[12][1] == 12 and first[5][1] == 4
