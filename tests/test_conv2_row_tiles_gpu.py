"""GPU: conv2's row-pure 4 x 16 tiling (`conv2_rows_kernel`, the eval forward on 10-row planes: 20-mel sub-bands)
against the 8 x 8 tiling it replaces there (`conv_kernel<2, 2, 0>`, selected per launch with MST_CONV2_TILES=8x8).

Both tilings add the same products in the same order (chunk -> tap -> 4 channels per output element); the new one only leaves
out MFMAs whose A operand is all zero padding.  So embeddings and the `pool_in` tap must agree BIT FOR BIT, and both meet the
1e-4 element-wise bar against `oracle.encoder` (test_encoder_gpu.close_elementwise).

With frames = 1 + T // 256, W1 = frames // 5, W2 = W1 // 4 the widths cover every tile kind of a plane:
  W2 = 2   fold tile only                                   W2 = 6   the contract's remainder (86 = 21 * 4 + 2); W1 = 27 leaves
  W2 = 4   one column block, no fold tile                            three columns behind the last window
  W2 = 5   fold tile with one valid window, one column      W2 = 7   a second top / bottom pair partly outside the plane
           behind the last window
B = 5 leaves the last set ragged among the pair tiles (4 blocks per set) and among the fold tiles (8 per set)."""
import pytest
import torch

import cases
from oracle import encoder as oenc
from oracle import mel as omel
from test_encoder_gpu import build_model, close_elementwise

pytestmark = pytest.mark.gpu

WIDTHS = {2: 256 * 39, 4: 256 * 79, 5: 256 * 104, 6: 256 * 138 + 100, 7: 256 * 149}
CFG_C5 = dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=256, split_size=20, overlap=10, embed_dim=768)
CFG_16_8 = dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=128, split_size=16, overlap=8, embed_dim=768)


@pytest.fixture(scope="module")
def default_model():
    return build_model(cases.CFG_DEFAULT)


def _inputs(model, B, T, seed):
    x = torch.stack([cases.synth_clip(c % 4, T) * (1.0 + 0.05 * c) for c in range(B)], 0)
    feats = torch.randn(B, 64, generator=torch.Generator().manual_seed(seed)).cuda()
    with torch.no_grad():
        lm = model.audio_encoder.mel_preprocessor(omel.tensor_to_stems_dict(x.cuda()))
    return lm, feats


def _both_tilings(model, lm, feats, monkeypatch):
    """(embeddings, pool_in) with the default tiling and with the 8 x 8 tiles."""
    with torch.no_grad():
        monkeypatch.delenv("MST_CONV2_TILES", raising=False)
        e_new, t_new = model.hip_encoder().forward(lm, feats, taps=True)
        monkeypatch.setenv("MST_CONV2_TILES", "8x8")
        e_old, t_old = model.hip_encoder().forward(lm, feats, taps=True)
        monkeypatch.delenv("MST_CONV2_TILES")
    torch.cuda.synchronize()
    return (e_new, t_new["pool_in"]), (e_old, t_old["pool_in"])


def _check_oracle(cfg, sd, lm, feats, emb, pool_in, name):
    otaps = {}
    oemb = oenc.encoder_from_logmel(sd, lm.cpu(), feats.cpu(), cfg["split_size"], cfg["overlap"], otaps)
    assert tuple(pool_in.shape) == tuple(otaps["pool_in"].shape)
    r_p = close_elementwise(pool_in.cpu(), otaps["pool_in"], name=f"conv2 row tiles {name} pool_in")
    r_e = close_elementwise(emb.cpu(), oemb, name=f"conv2 row tiles {name} embedding")
    print(f"{name}: pool_in {r_p}\n{name}: embedding {r_e}")


@pytest.mark.parametrize("W2", sorted(WIDTHS))
def test_row_tiles_equal_8x8_tiles_bit_for_bit(default_model, monkeypatch, W2):
    model, sd = default_model
    B, T = 5, WIDTHS[W2]
    lm, feats = _inputs(model, B, T, seed=W2)
    assert (1 + T // 256) // 5 // 4 == W2
    (e_new, p_new), (e_old, p_old) = _both_tilings(model, lm, feats, monkeypatch)
    assert tuple(p_new.shape) == (B, 11 * 64 * 2, W2)
    assert bool(torch.isfinite(e_new).all()) and float(p_new.abs().max()) > 0
    assert torch.equal(p_new, p_old), f"pool_in differs in {int((p_new != p_old).sum())} of {p_new.numel()} elements"
    assert torch.equal(e_new, e_old)
    # clip 3 alone: other sets, other waves, the same bits
    with torch.no_grad():
        e1, t1 = model.hip_encoder().forward(lm[3:4].contiguous(), feats[3:4].contiguous(), taps=True)
    assert torch.equal(t1["pool_in"][0], p_new[3]) and torch.equal(e1[0], e_new[3])
    _check_oracle(cases.CFG_DEFAULT, sd, lm, feats, e_new, p_new, f"W2={W2} B={B}")


def test_row_tiles_256_mels_24_bands(monkeypatch):
    model, sd = build_model(CFG_C5)
    assert model.audio_encoder.n_subbands == 24
    lm, feats = _inputs(model, 1, WIDTHS[6], seed=24)
    (e_new, p_new), (e_old, p_old) = _both_tilings(model, lm, feats, monkeypatch)
    assert tuple(p_new.shape) == (1, 24 * 64 * 2, 6)
    assert torch.equal(p_new, p_old) and torch.equal(e_new, e_old)
    _check_oracle(CFG_C5, sd, lm, feats, e_new, p_new, "256 mels W2=6 B=1")


def test_tile_variable_changes_nothing_on_four_row_planes(monkeypatch):
    """split 16 / overlap 8: 16-row planes after conv1, pooled plane 4 rows high -- the 8 x 8 tiles either way."""
    model, sd = build_model(CFG_16_8)
    assert model.audio_encoder.freq_dim == 4
    lm, feats = _inputs(model, 5, WIDTHS[6], seed=16)
    (e_new, p_new), (e_old, p_old) = _both_tilings(model, lm, feats, monkeypatch)
    assert tuple(p_new.shape) == (5, model.audio_encoder.n_subbands * 64 * 4, 6)
    assert torch.equal(p_new, p_old) and torch.equal(e_new, e_old)
    _check_oracle(CFG_16_8, sd, lm, feats, e_new, p_new, "split 16 / overlap 8 W2=6 B=5")


def test_tile_variable_changes_nothing_on_eleven_row_planes(monkeypatch):
    """split 35: 11-row planes, pooled plane 2 rows high -- input row 10 exists, which the row tiling's bottom tile leaves out as
    padding: the 8 x 8 tiles either way (test_encoder_gpu.test_first_pool_heights_of_three_and_more holds them to the oracle)."""
    cfg = dict(sample_rate=44100, n_fft=1024, hop_length=256, n_mels=128, split_size=35, overlap=31, embed_dim=256)
    model, sd = build_model(cfg)
    assert model.audio_encoder.freq_dim == 2
    lm, feats = _inputs(model, 2, WIDTHS[6], seed=35)
    (e_new, p_new), (e_old, p_old) = _both_tilings(model, lm, feats, monkeypatch)
    assert torch.equal(p_new, p_old) and torch.equal(e_new, e_old)
    _check_oracle(cfg, sd, lm, feats, e_new, p_new, "split 35 / overlap 31 W2=6 B=2")
