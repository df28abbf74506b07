"""CPU: host side of the log-mel waveform gradient -- the per-bin band table the backward kernel reads, the C ABI symbol, and
the refusal without a GPU (no CPU fallback)."""
import os

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (sys.path setup)
from mst_amd import _lib
from mst_amd.mixing_utils import LOGMEL_BAND_MAX, band_table_to_dense, mel_band_table, mel_bin_ranges
from mst_amd.model import MelSpectrogramPreprocessor, MixingStyleEncoder

GOLDEN = os.path.join(cases.ROOT, "tests", "golden", "fbanks.npz")
TABLES = ((1024, 128), (1024, 256), (2048, 80))


def _fb(n_fft, n_mels):
    return torch.from_numpy(np.load(GOLDEN)[f"fb_{n_fft}_{n_mels}"])


@pytest.mark.parametrize("n_fft,n_mels", TABLES)
def test_band_table_scatters_back_bit_for_bit(n_fft, n_mels):
    fb = _fb(n_fft, n_mels)
    first, count, weights = mel_band_table(fb)
    assert first.dtype == count.dtype == torch.int32 and weights.dtype == torch.float32
    assert first.shape == count.shape == (n_fft // 2 + 1,) and weights.shape[0] == n_fft // 2 + 1
    assert int(first.min()) >= 0 and int((first + count).max()) <= n_mels
    dense = band_table_to_dense(first, count, weights, n_mels)
    assert np.array_equal(dense.numpy().view(np.int32), fb.numpy().view(np.int32))   # bit patterns, the table's -0.0 included


@pytest.mark.parametrize("n_fft,n_mels", TABLES)
def test_widest_band_is_two(n_fft, n_mels):
    _, count, weights = mel_band_table(_fb(n_fft, n_mels))
    assert int(count.max()) == 2 == weights.shape[1] == LOGMEL_BAND_MAX


@pytest.mark.parametrize("n_fft,n_mels", TABLES)
def test_mel_ranges_are_the_transposed_table(n_fft, n_mels):
    """The per-mel runs of bins (what the kernel's mel sums walk) with the per-bin weights give the dense filterbank back."""
    fb = _fb(n_fft, n_mels)
    first, count, weights = mel_band_table(fb)
    ranges = mel_bin_ranges(first, count, n_mels)
    assert ranges.shape == (n_mels, 4) and ranges.dtype == torch.int32
    dense = torch.zeros_like(fb)
    for m in range(n_mels):
        a, na, b, nb = (int(v) for v in ranges[m])
        assert 0 <= a and a + na <= n_fft // 2 + 1 and 0 <= b and b + nb <= n_fft // 2 + 1
        dense[a:a + na, m] += weights[a:a + na, 0]
        dense[b:b + nb, m] += weights[b:b + nb, 1]
    assert torch.equal(dense, fb)


def test_filter_with_a_hole_is_refused():
    fb = _fb(1024, 128).clone()
    k = int((fb[:, 100] != 0).nonzero()[2])
    fb[k] = 0   # a bin inside filter 100's run that belongs to no filter
    first, count, _ = mel_band_table(fb)
    with pytest.raises(ValueError, match="contiguous run"):
        mel_bin_ranges(first, count, 128)


def test_wider_table_is_kept_whole():
    """A filterbank with three mels on one bin: the table carries all three (the kernel's entry point refuses it by its width;
    nothing is dropped on the way there)."""
    fb = _fb(1024, 128).clone()
    fb[100, 40:43] = torch.tensor([0.25, 0.5, 0.125])
    fb[100, :40] = 0
    fb[100, 43:] = 0
    first, count, weights = mel_band_table(fb)
    assert weights.shape[1] == 3 and int(count[100]) == 3 and int(first[100]) == 40
    assert torch.equal(band_table_to_dense(first, count, weights, 128), fb)


def test_symbol_declared_and_bound():
    src = open(os.path.join(cases.ROOT, "include", "mst.h")).read()
    for name in ("mst_logmel_backward", "mst_logmel_backward_workspace_bytes"):
        assert name + "(" in src and name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["mst_logmel_backward"][1]) == 17
    assert f"#define MST_LOGMEL_BAND_MAX {LOGMEL_BAND_MAX}" in src
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert hasattr(L, "mst_logmel_backward")
    assert L.mst_logmel_backward_workspace_bytes(16) >= 16 * 2 * 1024 * 4 and L.mst_logmel_backward_workspace_bytes(0) == 0


def _cpu_stems(T=4096):
    g = torch.Generator().manual_seed(5)
    return {s: (0.1 * torch.randn(1, 2, T, generator=g)).requires_grad_(s == "vocals") for s in cases.STEMS}


def test_cpu_stem_requiring_grad_raises_in_preprocessor():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MelSpectrogramPreprocessor()(_cpu_stems())


def test_cpu_stem_requiring_grad_raises_in_encoder():
    model = MixingStyleEncoder(embed_dim=32, feature_dim=64, encoder_backend="torch").eval()
    for q in model.parameters():
        q.requires_grad_(False)
    # (without a GPU the stage-A plan's device tables already fail to build; with one, the stems' device is refused)
    with pytest.raises(RuntimeError, match="no CPU fallback|no ROCm-capable device"):
        model(_cpu_stems(), torch.zeros(1, 64))
