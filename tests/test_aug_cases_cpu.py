"""The explicit-decision reference of the augmentation edge tests (tests/cases_aug.py) against the oracle and its goldens, and
the input conditions of tests/test_aug_edges_gpu.py -- all on the CPU: the yardstick is checked where no GPU is needed."""
import os

import numpy as np
import pytest
import torch

import cases
import cases_aug as ca
from oracle import augment as oaug
from oracle import mel as omel

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_trace_read_back_reproduces_the_oracle_bit_for_bit(seed):
    x = cases.feature_case("synth1", 33075)
    torch.manual_seed(seed)
    y, trace = oaug.augment_stems(omel.tensor_to_stems_dict(x))
    spec = ca.clip_from_trace(trace)
    got = ca.expected([spec], x[None])[0]
    assert torch.equal(got, omel.stems_dict_to_tensor(y))
    # ... and the stored samples of the reference's own run, at the tolerance tests/test_oracle_golden.py uses
    g = np.load(os.path.join(G, "augment.npz"))
    assert int(g[f"seed{seed}.reverb"]) == spec.reverb
    idx = torch.from_numpy(g[f"seed{seed}.idx"])
    np.testing.assert_allclose(got.flatten()[idx].double().numpy(), g[f"seed{seed}.samples"], rtol=1e-5, atol=1e-6)


def test_fill_clips_writes_what_the_spec_says():
    spec = ca.Clip((ca.Stem(gain=ca.gain_of_db(-9.0), tilt="high", compress=ca.DEFAULT_COMP, bw=(4, 4000.0)),
                    ca.Stem(tilt="low", bw=(2, 11999.0)), ca.Stem(compress=(-12.0, 2.0)), ca.Stem()), 1, ca.make_ir(7))
    clips, irs = ca.fill_clips([spec, ca.Clip()])
    s = clips[0].stem
    assert (s[0].tilt, s[0].compress, s[0].bw_sections) == (1, 1, 2) and s[0].gain == np.float32(10 ** (-9 / 20))
    assert (s[1].tilt, s[1].compress, s[1].bw_sections, s[1].gain) == (1, 0, 1, 1.0)
    assert (s[2].tilt, s[2].compress, s[2].bw_sections) == (0, 2, 0) and (s[2].comp_threshold_db, s[2].comp_ratio) == (-12.0, 2.0)
    assert (s[3].tilt, s[3].compress, s[3].bw_sections, s[3].gain) == (0, 0, 0, 1.0)
    from scipy.signal import butter
    assert list(s[0].tilt_sos) == butter(2, 2000, btype="high", fs=44100, output="sos")[0].tolist()
    assert list(s[1].bw_sos)[:6] == butter(2, 11999.0, btype="low", fs=44100, output="sos")[0].tolist()
    # the closed-form order-4 sections are scipy's cascade (sections normalised one by one): same transfer function
    ref4 = butter(4, 4000.0, btype="low", fs=44100, output="sos")
    mine = np.array(list(s[0].bw_sos)).reshape(2, 6)
    np.testing.assert_allclose(np.polymul(mine[0, :3], mine[1, :3]), np.polymul(ref4[0, :3], ref4[1, :3]), rtol=1e-12)
    np.testing.assert_allclose(np.polymul(mine[0, 3:], mine[1, 3:]), np.polymul(ref4[0, 3:], ref4[1, 3:]), rtol=1e-12)
    assert clips[0].reverb == 1 and clips[1].reverb == 0 and irs[1] is None and torch.equal(irs[0], spec.ir)


def test_float64_chain_is_close_to_the_float32_oracle():
    """`expected_f64` (the yardstick for the oracle's own rounding) runs the same decisions: it differs from the float32
    oracle by float32 rounding only."""
    x = ca.edge_input(1, 2049)
    spec = ca.Clip((ca.Stem(gain=ca.gain_of_db(-9.0), tilt="high", compress=ca.DEFAULT_COMP, bw=(4, 4000.0)),
                    ca.Stem(tilt="low", bw=(2, 11999.0)), ca.Stem(compress=(-12.0, 2.0)), ca.Stem()), 1, ca.make_ir(513))
    a, b = ca.expected([spec], x), ca.expected_f64([spec], x)
    assert b.dtype == torch.float64 and float((a.double() - b).abs().max()) < 1e-5 * float(b.abs().max())


def test_edge_input_has_impulses_on_both_sides_of_every_segment_boundary():
    x = ca.edge_input(2, 2 * ca.SEG + 1, seed=3)
    noise = 0.3 * torch.randn(2, 8, 2 * ca.SEG + 1, generator=torch.Generator().manual_seed(1003))
    for n in (ca.SEG - 1, 2 * ca.SEG - 1):
        assert float(((x - noise)[:, :, n].abs() - 1.0).abs().max()) < 1e-6
    for n in (ca.SEG, 2 * ca.SEG):
        assert float(((x - noise)[:, :, n].abs() - 0.75).abs().max()) < 1e-6
    assert torch.equal(x, ca.edge_input(2, 2 * ca.SEG + 1, seed=3))
    assert tuple(ca.edge_input(1, 1).shape) == (1, 8, 1)


# ---- the input conditions of every case of tests/test_aug_edges_gpu.py ----
@pytest.mark.parametrize("name", ca.CASE_NAMES)
def test_edge_case_input_conditions(name):
    specs, x, silent = ca.case(name)
    ca.check_conditions(specs, x, ca.reference(name), silent)


@pytest.mark.parametrize("T", ca.REVERB_T)
def test_mode2_case_is_not_silent(T):
    x, ref, _ = ca.mode2_case(T, 100 + T)
    assert bool(ref[0].any()) and bool(ref[1].any()) and not torch.equal(ref, x)
