"""CPU: the TCN mixer in train() mode -- the torch tree against the reference's training fixtures
(tests/golden/tcn_train_<case>.npz, written by tests/golden/make_golden_tcn_train.py) and the refusals of the training backend.

Tolerances (cases_tcn_train's parity rule, LeakyReLU masks of the fixture imposed on both precisions): float64 tree vs the
fixture's float64 -- 1e-9 relative (the same arithmetic on another CPU's kernels); fp32 tree -- per quantity group within
2 x the reference's own fp32-against-float64 error, y and dx also within 1e-4 norm-wise; block conv-bias gradients
(mathematically zero) within 2 x the reference's own fp32 noise."""
import numpy as np
import pytest
import torch

import cases_tcn as ct
import cases_tcn_train as ctt
from mst_amd import tcn_mixer as tm


def torch_mixer(c):
    m = tm.TCNMixer(**ct.mixer_kwargs(c))
    m.backend = "torch"
    return m


@pytest.mark.parametrize("name", list(ctt.CASES))
def test_torch_tree_reproduces_the_training_fixture(name, monkeypatch):
    c, g = ctt.CASES[name], np.load(ctt.fixture_path(name))
    masks, e_ref = ctt.unpack_masks(g, c), ctt.e_ref(g)
    assert list(g["param_names"]) == [k for k, _ in torch_mixer(c).named_parameters()]
    ref64 = ctt.fixture_groups(g, 64)
    for dtype, bits in ((torch.float64, 64), (torch.float32, 32)):
        monkeypatch.setattr(tm, "F", ctt.Pinned(masks))
        r = ctt.run_tree(lambda: torch_mixer(c), c, dtype)
        got = ctt.sampled_groups(r)
        assert r.nbt == int(g["nbt"]) == 101
        for k in ("rmean", "rvar"):
            assert ct.max_rel(getattr(r, k).numpy(), g[f"{k}64"])[0] <= (1e-9 if bits == 64 else 1e-5)
        for grp in ref64:
            e, nw = ct.max_rel(got[grp], ref64[grp])
            print(f"tcn train {name} {grp} fp{bits}: {e:.3e} normwise {nw:.3e} (e_ref {e_ref[grp]:.3e})")
            if bits == 64:
                assert e <= 1e-9, (grp, e)
            else:
                assert e <= 2 * e_ref[grp], (grp, e, e_ref[grp])
                assert grp not in ("y", "dx") or nw <= 1e-4, (grp, nw)
        if bits == 32:
            assert ctt.groups_of_run(r)[1] <= 2 * float(g["db32_max"])


def test_hip_train_refuses_cpu_tensors():
    c = ctt.CASES["t_h8"]
    m = tm.TCNMixer(**ct.mixer_kwargs(c))
    m.backend = "hip-train"
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(RuntimeError, match=r"no CPU fallback.*backend='torch'"):
            m(torch.zeros(1, 8, 64))


def test_hip_backend_still_refuses_train_mode():
    c = ctt.CASES["t_h8"]
    m = tm.TCNMixer(**ct.mixer_kwargs(c)).train()
    assert m.backend == "hip"
    with pytest.raises(RuntimeError, match=r"train\(\) mode.*backend='torch'"):
        m(torch.zeros(1, 8, 64))


def test_hip_train_refuses_cumulative_average_batchnorm():
    c = ctt.CASES["t_h8"]
    m = tm.TCNMixer(**ct.mixer_kwargs(c)).train()
    m.backend = "hip-train"
    m.blocks[1].norm2.momentum = None
    with pytest.raises(ValueError, match=r"momentum=None"):
        m(torch.zeros(1, 8, 64))
    m.blocks[1].norm2.momentum = 0.1
    m.blocks[0].norm1.track_running_stats = False
    with pytest.raises(ValueError, match=r"track_running_stats=False"):
        m(torch.zeros(1, 8, 64))


def test_film_generator_has_no_training_backend():
    gen = tm.TCNFiLMGenerator(embed_dim=16, num_blocks=2, hidden_channels=8)
    gen.backend = "hip-train"
    with pytest.raises(ValueError, match="backend must be"):
        gen(torch.zeros(1, 16))
