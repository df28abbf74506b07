"""CPU: the TCN mixer's Python layer (mst_amd.tcn_mixer) -- state-dict contract, the torch tree against the reference
fixtures (tests/golden/tcn_<case>.npz, written by tests/golden/make_golden_tcn.py), and the refusals of the HIP backend.

Tolerances: float64 tree vs the fixture's float64 -- 1e-12 relative (the same arithmetic on another CPU's kernels; ~1e3
accumulated terms of 1e-16).  fp32 tree -- the 2x rule of cases_tcn.TwoTimesRule (bit-equality across CPU generations is
not required)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import cases_tcn as ct
from mst_amd import _lib
from mst_amd import tcn_mixer as tm

FILM_KEYS = ("gamma1", "beta1", "gamma2", "beta2")


def build(c, dtype=torch.float32, E=ct.EMBED, backend="torch"):
    tcn = tm.TCNMixer(**ct.mixer_kwargs(c))
    tcn.load_state_dict(ct.make_tcn_state_dict(c), strict=True)
    tcn = tcn.to(dtype).eval()
    tcn.backend = backend
    gen = None
    if c["film"]:
        gen = tm.TCNFiLMGenerator(embed_dim=E, num_blocks=c["nb"], hidden_channels=c["H"])
        gen.load_state_dict(ct.make_film_state_dict(E, c), strict=True)
        gen = gen.to(dtype).eval()
        gen.backend = backend
    return tcn, gen


@pytest.mark.parametrize("name", list(ct.CASES))
def test_state_dict_contract(name):
    c, g = ct.CASES[name], np.load(ct.fixture_path(name))
    tcn, gen = build(c)
    sd = tcn.state_dict()
    assert list(sd.keys()) == list(g["tcn_keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["tcn_shapes"])
    assert tcn.receptive_field == int(g["receptive_field"]) == 1 + (2 ** c["nb"] - 1) * (c["K"] - 1)
    if gen is not None:
        fsd = gen.state_dict()
        assert list(fsd.keys()) == list(g["film_keys"])
        assert [",".join(map(str, v.shape)) for v in fsd.values()] == list(g["film_shapes"])
    # round trip
    other = tm.TCNMixer(**ct.mixer_kwargs(c))
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))
    assert np.allclose(cases.checksum(cases.pcm_batch(c["B"], c["T"])), g["x_checksum"], rtol=0, atol=0)


def test_default_initialisation_and_constructor():
    torch.manual_seed(0)
    tcn = tm.TCNMixer()
    assert (tcn.hidden_channels, tcn.num_blocks, tcn.causal, tcn.use_film, tcn.in_channels) == (128, 14, False, False, 8)
    assert tcn.receptive_field == 1 + (2 ** 14 - 1) * 14 == 229363
    assert tcn.backend == "hip"
    assert float(tcn.output_conv.weight.detach().std()) < 2e-3 and float(tcn.output_conv.bias.detach().abs().max()) == 0.0
    gen = tm.TCNFiLMGenerator(embed_dim=64, num_blocks=2, hidden_channels=8)
    assert 0.008 < float(gen.mlp[0].weight.detach().std()) < 0.012
    assert all(float(gen.mlp[i].bias.detach().abs().max()) == 0.0 for i in (0, 3, 6))
    assert isinstance(tcn.blocks[0], tm.ResidualBlock) and isinstance(tcn.blocks[0].conv1, tm.NonCausalConv1d)
    f = tm.TCNMixer(hidden_channels=8, num_blocks=2, causal=True, use_film=True)
    assert isinstance(f.blocks[1], tm.FiLMResidualBlock) and isinstance(f.blocks[1].conv2, tm.CausalConv1d)
    assert f.blocks[1].conv2.padding == 14 * 2 and tcn.blocks[3].conv1.padding == 7 * 8


def test_create_tcn_mixer_block_counts():
    assert tm.create_tcn_mixer(receptive_field_seconds=0.5).num_blocks == 11
    assert tm.create_tcn_mixer(receptive_field_seconds=2.0).num_blocks == 13
    m = tm.create_tcn_mixer()
    assert (m.num_blocks, m.hidden_channels, m.use_film) == (14, 8, False)
    assert tm.create_tcn_mixer(receptive_field_seconds=0.001).num_blocks == 6
    assert tm.create_tcn_mixer(receptive_field_seconds=60.0).num_blocks == 16


def test_value_errors():
    f = tm.TCNMixer(hidden_channels=8, num_blocks=3, kernel_size=5, use_film=True).eval()
    f.backend = "torch"
    x = torch.zeros(1, 8, 100)
    with pytest.raises(ValueError, match="film_params must be provided"):
        f(x)
    with pytest.raises(ValueError, match="Expected 3 FiLM parameter dicts, got 2"):
        f(x, film_params=[{}, {}])
    with pytest.raises(ValueError, match="odd kernel_size"):
        tm.TCNMixer(hidden_channels=8, num_blocks=2, kernel_size=4)
    tm.TCNMixer(hidden_channels=8, num_blocks=2, kernel_size=4, causal=True)   # causal keeps the length for any K


def _compare(name, dtype):
    c, g = ct.CASES[name], np.load(ct.fixture_path(name))
    tcn, gen = build(c, dtype)
    x = cases.pcm_batch(c["B"], c["T"]).to(dtype)
    taps = {k: None for k in ct.tap_blocks(c)}
    out = {}
    with torch.no_grad():
        params = None
        if gen is not None:
            params = gen(ct.embeddings(c["B"], ct.EMBED).to(dtype))
            assert len(params) == c["nb"] and set(params[0]) == set(FILM_KEYS) and params[0]["gamma1"].shape == (c["B"], c["H"])
            out["film"] = torch.stack([torch.stack([p[k] for k in FILM_KEYS], 1) for p in params], 1).numpy()
        y = tcn._forward_torch(x, params, taps)
        assert torch.equal(y, tcn(x, film_params=params))
    hi = ct.hidden_idx(c)
    out["y"] = ct.flat_y(y)
    for k in taps:
        out[f"h{k}"] = taps[k].reshape(-1)[hi].numpy()
    return c, g, out, ct.flat_y(x)


@pytest.mark.parametrize("name", list(ct.CASES))
def test_torch_tree_float64_matches_reference(name):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    c, g, out, _ = _compare(name, torch.float64)
    for k, v in out.items():
        ref = g["film64"] if k == "film" else (ct.golden_y(g, 64) if k == "y" else g[k + "_64"])
        rel, _ = ct.max_rel(v, ref)
        assert rel <= 1e-12, (name, k, rel)


@pytest.mark.parametrize("name", list(ct.CASES))
def test_torch_tree_fp32_within_two_times_rule(name):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    c, g, out, xs = _compare(name, torch.float32)
    rule = ct.TwoTimesRule(name + " torch-cpu", report=False)
    rule.add("y", out["y"], ct.golden_y(g, 32), ct.golden_y(g, 64))
    rule.add("y-x", out["y"] - xs, ct.golden_y(g, 32) - xs, ct.golden_y(g, 64) - xs)
    for k in ct.tap_blocks(c):
        rule.add(f"h{k}", out[f"h{k}"], g[f"h{k}_32"], g[f"h{k}_64"])
    if c["film"]:
        rule.add("film", out["film"], g["film32"], g["film64"])
    rule.check()


def test_film_generator_wide_embedding():
    c, g = ct.CASES["st_default"], np.load(ct.fixture_path("st_default"))
    _, gen = build(c, torch.float64, E=ct.EMBED_WIDE)
    with torch.no_grad():
        f = gen.film_tensor(ct.embeddings(c["B"], ct.EMBED_WIDE).double())
    assert f.shape == (c["B"], c["nb"], 4, c["H"])
    assert ct.max_rel(f.numpy(), g["film1536_64"])[0] <= 1e-12


def test_hip_backend_refusals():
    c = ct.CASES["loader_default"]
    tcn, gen = build(c, backend="hip")
    x, e = torch.zeros(1, 8, 256), torch.zeros(1, ct.EMBED)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback.*backend='torch'"):
            gen(e)
        gen.backend = "torch"
        params = gen(e)
        with pytest.raises(RuntimeError, match="no CPU fallback.*backend='torch'"):
            tcn(x, film_params=params)
        tcn.train()
        with pytest.raises(RuntimeError, match=r"train\(\) mode.*backend='torch'"):
            tcn(x, film_params=params)
        tcn.eval()
    with pytest.raises(RuntimeError, match="no backward.*backend='torch'"):
        tcn(x.requires_grad_(True), film_params=params)
    with pytest.raises(ValueError, match="backend must be"):
        tcn.backend = "eager"
        tcn(x, film_params=params)


def test_packed_film_is_recognised_without_copy():
    base = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).view(2, 3, 4, 8)
    dicts = [{k: base[:, i, q, :] for q, k in enumerate(FILM_KEYS)} for i in range(3)]
    assert tm._packed_film(dicts, 2, 3, 8).data_ptr() == base.data_ptr()
    loose = [{k: v.clone() for k, v in d.items()} for d in dicts]
    got = tm._packed_film(loose, 2, 3, 8)
    assert got.data_ptr() != base.data_ptr() and torch.equal(got, base)
    swapped = [dict(d, gamma1=d["beta1"], beta1=d["gamma1"]) for d in dicts]
    assert torch.equal(tm._packed_film(swapped, 2, 3, 8)[:, :, 0], base[:, :, 1])


def test_struct_layouts():
    assert C.sizeof(_lib.TcnConfig) == 7 * 4
    assert C.sizeof(_lib.TcnWeights) == 10 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.TcnFilmWeights) == 6 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.TcnTaps) == 4 + 4 * 4 + 4 + 4 * C.sizeof(C.c_void_p)   # n, block[4], padding, h[4]


def test_header_declares_stage_c():
    import os
    src = open(os.path.join(cases.ROOT, "include", "mst.h")).read()
    assert "Stage C: TCN mixer (eval)" in src and "MST_ABI_VERSION 1" in src
    for s in ("mst_tcn_create", "mst_tcn_forward", "mst_tcn_workspace_bytes", "mst_tcn_film_forward"):
        assert s in _lib.SYMBOLS and s in src
