"""GPU: the TCN mixer kernels (csrc/tcn.hip) through the C ABI (mst_tcn_*, bound by mst_amd.tcn_mixer).

Yardstick: the float64 evaluation of the reference (fixtures tests/golden/tcn_<case>.npz) or, at shapes too large for a
fixture, of the `backend="torch"` tree (pinned to the reference by tests/test_tcn_cpu.py) on the host CPUs.
Tolerance: cases_tcn.TwoTimesRule -- every maximum relative error of the kernels <= 2 x e_ref, where e_ref is the largest
maximum relative error of the reference's own fp32 evaluation over the case's quantities (y, y - x, hidden taps, FiLM
parameters), rel = |d| / max(|ref64|, 0.01 max|ref64|); plus max|d| / max|ref| <= 1e-4.  No element is left out.
Measured e_ref when the fixtures were written: 1.2e-5 (loader_default) ... 3.2e-5 (plain64)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import cases
import cases_tcn as ct
import cases_tcn_train as ctt
import parity
from mst_amd import _lib
from mst_amd import tcn_mixer as tm

pytestmark = pytest.mark.gpu
FILM_KEYS = ("gamma1", "beta1", "gamma2", "beta2")


def build(c, E=ct.EMBED, dtype=torch.float32, device="cuda", backend="hip", sd=None, generator=True):
    """The mixer with the seeded state dict (or `sd`) and, for a FiLM mixer unless `generator` is False, its generator."""
    tcn = tm.TCNMixer(**ct.mixer_kwargs(c))
    tcn.load_state_dict(sd if sd is not None else ct.make_tcn_state_dict(c), strict=True)
    tcn = tcn.to(device=device, dtype=dtype).eval()
    tcn.backend = backend
    gen = None
    if c["film"] and generator:
        gen = tm.TCNFiLMGenerator(embed_dim=E, num_blocks=c["nb"], hidden_channels=c["H"])
        gen.load_state_dict(ct.make_film_state_dict(E, c), strict=True)
        gen = gen.to(device=device, dtype=dtype).eval()
        gen.backend = backend
    return tcn, gen


def hip_forward(c, x, E=ct.EMBED, taps=(), film=None, sd=None):
    """y, film (B, nb, 4, H) or None, hidden taps -- all on the kernels.  `film`: the FiLM tensor itself instead of the
    generator's; `sd`: a state dict instead of the seeded one."""
    tcn, gen = build(c, E, sd=sd, generator=film is None)
    with torch.no_grad():
        if gen is not None:
            film = gen.film_tensor(ct.embeddings(x.shape[0], E).cuda())
        elif film is not None:
            film = film.cuda().contiguous()
        y, hs = tcn._forward_hip(x.cuda(), film, tuple(taps))
    torch.cuda.synchronize()
    return y.cpu(), None if film is None else film.cpu(), [h.cpu() for h in hs]


def torch_forward(c, x, dtype, E=ct.EMBED, taps=(), film=None, sd=None):
    """The same on the torch tree on the host CPUs."""
    tcn, gen = build(c, E, dtype, "cpu", "torch", sd=sd, generator=film is None)
    got = {k: None for k in taps}
    with torch.no_grad():
        params = None
        if gen is not None:
            params = gen(ct.embeddings(x.shape[0], E).to(dtype))
        elif film is not None:
            params = ctt.film_dicts(film.to(dtype))
        y = tcn._forward_torch(x.to(dtype), params, got)
    film = None if params is None else torch.stack([torch.stack([p[k] for k in FILM_KEYS], 1) for p in params], 1)
    return y, film, [got[k] for k in taps]


@pytest.mark.parametrize("name", list(ct.CASES))
def test_fixture_case(name):
    c, g = ct.CASES[name], np.load(ct.fixture_path(name))
    x = cases.pcm_batch(c["B"], c["T"])
    blocks = ct.tap_blocks(c)
    y, film, hs = hip_forward(c, x, taps=blocks)
    xs, hi = ct.flat_y(x), ct.hidden_idx(c)
    rule = ct.TwoTimesRule(name)
    rule.add("y", ct.flat_y(y), ct.golden_y(g, 32), ct.golden_y(g, 64))
    rule.add("y-x", ct.flat_y(y) - xs, ct.golden_y(g, 32) - xs, ct.golden_y(g, 64) - xs)
    for k, h in zip(blocks, hs):
        rule.add(f"h{k}", h.reshape(-1)[hi].numpy(), g[f"h{k}_32"], g[f"h{k}_64"])
    if c["film"]:
        rule.add("film", film.numpy(), g["film32"], g["film64"])
    rule.check()


def test_film_generator_wide_embedding():
    c, g = ct.CASES["st_default"], np.load(ct.fixture_path("st_default"))
    _, gen = build(c, ct.EMBED_WIDE)
    with torch.no_grad():
        params = gen(ct.embeddings(c["B"], ct.EMBED_WIDE).cuda())
    assert len(params) == c["nb"] and params[3]["beta2"].shape == (c["B"], c["H"])
    film = torch.stack([torch.stack([p[k] for k in FILM_KEYS], 1) for p in params], 1).cpu().numpy()
    rule = ct.TwoTimesRule("st_default E=1536")
    rule.add("film", film, g["film1536_32"], g["film1536_64"])
    rule.check()


@pytest.mark.parametrize("name,B,T", [("st_default", 2, 441000), ("wide128", 1, 100000)])
def test_contract_size(name, B, T):
    """10 s clips (interior samples with all 15 taps of the d = 8192 block inside the clip: T > 114 688) and the widest
    mixer at 100 000 samples (13 of those taps inside at the centre).  Every element of y and of the hidden taps is compared."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    c = ct.CASES[name]
    x = cases.pcm_batch(B, T)
    blocks = ct.tap_blocks(c)
    y, film, hs = hip_forward(c, x, taps=blocks)
    t0 = time.time()
    y32, film32, h32 = torch_forward(c, x, torch.float32, taps=blocks)
    y64, film64, h64 = torch_forward(c, x, torch.float64, taps=blocks)
    print(f"torch tree on the CPU, fp32 + float64: {time.time() - t0:.1f} s")
    x64 = x.double()
    rule = ct.TwoTimesRule(f"{name} {B}x{T}")
    rule.add("y", y.numpy(), y32.numpy(), y64.numpy())
    rule.add("y-x", (y.double() - x64).numpy(), (y32.double() - x64).numpy(), (y64 - x64).numpy())
    for k, h, a, b in zip(blocks, hs, h32, h64):
        rule.add(f"h{k}", h.numpy(), a.numpy(), b.numpy())
    rule.add("film", film.numpy(), film32.numpy(), film64.numpy())
    rule.check()


@pytest.mark.parametrize("name", ["loader_default", "plain64"])
def test_batch_independence(name):
    c = ct.CASES[name]
    x = cases.pcm_batch(3, 12345)
    tcn, gen = build(c)
    with torch.no_grad():
        emb = ct.embeddings(3, ct.EMBED).cuda()
        params = gen(emb) if gen is not None else None
        y = tcn(x.cuda(), film_params=params)
        for b in range(3):
            pb = gen(emb[b:b + 1]) if gen is not None else None
            if pb is not None:
                assert all(torch.equal(pb[i][k][0], params[i][k][b]) for i in range(c["nb"]) for k in FILM_KEYS)
            assert torch.equal(tcn(x[b:b + 1].cuda(), film_params=pb)[0], y[b]), f"clip {b} depends on its batch"


def test_long_stream():
    """95 s in one call (H = 16, T = 4 194 309), against the fp32 torch tree on the CPU, norm-wise."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    c, T = ct.CASES["st_default"], 4194309
    x = cases.pcm_batch(1, T)
    y, _, _ = hip_forward(c, x)
    y32, _, _ = torch_forward(c, x, torch.float32)
    row = parity.record(f"tcn long stream 1x{T} y [hip vs torch fp32]", y, y32)
    row2 = parity.record(f"tcn long stream 1x{T} y-x [hip vs torch fp32]", y - x, y32 - x)
    assert row["normwise"] <= 1e-4 and row2["normwise"] <= 1e-4, (row, row2)


def test_handle_refresh_after_load_state_dict():
    c = ct.CASES["loader_default"]
    x = cases.pcm_batch(1, 9000).cuda()
    tcn, gen = build(c)
    with torch.no_grad():
        params = gen(ct.embeddings(1, ct.EMBED).cuda())
        y0 = tcn(x, film_params=params)
        first = tcn._hip
        assert torch.equal(tcn(x, film_params=params), y0) and tcn._hip is first      # unchanged weights: same handle
        tcn.load_state_dict(ct.make_tcn_state_dict(c, seed=4201), strict=True)
        y1 = tcn(x, film_params=params)
        assert tcn._hip is not first and not torch.equal(y1, y0)
        fresh, _ = build(c)
        fresh.load_state_dict(ct.make_tcn_state_dict(c, seed=4201), strict=True)
        assert torch.equal(fresh(x, film_params=params), y1)
        with torch.no_grad():
            tcn.output_conv.bias.add_(0.25)                                           # in-place edit
        assert torch.allclose(tcn(x, film_params=params), y1 + 0.25, rtol=0, atol=1e-6)
        gen.load_state_dict(ct.make_film_state_dict(ct.EMBED, c, seed=4301), strict=True)
        assert not torch.equal(gen(ct.embeddings(1, ct.EMBED).cuda())[0]["gamma1"], params[0]["gamma1"])


def test_loose_film_dicts_equal_packed():
    c = ct.CASES["loader_default"]
    x = cases.pcm_batch(2, 5000).cuda()
    tcn, gen = build(c)
    with torch.no_grad():
        params = gen(ct.embeddings(2, ct.EMBED).cuda())
        loose = [{k: v.clone() for k, v in p.items()} for p in params]
        assert torch.equal(tcn(x, film_params=params), tcn(x, film_params=loose))


def test_shape_refusals():
    c = ct.CASES["wide128"]
    tcn, _ = build(c)
    h = tcn._handle(torch.device("cuda", torch.cuda.current_device()))
    L = _lib.lib()
    assert L.mst_tcn_workspace_bytes(h.ptr, 1, (1 << 31) // 128) == 0      # a size query: nothing is allocated or launched
    assert b"2^31" in L.mst_last_error()
    assert L.mst_tcn_workspace_bytes(h.ptr, 1, (1 << 31) // 128 - 1) > 0
    y = torch.empty(1, 8, 64, device="cuda")
    rc = L.mst_tcn_forward(h.ptr, _lib.dptr(y), None, 1, 64, _lib.dptr(y), None, _lib.dptr(y), 16, None)
    assert rc != 0 and b"film" in L.mst_last_error()
    cfg = _lib.TcnConfig(6, 16, 4, 5, 0, 0, 1e-5)
    ptr = C.c_void_p()
    assert L.mst_tcn_create(C.byref(ptr), C.byref(cfg), C.byref(_lib.TcnWeights())) != 0 and b"in_channels" in L.mst_last_error()
    plain, _ = build(ct.CASES["h8"])
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        plain(torch.zeros(1, 8, 64))


def test_apply_style_transfer_end_to_end():
    from mst_amd.mixing_utils import STEMS, deferred_features
    from mst_amd.model import MixingStyleEncoder
    from mst_amd.synth import synth_batch
    torch.manual_seed(0)
    enc = MixingStyleEncoder(feature_dim=64).cuda().eval()
    x = synth_batch(2, 33075)
    stems = {s: x[:, 2 * i:2 * i + 2].cuda() for i, s in enumerate(STEMS)}
    with torch.no_grad():
        emb = enc(stems, torch.stack([deferred_features(64)] * 2).cuda())
    c = dict(ct.CASES["loader_default"])
    tcn, gen = build(c, E=2 * emb.shape[1])
    dev = torch.device("cuda")
    out = tm.apply_style_transfer(tcn, gen, {s: x[0, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}, emb[1], emb[0], dev)
    assert set(out) == {"processed_stems", "processed_mixture"} and list(out["processed_stems"]) == list(STEMS)
    assert all(v.shape == (2, 33075) and v.device.type == "cpu" for v in out["processed_stems"].values())
    assert torch.equal(out["processed_mixture"], sum(out["processed_stems"].values()))
    # the same call on the torch tree
    tcn.backend = gen.backend = "torch"
    ref = tm.apply_style_transfer(tcn, gen, {s: x[0, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}, emb[1], emb[0], dev)
    row = parity.record("tcn apply_style_transfer mixture [hip vs torch on the GPU]", out["processed_mixture"], ref["processed_mixture"])
    assert row["normwise"] <= 1e-4 and float((out["processed_mixture"] - x[0, 0:2] - x[0, 2:4] - x[0, 4:6] - x[0, 6:8]).abs().max()) > 1e-2
