"""CPU: the training backend of TCNFiLMGenerator (`train_backend`) -- the attribute and its refusals, the two new ABI structs,
the host-only size functions, and the torch tree against the reference's fixture (tests/golden/tcn_film_train.npz, written by
tests/golden/make_golden_tcn_film_train.py).  float64 tree vs the fixture's float64: 1e-9 relative with the 1 % floor (the
same arithmetic on another CPU's kernels); fp32 tree: cases_tcn_film_train's rule against the reference's own fp32 run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases_tcn_film_train as cf
from mst_amd import _lib
from mst_amd import tcn_mixer as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tcn_film_train.npz")


def small():
    return tm.TCNFiLMGenerator(embed_dim=16, num_blocks=2, hidden_channels=8)


def test_train_backend_defaults_to_none_and_rejects_other_values():
    gen = small()
    assert gen.train_backend == "none" and gen.backend == "hip"
    for backend in ("hip", "torch"):
        gen.backend, gen.train_backend = backend, "hip-train"
        with pytest.raises(ValueError, match=r"train_backend must be 'none' \(default\) or 'hip'"):
            gen(torch.zeros(1, 16))
    gen.backend, gen.train_backend = "hip-train", "hip"     # the backend's own check comes first, as before
    with pytest.raises(ValueError, match="backend must be"):
        gen(torch.zeros(1, 16))


def test_without_a_training_backend_the_hip_backend_refuses_as_before():
    gen = small().train()
    with pytest.raises(RuntimeError, match=r"TCNFiLMGenerator.forward: the HIP backend is inference only and the module is in "
                                           r"train\(\) mode; backend='torch'"):
        gen(torch.zeros(1, 16))
    gen.eval()
    with pytest.raises(RuntimeError, match=r"TCNFiLMGenerator.forward: the HIP backend has no backward; call under "
                                           r"torch.no_grad\(\); backend='torch'"):
        gen(torch.zeros(1, 16))
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"no CPU fallback.*backend='torch'"):
        gen(torch.zeros(1, 16))


def test_film_base_stands_for_plain_slices_only():
    """`_film_base` hands TCNMixer's training forward the packed tensor in place of its slices only where nothing can tell."""
    B, nb, H = 3, 2, 8
    slices = lambda f: [{k: f[:, i, q, :] for q, k in enumerate(tm._FILM_KEYS)} for i in range(nb)]  # noqa: E731
    film = torch.randn(B, nb, 4, H, requires_grad=True)
    got = tm._film_base(slices(film), B, nb, H)
    assert got is not None and got.data_ptr() == film.data_ptr() and got.shape == (B, nb, 4, H) and got.requires_grad
    flat = torch.randn(B, nb * 4 * H)     # the torch backend's (B, out_dim) output, viewed
    assert tm._film_base(slices(flat.view(B, nb, 4, H)), B, nb, H).data_ptr() == flat.data_ptr()
    with torch.no_grad():     # the stack sends no gradient into the base: neither may this
        detached = slices(film)
    assert tm._film_base(detached, B, nb, H) is None
    kept = slices(film)
    kept[1]["beta2"].retain_grad()
    assert tm._film_base(kept, B, nb, H) is None
    hooked = slices(film)
    hooked[0]["gamma1"].register_hook(lambda g: g)
    assert tm._film_base(hooked, B, nb, H) is None
    assert tm._film_base([{k: v * 1.0 for k, v in d.items()} for d in slices(film)], B, nb, H) is None
    swapped = slices(film)
    swapped[0]["gamma1"], swapped[0]["beta1"] = swapped[0]["beta1"], swapped[0]["gamma1"]
    assert tm._film_base(swapped, B, nb, H) is None
    assert tm._film_base(slices(torch.randn(B, nb, 4, H + 1)[..., :H]), B, nb, H) is None     # slices of a wider tensor


def test_training_backend_refuses_cpu_tensors():
    gen = small()
    gen.train_backend = "hip"
    for mode in (gen.train, gen.eval):     # eval() with grad enabled and parameters that require grad needs a gradient
        mode()
        with pytest.raises(RuntimeError, match=r"no CPU fallback.*backend='torch'"):
            gen(torch.zeros(1, 16))
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"no CPU fallback.*backend='torch'"):     # the inference path
        gen(torch.zeros(1, 16))
    gen.backend = "torch"
    assert len(gen(torch.zeros(1, 16))) == 2 and gen.film_tensor(torch.zeros(3, 16)).shape == (3, 2, 4, 8)


def test_training_backend_refuses_two_different_slopes():
    gen = small().train()
    gen.train_backend = "hip"
    gen.mlp[4].negative_slope = 0.1
    with pytest.raises(ValueError, match=r"slope.*backend='torch'"):
        gen(torch.zeros(1, 16))
    gen.train_backend = "none"     # not looked at without the training backend
    with pytest.raises(RuntimeError, match=r"train\(\) mode"):
        gen(torch.zeros(1, 16))


def test_struct_layouts_match_the_header():
    assert C.sizeof(_lib.TcnFilmTrainDims) == 3 * 4
    assert C.sizeof(_lib.TcnFilmGrads) == 6 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _lib.TcnFilmTrainDims._fields_] == ["embed_dim", "mlp_hidden", "out_dim"]
    assert [n for n, _ in _lib.TcnFilmGrads._fields_] == [n for n, _ in _lib.TcnFilmWeights._fields_]


def test_size_functions_return_zero_for_refused_dims():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    sizes = lambda I, H, O, B: (L.mst_tcn_film_train_save_bytes(C.byref(_lib.TcnFilmTrainDims(I, H, O)), B),  # noqa: E731
                                L.mst_tcn_film_train_backward_workspace_bytes(C.byref(_lib.TcnFilmTrainDims(I, H, O)), B))
    for ok in ((1, 1, 1, 1), (4096, 2048, 8192, 65535), (1022, 512, 288, 8), (20, 512, 4, 1)):
        save, work = sizes(*ok)
        I, H, O, B = ok
        assert save >= 4 * 2 * B * H and work >= 4 * 2 * B * H, ok     # at least the two activations / their gradients
    for bad in ((0, 512, 896, 8), (4097, 512, 896, 8), (1024, 0, 896, 8), (1024, 2049, 896, 8), (1024, 512, 0, 8),
                (1024, 512, 8193, 8), (1024, 512, 896, 0), (1024, 512, 896, -1), (1024, 512, 896, 65536)):
        assert sizes(*bad) == (0, 0), bad
    assert L.mst_tcn_film_train_save_bytes(None, 8) == 0 and L.mst_tcn_film_train_backward_workspace_bytes(None, 8) == 0


def test_torch_tree_reproduces_the_reference_fixture():
    gold, c = np.load(GOLDEN), cf.FIXTURE
    sd, emb, R = cf.make_inputs(c["B"], c["embed_dim"], c["nb"], c["H"], c["seed"])
    pos = cf.w3_positions()
    ref32 = {k: gold[f"f32.{k}"].astype(np.float64) for k in cf.GROUPS}
    ref64 = {k: gold[f"f64.{k}"].astype(np.float64) for k in cf.GROUPS}
    for dt in (torch.float64, torch.float32):
        gen = tm.TCNFiLMGenerator(embed_dim=c["embed_dim"], num_blocks=c["nb"], hidden_channels=c["H"])
        gen.load_state_dict(sd, strict=True)
        gen.backend = "torch"
        got = cf.run_tree(gen.to(dt).eval(), emb, R)
        got["mlp.3.weight"] = got["mlp.3.weight"].ravel()[pos]
        if dt == torch.float64:
            for k in cf.GROUPS:
                assert cf.rel_err(got[k], ref64[k]) <= 1e-9, k
        else:
            assert not cf.check_rule("torch tree fp32", got, ref32, ref64)
