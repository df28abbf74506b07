"""GPU: TCNFiLMGenerator in training on libmst.so (csrc/head.hip: `mst_tcn_film_forward_train`, `mst_tcn_film_backward`) and
the Python layer over it (`TCNFiLMGenerator.train_backend = "hip"`).

Yardstick of the kernels: the float64 torch tree of mst_amd.tcn_mixer.TCNFiLMGenerator (backend "torch"; test_tcn_cpu.py pins it
to the reference) on the host, with the two Dropout masks the kernels derive made explicit through `mst_dropout_mask`; e_ref is
the same tree in fp32 on the host with the same masks.  Rule (cases_tcn_film_train.check_rule), per quantity group -- film,
demb, each of the six parameter gradients: every element is at most 2 e_ref max(|ref64|, 0.01 max|ref64|) + 1e-7 max|ref64|
from float64.  The fixture case pins the kernels (p = 0) to the reference's own values of tests/golden/tcn_film_train.npz."""
import contextlib
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

import cases_tcn_film_train as cf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tcn_film_train.npz")
SLOPE = 0.2
SEEDS = (1234567891011, 98765432123)


def _keep(p, seed, B):
    """(B, mlp_hidden) uint8 on the host: the kernels' keep decisions."""
    from mst_amd import _lib
    n = B * cf.MLP_HIDDEN
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().mst_dropout_mask(float(p), int(seed), n, _lib.dptr(keep), _lib.stream_ptr(keep.device)), "mst_dropout_mask")
    return keep.view(B, cf.MLP_HIDDEN).cpu()


def _masks(p, B, seeds=SEEDS):
    """The two scaled masks (float64, host) of Dropout(p) under `seeds`, or (None, None)."""
    if p == 0:
        return None, None
    return tuple(_keep(p, s, B).double() / (1.0 - p) for s in seeds)


def _abi(sd, emb, R, p1, p2, seeds=SEEDS, slope=SLOPE, want_demb=True):
    """One forward + backward of sum(film * R) through the C ABI -> {group: cuda tensor}."""
    from mst_amd import _lib
    L = _lib.lib()
    w = [sd[k].cuda().contiguous() for k in cf.PARAMS]
    x, dfilm = emb.cuda().contiguous(), R.cuda().contiguous()
    B, I, H, O = x.shape[0], w[0].shape[1], w[0].shape[0], w[4].shape[0]
    dims = _lib.TcnFilmTrainDims(I, H, O)
    nsave, nws = L.mst_tcn_film_train_save_bytes(C.byref(dims), B), L.mst_tcn_film_train_backward_workspace_bytes(C.byref(dims), B)
    assert nsave > 0 and nws > 0
    save = torch.empty(nsave, dtype=torch.uint8, device="cuda")
    work = torch.empty(nws, dtype=torch.uint8, device="cuda")
    film = torch.empty(B, O, device="cuda")
    grads = [torch.full_like(t, float("nan")) for t in w]     # overwritten, not accumulated
    demb = torch.full_like(x, float("nan")) if want_demb else None
    wp = _lib.TcnFilmWeights(*[t.data_ptr() for t in w])
    gp = _lib.TcnFilmGrads(*[t.data_ptr() for t in grads])
    st = _lib.stream_ptr(x.device)
    _lib.check(L.mst_tcn_film_forward_train(C.byref(dims), C.byref(wp), _lib.dptr(x), B, slope, p1, seeds[0], p2, seeds[1], _lib.dptr(film),
                                            _lib.dptr(save), nsave, st), "mst_tcn_film_forward_train")
    _lib.check(L.mst_tcn_film_backward(C.byref(dims), C.byref(wp), _lib.dptr(x), B, slope, p1, seeds[0], p2, seeds[1], _lib.dptr(dfilm),
                                       _lib.dptr(save), C.byref(gp), _lib.dptr(demb), _lib.dptr(work), nws, st), "mst_tcn_film_backward")
    out = {"film": film}
    if want_demb:
        out["demb"] = demb
    out.update(dict(zip(cf.PARAMS, grads)))
    return out


def _host(got):
    return {k: v.detach().double().cpu().numpy() for k, v in got.items()}


def _tree(sd, emb, R, nb, H, dtype, m1, m2):
    from mst_amd.tcn_mixer import TCNFiLMGenerator
    gen = TCNFiLMGenerator(embed_dim=emb.shape[1], num_blocks=nb, hidden_channels=H)
    gen.load_state_dict(sd, strict=True)
    gen.backend = "torch"
    return cf.run_tree(gen.to(dtype).train(), emb, R, m1, m2)


GEOMETRIES = [(1, 20, 1, 1, 0.0),          # one row, out_dim 4
              (3, 40, 3, 8, 0.1),
              (17, 100, 3, 24, 0.5),       # rows across the 16-row fragment; K no multiple of the 32-wide chunk; out_dim 288
              (65, 64, 2, 16, 0.1),        # rows across the 64-row tile
              (2, 1024, 16, 128, 0.1),     # out_dim 8192, the maximum
              (8, 1024, 14, 16, 0.1)]      # the trainer's own shape


@pytest.mark.parametrize("B,E,nb,H,p", GEOMETRIES)
def test_parity_with_the_float64_tree(B, E, nb, H, p):
    sd, emb, R = cf.make_inputs(B, E, nb, H, seed=1000 * B + E)
    m1, m2 = _masks(p, B)
    if p > 0:
        assert not torch.equal(m1, m2)
        for m in (m1, m2):
            keep = (m > 0).double().mean().item()
            assert abs(keep - (1 - p)) <= 4 * (p * (1 - p) / m.numel()) ** 0.5, keep
    got = _host(_abi(sd, emb, R, p, p))
    ref64, ref32 = _tree(sd, emb, R, nb, H, torch.float64, m1, m2), _tree(sd, emb, R, nb, H, torch.float32, m1, m2)
    assert np.abs(ref64["film"]).max() > 0.05     # (not the module's own near-zero initialisation)
    assert not cf.check_rule(f"film train B={B} E={E} nb={nb} H={H} p={p}", got, ref32, ref64)


def test_fixture_case_against_the_reference_values():
    gold, c = np.load(GOLDEN), cf.FIXTURE
    sd, emb, R = cf.make_inputs(c["B"], c["embed_dim"], c["nb"], c["H"], c["seed"])
    got = _host(_abi(sd, emb, R, 0.0, 0.0, seeds=(0, 0)))
    got["mlp.3.weight"] = got["mlp.3.weight"].ravel()[cf.w3_positions()]
    ref32 = {k: gold[f"f32.{k}"].astype(np.float64) for k in cf.GROUPS}
    ref64 = {k: gold[f"f64.{k}"].astype(np.float64) for k in cf.GROUPS}
    assert not cf.check_rule("film train fixture", got, ref32, ref64)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_zero_pre_activation_takes_the_slope_unless_dropped(p):
    """z1[:, 7] == 0 exactly: the saved activation is 0 whether the unit was dropped or not.  A kept row contributes
    slope * scale * dh1 to d mlp.0.bias[7] (PyTorch's branch for x <= 0), a dropped row nothing."""
    B, E, nb, H = 16, 40, 3, 8
    sd, emb, R = cf.make_inputs(B, E, nb, H, seed=77)
    sd["mlp.0.weight"][7] = 0.0
    sd["mlp.0.bias"][7] = 0.0
    m1, m2 = _masks(p, B)
    got = _host(_abi(sd, emb, R, p, p))
    ref64, ref32 = _tree(sd, emb, R, nb, H, torch.float64, m1, m2), _tree(sd, emb, R, nb, H, torch.float32, m1, m2)
    # dh1 of the float64 tree: d loss / d (the Dropout's output)
    W = {k: v.double() for k, v in sd.items()}
    lrelu = lambda z: torch.where(z > 0, z, SLOPE * z)  # noqa: E731
    one = torch.ones(B, cf.MLP_HIDDEN, dtype=torch.float64)
    k1, k2 = (one, one) if p == 0 else (m1, m2)
    z1 = emb.double() @ W["mlp.0.weight"].T + W["mlp.0.bias"]
    assert bool((z1[:, 7] == 0).all())
    h1 = (lrelu(z1) * k1).requires_grad_(True)
    h2 = lrelu(h1 @ W["mlp.3.weight"].T + W["mlp.3.bias"]) * k2
    ((h2 @ W["mlp.6.weight"].T + W["mlp.6.bias"]) * R.double().reshape(B, -1)).sum().backward()
    want = float((SLOPE * k1[:, 7] * h1.grad[:, 7]).sum())
    if p > 0:
        kept = k1[:, 7] > 0
        assert 0 < int(kept.sum()) < B     # both kinds of rows
        assert abs(want - float(SLOPE * 2.0 * h1.grad[kept, 7].sum())) <= 1e-12 * abs(want)
    assert abs(ref64["mlp.0.bias"][7] - want) <= 1e-12 * abs(want)
    scale = float(np.abs(ref64["mlp.0.bias"]).max())
    assert abs(want) > 1e-3 * scale     # not 0, and far above the rule's bound
    e_ref = cf.rel_err(ref32["mlp.0.bias"], ref64["mlp.0.bias"])
    bound = 2 * e_ref * max(abs(want), 0.01 * scale) + 1e-7 * scale
    print(f"d mlp.0.bias[7] p={p}: kernels {got['mlp.0.bias'][7]:.9e}  float64 {want:.9e}  bound {bound:.3e}")
    assert abs(got["mlp.0.bias"][7] - want) <= bound
    assert not cf.check_rule(f"film train zero pre-activation p={p}", got, ref32, ref64)


def test_same_seeds_same_bits_and_rows_do_not_depend_on_the_batch():
    B, E, nb, H = 17, 100, 3, 24
    sd, emb, R = cf.make_inputs(B, E, nb, H, seed=5)
    a, b = _abi(sd, emb, R, 0.1, 0.3), _abi(sd, emb, R, 0.1, 0.3)
    assert set(a) == set(cf.GROUPS)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    other = _abi(sd, emb, R, 0.1, 0.3, seeds=(SEEDS[0] + 1, SEEDS[1]))
    assert not torch.equal(a["film"], other["film"])
    # demb == NULL: skipped, everything else the same bits
    c = _abi(sd, emb, R, 0.1, 0.3, want_demb=False)
    for k in c:
        assert torch.equal(a[k], c[k]), k
    whole = _abi(sd, emb, R, 0.0, 0.0)["film"]
    for m in (0, 5, 15, 16):
        alone = _abi(sd, emb[m:m + 1], R[m:m + 1], 0.0, 0.0)["film"]
        assert torch.equal(alone[0], whole[m]), m


def test_refusals_by_name():
    from mst_amd import _lib
    L = _lib.lib()
    sd, emb, R = cf.make_inputs(2, 20, 1, 1, seed=1)
    w = [sd[k].cuda() for k in cf.PARAMS]
    wp = _lib.TcnFilmWeights(*[t.data_ptr() for t in w])
    grads = [torch.empty_like(t) for t in w]
    gp = _lib.TcnFilmGrads(*[t.data_ptr() for t in grads])
    x, film = emb.cuda(), torch.empty(2, 4, device="cuda")
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr(x.device)

    def fwd(dims, B=2, slope=0.2, p1=0.0, p2=0.0, nbytes=buf.numel()):
        return L.mst_tcn_film_forward_train(C.byref(dims), C.byref(wp), _lib.dptr(x), B, slope, p1, 0, p2, 0, _lib.dptr(film), _lib.dptr(buf),
                                            nbytes, st)

    def bwd(dims, B=2, slope=0.2, p1=0.0, p2=0.0, nbytes=buf.numel()):
        return L.mst_tcn_film_backward(C.byref(dims), C.byref(wp), _lib.dptr(x), B, slope, p1, 0, p2, 0, _lib.dptr(film), _lib.dptr(buf),
                                       C.byref(gp), None, _lib.dptr(buf), nbytes, st)

    good = _lib.TcnFilmTrainDims(20, 512, 4)
    for fn, name in ((fwd, b"mst_tcn_film_forward_train"), (bwd, b"mst_tcn_film_backward")):
        for kw in (dict(dims=_lib.TcnFilmTrainDims(4097, 512, 4)), dict(dims=_lib.TcnFilmTrainDims(20, 2049, 4)),
                   dict(dims=_lib.TcnFilmTrainDims(20, 512, 8193)), dict(dims=_lib.TcnFilmTrainDims(0, 512, 4)),
                   dict(dims=good, B=0), dict(dims=good, B=65536), dict(dims=good, p1=1.0), dict(dims=good, p2=-0.1),
                   dict(dims=good, slope=1.5), dict(dims=good, slope=-0.1)):
            assert fn(**kw) == -1 and name in L.mst_last_error(), kw
        assert fn(dims=good, nbytes=16) == -2 and name in L.mst_last_error()     # MST_ENOMEM
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# through the module
# ---------------------------------------------------------------------------------------------------------------------
def _module(E=32, nb=2, H=8, seed=11):
    from mst_amd.tcn_mixer import TCNFiLMGenerator
    gen = TCNFiLMGenerator(embed_dim=E, num_blocks=nb, hidden_channels=H)
    gen.load_state_dict(cf.make_inputs(1, E, nb, H, seed)[0], strict=True)
    gen = gen.cuda().train()
    gen.backend, gen.train_backend = "hip", "hip"
    return gen


def _grads(gen):
    return [q.grad.clone() for q in gen.parameters()]


def test_the_steps_call_pattern_through_the_module():
    B, E, nb, H = 3, 32, 2, 8
    gen = _module(E, nb, H)
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(B, E // 2, generator=g).cuda(), torch.randn(B, E // 2, generator=g).cuda()
    R1, R2 = torch.randn(B, nb, 4, H, generator=g).cuda(), torch.randn(B, nb, 4, H, generator=g).cuda()
    ab, ba = torch.cat([a, b], 1), torch.cat([b, a], 1)

    def step():     # two forwards, one backward; the RNG state between the two calls
        torch.manual_seed(5)
        f1 = gen.film_tensor(ab)
        mid = torch.get_rng_state()
        f2 = gen.film_tensor(ba)
        assert f1.shape == f2.shape == (B, nb, 4, H) and f1.requires_grad
        ((f1 * R1).sum() + (f2 * R2).sum()).backward()
        return f1.detach(), f2.detach(), mid

    f1, f2, mid = step()
    both = _grads(gen)
    assert not torch.equal(f1, f2)
    # .grad is the fp32 sum of the two calls' gradients
    gen.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    o1 = gen.film_tensor(ab)
    assert torch.equal(o1.detach(), f1)
    (o1 * R1).sum().backward()
    g1 = _grads(gen)
    gen.zero_grad(set_to_none=True)
    torch.set_rng_state(mid)
    o2 = gen.film_tensor(ba)
    assert torch.equal(o2.detach(), f2)
    (o2 * R2).sum().backward()
    g2 = _grads(gen)
    for s, x, y in zip(both, g1, g2):
        assert torch.equal(s, x + y)
    # a second backward without zero_grad() accumulates
    gen.zero_grad(set_to_none=True)
    step()
    step()
    for s, q in zip(both, gen.parameters()):
        assert torch.equal(q.grad, s + s)
    # the embedding's gradient only when asked for; None for a frozen parameter
    gen.zero_grad(set_to_none=True)
    gen.mlp[3].bias.requires_grad_(False)
    e = ab.clone().requires_grad_(True)
    torch.manual_seed(5)
    (gen.film_tensor(e) * R1).sum().backward()
    assert e.grad is not None and e.grad.shape == e.shape and bool(e.grad.any()) and gen.mlp[3].bias.grad is None
    assert torch.equal(gen.mlp[0].weight.grad, g1[0])
    gen.mlp[3].bias.requires_grad_(True)
    # an in-place parameter edit between forward and backward raises
    gen.zero_grad(set_to_none=True)
    out = gen.film_tensor(ab)
    with torch.no_grad():
        gen.mlp[3].weight.mul_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    # after an optimiser step the next forward reads the new values: a fresh module loaded from the updated state_dict agrees
    gen.zero_grad(set_to_none=True)
    opt = torch.optim.AdamW(gen.parameters(), lr=1e-2)
    step()
    opt.step()
    torch.manual_seed(7)
    after = gen.film_tensor(ab).detach()
    assert not torch.equal(after, f1)
    from mst_amd.tcn_mixer import TCNFiLMGenerator
    fresh = TCNFiLMGenerator(embed_dim=E, num_blocks=nb, hidden_channels=H)
    fresh.load_state_dict({k: v.cpu() for k, v in gen.state_dict().items()}, strict=True)
    fresh = fresh.cuda().train()
    fresh.backend, fresh.train_backend = "hip", "hip"
    torch.manual_seed(7)
    assert torch.equal(fresh.film_tensor(ab).detach(), after)
    # B = 0: the empty tensor, no launch
    assert gen.film_tensor(ab[:0]).shape == (0, nb, 4, H)
    # forward() hands out the same list of dicts, views of one packed tensor
    from mst_amd.tcn_mixer import _packed_film
    dicts = gen(ab)
    assert len(dicts) == nb and sorted(dicts[0]) == ["beta1", "beta2", "gamma1", "gamma2"]
    assert _packed_film(dicts, B, nb, H).data_ptr() == dicts[0]["gamma1"].data_ptr()


def test_eval_mode_through_the_module():
    B, E, nb, H = 3, 32, 2, 8
    gen = _module(E, nb, H)
    x = torch.randn(B, E, generator=torch.Generator().manual_seed(3)).cuda()
    R = torch.randn(B, nb, 4, H, generator=torch.Generator().manual_seed(4)).cuda()
    # eval() without gradients is the inference path, bit for bit
    gen.eval()
    with torch.no_grad():
        with_backend = gen.film_tensor(x)
        gen.train_backend = "none"
        inference = gen.film_tensor(x)
        gen.train_backend = "hip"
    assert torch.equal(with_backend, inference)
    # eval() with gradients: both Dropouts off, no seed drawn
    state = torch.get_rng_state()
    f_eval = gen.film_tensor(x)
    assert torch.equal(torch.get_rng_state(), state) and f_eval.requires_grad
    (f_eval * R).sum().backward()
    g_eval = _grads(gen)
    gen.zero_grad(set_to_none=True)
    gen.train()
    gen.mlp[2].p = gen.mlp[5].p = 0.0
    f_p0 = gen.film_tensor(x)
    (f_p0 * R).sum().backward()
    assert torch.equal(f_eval.detach(), f_p0.detach())
    for u, v in zip(g_eval, _grads(gen)):
        assert torch.equal(u, v)
    gen.mlp[2].p = gen.mlp[5].p = 0.1
    gen.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    assert not torch.equal(gen.film_tensor(x).detach(), f_p0.detach())     # train() mode drops
    # refusals of this path name the opt-in
    with pytest.raises(RuntimeError, match=r"fp32.*backend='torch'"):
        gen.film_tensor(x.double())
    with pytest.raises(ValueError, match="expected"):
        gen.film_tensor(x[:, :-1])


def test_with_the_mixer_in_one_graph():
    from mst_amd.tcn_mixer import TCNFiLMGenerator, TCNMixer, _FILM_KEYS, _film_base, _packed_film
    B, T, nb, H, E = 2, 300, 2, 8, 16
    torch.manual_seed(21)
    tcn = TCNMixer(hidden_channels=H, num_blocks=nb, kernel_size=3, use_film=True).cuda().train()
    tcn.backend = "hip-train"
    gen = TCNFiLMGenerator(embed_dim=E, num_blocks=nb, hidden_channels=H)
    gen.load_state_dict(cf.make_inputs(1, E, nb, H, seed=8)[0], strict=True)
    gen = gen.cuda().train()
    gen.backend, gen.train_backend = "hip", "hip"
    x = torch.randn(B, 8, T, device="cuda") * 0.1
    R = torch.randn(B, 8, T, device="cuda")
    e = torch.randn(B, E, device="cuda")
    torch.manual_seed(3)
    film = gen.film_tensor(e)
    film.retain_grad()
    dicts = [{k: film[:, i, q, :] for q, k in enumerate(_FILM_KEYS)} for i in range(nb)]
    # no copy between the generator and the mixer's kernels: the inference path and the training path both find the packed tensor
    assert _packed_film(dicts, B, nb, H).data_ptr() == film.data_ptr()
    assert _film_base(dicts, B, nb, H).data_ptr() == film.data_ptr()
    assert _film_base([{k: v * 1.0 for k, v in d.items()} for d in dicts], B, nb, H) is None     # anything else is stacked
    y = tcn(x, film_params=dicts)
    (y * R).sum().backward()
    assert film.grad is not None and bool(film.grad.any())
    params = list(gen.parameters())
    torch.manual_seed(3)
    again = gen.film_tensor(e)
    assert torch.equal(again.detach(), film.detach())
    want = torch.autograd.grad(again, params, grad_outputs=film.grad)
    for q, w in zip(params, want):
        assert torch.equal(q.grad, w)
    assert all(q.grad is not None and bool(q.grad.any()) for q in tcn.parameters() if q.dim() > 1)
    # the stacked route (dicts that are not plain slices of one tensor) is the same function, bit for bit
    film2 = film.detach().clone().requires_grad_(True)
    y2 = tcn(x, film_params=[{k: film2[:, i, q, :] * 1.0 for q, k in enumerate(_FILM_KEYS)} for i in range(nb)])
    (y2 * R).sum().backward()
    assert torch.equal(y2.detach(), y.detach()) and torch.equal(film2.grad, film.grad)


def test_example_with_the_hip_film_generator():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_tcn_mixer
    runs = []
    for _ in range(2):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            train_tcn_mixer.main(["--steps", "3", "--seconds", "0.5", "--batch-size", "2", "--film-generator", "hip"])
        runs.append([l for l in out.getvalue().splitlines() if l.startswith("step")])
    losses = [float(l.split("loss")[1].split()[0]) for l in runs[0]]
    assert len(losses) == 3 and all(np.isfinite(l) and abs(l) < 1e6 for l in losses), runs[0]
    assert runs[0] == runs[1]
