"""GPU: TCNMixer with backend='hip-train' -- the train-mode forward and the full backward on the kernels of
csrc/tcn_train.inc, against the float64 torch tree with the LeakyReLU masks of the run under test imposed.

The parity rule is cases_tcn_train's: per quantity group the maximum relative error (cases_tcn.max_rel) stays within
2 x the reference's own fp32-against-float64 error of that group (the fixture's e_ref, taken on the fixture's sample
positions, which are the positions compared here), y and dx also within 1e-4 norm-wise; the block conv-bias gradients
(mathematically zero) within 2 x the reference's own fp32 noise.

The linear kernels alone (input gradient, weight gradient) are compared with float64 autograd of F.conv1d.  Bound: the
fp32 MFMA is an fmaf chain whose measured error is 0.75-1.5e-7 * sum|a b| up to 1024 terms; the chains here are at most
128 MFMAs (weight gradient, then double) or H terms per tap (input gradient), so 1e-6 * sum|a b| per element."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import cases_tcn as ct
import cases_tcn_train as ctt
from mst_amd import _lib
from mst_amd import tcn_mixer as tm

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build(c, backend="hip-train", sd=None):
    m = tm.TCNMixer(**ct.mixer_kwargs(c))
    m.load_state_dict(sd if sd is not None else ct.make_tcn_state_dict(c), strict=True)
    m.backend = backend
    return m.to(DEV).train()


def inputs(c, grad=True):
    x = cases.pcm_batch(c["B"], c["T"]).to(DEV).requires_grad_(grad)
    film = ctt.film_tensor(c).to(DEV).requires_grad_(grad) if c["film"] else None
    return x, film


def hip_masks(m, c, x, film):
    """(2 nb, B, H, T) bool from mst_tcn_train_masks, of a forward of its own on module m."""
    _, save, h = m._train_forward(x.detach().contiguous(), None if film is None else film.detach().contiguous(), want_save=True)
    out = torch.empty(2 * c["nb"], c["B"], c["H"], c["T"], device=DEV, dtype=torch.uint8)
    _lib.check(_lib.lib().mst_tcn_train_masks(h.ptr, _lib.dptr(save), save.numel(), c["B"], c["T"], _lib.dptr(out),
                                              _lib.stream_ptr(x.device)), "mst_tcn_train_masks")
    return out.bool().cpu()


def hip_step(c):
    """One forward + backward through the public interface; the result in run_tree's form (CPU tensors)."""
    m = build(c)
    x, film = inputs(c)
    y = m(x, film_params=ctt.film_dicts(film) if c["film"] else None)
    (y * ctt.dy_tensor(c).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    norms = m._norms()
    bmean, bvar = m._last_batch_stats
    return SimpleNamespace(y=y.detach().cpu(), dx=x.grad.cpu(), dfilm=film.grad.cpu() if c["film"] else None,
                           grads={k: p.grad.cpu() for k, p in m.named_parameters()}, bmean=bmean.reshape(-1, c["H"]).cpu(),
                           bvar=bvar.reshape(-1, c["H"]).cpu(), rmean=torch.stack([n.running_mean for n in norms]).cpu(),
                           rvar=torch.stack([n.running_var for n in norms]).cpu(), nbt=[int(n.num_batches_tracked) for n in norms])


_RUNS = {}


def runs(name, monkeypatch):
    """The HIP step of a case, its masks, and the float64 yardsticks: computed once, shared by the tests, never changed."""
    if name not in _RUNS:
        c = ctt.CASES[name]
        r = hip_step(c)
        masks = hip_masks(build(c), c, *inputs(c, grad=False))
        torch_mixer = lambda: build(c, "torch").cpu()  # noqa: E731
        with monkeypatch.context() as mp:   # the F that the torch tree sees; torch.nn.functional itself is left alone
            mp.setattr(tm, "F", ctt.Pinned(masks))
            pinned = ctt.run_tree(torch_mixer, c, torch.float64)
            free = ctt.Recorder()
            mp.setattr(tm, "F", free)
            ctt.run_tree(torch_mixer, c, torch.float64)
        _RUNS[name] = (r, masks, pinned, free.stacked())
    return _RUNS[name]


@pytest.mark.parametrize("name", list(ctt.CASES))
def test_forward_statistics_and_running_buffers(name, monkeypatch):
    c, g = ctt.CASES[name], np.load(ctt.fixture_path(name))
    r, _, p64, _ = runs(name, monkeypatch)
    e_ref = ctt.e_ref(g)
    got, ref = ctt.sampled_groups(r), ctt.sampled_groups(p64)
    for grp in ("y", "stats"):
        e, nw = ct.max_rel(got[grp], ref[grp])
        print(f"tcn train {name} {grp}: hip {e:.3e} normwise {nw:.3e}  e_ref {e_ref[grp]:.3e}")
        assert e <= 2 * e_ref[grp], (grp, e, e_ref[grp])
        assert grp != "y" or nw <= 1e-4
    assert r.nbt == [101] * (2 * c["nb"])
    # running = (1 - m) * old + m * batch (the variance unbiased first), m = 0.1: it inherits m times the error allowed to the
    # batch statistic (2 e_ref of max(|value|, 1 % of the group's maximum), the rule's own scale) and adds at most four fp32
    # roundings (the scaling by n / (n - 1), the two products, the sum) of quantities no larger than |(1 - m) old| + |m batch|
    sd, m, n = ct.make_tcn_state_dict(c), 0.1, c["B"] * c["T"]
    for k, key, batch in (("rmean", "running_mean", p64.bmean), ("rvar", "running_var", p64.bvar * (n / (n - 1)))):
        old = torch.stack([sd[f"blocks.{i}.norm{l}.{key}"] for i in range(c["nb"]) for l in (1, 2)]).double()
        scale = torch.clamp(batch.abs(), min=0.01 * float(torch.cat([p64.bmean, p64.bvar]).abs().max()))
        bound = m * 2 * e_ref["stats"] * scale + 4 * 2.0 ** -24 * ((1 - m) * old.abs() + m * batch.abs())
        err = (getattr(r, k).double() - getattr(p64, k)).abs()
        print(f"tcn train {name} {k}: max error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), k


@pytest.mark.parametrize("name", list(ctt.CASES))
def test_gradients_within_the_parity_rule(name, monkeypatch):
    c, g = ctt.CASES[name], np.load(ctt.fixture_path(name))
    r, _, p64, _ = runs(name, monkeypatch)
    e_ref = ctt.e_ref(g)
    got, ref = ctt.sampled_groups(r), ctt.sampled_groups(p64)
    bad = []
    for grp in ref:
        if grp in ("y", "stats"):
            continue
        e, nw = ct.max_rel(got[grp], ref[grp])
        print(f"tcn train {name} {grp}: hip {e:.3e} normwise {nw:.3e}  e_ref {e_ref[grp]:.3e}")
        if not (e <= 2 * e_ref[grp] and (grp != "dx" or nw <= 1e-4)):
            bad.append((grp, e, nw, e_ref[grp]))
    # Every element, not only the fixture's sample positions: max|d| / max|ref| of a group never exceeds the rule's relative
    # error with its floor (the denominator there is at most max|ref|), so the rule's bound holds for it on whole tensors.
    whole, whole64 = ctt.groups_of_run(r)[0], ctt.groups_of_run(p64)[0]
    for grp in whole64:
        if grp in ("y", "stats"):
            continue
        nw = ct.max_rel(whole[grp], whole64[grp])[1]
        print(f"tcn train {name} {grp}, every element: normwise {nw:.3e}  e_ref {e_ref[grp]:.3e}")
        if not nw <= 2 * e_ref[grp]:
            bad.append((grp + " (every element)", nw, e_ref[grp]))
    db = ctt.groups_of_run(r)[1]
    print(f"tcn train {name} block conv bias: max|db| hip {db:.3e}  reference fp32 {float(g['db32_max']):.3e}")
    assert not bad, bad
    assert db <= 2 * float(g["db32_max"])
    assert set(got) == set(ref) and ("dfilm" in got) == c["film"]


@pytest.mark.parametrize("name", list(ctt.CASES))
def test_masks_are_the_float64_tree_s_up_to_rounding(name, monkeypatch):
    _, masks, _, free = runs(name, monkeypatch)
    diff = int((masks != free).sum())
    print(f"tcn train {name}: {diff} of {masks.numel()} masks differ from the free float64 run")
    assert diff <= 1e-4 * masks.numel()
    assert 0.05 < masks.float().mean() < 0.95


def test_two_runs_give_the_same_bits(monkeypatch):
    c = ctt.CASES["t_plain40"]
    a, b = hip_step(c), hip_step(c)
    assert torch.equal(a.y, b.y) and torch.equal(a.dx, b.dx)
    assert all(torch.equal(a.grads[k], b.grads[k]) for k in a.grads)
    c = ctt.CASES["t_st"]
    a, b = runs("t_st", monkeypatch)[0], hip_step(c)
    assert torch.equal(a.y, b.y) and torch.equal(a.dx, b.dx) and torch.equal(a.dfilm, b.dfilm)
    assert all(torch.equal(a.grads[k], b.grads[k]) for k in a.grads)


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def _ws(h, B, T):
    n = _lib.lib().mst_tcn_train_workspace_bytes(h.ptr, B, T)
    assert n > 0
    return torch.empty(n, device=DEV, dtype=torch.uint8), n


@pytest.mark.parametrize("H,K,causal,T,block", [
    (8, 15, False, 1, 0), (16, 15, False, 37, 2), (16, 15, False, 37, 6), (40, 5, False, 2049, 1), (128, 15, False, 2049, 3),
    (16, 4, True, 2049, 2), (16, 4, True, 37, 6), (40, 5, True, 1, 0), (8, 15, False, 2049, 12),
    # the remaining tile counts NT = ceil(H / 16): 2, 4, 5, 6, 7 (5 and 7: the odd split of the output tiles), one channel,
    # K = 1, and dilation 32768
    (24, 7, False, 65, 1), (32, 6, True, 2049, 2), (64, 15, False, 257, 3), (72, 15, False, 2049, 2), (80, 4, True, 37, 1),
    (96, 9, False, 129, 0), (100, 15, False, 2049, 4), (112, 1, False, 65, 0), (1, 3, False, 37, 0), (16, 15, False, 37, 15)])
def test_conv_gradient_kernels_alone(H, K, causal, T, block):
    """Input and weight gradient of one convolution on a seeded du: linear, so no masks.  Blocks 6 (at T = 37), 12 and 15
    have dilation >= T.  With all rows: NT = 1 .. 8 of the RAW convolution and of the NT x NT grid of tcn_wgrad_kernel."""
    B, nb = 2, block + 1
    c = dict(H=H, nb=nb, K=K, causal=causal, film=False, B=B, T=T)
    m = build(c)
    h = m._handle_train(torch.device(DEV, torch.cuda.current_device()))
    g = cases._g(77)
    du, xin = ct._u(g, (B, H, T), 1.0), ct._u(g, (B, H, T), 1.0)
    du_d, xin_d = du.to(DEV), xin.to(DEV)
    for layer in (0, 1):
        conv = getattr(m.blocks[block], f"conv{layer + 1}")
        w = conv.conv.weight.detach().cpu().double()
        dil, pad = 2 ** block, conv.padding

        def fwd(inp, wt):
            o = F.conv1d(inp, wt, None, padding=pad, dilation=dil)
            return o[:, :, :T] if causal else o

        i64, w64 = xin.double().requires_grad_(), w.clone().requires_grad_()
        (fwd(i64, w64) * du.double()).sum().backward()
        ia, wa = xin.double().abs().requires_grad_(), w.abs().requires_grad_()   # sum |a b| of every output element
        (fwd(ia, wa) * du.double().abs()).sum().backward()
        din = torch.empty(B, H, T, device=DEV)
        dw = torch.empty(H, H, K, device=DEV)
        ws, n = _ws(h, B, T)
        _lib.check(_lib.lib().mst_tcn_train_conv_grads(h.ptr, block, layer, _lib.dptr(du_d), _lib.dptr(xin_d), B, T,
                                                       _lib.dptr(din), _lib.dptr(dw), _lib.dptr(ws), n, _lib.stream_ptr()),
                   "mst_tcn_train_conv_grads")
        for name, got, ref, mag in (("din", din, i64.grad, ia.grad), ("dw", dw, w64.grad, wa.grad)):
            err = (got.cpu().double() - ref).abs()
            ratio = float((err / (mag + 1e-30)).max()) if float(mag.max()) > 0 else float(err.max())
            print(f"conv grads H {H} K {K} causal {causal} T {T} block {block} layer {layer} {name}: max err / sum|ab| {ratio:.2e}")
            assert float((err - 1e-6 * mag).max()) <= 0, (name, ratio)
            assert bool(((mag == 0) <= (got.cpu() == 0)).all())   # taps wholly outside the clip: exact zeros


def test_forward_without_save_gives_the_same_y(monkeypatch):
    c = ctt.CASES["t_causal"]
    x, film = inputs(c, grad=False)
    with torch.no_grad():
        y0 = build(c)(x, film_params=ctt.film_dicts(film))
    assert torch.equal(y0.cpu(), runs("t_causal", monkeypatch)[0].y)


def test_c_abi_refuses_bad_arguments_without_launching():
    c = ctt.CASES["t_h8"]
    m = build(c)
    x, _ = inputs(c, grad=False)
    h = m._handle_train(x.device)
    L = _lib.lib()
    B, T, nb, H = c["B"], c["T"], c["nb"], c["H"]
    ws, n = _ws(h, B, T)
    y = torch.full_like(x, 7.0)
    mean, var = torch.empty(2 * nb, H, device=DEV), torch.empty(2 * nb, H, device=DEV)
    film = torch.ones(B, nb, 4, H, device=DEV)
    call = lambda film, nws: L.mst_tcn_forward_train(h.ptr, _lib.dptr(x), _lib.dptr(film), B, T, _lib.dptr(y), _lib.dptr(mean),  # noqa: E731
                                                     _lib.dptr(var), None, 0, _lib.dptr(ws), nws, _lib.stream_ptr())
    assert call(None, n - 1) != 0 and b"workspace" in L.mst_last_error()
    assert call(film, n) != 0 and b"film" in L.mst_last_error()          # a plain mixer takes no FiLM tensor
    save = torch.empty(16, device=DEV, dtype=torch.uint8)
    assert L.mst_tcn_forward_train(h.ptr, _lib.dptr(x), None, B, T, _lib.dptr(y), _lib.dptr(mean), _lib.dptr(var), _lib.dptr(save), 16,
                                   _lib.dptr(ws), n, _lib.stream_ptr()) != 0 and b"save" in L.mst_last_error()
    assert L.mst_tcn_train_workspace_bytes(h.ptr, 0, T) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                          # nothing was launched
    assert call(None, n) == 0
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any())


def test_backward_refuses_bad_arguments_without_launching():
    c = ctt.CASES["t_h8"]
    m = build(c)
    x, _ = inputs(c, grad=False)
    _, save, h = m._train_forward(x, None, want_save=True)
    L = _lib.lib()
    B, T, nb, H, K = c["B"], c["T"], c["nb"], c["H"], c["K"]
    ws, n = _ws(h, B, T)
    dy = ctt.dy_tensor(c).to(DEV)
    shapes = dict(input_w=(H, 8, 1), input_b=(H,), conv_w=(nb, 2, H, H, K), conv_b=(nb, 2, H), bn_w=(nb, 2, H), bn_b=(nb, 2, H),
                  output_w=(8, H, 1), output_b=(8,))
    g = {k: torch.full(v, 7.0, device=DEV) for k, v in shapes.items()}
    dx, dfilm = torch.full_like(x, 7.0), torch.full((B, nb, 4, H), 7.0, device=DEV)

    def call(grads=None, nsave=save.numel(), nws=n, dfilm=None):
        gs = _lib.TcnGrads(**{k: v.data_ptr() for k, v in g.items()}) if grads is None else grads
        return L.mst_tcn_backward(h.ptr, _lib.dptr(dy), _lib.dptr(x), None, B, T, _lib.dptr(save), nsave, C.byref(gs), _lib.dptr(dx),
                                  _lib.dptr(dfilm), _lib.dptr(ws), nws, _lib.stream_ptr())

    assert call(nws=n - 1) != 0 and b"workspace" in L.mst_last_error()
    assert call(nsave=save.numel() - 1) != 0 and b"save" in L.mst_last_error()
    missing = _lib.TcnGrads(**{k: v.data_ptr() for k, v in g.items() if k != "bn_w"})
    assert call(grads=missing) != 0 and b"gradient pointer" in L.mst_last_error()
    assert call(dfilm=dfilm) != 0 and b"dfilm" in L.mst_last_error()        # a plain mixer has no FiLM gradient
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (*g.values(), dx, dfilm))    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not any(bool((t == 7.0).any()) for t in (*g.values(), dx))


def test_training_calls_need_update_params_first():
    c = ctt.CASES["t_h8"]
    m = build(c, "hip")
    x, _ = inputs(c, grad=False)
    h = m._handle(x.device)              # mst_tcn_create alone: no training copies of the weights yet
    L = _lib.lib()
    B, T, nb, H = c["B"], c["T"], c["nb"], c["H"]
    ws, n = _ws(h, B, T)
    y = torch.full_like(x, 7.0)
    mean, var = torch.empty(2 * nb, H, device=DEV), torch.empty(2 * nb, H, device=DEV)
    assert L.mst_tcn_forward_train(h.ptr, _lib.dptr(x), None, B, T, _lib.dptr(y), _lib.dptr(mean), _lib.dptr(var), None, 0,
                                   _lib.dptr(ws), n, _lib.stream_ptr()) != 0
    assert b"mst_tcn_update_params" in L.mst_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_second_forward_of_a_step_does_not_refresh_the_weights():
    """Only a moved parameter triggers mst_tcn_update_params; the running statistics, which every train-mode forward moves,
    are refreshed for the inference path alone."""
    c = ctt.CASES["t_h8"]
    m = build(c)
    x, _ = inputs(c, grad=False)
    calls = []
    real = _lib.lib().mst_tcn_update_params
    try:
        _lib.lib().mst_tcn_update_params = lambda *a: (calls.append(1), real(*a))[1]
        with torch.no_grad():
            m(x), m(x)
            assert len(calls) == 1
            m.eval()
            y = m(x)
            assert len(calls) == 2
            assert torch.equal(y, build(c, "hip", sd={k: v.clone() for k, v in m.state_dict().items()}).eval()(x))
    finally:
        _lib.lib().mst_tcn_update_params = real


def test_parameter_refresh_after_an_optimiser_step(monkeypatch):
    c = ctt.CASES["t_st"]
    a = build(c)
    x, film = inputs(c, grad=False)
    fp = ctt.film_dicts(film)
    opt = torch.optim.AdamW(a.parameters(), lr=1e-2)
    (a(x, film_params=fp) * ctt.dy_tensor(c).to(DEV)).sum().backward()
    handle = a._hip
    opt.step()
    fresh = build(c, sd={k: v.detach().clone() for k, v in a.state_dict().items()})
    with torch.no_grad():
        ya, yf = a(x, film_params=fp), fresh(x, film_params=fp)
    assert a._hip is handle                     # refreshed on the device, not rebuilt
    assert torch.equal(ya, yf)
    assert not torch.equal(ya.cpu(), runs("t_st", monkeypatch)[0].y)   # the step did move the parameters


def test_eval_without_gradients_is_the_inference_path():
    c = ctt.CASES["t_st"]
    x, film = inputs(c, grad=False)
    fp = ctt.film_dicts(film)
    a, b = build(c).eval(), build(c, "hip").eval()
    with torch.no_grad():
        assert torch.equal(a(x, film_params=fp), b(x, film_params=fp))
    with pytest.raises(RuntimeError, match=r"eval\(\) mode.*backend='torch'"):
        a(x, film_params=fp)


def test_autograd_plumbing():
    c = ctt.CASES["t_causal"]
    m = build(c)
    gen = tm.TCNFiLMGenerator(embed_dim=64, num_blocks=c["nb"], hidden_channels=c["H"])
    gen.load_state_dict(ct.make_film_state_dict(64, c), strict=True)
    gen.backend = "torch"
    gen = gen.to(DEV).train()
    x, _ = inputs(c, grad=False)
    y = m(x, film_params=gen(ct.embeddings(c["B"], 64).to(DEV)))     # dict FiLM tensors from the generator
    loss = (y * ctt.dy_tensor(c).to(DEV)).sum()
    loss.backward()
    assert x.grad is None
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in gen.parameters())
    assert all(p.grad is not None for p in m.parameters())
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        loss.backward()


def test_training_example_learns_and_repeats():
    script = os.path.join(cases.ROOT, "examples", "train_tcn_mixer.py")
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, script, "--steps", "6", "--seconds", "0.4"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([float(l.split("loss")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("step")])
    assert len(outs[0]) == 6 and outs[0][5] < outs[0][0], outs[0]
    assert outs[0] == outs[1]
