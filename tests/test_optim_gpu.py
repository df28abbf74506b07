"""GPU: the optimiser step on the kernels of csrc/optim.hip (mst_amd.optim) -- clip_grad_norm_, Adam / AdamW / SGD, keep_best.

Parity is judged on ONE step from a given fp32 state, three ways: the kernels, PyTorch's fp32 optimiser (foreach=False) and the
same optimiser in float64, all from identical fp32 inputs.  Per quantity group (parameters, exp_avg, exp_avg_sq,
momentum_buffer), with rel = |d| / max(|ref64|, 0.01 max|ref64|), the kernels stay within 2 x PyTorch fp32's own distance from
float64.  (A free-running trajectory is no yardstick: m / sqrt(v) amplifies earlier rounding, and a merely re-ordered fp32
restatement reaches 2.5 x after ten steps.)  Two states: all-zero (step 1) and the state after nine PyTorch fp32 steps (step 10).

Measured on an MI355X: e_hip 4.8e-8 ... 6.0e-8 in every group (the kernels evaluate in double and round once, so an element is
as close to float64 as an fp32 value can be), e_torch_fp32 5.9e-8 ... 1.8e-7 (5.9e-8 ... 1.4e-7 from the nine-step state: not
degenerate), ratios 0.31 ... 1.00; the table is in DESIGN.md section 3.14."""
import copy

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (sys.path setup)
import parity
from mst_amd import optim as hip_optim
from mst_amd.tcn_mixer import TCNMixer

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 70001)
VIEW_N, GVIEW_N = 301, 515


def _scales(n, lo=1e-2, hi=10.0):
    return [float(lo * (hi / lo) ** (i / (n - 1))) for i in range(n)]


def host_params(seed=100):
    g = torch.Generator().manual_seed(seed)
    sizes = SIZES + (VIEW_N, GVIEW_N)
    return [s * torch.randn(n, generator=g) for n, s in zip(sizes, _scales(len(sizes)))]


def host_grads(k):
    """Seeded gradients of step k: per-tensor magnitudes 1e-2 ... 10 (reversed against the parameters'), times a per-step factor."""
    g = torch.Generator().manual_seed(1000 + k)
    sizes = SIZES + (VIEW_N, GVIEW_N)
    f = 10.0 ** (((k * 7) % 5 - 2) / 2.0)
    return [f * s * torch.randn(n, generator=g) for n, s in zip(sizes, reversed(_scales(len(sizes))))]


def device_list(params, grads, views=True):
    """The list on the GPU, with one parameter without a gradient at position 3: plain tensors, or (views) the last two as
    odd-offset views of larger buffers."""
    out = []
    for i, (p, g) in enumerate(zip(params, grads)):
        p, g = p.cuda(), g.cuda()
        if views and i == len(params) - 2:      # the parameter itself is a view at an odd element offset
            buf = torch.zeros(p.numel() + 8, device="cuda")
            buf[3:3 + p.numel()] = p
            p = buf[3:3 + p.numel()]
            assert p.data_ptr() % 16 == 12
        q = torch.nn.Parameter(p)
        if views and i == len(params) - 1:      # its gradient is
            gbuf = torch.zeros(g.numel() + 8, device="cuda")
            gbuf[1:1 + g.numel()] = g
            g = gbuf[1:1 + g.numel()]
            assert g.data_ptr() % 16 == 4
        q.grad = g
        out.append(q)
    out.insert(3, torch.nn.Parameter(torch.ones(17, device="cuda")))   # .grad is None: skipped, as in torch
    return out


def with_grad(ps):
    return [p for p in ps if p.grad is not None]


def group_of(i, n, groups):
    return 0 if len(groups) == 1 or i < n // 2 else 1


CONFIGS = {
    "adam": (hip_optim.Adam, torch.optim.Adam, [dict(lr=1e-2, weight_decay=1e-2)], ("exp_avg", "exp_avg_sq")),
    "adamw": (hip_optim.AdamW, torch.optim.AdamW, [dict(lr=1e-2, weight_decay=1e-2), dict(lr=3e-3, weight_decay=1e-4, betas=(0.8, 0.99))],
              ("exp_avg", "exp_avg_sq")),
    "sgd": (hip_optim.SGD, torch.optim.SGD, [dict(lr=1e-2, momentum=0.9, weight_decay=1e-3)], ("momentum_buffer",)),
}


def build(cls, params, groups, **kw):
    if len(groups) == 1:
        return cls(params, **groups[0], **kw)
    half = len(params) // 2
    return cls([dict(params=params[:half], **groups[0]), dict(params=params[half:], **groups[1])], **kw)


_STATE = {}


def nine_step_state(name):
    """(params, a copy of the optimizer state_dict) after nine PyTorch fp32 steps; computed once per optimiser."""
    if name not in _STATE:
        _, tcls, groups, _ = CONFIGS[name]
        ps = device_list(host_params(), host_grads(0), views=False)
        opt = build(tcls, ps, groups, foreach=False)
        for k in range(1, 10):
            for p, g in zip(with_grad(ps), host_grads(k)):
                p.grad = g.cuda()
            opt.step()
        _STATE[name] = ([p.detach().cpu().clone() for p in with_grad(ps)], opt.state_dict())
    params, sd = _STATE[name]
    return params, copy.deepcopy(sd)   # (load_state_dict keeps the tensors it is given, and a step then writes into them)


def one_step(name, state, how):
    """One step from `state` ("zero" or "nine"): how = "hip", "torch32", "torch64".  Returns {group: concatenated result}."""
    hcls, tcls, groups, keys = CONFIGS[name]
    params, sd = (host_params(), None) if state == "zero" else nine_step_state(name)
    grads = host_grads(10)
    ps = device_list(params, grads, views=how == "hip")
    if how == "torch64":
        for i, p in enumerate(ps):
            g = None if p.grad is None else p.grad.double()
            ps[i] = torch.nn.Parameter(p.detach().double())
            ps[i].grad = g
    stepped = with_grad(ps)
    opt = build(hcls if how == "hip" else tcls, ps, groups, **({} if how == "hip" else {"foreach": False}))
    if sd is not None:
        opt.load_state_dict(sd)
    before = [p._version for p in stepped]
    opt.step()
    if how == "hip":
        assert all(p._version > v for p, v in zip(stepped, before)), "a stepped parameter's version counter did not move"
        skipped = [p for p in ps if p.grad is None]
        assert skipped and all(torch.equal(p, torch.ones_like(p)) and not opt.state[p] for p in skipped)
    out = {"param": torch.cat([p.detach().flatten() for p in stepped])}
    for k in keys:
        out[k] = torch.cat([opt.state[p][k].flatten() for p in stepped])
    if "exp_avg" in keys:
        steps = {float(opt.state[p]["step"]) for p in stepped}
        assert steps == {1.0 if state == "zero" else 10.0}, steps
    return out


def rel_err(got, ref64):
    ref = ref64.double()
    return float(((got.double() - ref).abs() / ref.abs().clamp(min=0.01 * float(ref.abs().max()))).max())


@pytest.mark.parametrize("state", ["zero", "nine"])
@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_one_step_parity_against_float64(name, state):
    hip, t32, t64 = (one_step(name, state, how) for how in ("hip", "torch32", "torch64"))
    for group in hip:
        e_hip, e_ref = rel_err(hip[group], t64[group]), rel_err(t32[group], t64[group])
        parity.note(f"optim {name} step-{'1' if state == 'zero' else '10'} {group}", e_hip=e_hip, e_torch_fp32=e_ref,
                    ratio=e_hip / e_ref if e_ref else float("inf"))
        print(f"{name} {state} {group}: e_hip {e_hip:.3e}, e_torch_fp32 {e_ref:.3e}, ratio {e_hip / max(e_ref, 1e-300):.3f}")
        assert e_ref > 1e-9, f"degenerate fixture: PyTorch fp32 is within {e_ref:.1e} of float64 for {group}"
        assert e_hip <= 2.0 * e_ref, (group, e_hip, e_ref)


@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_list_independence_and_repeatability(name):
    hcls, _, groups, keys = CONFIGS[name]
    params, sd = nine_step_state(name)
    whole = one_step(name, "nine", "hip")
    again = one_step(name, "nine", "hip")
    for k in whole:
        assert torch.equal(whole[k], again[k]), f"{k}: two identical runs differ"
    # every tensor in a call of its own (its own list, position 0, plain storage: no views), with its group's hyper-parameters
    ps = device_list(params, host_grads(10), views=False)
    outs = {k: [] for k in whole}
    for i, p in enumerate(ps):
        if p.grad is None:
            continue
        gi = group_of(i, len(ps), groups)
        opt = hcls([p], **groups[gi])
        opt.load_state_dict({"state": {0: sd["state"][i]}, "param_groups": [dict(sd["param_groups"][gi], params=[0])]})
        opt.step()
        outs["param"].append(p.detach().flatten())
        for k in keys:
            outs[k].append(opt.state[p][k].flatten())
    for k in whole:
        assert torch.equal(whole[k], torch.cat(outs[k])), f"{k}: the result depends on the list an element sits in"


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_equally_offset_views_take_the_wide_path_with_head_and_tail(name, offset):
    """Parameter, gradient and state as slices of stacked buffers at ONE odd element offset (what a gradient reducer hands out):
    16-byte accesses between a scalar head and tail.  Same bits as the plain tensors."""
    hcls, _, groups, keys = CONFIGS[name]
    n = 4096 + 1030   # two chunks, the second one partial
    g = torch.Generator().manual_seed(offset)
    vals = {k: torch.randn(n, generator=g).cuda() for k in ("param", "grad") + keys}
    if "exp_avg_sq" in vals:
        vals["exp_avg_sq"] = vals["exp_avg_sq"].square()

    def run(off):
        def put(v):
            buf = torch.zeros(n + 8, device="cuda")
            buf[off:off + n] = v
            return buf[off:off + n]
        p = torch.nn.Parameter(put(vals["param"]))
        p.grad = put(vals["grad"])
        opt = hcls([p], **groups[0])
        opt.state[p] = {k: put(vals[k]) for k in keys}
        if name != "sgd":
            opt.state[p]["step"] = torch.full((), 4.0, device="cuda")
        opt.step()
        return [p.detach().clone()] + [opt.state[p][k].clone() for k in keys]

    plain, view = run(0), run(offset)
    assert view[0].data_ptr() % 16 == 0 and all(torch.equal(a, b) for a, b in zip(plain, view))
    assert not torch.equal(plain[0], vals["param"])


@pytest.mark.parametrize("name", ["adamw", "sgd"])
def test_found_inf_and_grad_scale(name):
    hcls, _, groups, keys = CONFIGS[name]

    def fresh(scale=1.0):
        params, sd = nine_step_state(name)
        ps = device_list(params, [g * scale for g in host_grads(10)], views=False)
        opt = build(hcls, ps, groups)
        opt.load_state_dict(sd)
        return with_grad(ps), opt

    def snapshot(ps, opt):
        return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in keys + (("step",) if name != "sgd" else ())]

    ps, opt = fresh()
    before = snapshot(ps, opt)
    opt.grad_scale, opt.found_inf = torch.full((), 1024.0, device="cuda"), torch.ones((), device="cuda")
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot(ps, opt))), "found_inf = 1 changed parameters, state or step"
    ps1, opt1 = fresh()
    opt1.step()
    ps2, opt2 = fresh(1024.0)
    opt2.grad_scale, opt2.found_inf = torch.full((), 1024.0, device="cuda"), torch.zeros((), device="cuda")
    opt2.step()
    assert all(torch.equal(a, b) for a, b in zip(snapshot(ps1, opt1), snapshot(ps2, opt2))), "grad_scale = 1024 is not the unscaled step"
    assert not any(torch.equal(a, b) for a, b in zip(before[:len(ps)], snapshot(ps1, opt1)[:len(ps)]))   # (the step does move them)


def test_grad_scaler_takes_the_attribute_path(monkeypatch):
    torch.manual_seed(3)
    w = torch.randn(300, device="cuda")

    def run(scaled):
        p = torch.nn.Parameter(torch.linspace(-1, 1, 300, device="cuda"))
        opt = hip_optim.AdamW([p], lr=1e-2)
        loss = (p * w).sum()
        if not scaled:
            loss.backward()
            opt.step()
            return p, opt
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        scaler.scale(loss).backward()

        def no_host_read(self, *a, **k):
            raise AssertionError("a host read inside GradScaler.step")
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "item", no_host_read)
            m.setattr(torch.Tensor, "tolist", no_host_read)
            m.setattr(torch.Tensor, "__bool__", no_host_read)
            m.setattr(torch.Tensor, "__float__", no_host_read)
            scaler.step(opt)
        scaler.update()
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
        return p, opt

    p0, opt0 = run(False)
    p1, opt1 = run(True)
    assert opt0.amp_steps == 0 and opt1.amp_steps == 1
    assert torch.equal(p0, p1) and float(opt1.state[p1]["step"]) == 1.0


def test_stepped_mixer_equals_a_fresh_one():
    """Version counters: the mixer's device weights follow the optimiser's in-place update."""
    torch.manual_seed(11)
    tcn = TCNMixer(hidden_channels=8, num_blocks=3, kernel_size=5).cuda().train()
    tcn.backend = "hip-train"
    x = 0.1 * torch.randn(1, 8, 3000, device="cuda")
    opt = hip_optim.AdamW(tcn.parameters(), lr=1e-2)
    tcn(x).square().mean().backward()
    before = [p._version for p in tcn.parameters()]
    norm = hip_optim.clip_grad_norm_(tcn.parameters(), 1.0)
    opt.step()
    assert float(norm) > 0 and all(p._version > v for p, v in zip(tcn.parameters(), before))
    fresh = TCNMixer(hidden_channels=8, num_blocks=3, kernel_size=5)
    fresh.load_state_dict(tcn.state_dict())
    fresh = fresh.cuda().train()
    fresh.backend = "hip-train"
    with torch.no_grad():
        y_live, y_fresh = tcn(x), fresh(x)
    assert torch.equal(y_live, y_fresh)
    assert not torch.equal(y_live, x)


# ---- clip ----------------------------------------------------------------------------------------------------------------------
def clip_list(inf_at=None):
    ps = device_list(host_params(), host_grads(10))
    if inf_at is not None:
        with_grad = [p for p in ps if p.grad is not None]
        with_grad[inf_at].grad[0] = float("inf")
    return ps


def test_clip_norm_coefficient_and_scaling():
    ps = clip_list()
    grads = [p.grad.clone() for p in ps if p.grad is not None]
    exact = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in grads)))
    max_norm = 0.37
    norm = hip_optim.clip_grad_norm_(ps, max_norm)
    assert norm.shape == () and norm.is_cuda and norm.dtype == torch.float32
    rel = abs(float(norm) - exact) / exact
    parity.note("optim clip norm vs float64", rel=rel)
    assert rel <= 2.0 ** -23, rel
    n32 = np.float32(float(norm))
    # the fp32 evaluation of clip_grad_norm_'s formula on that norm (IEEE on the host; torch's scalar / tensor is reciprocal * scalar)
    coef_np = min(np.float32(1.0), np.float32(max_norm) * (np.float32(1.0) / (n32 + np.float32(1e-6))))
    coef = hip_optim.clip_grad_norm_.last_coef
    assert float(coef) == float(coef_np) and float(coef) < 1.0
    # ... and the library's own evaluation on the device, whose reciprocal kernel need not round correctly: within one ulp
    coef_t = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    assert abs(float(coef_t) - float(coef)) <= float(np.spacing(coef_np))
    for p, g in zip([p for p in ps if p.grad is not None], grads):
        assert torch.equal(p.grad, g * coef)
    # twice: the same bits
    ps2 = clip_list()
    norm2 = hip_optim.clip_grad_norm_(ps2, max_norm)
    assert torch.equal(norm, norm2)
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(ps, ps2) if a.grad is not None)
    # torch's own value of the same list, for the record (its reduction order is the library's)
    ps3 = clip_list()
    ref = torch.nn.utils.clip_grad_norm_(ps3, max_norm, foreach=False)
    assert abs(float(ref) - exact) / exact < 1e-5


def test_clip_leaves_small_gradients_alone_and_reports_inf():
    ps = clip_list()
    grads = [p.grad.clone() for p in ps if p.grad is not None]
    norm = hip_optim.clip_grad_norm_(ps, 1e9)
    assert float(hip_optim.clip_grad_norm_.last_coef) == 1.0 and float(norm) > 1.0
    for p, g in zip([p for p in ps if p.grad is not None], grads):
        assert torch.equal(p.grad, g)
    bad = clip_list(inf_at=6)
    assert not torch.isfinite(hip_optim.clip_grad_norm_(bad, 1.0))
    nan = clip_list()
    [p for p in nan if p.grad is not None][9].grad[70000] = float("nan")
    assert torch.isnan(hip_optim.clip_grad_norm_(nan, 1.0)) and torch.isnan(hip_optim.clip_grad_norm_.last_coef)


def test_tables_are_rebuilt_only_when_a_pointer_changed():
    """The table is rebuilt only when a pointer in it has changed; a second call on the same gradients builds nothing."""
    ps = clip_list()
    hip_optim.clip_grad_norm_(ps, 1.0)
    tables = dict(hip_optim._CLIP_TABLES)
    hip_optim.clip_grad_norm_(ps, 1.0)
    assert list(hip_optim._CLIP_TABLES.values())[-1] is list(tables.values())[-1]
    opt = hip_optim.SGD(ps, lr=1e-3, momentum=0.9)
    opt.step()
    t1 = opt._tables[0]
    opt.step()
    assert opt._tables[0] is t1
    ps[0].grad = ps[0].grad.clone()
    opt.step()
    assert opt._tables[0] is not t1


# ---- keep_best -----------------------------------------------------------------------------------------------------------------
def test_keep_best_sequence():
    losses = [0.5, 0.7, 0.3, 0.3, float("nan"), 0.4]
    best = torch.full((), float("inf"), device="cuda")
    index = torch.full((), -1, dtype=torch.int32, device="cuda")
    history = torch.full((len(losses),), -1.0, device="cuda")
    a, b = torch.empty(1000, device="cuda"), torch.empty(3, 77, device="cuda")
    da, db = torch.zeros_like(a), torch.zeros_like(b)
    for i, l in enumerate(losses):
        a.fill_(float(i)), b.fill_(10.0 + i)
        hip_optim.keep_best(torch.tensor(l, device="cuda"), best, index, history, i, [(a, da), (b, db)])
    assert float(best) == np.float32(0.3) and int(index) == 2
    assert torch.equal(da, torch.full_like(da, 2.0)) and torch.equal(db, torch.full_like(db, 12.0))
    h = history.cpu().numpy()
    assert np.array_equal(h[[0, 1, 2, 3, 5]], np.float32([0.5, 0.7, 0.3, 0.3, 0.4])) and np.isnan(h[4])


def test_contrastive_example_with_the_hip_optimiser(tmp_path):
    """examples/train_contrastive.py --optimizer hip: the encoder's ~100 parameters (views of stacked tensors among them) through
    mst_amd.optim.AdamW; the loss stays finite and the parameters' versions reach the training trunk (it would refuse stale ones)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(cases.ROOT, "examples"))
    import train_contrastive as tc
    losses = tc.main(["--shards", str(tmp_path / "shards"), "--synthetic", "6", "--track-seconds", "3.0", "--clip-seconds", "1.0",
                      "--batch-size", "6", "--steps", "4", "--lr", "3e-4", "--optimizer", "hip"])
    assert len(losses) == 4 and all(l == l and l < 10 for l in losses)
