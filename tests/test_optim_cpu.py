"""CPU: mst_amd.optim's classes against their torch.optim namesakes -- constructor defaults, param-group keys, the state-dict
round trip in both directions (without stepping: the step is GPU only), every refusal by name -- and the refusals of the
per-pair fit `optimize_tcn_style_transfer` that are decided before anything touches a GPU."""
import copy
import inspect

import pytest
import torch

import cases  # noqa: F401  (sys.path setup)
from mst_amd import optim as hip_optim
from mst_amd.model import MixingStyleEncoder
from mst_amd.tcn_mixer import TCNMixer, optimize_tcn_style_transfer

PAIRS = [(hip_optim.Adam, torch.optim.Adam), (hip_optim.AdamW, torch.optim.AdamW), (hip_optim.SGD, torch.optim.SGD)]


def params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (3, 8, 5)]


@pytest.mark.parametrize("mine,theirs", PAIRS)
def test_defaults_signature_and_group_keys(mine, theirs):
    a, b = mine(params()), theirs(params())
    assert isinstance(a, torch.optim.Optimizer)
    assert a.defaults == b.defaults
    assert list(a.param_groups[0].keys()) == list(b.param_groups[0].keys())
    sa, sb = inspect.signature(mine.__init__), inspect.signature(theirs.__init__)
    assert list(sa.parameters) == list(sb.parameters)
    assert all(sa.parameters[k].default == sb.parameters[k].default and sa.parameters[k].kind == sb.parameters[k].kind
               for k in sa.parameters)
    assert "grad_scaler" not in sa.parameters and "grad_scaler" not in inspect.signature(mine.step).parameters
    assert mine._step_supports_amp_scaling is True


def test_groups_and_schedulers():
    ps = params()
    opt = hip_optim.AdamW([dict(params=ps[:1], lr=1e-3, weight_decay=1e-4), dict(params=ps[1:], lr=3e-3)], weight_decay=0.5)
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 3e-3] and [g["weight_decay"] for g in opt.param_groups] == [1e-4, 0.5]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(hip_optim.SGD(params(), lr=0.1, momentum=0.9), T_max=10)
    assert sched.get_last_lr() == [1e-3, 3e-3] and cos.get_last_lr() == [0.1]


def _torch_state(theirs, ps, **kw):
    """A stepped torch.optim optimiser on CPU parameters (the checkpoint a reference run writes)."""
    opt = theirs(ps, **kw)
    for k in range(3):
        for p in ps:
            p.grad = torch.full_like(p, 0.1 * (k + 1))
        opt.step()
    return opt


@pytest.mark.parametrize("mine,theirs,kw", [(hip_optim.Adam, torch.optim.Adam, dict(lr=1e-2, weight_decay=1e-3)),
                                            (hip_optim.AdamW, torch.optim.AdamW, dict(lr=1e-2)),
                                            (hip_optim.SGD, torch.optim.SGD, dict(lr=1e-2, momentum=0.9))])
def test_state_dict_round_trip_both_directions(mine, theirs, kw):
    ps = params()
    ref = _torch_state(theirs, ps, **kw)
    sd = ref.state_dict()
    a = mine(ps, lr=123.0)
    a.load_state_dict(copy.deepcopy(sd))       # torch -> here (a copy: load_state_dict keeps the tensors it is given)
    assert a.param_groups[0]["lr"] == kw["lr"]
    for p in ps:
        assert set(a.state[p]) == set(ref.state[p])
        for k, v in ref.state[p].items():
            got = a.state[p][k]
            assert torch.equal(got.cpu().float().reshape(v.shape), v.float()), k
            if k == "step":   # lives next to the parameter, as torch's capturable / fused step does
                assert got.dtype == torch.float32 and got.device == p.device and got.shape == ()
    back = theirs(ps, lr=456.0)
    back.load_state_dict(copy.deepcopy(a.state_dict()))   # here -> torch
    assert back.param_groups[0]["lr"] == kw["lr"]
    for p in ps:
        assert set(back.state[p]) == set(ref.state[p])
        assert all(torch.equal(torch.as_tensor(back.state[p][k]).float(), torch.as_tensor(v).float()) for k, v in ref.state[p].items())
    # ... and the torch class continues from it exactly as from its own checkpoint
    twin_ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    twin = theirs(twin_ps, **kw)
    twin.load_state_dict(copy.deepcopy(sd))
    for q, p in zip(twin_ps, ps):
        q.grad = torch.full_like(q, -0.3)
        p.grad = torch.full_like(p, -0.3)
    twin.step(), back.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, twin_ps))


REFUSALS = [
    (lambda ps: hip_optim.Adam(ps, amsgrad=True), "amsgrad", "torch.optim.Adam"),
    (lambda ps: hip_optim.AdamW(ps, amsgrad=True), "amsgrad", "torch.optim.AdamW"),
    (lambda ps: hip_optim.Adam(ps, maximize=True), "maximize", "torch.optim.Adam"),
    (lambda ps: hip_optim.AdamW(ps, differentiable=True), "differentiable", "torch.optim.AdamW"),
    (lambda ps: hip_optim.AdamW(ps, lr=torch.tensor(1e-3)), "tensor lr", "torch.optim.AdamW"),
    (lambda ps: hip_optim.SGD(ps, momentum=0.9, nesterov=True), "nesterov", "torch.optim.SGD"),
    (lambda ps: hip_optim.SGD(ps, momentum=0.9, dampening=0.1), "dampening", "torch.optim.SGD"),
    (lambda ps: hip_optim.SGD(ps, maximize=True), "maximize", "torch.optim.SGD"),
]


@pytest.mark.parametrize("make,reason,alternative", REFUSALS)
def test_refused_options_name_the_reason_and_torch(make, reason, alternative):
    with pytest.raises(RuntimeError) as e:
        make(params())
    assert reason in str(e.value) and alternative in str(e.value)


def test_refused_options_arriving_through_a_state_dict():
    ps = params()
    sd = torch.optim.Adam(ps, amsgrad=True).state_dict()
    with pytest.raises(RuntimeError, match="amsgrad"):
        hip_optim.Adam(ps).load_state_dict(sd)


@pytest.mark.parametrize("mine", [hip_optim.Adam, hip_optim.AdamW, hip_optim.SGD])
def test_step_refuses_tensors_the_kernels_cannot_take(mine):
    ps = params()
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match=r"cpu.*no CPU fallback.*torch\.optim\." + mine.__name__):
        mine(ps).step()
    assert all(torch.equal(p, q) for p, q in zip(ps, params()))   # nothing moved: there is no silent library path
    ps = params()
    ps[1].grad = torch.sparse_coo_tensor(torch.tensor([[0]]), torch.tensor([1.0]), (8,))
    with pytest.raises(RuntimeError, match="sparse"):
        mine(ps).step()
    half = [torch.nn.Parameter(p.detach().half()) for p in params()]
    for p in half:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="float16.*fp32"):
        mine(half).step()
    mine(params()).step()   # no gradient anywhere: nothing to do, as in torch


def test_clip_refusals():
    ps = params()
    for p in ps:
        p.grad = torch.ones_like(p)
    for kw, reason in ((dict(norm_type=1.0), "norm_type"), (dict(norm_type=float("inf")), "norm_type"),
                       (dict(error_if_nonfinite=True), "error_if_nonfinite"), ({}, "cpu")):
        with pytest.raises(RuntimeError) as e:
            hip_optim.clip_grad_norm_(ps, 1.0, **kw)
        assert reason in str(e.value) and "torch.nn.utils.clip_grad_norm_" in str(e.value)
    assert all(torch.equal(p.grad, torch.ones_like(p)) for p in ps)
    assert float(hip_optim.clip_grad_norm_(params(), 1.0)) == 0.0   # no gradients: torch's answer
    assert list(inspect.signature(hip_optim.clip_grad_norm_).parameters)[:3] == ["parameters", "max_norm", "norm_type"]


def _fit_args():
    tcn = TCNMixer(hidden_channels=8, num_blocks=3, kernel_size=5)
    enc = MixingStyleEncoder(n_fft=1024, hop_length=256, n_mels=128, embed_dim=32, feature_dim=64).eval()
    for q in enc.parameters():
        q.requires_grad_(False)
    enc.input_grad_backend = "hip"
    stems = {s: torch.zeros(2, 4096) for s in ("vocals", "bass", "drums", "other")}
    return tcn, stems, torch.ones(32), enc


def test_fit_refuses_a_training_or_live_encoder_by_name():
    tcn, stems, target, enc = _fit_args()
    enc.train()
    with pytest.raises(RuntimeError, match=r"train\(\) mode.*mixing_model\.eval\(\)"):
        optimize_tcn_style_transfer(tcn, stems, target, enc, None, "cpu", num_steps=1, verbose=False)
    enc.eval()
    next(enc.parameters()).requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"1 parameters of mixing_model require grad.*requires_grad_\(False\)"):
        optimize_tcn_style_transfer(tcn, stems, target, enc, None, "cpu", num_steps=1, verbose=False)
    next(enc.parameters()).requires_grad_(False)
    enc.input_grad_backend = "none"
    with pytest.raises(RuntimeError, match="input_grad_backend='hip'"):
        optimize_tcn_style_transfer(tcn, stems, target, enc, None, "cpu", num_steps=1, verbose=False)
    enc.input_grad_backend = "hip"
    for kw, reason in ((dict(optimizer="rmsprop"), "optimizer="), (dict(sync="never"), "sync=")):
        with pytest.raises(RuntimeError, match=reason):
            optimize_tcn_style_transfer(tcn, stems, target, enc, None, "cpu", num_steps=1, verbose=False, **kw)
    sig = inspect.signature(optimize_tcn_style_transfer)
    assert list(sig.parameters) == ["tcn", "stems_input", "target_emb", "mixing_model", "feature_extractor", "device", "num_steps",
                                    "lr", "verbose", "optimizer", "sync"]
    assert (sig.parameters["num_steps"].default, sig.parameters["lr"].default, sig.parameters["verbose"].default) == (200, 0.01, True)
    assert sig.parameters["optimizer"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["sync"].kind is inspect.Parameter.KEYWORD_ONLY
