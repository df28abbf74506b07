"""CPU: MultiResolutionSTFTLoss(backend="torch") reproduces the reference's fixture (tests/golden/mrstft.npz, written by
tests/golden/make_golden_mrstft.py), has the reference's signature, and backend="hip" refuses what it cannot run."""
import inspect

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (sys.path setup)
import cases_mrstft as cm
from mst_amd.loss import MultiResolutionSTFTLoss


@pytest.fixture(scope="module")
def golden():
    return np.load(cm.GOLDEN)


def _evaluate(case, dtype, term="full"):
    x, y = cm.inputs(case)
    scw, lw = cm.TERMS[term]
    m = MultiResolutionSTFTLoss(backend="torch", sc_weight=scw, log_weight=lw)
    x = x.to(dtype).requires_grad_(True)
    loss = m(x, y.to(dtype))
    loss.backward()
    return m, loss.detach(), x.grad, x.detach(), y.to(dtype)


@pytest.mark.parametrize("case", cm.case_ids())
def test_torch_backend_reproduces_reference_values(golden, case):
    for dtype, bits in ((torch.float32, 32), (torch.float64, 64)):
        m, loss, _, x, y = _evaluate(case, dtype)
        assert loss.dtype == dtype and loss.dim() == 0
        ref = float(golden[f"{case}_loss{bits}"])
        assert abs(loss.item() - ref) <= 1e-6 * abs(ref), (bits, loss.item(), ref)
        comp = m.components(x, y)
        assert comp.shape == (3, 2) and not comp.requires_grad
        np.testing.assert_allclose(comp.double().numpy(), golden[f"{case}_comp{bits}"].astype(np.float64), rtol=1e-6, atol=0)


@pytest.mark.parametrize("term", list(cm.TERMS))
@pytest.mark.parametrize("case", cm.case_ids())
def test_torch_backend_reproduces_reference_gradients_f64(golden, case, term):
    _, _, g, _, _ = _evaluate(case, torch.float64, term)
    ref = golden[f"{case}_g{term}64"]
    d = cm.l2(cm.grad_samples(g) - ref)
    assert d <= 1e-9 * cm.l2(ref), (d, cm.l2(ref))
    n, nref = cm.l2(g.numpy()), float(golden[f"{case}_g{term}_norm64"])
    assert abs(n - nref) <= 1e-9 * nref


def test_signature_and_defaults_are_the_references():
    sig = inspect.signature(MultiResolutionSTFTLoss.__init__)
    params = list(sig.parameters.values())[1:]
    assert [p.name for p in params[:4]] == ["fft_sizes", "hop_sizes", "win_sizes", "window"]
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:4])
    assert [p.default for p in params[:4]] == [[1024, 2048, 512], [256, 512, 128], [1024, 2048, 512], "hann"]
    extra = {p.name: p for p in params[4:]}
    assert set(extra) == {"sc_weight", "log_weight", "backend"}
    assert all(p.kind == inspect.Parameter.KEYWORD_ONLY for p in extra.values())
    assert (extra["sc_weight"].default, extra["log_weight"].default, extra["backend"].default) == (1.0, 1.0, "hip")
    m = MultiResolutionSTFTLoss([512], [128], [512], "hann")
    assert (m.fft_sizes, m.hop_sizes, m.win_sizes, m.window) == ([512], [128], [512], "hann")
    assert isinstance(m, torch.nn.Module) and not list(m.parameters())


def test_term_weights_sum_to_the_default():
    case = "t6000_near"
    _, l, g, _, _ = _evaluate(case, torch.float64)
    _, lsc, gsc, _, _ = _evaluate(case, torch.float64, "sc")
    _, llog, glog, _, _ = _evaluate(case, torch.float64, "log")
    assert abs((lsc + llog - l).item()) <= 1e-12 * abs(l.item())
    assert cm.l2((gsc + glog - g).numpy()) <= 1e-12 * cm.l2(g.numpy())
    assert lsc.item() > 0 and llog.item() > 0


def test_torch_backend_differentiates_both_arguments_and_2d_equals_3d():
    x, y = cm.inputs("2d4096_near")
    m = MultiResolutionSTFTLoss(backend="torch")
    x, y = x.requires_grad_(True), y.requires_grad_(True)
    l2d = m(x, y)
    l2d.backward()
    assert x.grad.abs().sum() > 0 and y.grad.abs().sum() > 0
    assert torch.equal(l2d.detach(), m(x.detach()[None], y.detach()[None]))


def _hip_raises(m, x, y):
    with pytest.raises(RuntimeError, match="backend='torch'") as e:
        m(x, y)
    return str(e.value)


def test_hip_backend_refuses_cpu_tensors_and_names_torch_backend():
    x, y = cm.inputs("t6000_near")
    assert "CUDA" in _hip_raises(MultiResolutionSTFTLoss(), x, y)
    with pytest.raises(RuntimeError, match="backend='torch'"):
        MultiResolutionSTFTLoss().components(x, y)


@pytest.mark.parametrize("kwargs,T,y_grad,word", [
    (dict(fft_sizes=[1024], hop_sizes=[256], win_sizes=[512]), 6000, False, "win_size"),
    (dict(fft_sizes=[1024], hop_sizes=[100], win_sizes=[1024]), 6000, False, "hop_size"),
    (dict(fft_sizes=[1024], hop_sizes=[1024], win_sizes=[1024]), 6000, False, "hop_size"),
    (dict(fft_sizes=[256], hop_sizes=[64], win_sizes=[256]), 6000, False, "fft_size"),
    (dict(), 1024, False, "T >"),
    (dict(), 6000, True, "target"),
    (dict(window="hamming"), 6000, False, "window"),
])
def test_hip_backend_refuses_unsupported_configurations(kwargs, T, y_grad, word):
    """With a GPU: CUDA tensors, the raised text names the offending setting.  Without one: CPU tensors are refused in any
    case, and the configuration's own refusal is read from the module's check with tensors that report `is_cuda`."""
    m = MultiResolutionSTFTLoss(**kwargs)
    x, y = cm.make_xy(1, T, "near")
    if torch.cuda.is_available():
        x, y = x.cuda(), y.cuda()
        y.requires_grad_(y_grad)
        assert word in _hip_raises(m, x, y)
    else:
        y.requires_grad_(y_grad)
        _hip_raises(m, x, y)                                  # CPU tensors: refused in any case
        msg = m._hip_refusal(_AsCuda(x), _AsCuda(y))          # the configuration's own refusal
        assert msg is not None and word in msg


class _AsCuda:
    """A CPU tensor that reports is_cuda: reaches the configuration checks of the refusal without a GPU."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, k):
        return getattr(self._t, k)


def test_hip_backend_accepts_the_supported_configuration_checks():
    x, y = cm.make_xy(1, 1025, "near")
    assert MultiResolutionSTFTLoss()._hip_refusal(_AsCuda(x), _AsCuda(y)) is None
    for h in (64, 128, 256):
        assert MultiResolutionSTFTLoss([512], [h], [512])._hip_refusal(_AsCuda(x), _AsCuda(y)) is None
