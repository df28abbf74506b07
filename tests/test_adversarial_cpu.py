"""CPU: the adversarial branch's Python layer against tests/golden/adversarial.npz -- the reference's own src/grl.py and
SongIdentityDiscriminator (src/model.py:545-587) run through src/train.py:182-202 by tests/golden/make_golden_adv.py.

The schedules and, with `backend="torch"` in float64, the prediction, the loss and every gradient equal the fixture's float64
values to 1e-12 (the same operations on the same numbers).  The HIP backend itself is tested in test_adversarial_gpu.py; here
only its refusal of a CPU tensor."""
import os

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (sys.path setup)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adversarial.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _discriminator(gold, dtype=torch.float32):
    from mst_amd.model import SongIdentityDiscriminator
    w0, w6 = gold["weight.network.0.weight"], gold["weight.network.6.weight"]
    d = SongIdentityDiscriminator(input_dim=w0.shape[1], hidden_dim=w0.shape[0], output_dim=w6.shape[0], dropout=0.3)
    d.load_state_dict({k: torch.from_numpy(gold[f"weight.{k}"]) for k in gold["state_dict_keys"]}, strict=True)
    return d.to(dtype)


def test_schedules_equal_the_reference_tables(gold):
    from mst_amd.grl import compute_adversarial_lambda, compute_grl_lambda
    total, warmup = (int(v) for v in gold["schedule.total_warmup"])
    steps = [int(s) for s in gold["schedule.steps"]]
    assert steps == [0, 1999, 2000, 2001, 6000, 10000, 12000]
    got = np.array([compute_grl_lambda(s, total, warmup) for s in steps], dtype=np.float64)
    assert np.abs(got - gold["schedule.grl"]).max() <= 1e-12
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.0 and 0.0 < got[3] < got[4] < got[5] == got[6]
    for key, lo, hi in (("schedule.adv_0_1", 0.0, 1.0), ("schedule.adv_02_05", 0.2, 0.5)):
        got = np.array([compute_adversarial_lambda(s, total, warmup, lo, hi) for s in steps], dtype=np.float64)
        assert np.abs(got - gold[key]).max() <= 1e-12, key
        assert got[0] == lo and abs(got[-1] - hi) <= 1e-12
    assert compute_grl_lambda(10, 100) == 0.0     # default warmup_steps = 2000


def test_gradient_reversal_is_identity_forward_and_scaled_negation_backward():
    from mst_amd.grl import GradientReversalFunction, GradientReversalLayer
    layer = GradientReversalLayer()
    assert layer.lambda_param == 1.0 and len(layer.state_dict()) == 0
    layer.set_lambda(0.37)
    x = torch.randn(5, 12, generator=torch.Generator().manual_seed(0), dtype=torch.float64, requires_grad=True)
    g = torch.randn(5, 12, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y = layer(x)
    assert torch.equal(y, x) and y.data_ptr() == x.data_ptr()     # a view, not a copy
    (y * g).sum().backward()
    assert torch.equal(x.grad, -0.37 * g)
    x.grad = None
    (GradientReversalFunction.apply(x, 0.0) * g).sum().backward()
    assert torch.equal(x.grad, torch.zeros_like(g))


def test_discriminator_state_dict_is_the_reference_layout(gold):
    from mst_amd.model import SongIdentityDiscriminator
    d = SongIdentityDiscriminator(input_dim=96, hidden_dim=80, output_dim=48, dropout=0.3)
    sd = d.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold["state_dict_keys"]]
    assert list(sd.keys()) == ["network.0.weight", "network.0.bias", "network.3.weight", "network.3.bias", "network.6.weight",
                               "network.6.bias"]
    for (k, v), shape in zip(sd.items(), gold["state_dict_shapes"]):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]], k
    _discriminator(gold)     # load_state_dict(strict=True) of the fixture's tensors
    dflt = SongIdentityDiscriminator()
    assert dflt.network[0].in_features == dflt.network[3].out_features == dflt.network[6].out_features == 512
    assert dflt.network[2].p == dflt.network[5].p == 0.3 and dflt.backend == "hip"


def test_torch_backend_in_float64_equals_the_reference(gold):
    """src/train.py:182-202 on this package's modules, float64, eval mode: the fixture's float64 values to 1e-12."""
    from mst_amd.grl import GradientReversalLayer
    from mst_amd.loss import cosine_distance_loss
    d = _discriminator(gold, torch.float64).eval()
    d.backend = "torch"
    layer = GradientReversalLayer(init_lambda=0.0)
    layer.set_lambda(float(gold["grl_lambda"]))
    e = torch.from_numpy(gold["embeddings"]).double().requires_grad_(True)
    target = torch.from_numpy(gold["targets"]).double()
    valid = e[torch.from_numpy(gold["valid_indices"]).long()]
    pred = d(layer(valid))
    loss = cosine_distance_loss(pred, target, backend="torch")
    loss.backward()
    assert (pred.detach().numpy() - gold["f64.pred"]).__abs__().max() <= 1e-12
    assert abs(loss.item() - float(gold["f64.loss"])) <= 1e-12
    assert np.abs(e.grad.numpy() - gold["f64.grad_embeddings"]).max() <= 1e-12
    skipped = sorted(set(range(e.shape[0])) - set(int(i) for i in gold["valid_indices"]))
    assert len(skipped) == 3 and not e.grad[skipped].any()     # rows without a song-id embedding get no gradient
    for k, q in d.named_parameters():
        assert np.abs(q.grad.numpy() - gold[f"f64.grad.{k}"]).max() <= 1e-12, k


def test_hip_backend_refuses_a_cpu_tensor(gold):
    from mst_amd.loss import cosine_distance_loss
    d = _discriminator(gold).eval()
    x = torch.from_numpy(gold["embeddings"])
    with pytest.raises(RuntimeError, match="CUDA"):
        d(x)
    with pytest.raises(RuntimeError, match="CUDA"):
        cosine_distance_loss(torch.zeros(3, 8), torch.ones(3, 8))
    d.backend = "torch"
    assert d(x).shape == (10, 48)
    d.backend = "eager"
    with pytest.raises(ValueError):
        d(x)
