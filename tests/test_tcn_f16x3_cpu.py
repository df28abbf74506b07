"""CPU: the Python and header side of the TCN mixer's opt-in split-precision mode (TCNMixer.precision = "f16x3",
mst_tcn_set_precision / mst_tcn_get_precision) -- declarations, bindings, the default, and the refusals.  The arithmetic
is tested on the GPU (tests/test_tcn_f16x3_gpu.py)."""
import ctypes as C
import os
import re

import pytest
import torch

import cases
import cases_tcn as ct
from mst_amd import _lib
from mst_amd import tcn_mixer as tm


def mixer(name="h8", backend="hip", precision=None):
    c = ct.CASES[name]
    tcn = tm.TCNMixer(**ct.mixer_kwargs(c))
    tcn.load_state_dict(ct.make_tcn_state_dict(c), strict=True)
    tcn.eval()
    tcn.backend = backend
    if precision is not None:
        tcn.precision = precision
    return tcn


def test_header_declares_the_mode():
    src = open(os.path.join(cases.ROOT, "include", "mst.h")).read()
    assert re.search(r"enum\s*\{\s*MST_TCN_FP32\s*=\s*0\s*,\s*MST_TCN_F16X3\s*=\s*1\s*\}", src)
    assert re.search(r"int\s+mst_tcn_set_precision\(mst_tcn\*\s*\w*,\s*int\s+\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+mst_tcn_get_precision\(const\s+mst_tcn\*\s*\w*\);", src)
    assert "IGNORE the mode" in src   # the training entry points compute in fp32


def test_lib_binds_the_two_functions():
    assert _lib.SYMBOLS["mst_tcn_set_precision"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])
    assert _lib.SYMBOLS["mst_tcn_get_precision"] == (C.c_int, [C.c_void_p])
    assert tm._PRECISIONS == {"fp32": 0, "f16x3": 1}


def test_precision_defaults_to_fp32():
    assert tm.TCNMixer().precision == "fp32"
    assert tm.create_tcn_mixer().precision == "fp32"


@pytest.mark.parametrize("backend", ["hip", "hip-train"])
def test_bad_value_raises_value_error(backend):
    tcn = mixer(backend=backend, precision="f16")
    with pytest.raises(ValueError, match="precision must be 'fp32'"), torch.no_grad():
        tcn(torch.zeros(1, 8, 64))


def test_hip_train_refuses_f16x3_and_names_the_reason():
    tcn = mixer(backend="hip-train", precision="f16x3")
    with pytest.raises(RuntimeError, match="inference only") as e, torch.no_grad():
        tcn(torch.zeros(1, 8, 64))
    assert "f16x3" in str(e.value) and "backend='torch'" in str(e.value)
    tcn.train()
    with pytest.raises(RuntimeError, match="inference only"):
        tcn(torch.zeros(2, 8, 64))


def test_cpu_tensor_with_f16x3_raises_and_names_the_reason():
    tcn = mixer(precision="f16x3")
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        tcn(torch.zeros(1, 8, 64))


def test_torch_backend_ignores_the_attribute():
    x = cases.pcm_batch(1, 300)
    with torch.no_grad():
        y0 = mixer(backend="torch")(x)
        assert torch.equal(mixer(backend="torch", precision="f16x3")(x), y0)
        assert torch.equal(mixer(backend="torch", precision="no such mode")(x), y0)
