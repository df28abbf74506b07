"""The optimiser step on the kernels of `csrc/optim.hip`: `Adam`, `AdamW`, `SGD` and `clip_grad_norm_`, the tail the
reference runs after every backward (clip + AdamW src/train_style_transfer.py:284-288, 602-605; AdamW under GradScaler
src/train.py:292-296; Adam / AdamW / SGD(momentum=0.9) in the per-pair fit, inference/test_tcn_style_transfer.py:130).

    from mst_amd.optim import AdamW, clip_grad_norm_          # instead of torch.optim / torch.nn.utils

The classes are `torch.optim.Optimizer` subclasses with the constructor arguments, defaults, param-group keys and per-parameter
state keys (`step`, `exp_avg`, `exp_avg_sq`; `momentum_buffer`) of their `torch.optim` namesakes: LR schedulers work unchanged,
a `state_dict()` of the torch class loads here and continues, and the other way round.  A step is two launches per param
group (one for SGD) whatever the number of tensors, `clip_grad_norm_` three; nothing reads a value back to the host.  `step`
is a 0-d fp32 tensor on the parameter's device (what torch keeps for `capturable` / `fused`).

The selectors `foreach`, `fused` and `capturable` are accepted and not read: there is one implementation.  What the kernels
cannot take -- CPU or non-fp32 tensors, sparse gradients, non-contiguous parameters, `amsgrad`, `maximize`, `differentiable`,
Nesterov, dampening != 0, a tensor `lr`, norms other than 2 -- raises RuntimeError naming the reason and the torch class or
function that does it; nothing falls back silently.

Under `torch.amp.GradScaler` the classes take `grad_scale` / `found_inf` as attributes (`_step_supports_amp_scaling`), on the
device: a step with a non-finite gradient changes nothing, with no host read.  The stored gradients stay scaled.

After a step every updated parameter's version counter is moved (`torch.autograd.graph.increment_version`): the kernels
write through `data_ptr()`, and `TCNMixer` / `HipEncoder` handle refresh, `TCNFiLMGenerator`'s live-parameter check and
autograd's saved-tensor check all read the counter.  (Under `found_inf` it moves although nothing changed: harmless.)
"""
import ctypes as C

import torch
from torch.optim.optimizer import Optimizer

from . import _lib

__all__ = ["Adam", "AdamW", "SGD", "clip_grad_norm_", "keep_best"]


def _refuse(who, why, alternative):
    raise RuntimeError(f"{who}: {why}; {alternative} does this on PyTorch ops (the HIP kernels have no silent library path)")


def _tensor_why(*named):
    """Why the kernels cannot take the (name, tensor) pairs (None = they can): layout first, then dtype, device, strides."""
    for name, t in named:
        if t.is_sparse or t.layout != torch.strided:
            return f"{name} is sparse ({t.layout})"
    for name, t in named:
        if t.dtype != torch.float32:
            return f"{name} is {t.dtype}: the kernels are fp32"
    for name, t in named:
        if not t.is_cuda:
            return f"{name} is on {t.device}: the kernels need CUDA tensors and there is no CPU fallback"
    for name, t in named:
        if not t.is_contiguous():
            return f"{name} is not contiguous (shape {tuple(t.shape)}, strides {t.stride()})"
    return None


def _ok(t):
    """The fast form of `_tensor_why(...) is None` for one tensor (the step's host time is these checks)."""
    return t.dtype is torch.float32 and t.is_cuda and t.layout is torch.strided and t.is_contiguous()


class _Table:
    """The device tables of one tensor list (include/mst.h mst_optim_list) and its workspace.  `key` = every pointer and size in it."""

    def __init__(self, key, rows, device):
        chunk = _lib.lib().mst_optim_chunk_elems()
        cmap = [(i, c) for i, row in enumerate(rows) for c in range((row[5] + chunk - 1) // chunk)]
        self.key, self.device = key, device
        self.tensors = torch.tensor(rows, dtype=torch.int64).to(device)
        self.chunk_map = torch.tensor(cmap, dtype=torch.int32).to(device)
        self.list = _lib.OptimList(self.tensors.data_ptr(), self.chunk_map.data_ptr(), len(rows), len(cmap))
        self.workspace = None

    def work(self, nbytes):
        if self.workspace is None or self.workspace.numel() < nbytes:
            self.workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
        return self.workspace


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class _HipOptimizer(Optimizer):
    _step_supports_amp_scaling = True   # GradScaler.step hands grad_scale / found_inf over as attributes, on the device
    _torch_name = "torch.optim"

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._tables = {}
        self.amp_steps = 0   # steps that took GradScaler's attribute path (read by the tests)
        for group in self.param_groups:
            self._check_group(group)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_tables", {})
        self.__dict__.setdefault("amp_steps", 0)

    def _refuse(self, why):
        _refuse(type(self).__name__, why, self._torch_name)

    def _check_common(self, group):
        if isinstance(group["lr"], torch.Tensor):
            self._refuse("a tensor lr would be read on the host every step; pass a float")
        if group.get("maximize"):
            self._refuse("maximize=True is not built")
        if group.get("differentiable"):
            self._refuse("differentiable=True is not built (the kernels are outside autograd)")

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        # torch.optim keeps `step` on the host unless capturable / fused; here it lives next to the parameter
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device).reshape(())
        self._tables = {}

    def _gather(self, group):
        """Parameters of the group that have a gradient, checked."""
        ps = [p for p in group["params"] if p.grad is not None and p.numel() > 0]
        dev = ps[0].device if ps else None
        for p in ps:
            g = p.grad
            if _ok(p) and _ok(g) and p.device == dev and g.device == dev:
                continue
            why = _tensor_why(("a parameter", p), ("a gradient", g))
            if why is None and g.device != p.device:
                why = f"a gradient is on {g.device} and its parameter on {p.device}"
            if why is None:
                why = f"one param group spans {dev} and {p.device}: the kernels take one device per group"
            self._refuse(why)
        return ps

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        if grad_scale is not None or found_inf is not None:
            self.amp_steps += 1
        L = _lib.lib()
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            ps = self._gather(group)
            if not ps:
                continue
            dev = ps[0].device
            for s in (grad_scale, found_inf):
                if s is not None and (s.device != dev or s.dtype != torch.float32 or s.numel() != 1):
                    self._refuse(f"grad_scale / found_inf must be one fp32 value on {dev}, got {s.dtype} {tuple(s.shape)} on {s.device}")
            rows = [self._row(p, group) for p in ps]
            key = tuple(rows)
            table = self._tables.get(gi)
            if table is None or table.key != key:   # rebuilt only when a pointer (or a size) in it has changed
                table = self._tables[gi] = _Table(key, rows, dev)
            hyper = self._hyper(group)
            with torch.cuda.device(dev):
                nws = L.mst_optim_step_workspace_bytes(len(rows))
                _lib.check(L.mst_optim_step(C.byref(table.list), C.byref(hyper), _lib.dptr(grad_scale), _lib.dptr(found_inf),
                                            _lib.dptr(table.work(nws)), nws, _lib.stream_ptr(dev)), "mst_optim_step")
            torch.autograd.graph.increment_version(ps)
        return loss


class Adam(_HipOptimizer):
    """torch.optim.Adam (L2 weight decay added to the gradient; `decoupled_weight_decay=True` is AdamW) on `mst_optim_step`."""
    _torch_name = "torch.optim.Adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if not isinstance(lr, torch.Tensor) and not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=decoupled_weight_decay))

    def _check_group(self, group):
        self._check_common(group)
        if group.get("amsgrad"):
            self._refuse("amsgrad=True is not built")
        if any(isinstance(b, torch.Tensor) for b in group["betas"]):
            self._refuse("tensor betas would be read on the host every step; pass floats")

    def _row(self, p, group):
        st = self.state[p]
        if "exp_avg" not in st:   # (torch's lazy state initialisation, `step` on the device)
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        m, v, t = st["exp_avg"], st["exp_avg_sq"], st["step"]
        if not (_ok(m) and _ok(v) and _ok(t) and m.shape == p.shape and v.shape == p.shape and t.numel() == 1
                and m.device == v.device == t.device == p.device):
            for k in ("exp_avg", "exp_avg_sq", "step"):
                why = _tensor_why((f"state['{k}']", st[k]))
                if why is None and st[k].device != p.device:
                    why = f"state['{k}'] is on {st[k].device}, its parameter on {p.device}"
                if why is None and st[k].shape != (p.shape if k != "step" else ()):
                    why = f"state['{k}'] has shape {tuple(st[k].shape)}, its parameter {tuple(p.shape)}"
                if why:
                    self._refuse(why)
        return (p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(), p.numel())

    def _hyper(self, group):
        return _lib.OptimHyper(algo=_lib.OPTIM_ADAMW if group.get("decoupled_weight_decay") else _lib.OPTIM_ADAM, lr=float(group["lr"]),
                               beta1=float(group["betas"][0]), beta2=float(group["betas"][1]), eps=float(group["eps"]),
                               weight_decay=float(group["weight_decay"]))


class AdamW(Adam):
    """torch.optim.AdamW (decoupled weight decay) on `mst_optim_step`."""
    _torch_name = "torch.optim.AdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)


class SGD(_HipOptimizer):
    """torch.optim.SGD with momentum (dampening 0, no Nesterov) on `mst_optim_step`.  A new momentum buffer starts at zero, which
    makes the first step's `momentum * buf + g` the copy of the gradient torch makes."""
    _torch_name = "torch.optim.SGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not isinstance(weight_decay, torch.Tensor) and weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused))

    def _check_group(self, group):
        self._check_common(group)
        if group.get("nesterov"):
            self._refuse("nesterov=True is not built")
        if group.get("dampening", 0) != 0:
            self._refuse(f"dampening={group['dampening']} is not built (0 only)")
        if isinstance(group["weight_decay"], torch.Tensor):
            self._refuse("a tensor weight_decay would be read on the host every step; pass a float")

    def _row(self, p, group):
        st = self.state[p]
        buf = None
        if group["momentum"] != 0:
            if st.get("momentum_buffer") is None:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            buf = st["momentum_buffer"]
            if not (_ok(buf) and buf.shape == p.shape and buf.device == p.device):
                why = _tensor_why(("state['momentum_buffer']", buf))
                if why is None and buf.device != p.device:
                    why = f"state['momentum_buffer'] is on {buf.device}, its parameter on {p.device}"
                self._refuse(why or f"state['momentum_buffer'] has shape {tuple(buf.shape)}, its parameter {tuple(p.shape)}")
        return (p.data_ptr(), p.grad.data_ptr(), _ptr(buf), 0, 0, p.numel())

    def _hyper(self, group):
        return _lib.OptimHyper(algo=_lib.OPTIM_SGD, lr=float(group["lr"]), weight_decay=float(group["weight_decay"]),
                               momentum=float(group["momentum"]))


_CLIP_TABLES = {}   # the last few gradient lists' tables, by their pointers and sizes
_CLIP_TABLES_MAX = 8


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ on `mst_optim_grad_norm` + `mst_optim_scale_grads`: the total L2 norm of the gradients as a
    0-d device tensor, the gradients scaled in place by min(1, max_norm / (norm + 1e-6)).  Three launches whatever the number of
    tensors, no host read; squares and sums in double in a fixed order, so the norm has the same bits from run to run."""
    who, alt = "clip_grad_norm_", "torch.nn.utils.clip_grad_norm_"
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if float(norm_type) != 2.0:
        _refuse(who, f"norm_type={norm_type} is not built (the L2 norm only)", alt)
    if error_if_nonfinite:
        _refuse(who, "error_if_nonfinite=True needs a host read of the norm", alt)
    if not grads:
        return torch.tensor(0.0)
    for g in grads:
        why = _tensor_why(("a gradient", g))
        if why is None and g.device != grads[0].device:
            why = f"the gradients span {grads[0].device} and {g.device}: the kernels take one device per call"
        if why:
            _refuse(who, why, alt)
    dev = grads[0].device
    live = [g for g in grads if g.numel() > 0]
    if not live:
        return torch.zeros((), dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)   # norm, coefficient: both written by the fold launch
    rows = [(0, g.data_ptr(), 0, 0, 0, g.numel()) for g in live]
    key = (dev,) + tuple(rows)
    table = _CLIP_TABLES.pop(key, None)
    if table is None:
        table = _Table(key, rows, dev)
        while len(_CLIP_TABLES) >= _CLIP_TABLES_MAX:
            _CLIP_TABLES.pop(next(iter(_CLIP_TABLES)))
    _CLIP_TABLES[key] = table   # (most recently used last)
    L = _lib.lib()
    with torch.cuda.device(dev):
        nws = L.mst_optim_grad_norm_workspace_bytes(table.list.n_chunks)
        st = _lib.stream_ptr(dev)
        _lib.check(L.mst_optim_grad_norm(C.byref(table.list), float(max_norm), out.data_ptr(), out.data_ptr() + 4,
                                         _lib.dptr(table.work(nws)), nws, st), "mst_optim_grad_norm")
        _lib.check(L.mst_optim_scale_grads(C.byref(table.list), out.data_ptr() + 4, st), "mst_optim_scale_grads")
    torch.autograd.graph.increment_version(live)
    clip_grad_norm_.last_coef = out[1]   # read by the tests
    return out[0]


def keep_best(loss, best, best_index, history, index, copies):
    """`mst_keep_best`: history[index] = loss; if loss < best (device scalars; strictly, a NaN never wins): best = loss,
    best_index = index and every (src, dst) pair of `copies` is copied -- without a host read.  fp32 CUDA tensors, contiguous."""
    dev = loss.device
    for name, t, dt in (("loss", loss, torch.float32), ("best", best, torch.float32), ("best_index", best_index, torch.int32)):
        if not t.is_cuda or t.dtype != dt or t.numel() != 1 or t.device != dev:
            raise RuntimeError(f"keep_best: {name} must be one {dt} value on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if history is not None and (history.device != dev or history.dtype != torch.float32 or not history.is_contiguous()
                                or not 0 <= index < history.numel()):
        raise RuntimeError(f"keep_best: history must be a contiguous fp32 tensor on {dev} with more than index = {index} elements")
    arr = (_lib.KeepCopy * max(len(copies), 1))()
    for k, (src, dst) in enumerate(copies):
        if src.device != dev or dst.device != dev or src.dtype != dst.dtype or src.shape != dst.shape or src.element_size() % 4 \
                or not src.is_contiguous() or not dst.is_contiguous():
            raise RuntimeError(f"keep_best: copy {k}: source and destination must be contiguous tensors of one shape and a 4-byte-multiple "
                               f"dtype on {dev}")
        arr[k] = _lib.KeepCopy(src.data_ptr(), dst.data_ptr(), src.numel() * src.element_size())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mst_keep_best(_lib.dptr(loss), _lib.dptr(best), _lib.dptr(best_index), _lib.dptr(history), int(index), arr,
                                            len(copies), _lib.stream_ptr(dev)), "mst_keep_best")
