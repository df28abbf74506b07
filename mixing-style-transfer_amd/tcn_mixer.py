"""Stage C: the TCN mixer that turns a pair of mixing-style embeddings into processed stems (the reference's
`src/tcn_mixer.py`, driven by `inference/inference_e2e_style_transfer.py:124-177`).

Same class names, constructor arguments, defaults and `state_dict` keys as the reference, so a reference checkpoint's
`tcn_state_dict` / `film_generator_state_dict` loads with `strict=True`.  Backends:

  * `backend = "hip"` (default): inference on the kernels of `csrc/tcn.hip` (exact fp32 MFMA).  Needs `eval()`, CUDA
    tensors, fp32 and no gradients; anything else RAISES and names the opt-in (no silent library path, no CPU fallback).
    `TCNMixer.precision = "f16x3"` (default "fp32") is the opt-in split-precision mode of this path: the dilated
    convolutions on the f16 MFMA with hi + lo operands (csrc/tcn_f16x3.inc), same parity bar, inference only.
  * `backend = "torch"`: the plain module tree on PyTorch (any device, any dtype, autograd).  It is the opt-in for
    training and the arithmetic the tests pin to the reference.
  * `backend = "hip-train"` (TCNMixer only): training on the kernels of `csrc/tcn_train.inc`.  In `train()` mode the
    forward uses batch statistics and updates the running ones, and with grad enabled it is an autograd function whose
    backward returns the gradients of x, of the FiLM tensors and of every parameter.  In `eval()` without gradients it
    is the inference path of "hip".  The device weights follow in-place parameter updates (an optimiser step) through a
    device kernel, without a host copy.  CUDA fp32 only; `eval()` with gradients raises and names `backend = "torch"`.
  * `train_backend = "hip"` (TCNFiLMGenerator only, next to `backend = "hip"`; default "none"): a call in `train()` mode
    or one that needs a gradient runs `mst_tcn_film_forward_train` / `mst_tcn_film_backward` (csrc/head.hip) as an autograd
    function on the module's live parameters: Dropout from seeds of torch's CPU generator, all six parameter gradients and,
    when the embedding requires one, its gradient.  `eval()` without gradients stays on the inference handle.

`TCNMixer.stream()` returns a `TCNStream`: block-wise inference of a causal mixer on audio as it arrives (`push`, `reset`,
`position`), on the kernels of `csrc/tcn_stream.inc` with `backend = "hip"` (bit-equal to the whole-clip forward whatever the
block sizes) or on history tensors with `backend = "torch"`.  `TCNMixer.lookahead_stream()` returns a `TCNLookaheadStream`: the
same for a NON-CAUSAL mixer with the fixed latency (K-1) * (2**num_blocks - 1) samples (`push`, `flush`, `reset`, `latency`), on the
kernels of `csrc/tcn_lookahead.inc`; `TCNMixer.forward_blockwise` runs a clip of any length through it (state independent of T).

`optimize_tcn_style_transfer` is the reference's per-pair fit (inference/test_tcn_style_transfer.py:84-201) on these backends and
`mst_amd.optim`, without a host synchronisation inside its loop.
"""
import ctypes as C
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._mlp import TCN_FILM, _HipMLP

STEM_ORDER = ("vocals", "bass", "drums", "other")
_BACKENDS = ("hip", "torch")
_MIXER_BACKENDS = _BACKENDS + ("hip-train",)
_PRECISIONS = {"fp32": 0, "f16x3": 1}   # MST_TCN_FP32, MST_TCN_F16X3


class CausalConv1d(nn.Module):
    """Conv1d that sees the past only: (K-1)*d zeros on the left of its input."""

    def __init__(self, in_channels, out_channels, kernel_size, dilation=1):
        super().__init__()
        self.padding = (kernel_size - 1) * dilation
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, padding=self.padding, dilation=dilation)

    def forward(self, x):
        y = self.conv(x)
        return y[:, :, :-self.padding] if self.padding > 0 else y


class NonCausalConv1d(nn.Module):
    """Conv1d with ((K-1)*d)//2 zeros on both sides; K must be odd for the length to be kept."""

    def __init__(self, in_channels, out_channels, kernel_size, dilation=1):
        super().__init__()
        self.padding = ((kernel_size - 1) * dilation) // 2
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, padding=self.padding, dilation=dilation)

    def forward(self, x):
        return self.conv(x)


def _check_kernel(kernel_size, causal):
    if not causal and kernel_size % 2 == 0:
        raise ValueError(f"a non-causal TCN block needs an odd kernel_size: symmetric padding of kernel_size={kernel_size} "
                         f"shortens the signal, so the residual sum cannot be formed (use causal=True for even kernels)")


class ResidualBlock(nn.Module):
    """conv-BN-LeakyReLU, conv-BN, residual sum, LeakyReLU (the activation is after the sum)."""

    def __init__(self, channels, kernel_size, dilation, causal=False):
        super().__init__()
        _check_kernel(kernel_size, causal)
        conv = CausalConv1d if causal else NonCausalConv1d
        self.conv1 = conv(channels, channels, kernel_size, dilation)
        self.conv2 = conv(channels, channels, kernel_size, dilation)
        self.norm1 = nn.BatchNorm1d(channels)
        self.norm2 = nn.BatchNorm1d(channels)

    def forward(self, x):
        g = F.leaky_relu(self.norm1(self.conv1(x)), negative_slope=0.2)
        g = self.norm2(self.conv2(g))
        return F.leaky_relu(g + x, negative_slope=0.2)


class FiLMResidualBlock(nn.Module):
    """conv-BN-FiLM-LeakyReLU twice, then the residual sum (no activation after it)."""

    def __init__(self, channels, kernel_size, dilation, causal=False):
        super().__init__()
        _check_kernel(kernel_size, causal)
        conv = CausalConv1d if causal else NonCausalConv1d
        self.conv1 = conv(channels, channels, kernel_size, dilation)
        self.conv2 = conv(channels, channels, kernel_size, dilation)
        self.norm1 = nn.BatchNorm1d(channels)
        self.norm2 = nn.BatchNorm1d(channels)
        self.channels = channels

    def forward(self, x, gamma1, beta1, gamma2, beta2):
        g = self.norm1(self.conv1(x))
        g = F.leaky_relu(gamma1.unsqueeze(-1) * g + beta1.unsqueeze(-1), negative_slope=0.2)
        g = self.norm2(self.conv2(g))
        g = F.leaky_relu(gamma2.unsqueeze(-1) * g + beta2.unsqueeze(-1), negative_slope=0.2)
        return g + x


def _state_key(module):
    """Identity of every parameter and buffer: changes on load_state_dict, .to(), in-place edits."""
    return tuple((k, v.data_ptr(), v._version, v.device, v.dtype) for k, v in module.state_dict(keep_vars=True).items())


def _host(t):
    return t.detach().to("cpu", torch.float32).contiguous()


def _hip_refusal(module, what, *tensors):
    """Why the kernels cannot take this call, or None."""
    if module.training:
        return f"{what}: the HIP backend is inference only and the module is in train() mode"
    if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors)
                                    or any(p.requires_grad for p in module.parameters())):
        return f"{what}: the HIP backend has no backward; call under torch.no_grad()"
    return _tensor_refusal(what, *tensors)


def _tensor_refusal(what, *tensors):
    """The device / dtype part of _hip_refusal."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            return f"{what}: the HIP backend needs CUDA tensors (there is no CPU fallback), got a {t.device} tensor"
        if t.dtype != torch.float32:
            return f"{what}: the HIP backend is fp32, got {t.dtype}"
    return None


def _raise_refusal(msg):
    raise RuntimeError(msg + "; backend='torch' runs the plain module tree on PyTorch (any device, dtype, autograd)")


class _Handle:
    """Owner of one C handle; destroyed with the object."""

    def __init__(self, ptr, destroy, key, device):
        self.ptr, self._destroy, self.key, self.device = ptr, destroy, key, device

    def __deepcopy__(self, memo):   # a copied or pickled module builds its own handle on first use
        return None

    def __reduce__(self):
        return (type(None), ())

    def __del__(self):
        try:
            if self.ptr:
                self._destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


class TCNFiLMGenerator(nn.Module):
    """MLP from the concatenated (input, target) embedding to gamma1, beta1, gamma2, beta2 of every TCN block."""

    def __init__(self, embed_dim=1536, num_blocks=14, hidden_channels=128):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_blocks = num_blocks
        self.hidden_channels = hidden_channels
        self.mlp = nn.Sequential(
            nn.Linear(embed_dim, 512), nn.LeakyReLU(0.2), nn.Dropout(0.1),
            nn.Linear(512, 512), nn.LeakyReLU(0.2), nn.Dropout(0.1),
            nn.Linear(512, num_blocks * 4 * hidden_channels))
        for layer in self.mlp:
            if isinstance(layer, nn.Linear):
                nn.init.normal_(layer.weight, mean=0.0, std=0.01)
                nn.init.zeros_(layer.bias)
        self.backend = "hip"
        # training with backend == "hip": "none" (default) = there is none (train() mode or a needed gradient raises and names
        # backend="torch"); "hip" = train-mode forward and full backward in libmst.so (_mlp._HipMLP) for a call in train() mode or
        # one that needs a gradient -- eval() without gradients stays on the inference handle
        self.train_backend = "none"
        self._hip = None

    def _train_params(self):
        """The parameters in the order of mst_tcn_film_weights / mst_tcn_film_grads."""
        return [self.mlp[0].weight, self.mlp[0].bias, self.mlp[3].weight, self.mlp[3].bias, self.mlp[6].weight, self.mlp[6].bias]

    def _film_tensor_train(self, emb):
        what = "TCNFiLMGenerator.forward (train_backend='hip')"
        slopes = {float(self.mlp[1].negative_slope), float(self.mlp[4].negative_slope)}
        if len(slopes) != 1:
            raise ValueError(f"{what}: one LeakyReLU slope for both layers is built, got {sorted(slopes)}; backend='torch' runs "
                             f"the plain module tree")
        params = self._train_params()
        msg = _tensor_refusal(what, emb, *params)
        if msg is None and any(p.device != emb.device for p in params):
            msg = f"{what}: the embedding is on {emb.device} and a parameter on {next(p.device for p in params if p.device != emb.device)}; the kernels need one device"
        if msg is None and not all(p.is_contiguous() for p in params):
            msg = f"{what}: the kernels read the live parameters by pointer and need them contiguous"
        if msg:
            _raise_refusal(msg)
        if emb.dim() != 2 or emb.shape[1] != self.mlp[0].in_features:
            raise ValueError(f"expected (B, {self.mlp[0].in_features}) embeddings, got {tuple(emb.shape)}")
        B = emb.shape[0]
        if self.mlp[6].out_features != self.num_blocks * 4 * self.hidden_channels:
            raise ValueError(f"{what}: mlp[6] has {self.mlp[6].out_features} outputs, expected num_blocks * 4 * hidden_channels")
        if B == 0:
            return torch.empty(0, self.num_blocks, 4, self.hidden_channels, device=emb.device, dtype=torch.float32)
        p1, p2 = (float(self.mlp[i].p) if self.training else 0.0 for i in (2, 5))
        return _HipMLP.apply(TCN_FILM, emb, (self.num_blocks, 4, self.hidden_channels), p1, p2, slopes.pop(), *params)

    def _handle(self, device):
        key = _state_key(self)
        if self._hip is None or self._hip.key != key or self._hip.device != device:
            keep = [_host(self.mlp[i].weight) for i in (0, 3, 6)] + [_host(self.mlp[i].bias) for i in (0, 3, 6)]
            w = _lib.TcnFilmWeights(*[C.c_void_p(t.data_ptr()) for t in (keep[0], keep[3], keep[1], keep[4], keep[2], keep[5])])
            ptr = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.lib().mst_tcn_film_create(C.byref(ptr), self.embed_dim, self.num_blocks, self.hidden_channels,
                                                          C.byref(w)), "mst_tcn_film_create")
            self._hip = _Handle(ptr, _lib.lib().mst_tcn_film_destroy, key, device)
        return self._hip

    def film_tensor(self, concat_embeddings):
        """(B, num_blocks, 4, hidden_channels): gamma1, beta1, gamma2, beta2 per block."""
        if self.backend not in _BACKENDS:
            raise ValueError("backend must be 'hip' (default) or 'torch'")
        if self.train_backend not in ("none", "hip"):
            raise ValueError("train_backend must be 'none' (default) or 'hip'")
        B = concat_embeddings.shape[0]
        if self.backend == "torch":
            return self.mlp(concat_embeddings).view(B, self.num_blocks, 4, self.hidden_channels)
        if self.train_backend == "hip" and (self.training or (torch.is_grad_enabled() and (
                concat_embeddings.requires_grad or any(p.requires_grad for p in self.parameters())))):
            return self._film_tensor_train(concat_embeddings)
        msg = _hip_refusal(self, "TCNFiLMGenerator.forward", concat_embeddings)
        if msg:
            _raise_refusal(msg)
        if concat_embeddings.dim() != 2 or concat_embeddings.shape[1] != self.embed_dim:
            raise ValueError(f"expected (B, {self.embed_dim}) embeddings, got {tuple(concat_embeddings.shape)}")
        emb = concat_embeddings.contiguous()
        dev = emb.device
        h = self._handle(dev)
        out = torch.empty(B, self.num_blocks, 4, self.hidden_channels, device=dev, dtype=torch.float32)
        if B == 0:
            return out
        with torch.cuda.device(dev):
            L = _lib.lib()
            nbytes = L.mst_tcn_film_workspace_bytes(h.ptr, B)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            _lib.check(L.mst_tcn_film_forward(h.ptr, _lib.dptr(emb), B, _lib.dptr(out), _lib.dptr(ws), nbytes,
                                              _lib.stream_ptr(dev)), "mst_tcn_film_forward")
        return out

    def forward(self, concat_embeddings):
        params = self.film_tensor(concat_embeddings)
        return [{"gamma1": params[:, i, 0, :], "beta1": params[:, i, 1, :], "gamma2": params[:, i, 2, :],
                 "beta2": params[:, i, 3, :]} for i in range(self.num_blocks)]


_FILM_KEYS = ("gamma1", "beta1", "gamma2", "beta2")


def _packed_film(film_params, B, nb, H):
    """The (B, nb, 4, H) tensor behind a list of dicts: the generator's own packing without a copy, else stacked."""
    first = film_params[0]["gamma1"]
    es, p0, store = first.element_size(), first.data_ptr(), first.untyped_storage().data_ptr()
    if all(t.data_ptr() == p0 + (i * 4 + q) * H * es and tuple(t.shape) == (B, H) and t.stride() == (nb * 4 * H, 1)
           and t.untyped_storage().data_ptr() == store and t.dtype == first.dtype
           for i in range(nb) for q, k in enumerate(_FILM_KEYS) for t in (film_params[i][k],)):
        return first.as_strided((B, nb, 4, H), (nb * 4 * H, 4 * H, H, 1))
    return torch.stack([torch.stack([film_params[i][k] for k in _FILM_KEYS], 1) for i in range(nb)], 1).contiguous()


def _film_base(film_params, B, nb, H):
    """The (B, nb, 4, H) tensor the dicts are the plain slices of, as AUTOGRAD knows it (the views' common `_base`, e.g. the
    generator's output): its gradient is the slices' gradients side by side, so it can stand for them without a copy.  None
    when the dicts are anything else.  With the base as the function's input the slices are no longer nodes of the graph, so
    the stack is kept wherever that could be seen: a slice that is not connected to the base as the base's `requires_grad`
    says it should be (taken under `torch.no_grad()`, it has no `grad_fn` and the stack sends no gradient into the base), a
    slice with `retain_grad()` or a tensor hook on it."""
    base = getattr(film_params[0]["gamma1"], "_base", None)   # (a private attribute: without it, the stack)
    if base is None or base.numel() != B * nb * 4 * H or not base.is_contiguous() or base.dtype != torch.float32:
        return None
    es, p0 = base.element_size(), base.data_ptr()
    if all(t._base is base and t.data_ptr() == p0 + (i * 4 + q) * H * es and tuple(t.shape) == (B, H) and t.stride() == (nb * 4 * H, 1)
           and t.requires_grad == base.requires_grad and (t.grad_fn is not None) == base.requires_grad
           and not t.retains_grad and not t._backward_hooks
           for i in range(nb) for q, k in enumerate(_FILM_KEYS) for t in (film_params[i][k],)):
        return base.view(B, nb, 4, H)
    return None


class TCNMixer(nn.Module):
    """8-channel stems -> 1x1 conv -> num_blocks dilated residual blocks (dilation 2^i) -> 1x1 conv -> + input."""

    MAX_HIDDEN, MAX_KERNEL, MAX_BLOCKS = 128, 15, 16

    def __init__(self, in_channels=8, hidden_channels=128, num_blocks=14, kernel_size=15, causal=False, use_film=False):
        super().__init__()
        self.in_channels = in_channels
        self.hidden_channels = hidden_channels
        self.use_film = use_film
        self.num_blocks = num_blocks
        self.kernel_size = kernel_size
        self.causal = causal
        self.input_conv = nn.Conv1d(in_channels, hidden_channels, kernel_size=1)
        block = FiLMResidualBlock if use_film else ResidualBlock
        self.blocks = nn.ModuleList([block(hidden_channels, kernel_size, 2 ** i, causal=causal) for i in range(num_blocks)])
        self.output_conv = nn.Conv1d(hidden_channels, in_channels, kernel_size=1)
        nn.init.normal_(self.output_conv.weight, mean=0.0, std=0.001)
        nn.init.zeros_(self.output_conv.bias)
        self.receptive_field = 1 + sum(2 ** i * (kernel_size - 1) for i in range(num_blocks))
        self.backend = "hip"
        # backend == "hip" only: "fp32" (default) = the exact-fp32 MFMA kernels; "f16x3" = split-precision inference on the
        # f16 MFMA (mst_tcn_set_precision).  "hip-train" refuses "f16x3"; "torch" does not read it
        self.precision = "fp32"
        self._hip = None

    # ---- torch tree ------------------------------------------------------------------------------------------------
    def _forward_torch(self, x, film_params, taps=None):
        h = self.input_conv(x)
        for i, blk in enumerate(self.blocks):
            if self.use_film:
                p = film_params[i]
                h = blk(h, p["gamma1"], p["beta1"], p["gamma2"], p["beta2"])
            else:
                h = blk(h)
            if taps is not None and i in taps:
                taps[i] = h
        return self.output_conv(h) + x

    # ---- HIP -------------------------------------------------------------------------------------------------------
    def _handle(self, device):
        key = _state_key(self)
        if self._hip is None or self._hip.key != key or self._hip.device != device:
            eps = {float(b.norm1.eps) for b in self.blocks} | {float(b.norm2.eps) for b in self.blocks}
            if len(eps) != 1:
                raise ValueError(f"TCNMixer: the HIP backend needs one BatchNorm eps for all blocks, got {sorted(eps)}")
            cfg = _lib.TcnConfig(self.in_channels, self.hidden_channels, self.num_blocks, self.kernel_size, int(self.causal),
                                 int(self.use_film), eps.pop())
            st = lambda f: _host(torch.stack([torch.stack([f(b, 1), f(b, 2)]) for b in self.blocks]))  # noqa: E731
            keep = [_host(self.input_conv.weight), _host(self.input_conv.bias),
                    st(lambda b, l: getattr(b, f"conv{l}").conv.weight), st(lambda b, l: getattr(b, f"conv{l}").conv.bias),
                    st(lambda b, l: getattr(b, f"norm{l}").weight), st(lambda b, l: getattr(b, f"norm{l}").bias),
                    st(lambda b, l: getattr(b, f"norm{l}").running_mean), st(lambda b, l: getattr(b, f"norm{l}").running_var),
                    _host(self.output_conv.weight), _host(self.output_conv.bias)]
            w = _lib.TcnWeights(*[C.c_void_p(t.data_ptr()) for t in keep])
            ptr = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.lib().mst_tcn_create(C.byref(ptr), C.byref(cfg), C.byref(w)), "mst_tcn_create")
            self._hip = _Handle(ptr, _lib.lib().mst_tcn_destroy, key, device)
        return self._hip

    def _forward_hip(self, x, film, tap_blocks=(), handle=None):
        """x (B, 8, T) cuda fp32, film (B, nb, 4, H) or None -> y, [hidden state after each block of tap_blocks]."""
        dev = x.device
        h = handle or self._handle(dev)
        x = x.contiguous()
        B, _, T = x.shape
        H = self.hidden_channels
        y = torch.empty_like(x)
        taps_out = [torch.empty(B, H, T, device=dev, dtype=torch.float32) for _ in tap_blocks]
        if B == 0 or T == 0:
            return y, taps_out
        L = _lib.lib()
        with torch.cuda.device(dev):
            if getattr(h, "precision", "fp32") != self.precision:   # on first use and on change; a new handle starts in fp32
                _lib.check(L.mst_tcn_set_precision(h.ptr, _PRECISIONS[self.precision], _lib.stream_ptr(dev)), "mst_tcn_set_precision")
                h.precision = self.precision
            per_clip = L.mst_tcn_workspace_bytes(h.ptr, 1, T)
            if per_clip == 0:
                _lib.check(-1, "mst_tcn_workspace_bytes")
            # split over B so that the workspace stays below ~2 GiB and no call is refused for its batch size
            step = max(1, min(B, 65535, (2 << 30) // per_clip))
            nbytes = L.mst_tcn_workspace_bytes(h.ptr, step, T)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            for b0 in range(0, B, step):
                nbat = min(step, B - b0)
                taps = None
                if tap_blocks:
                    taps = _lib.TcnTaps()
                    taps.n = len(tap_blocks)
                    for i, k in enumerate(tap_blocks):
                        taps.block[i] = int(k)
                        taps.h[i] = taps_out[i][b0:b0 + nbat].data_ptr()
                _lib.check(L.mst_tcn_forward(h.ptr, _lib.dptr(x[b0:b0 + nbat]), _lib.dptr(None if film is None else film[b0:b0 + nbat]),
                                             nbat, T, _lib.dptr(y[b0:b0 + nbat]), None if taps is None else C.byref(taps),
                                             _lib.dptr(ws), nbytes, _lib.stream_ptr(dev)), "mst_tcn_forward")
        return y, taps_out

    # ---- HIP, training ---------------------------------------------------------------------------------------------
    def _norms(self):
        return [getattr(b, f"norm{l}") for b in self.blocks for l in (1, 2)]

    def _train_params(self):
        """Every parameter in the order _TCNTrainFn.backward returns gradients."""
        ps = [self.input_conv.weight, self.input_conv.bias]
        for b in self.blocks:
            ps += [b.conv1.conv.weight, b.conv1.conv.bias, b.conv2.conv.weight, b.conv2.conv.bias,
                   b.norm1.weight, b.norm1.bias, b.norm2.weight, b.norm2.bias]
        return ps + [self.output_conv.weight, self.output_conv.bias]

    def _handle_train(self, device, running_stats=False):
        """The handle with its device weights current: built once from host copies, then refreshed on the device when a
        parameter's version moved (mst_tcn_update_params: no host copy, no synchronisation).  The running statistics, which
        every train-mode forward moves and only the inference path reads, are refreshed only with `running_stats`."""
        state = self.state_dict(keep_vars=True)
        msg = _tensor_refusal("TCNMixer (backend='hip-train')", *[v for v in state.values() if v.is_floating_point()])
        if msg:
            _raise_refusal(msg)
        key = ("hip-train",) + tuple((k, v.data_ptr(), v.device, v.dtype) for k, v in state.items())
        if self._hip is None or self._hip.key != key or self._hip.device != device:
            self._hip = None
            h = self._handle(device)
            h.key, h.param_versions, h.stat_versions = key, None, None
        h = self._hip
        norms = self._norms()
        params = self._train_params()
        pv = tuple(p._version for p in params)
        sv = tuple(b._version for n in norms for b in (n.running_mean, n.running_var)) if running_stats else h.stat_versions
        if h.param_versions == pv and h.stat_versions == sv:
            return h
        w = _lib.TcnWeights()
        keep = []

        def put(field, t):
            t = t.detach().contiguous()
            keep.append(t)
            setattr(w, field, t.data_ptr())

        cat = lambda f: torch.stack([f(b, l) for b in self.blocks for l in (1, 2)])  # noqa: E731
        if h.param_versions != pv:
            put("input_w", self.input_conv.weight), put("input_b", self.input_conv.bias)
            put("conv_w", cat(lambda b, l: getattr(b, f"conv{l}").conv.weight.detach()))
            put("conv_b", cat(lambda b, l: getattr(b, f"conv{l}").conv.bias.detach()))
            put("bn_w", cat(lambda b, l: getattr(b, f"norm{l}").weight.detach()))
            put("bn_b", cat(lambda b, l: getattr(b, f"norm{l}").bias.detach()))
            put("output_w", self.output_conv.weight), put("output_b", self.output_conv.bias)
        if h.stat_versions != sv:
            put("bn_mean", torch.stack([n.running_mean for n in norms])), put("bn_var", torch.stack([n.running_var for n in norms]))
        with torch.cuda.device(device):
            _lib.check(_lib.lib().mst_tcn_update_params(h.ptr, C.byref(w), _lib.stream_ptr(device)), "mst_tcn_update_params")
        h.param_versions, h.stat_versions = pv, sv
        return h

    def _train_forward(self, x, film, want_save):
        """Train-mode forward of the whole batch in one call (batch statistics).  Returns y, save (or None), handle;
        `_last_batch_stats` keeps the batch mean and biased variance, (nb, 2, H) each."""
        dev = x.device
        h = self._handle_train(dev)
        B, _, T = x.shape
        if B * T < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        nb, H = self.num_blocks, self.hidden_channels
        y = torch.empty_like(x)
        mean = torch.empty(nb * 2, H, device=dev, dtype=torch.float32)
        var = torch.empty_like(mean)
        L = _lib.lib()
        with torch.cuda.device(dev):
            nws = L.mst_tcn_train_workspace_bytes(h.ptr, B, T)
            nsave = L.mst_tcn_train_save_bytes(h.ptr, B, T) if want_save else 0
            if nws == 0 or (want_save and nsave == 0):
                _lib.check(-1, "mst_tcn_train_workspace_bytes")
            ws = torch.empty(nws, device=dev, dtype=torch.uint8)
            save = torch.empty(nsave, device=dev, dtype=torch.uint8) if want_save else None
            _lib.check(L.mst_tcn_forward_train(h.ptr, _lib.dptr(x), _lib.dptr(film), B, T, _lib.dptr(y), _lib.dptr(mean), _lib.dptr(var),
                                               _lib.dptr(save), nsave, _lib.dptr(ws), nws, _lib.stream_ptr(dev)), "mst_tcn_forward_train")
        # running statistics as nn.BatchNorm1d keeps them: (1 - m) * running + m * batch, unbiased variance
        with torch.no_grad():
            norms = self._norms()
            unbiased = var * (B * T / (B * T - 1))
            for m in sorted({float(n.momentum) for n in norms}):
                idx = [i for i, n in enumerate(norms) if float(n.momentum) == m]
                for bufs, stat in (([norms[i].running_mean for i in idx], mean), ([norms[i].running_var for i in idx], unbiased)):
                    torch._foreach_mul_(bufs, 1.0 - m)
                    torch._foreach_add_(bufs, [stat[i] for i in idx], alpha=m)
            torch._foreach_add_([n.num_batches_tracked for n in norms], 1)
        self._last_batch_stats = (mean.view(nb, 2, H), var.view(nb, 2, H))   # read by the tests
        return y, save, h

    def _forward_hip_train(self, x, film_params, fl):
        what = "TCNMixer.forward (backend='hip-train')"
        if self.training:
            for n in self._norms():
                if n.momentum is None:
                    raise ValueError(f"{what}: BatchNorm1d momentum=None (cumulative average) is not supported; "
                                     f"backend='torch' runs it")
                if not n.track_running_stats or n.running_mean is None:
                    raise ValueError(f"{what}: BatchNorm1d track_running_stats=False is not supported; backend='torch' runs it")
        msg = _tensor_refusal(what, x, *fl)
        if msg:
            _raise_refusal(msg)
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"expected (B, {self.in_channels}, T) stems, got {tuple(x.shape)}")
        B, nb, H = x.shape[0], self.num_blocks, self.hidden_channels
        grad = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in fl)
                                            or any(p.requires_grad for p in self.parameters()))
        if not self.training:
            if grad:
                _raise_refusal(f"{what}: gradients in eval() mode (frozen BatchNorm statistics) are not built")
            film = _packed_film(film_params, B, nb, H) if self.use_film else None
            return self._forward_hip(x, film, handle=self._handle_train(x.device, running_stats=True))[0]
        if x.numel() == 0:
            raise ValueError(f"{what}: empty input {tuple(x.shape)}")
        film = None
        if self.use_film:
            film = _film_base(film_params, B, nb, H)
        if self.use_film and film is None:   # stacked with ops autograd follows (not the as_strided view of _packed_film)
            film = torch.stack([torch.stack([film_params[i][k] for k in _FILM_KEYS], 1) for i in range(nb)], 1)
            if tuple(film.shape) != (B, nb, 4, H):
                raise ValueError(f"expected FiLM tensors of shape ({B}, {H}), got a stack of {tuple(film.shape)}")
            film = film.contiguous()
        if not grad:
            return self._train_forward(x.contiguous(), film, want_save=False)[0]
        return _TCNTrainFn.apply(self, x, film, *self._train_params())

    def forward(self, x, film_params=None):
        if self.use_film:
            if film_params is None:
                raise ValueError("film_params must be provided when use_film=True")
            if len(film_params) != self.num_blocks:
                raise ValueError(f"Expected {self.num_blocks} FiLM parameter dicts, got {len(film_params)}")
        if self.backend not in _MIXER_BACKENDS:
            raise ValueError("backend must be 'hip' (default), 'torch' or 'hip-train'")
        if self.backend == "torch":
            return self._forward_torch(x, film_params)
        if self.precision not in _PRECISIONS:
            raise ValueError(f"precision must be 'fp32' (default) or 'f16x3', got {self.precision!r}")
        fl = [p[k] for p in film_params for k in _FILM_KEYS] if self.use_film else []
        if self.backend == "hip-train":
            if self.precision != "fp32":
                _raise_refusal(f"TCNMixer.forward (backend='hip-train'): precision={self.precision!r} is inference only (the "
                               f"training kernels compute in fp32); set precision='fp32', or backend='hip' for f16x3 inference")
            return self._forward_hip_train(x, film_params, fl)
        msg = _hip_refusal(self, "TCNMixer.forward", x, *fl)
        if msg:
            _raise_refusal(msg)
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"expected (B, {self.in_channels}, T) stems, got {tuple(x.shape)}")
        film = _packed_film(film_params, x.shape[0], self.num_blocks, self.hidden_channels) if self.use_film else None
        return self._forward_hip(x, film)[0]

    def stream(self, batch_size=1, max_block=4096, film_params=None):
        """A `TCNStream`: block-wise inference of this (causal) mixer on audio as it arrives.  `film_params` as `forward`
        takes them, fixed until the next `reset`."""
        return TCNStream(self, batch_size, max_block, film_params)

    def lookahead_stream(self, batch_size=1, max_block=4096, film_params=None):
        """A `TCNLookaheadStream`: block-wise inference of this mixer, non-causal included, with the fixed latency
        (K-1) * (2**num_blocks - 1) samples (0 for a causal mixer) and a `flush()` at the clip's end."""
        return TCNLookaheadStream(self, batch_size, max_block, film_params)

    def forward_blockwise(self, x, film_params=None, block=65536):
        """`forward(x, film_params)` of a clip (B, 8, T) of any length, computed in blocks of `block` samples through the
        lookahead stream (`stream()` for a causal mixer): the state does not grow with T and T has no 2^31 limit.  On
        `backend="hip"` the bits of `forward`."""
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"expected (B, {self.in_channels}, T) stems, got {tuple(x.shape)}")
        if int(block) < 1:
            raise ValueError(f"TCNMixer.forward_blockwise: block must be positive, got {block}")
        B, _, T = x.shape
        y = torch.empty_like(x)
        if B == 0 or T == 0:
            return y
        block = min(int(block), T)
        if self.causal:
            s = self.stream(batch_size=B, max_block=block, film_params=film_params)
            for t in range(0, T, block):
                y[:, :, t:t + block] = s.push(x[:, :, t:t + block])
            return y
        s = self.lookahead_stream(batch_size=B, max_block=block, film_params=film_params)
        at = -s.latency   # time of the next output sample

        def put(piece, at):
            n = piece.shape[2]
            lo, hi = max(at, 0), min(at + n, T)
            if hi > lo:
                y[:, :, lo:hi] = piece[:, :, lo - at:hi - at]
            return at + n

        for t in range(0, T, block):
            at = put(s.push(x[:, :, t:t + block]), at)
        for piece in s._drain():
            at = put(piece, at)
        return y

    def process_stems_dict(self, stems_dict, film_params=None):
        stacked = torch.cat([stems_dict[s] for s in STEM_ORDER], dim=0).unsqueeze(0)
        out = self.forward(stacked, film_params=film_params).squeeze(0)
        return {s: out[2 * i:2 * i + 2, :] for i, s in enumerate(STEM_ORDER)}


class TCNStream:
    """Block-wise inference of a causal `TCNMixer` on audio as it arrives (`TCNMixer.stream`).

    `push(x)` takes the next N samples, (B, 8, N) with 1 <= N <= max_block, and returns their N output samples.  Every
    dilated convolution keeps the last (K-1)*d samples of its own input, zeros at the start, so the pushes concatenated are
    the whole-clip `mixer(x, film_params)` whatever the block sizes: bit for bit on `backend="hip"` (the kernels of
    csrc/tcn_stream.inc run the offline kernels' arithmetic on ring buffers), to rounding on `backend="torch"` (torch
    picks its summation order by length).  FiLM is fixed per `reset`.  The stream binds the mixer's parameters and buffers
    as they are at `stream()` / `reset()`: a push after any of them changed raises and names `reset()`.

    `backend="hip"` needs eval(), causal=True, precision="fp32", CUDA fp32 input and no gradients, makes no host
    synchronisation and allocates its state once (`state_bytes`); `backend="torch"` is the plain restatement (history
    tensors concatenated in front of the block; any device and dtype, eval() only, no gradients) and the explicit opt-in for
    everything else.  A non-causal mixer and `backend="hip-train"` raise.  `position`: samples pushed since position 0."""

    def __init__(self, mixer, batch_size=1, max_block=4096, film_params=None):
        if int(batch_size) < 1 or int(max_block) < 1:
            raise ValueError(f"TCNMixer.stream: batch_size and max_block must be positive, got {batch_size}, {max_block}")
        self.mixer, self.batch_size, self.max_block = mixer, int(batch_size), int(max_block)
        self.position = 0
        self._film_params = self._state = self._work = None
        self.reset(film_params)

    # ---- what both backends refuse -----------------------------------------------------------------------------------
    _name, _needs_causal = "TCNStream", True    # (TCNLookaheadStream overrides both)

    def _check_mixer(self, what):
        m = self.mixer
        if m.backend not in _MIXER_BACKENDS:
            raise ValueError("backend must be 'hip' (default), 'torch' or 'hip-train'")
        if self._needs_causal and not m.causal:
            raise RuntimeError(f"{what}: streaming needs a causal mixer (causal=True); a non-causal one looks ahead ((K-1)*d)//2 "
                               f"samples per layer, which a block-wise call does not have: evaluate whole clips with TCNMixer.forward, "
                               f"or stream with a fixed latency through TCNMixer.lookahead_stream")
        if m.backend == "hip-train":
            raise RuntimeError(f"{what}: backend='hip-train' is the training path and streaming is inference only; set "
                               f"backend='hip' (or 'torch')")
        if m.training:
            msg = f"{what}: streaming is inference only and the module is in train() mode (batch statistics depend on the block); call eval()"
            if m.backend == "hip":
                _raise_refusal(msg)
            raise RuntimeError(msg)
        if m.backend == "hip":
            if m.precision not in _PRECISIONS:
                raise ValueError(f"precision must be 'fp32' (default) or 'f16x3', got {m.precision!r}")
            if m.precision != "fp32":
                _raise_refusal(f"{what}: precision={m.precision!r} cannot stream (its per-clip range scale is a function of the "
                               f"whole clip); set precision='fp32'")

    @property
    def state_bytes(self):
        """Device bytes of the HIP state (0 on backend='torch' before the first push allocates its history tensors)."""
        return 0 if self._state is None else self._state.numel()

    def reset(self, film_params=None, position=0):
        """Zero history; new FiLM parameters if given (else those of the last reset); `position` = sample index of the next
        push.  Binds the mixer's current parameters and buffers."""
        m = self.mixer
        self._check_mixer(f"{self._name}.reset")
        if int(position) < 0:
            raise ValueError(f"{self._name}.reset: position must not be negative, got {position}")
        film_params = self._film_params if film_params is None else film_params
        if m.use_film:
            if film_params is None:
                raise ValueError("film_params must be provided when use_film=True")
            if len(film_params) != m.num_blocks:
                raise ValueError(f"Expected {m.num_blocks} FiLM parameter dicts, got {len(film_params)}")
        elif film_params is not None:
            raise ValueError("film_params given for a mixer with use_film=False")
        self._backend = m.backend
        self._hist = None
        if m.backend == "hip":
            self._reset_hip(film_params)
        self._film_params = film_params
        self._key = _state_key(m)
        self.position = int(position)

    def _reset_hip(self, film_params):
        h, film, dev = self._reset_hip_args(film_params)
        B, L = self.batch_size, _lib.lib()
        with torch.cuda.device(dev):
            nstate = L.mst_tcn_stream_state_bytes(h.ptr, B, self.max_block)
            nwork = L.mst_tcn_stream_workspace_bytes(h.ptr, B, self.max_block)
            if nstate == 0 or nwork == 0:
                _lib.check(-1, "mst_tcn_stream_state_bytes")
            if self._state is None or self._state.numel() != nstate or self._state.device != dev:
                self._state = self._work = None
                self._state = torch.empty(nstate, device=dev, dtype=torch.uint8)
                self._work = torch.empty(nwork, device=dev, dtype=torch.uint8)
            _lib.check(L.mst_tcn_stream_reset(h.ptr, _lib.dptr(self._state), nstate, B, self.max_block, _lib.dptr(film),
                                              _lib.stream_ptr(dev)), "mst_tcn_stream_reset")
        self._handle = h   # (keeps the C handle alive while the stream uses it)

    def _reset_hip_args(self, film_params):
        """The handle in fp32 mode, the packed FiLM tensor (or None) and the device of a reset on the kernels."""
        m, B = self.mixer, self.batch_size
        what = f"{self._name}.reset"
        fl = [p[k] for p in film_params for k in _FILM_KEYS] if m.use_film else []
        dev = m.input_conv.weight.device
        msg = _tensor_refusal(what, m.input_conv.weight, *fl)
        if msg is None and any(t.device != dev for t in fl):
            msg = f"{what}: the mixer is on {dev} and a FiLM tensor on another device; the kernels need one device"
        if msg:
            _raise_refusal(msg)
        h = m._handle(dev)
        film = _packed_film(film_params, B, m.num_blocks, m.hidden_channels) if m.use_film else None
        if film is not None and tuple(film.shape) != (B, m.num_blocks, 4, m.hidden_channels):
            raise ValueError(f"expected FiLM tensors of shape ({B}, {m.hidden_channels}), got a stack of {tuple(film.shape)}")
        with torch.cuda.device(dev):
            if getattr(h, "precision", "fp32") != "fp32":
                _lib.check(_lib.lib().mst_tcn_set_precision(h.ptr, _PRECISIONS["fp32"], _lib.stream_ptr(dev)), "mst_tcn_set_precision")
                h.precision = "fp32"
        return h, film, dev

    def _check_bound(self, what):
        """The mixer is still one the stream can run, and the one it was bound to."""
        m = self.mixer
        self._check_mixer(what)
        if m.backend != self._backend or _state_key(m) != self._key:
            raise RuntimeError(f"{what}: the mixer's backend, parameters or buffers changed since the stream was bound "
                               "(load_state_dict, .to(), an in-place edit, an optimiser step); the carried history and the folded "
                               "BatchNorm / FiLM table belong to the old ones: call reset()")

    def push(self, x):
        """x (B, 8, N), 1 <= N <= max_block -> (B, 8, N), the next N output samples."""
        m = self.mixer
        self._check_bound(f"{self._name}.push")
        if x.dim() != 3 or x.shape[1] != m.in_channels:
            raise ValueError(f"expected (B, {m.in_channels}, N) stems, got {tuple(x.shape)}")
        B, _, N = x.shape
        if B != self.batch_size:
            raise ValueError(f"{self._name}.push: the stream was made for batch_size={self.batch_size}, got a batch of {B}")
        if N < 1 or N > self.max_block:
            raise ValueError(f"{self._name}.push: a block holds 1..max_block={self.max_block} samples, got {N}")
        y = self._push_hip(x) if m.backend == "hip" else self._push_torch(x)
        self.position += N
        return y

    def _hip_input(self, x):
        """x as the kernels take it, or the refusal."""
        msg = _hip_refusal(self.mixer, f"{self._name}.push", x)
        if msg is None and x.device != self._state.device:
            msg = f"{self._name}.push: the stream's state is on {self._state.device} and x on {x.device}"
        if msg:
            _raise_refusal(msg)
        return x.contiguous()

    def _push_hip(self, x):
        x = self._hip_input(x)
        y = torch.empty_like(x)
        dev, L = x.device, _lib.lib()
        with torch.cuda.device(dev):
            _lib.check(L.mst_tcn_stream_push(self._handle.ptr, _lib.dptr(self._state), self._state.numel(), self.batch_size,
                                             self.max_block, self.position, _lib.dptr(x), x.shape[2], _lib.dptr(y),
                                             _lib.dptr(self._work), self._work.numel(), _lib.stream_ptr(dev)), "mst_tcn_stream_push")
        return y

    def _push_torch(self, x):
        m, film = self.mixer, self._film_params
        N = x.shape[2]
        with torch.no_grad():
            if self._hist is None:
                self._hist = [x.new_zeros(x.shape[0], m.hidden_channels, (m.kernel_size - 1) * 2 ** (i // 2))
                              for i in range(2 * m.num_blocks)]

            def conv(c, h, i):   # the causal convolution on (its history, the block); keeps the last (K-1)*d input samples
                z = torch.cat([self._hist[i], h], dim=2)
                self._hist[i] = z[:, :, N:]
                return F.conv1d(z, c.conv.weight, c.conv.bias, dilation=c.conv.dilation)

            h = m.input_conv(x)
            for i, blk in enumerate(m.blocks):
                g = blk.norm1(conv(blk.conv1, h, 2 * i))
                if m.use_film:
                    p = film[i]
                    g = F.leaky_relu(p["gamma1"].unsqueeze(-1) * g + p["beta1"].unsqueeze(-1), negative_slope=0.2)
                    g = blk.norm2(conv(blk.conv2, g, 2 * i + 1))
                    h = F.leaky_relu(p["gamma2"].unsqueeze(-1) * g + p["beta2"].unsqueeze(-1), negative_slope=0.2) + h
                else:
                    g = blk.norm2(conv(blk.conv2, F.leaky_relu(g, negative_slope=0.2), 2 * i + 1))
                    h = F.leaky_relu(g + h, negative_slope=0.2)
            return m.output_conv(h) + x


class TCNLookaheadStream(TCNStream):
    """Block-wise inference of a non-causal `TCNMixer` with a fixed latency (`TCNMixer.lookahead_stream`).

    Every layer runs ((K-1)*d)//2 samples behind its input, so `push(x)`, (B, 8, N) with 1 <= N <= max_block, returns the N
    output samples that lie `latency = (K-1) * (2**num_blocks - 1)` samples back (zeros before the clip's start), and
    `flush()` ends the clip and returns the last `latency` samples:

        torch.cat(pushes + [flush], 2)[:, :, latency:]  is  mixer(x, film_params)

    for a clip of any length T >= 1, shorter than the latency included: bit for bit on `backend="hip"` (csrc/tcn_lookahead.inc),
    to rounding on `backend="torch"`.  Rows of every layer outside the clip are zeros of that layer's own input, as the
    whole-clip forward pads them.  After `flush()` the stream is closed until `reset()`.  A causal mixer has latency 0 and an
    empty flush.  Backend rules, FiLM and the binding of the mixer's parameters are those of `TCNStream`; the state does not
    depend on the clip's length.  `position`: samples pushed since position 0."""

    _name, _needs_causal = "TCNLookaheadStream", False

    @property
    def latency(self):
        m = self.mixer
        return 0 if m.causal else (m.kernel_size - 1) * (2 ** m.num_blocks - 1)

    def reset(self, film_params=None, position=0):
        """Zero history and an open stream; new FiLM parameters if given (else those of the last reset); `position` = sample
        index of the next push (a label: the clip starts at the reset).  Binds the mixer's current parameters and buffers."""
        super().reset(film_params, position)
        self._xdelay = None
        self._pushed, self._closed = 0, False   # samples since the reset, drained ones included; flush() was called

    def _reset_hip(self, film_params):
        h, film, dev = self._reset_hip_args(film_params)
        B, L = self.batch_size, _lib.lib()
        with torch.cuda.device(dev):
            nstate = L.mst_tcn_lookahead_state_bytes(h.ptr, B, self.max_block)
            if nstate == 0:
                _lib.check(-1, "mst_tcn_lookahead_state_bytes")
            if self._state is None or self._state.numel() != nstate or self._state.device != dev:
                self._state = None
                self._state = torch.empty(nstate, device=dev, dtype=torch.uint8)
            _lib.check(L.mst_tcn_lookahead_reset(h.ptr, _lib.dptr(self._state), nstate, B, self.max_block, _lib.dptr(film),
                                                 _lib.stream_ptr(dev)), "mst_tcn_lookahead_reset")
        self._handle = h   # (keeps the C handle alive while the stream uses it)

    def _check_bound(self, what):
        super()._check_bound(what)
        if self._closed:
            raise RuntimeError(f"{what}: flush() closed the stream (the clip has ended and its last samples were drained); "
                               f"call reset() to start the next clip")

    def push(self, x):
        """x (B, 8, N), 1 <= N <= max_block -> (B, 8, N): the output samples at position - latency ... (zeros before the start)."""
        y = super().push(x)
        self._pushed += x.shape[2]
        return y

    def _push_hip(self, x):
        return self._step_hip(self._hip_input(x), x.shape[2], -1)

    def _push_torch(self, x):
        return self._step_torch(x, x.shape[2], None)

    def _drain(self):
        """Closes the stream and yields the last `latency` output samples in pieces of at most max_block."""
        m = self.mixer
        self._check_bound("TCNLookaheadStream.flush")
        if m.backend == "hip":
            msg = _hip_refusal(m, "TCNLookaheadStream.flush")
            if msg:
                _raise_refusal(msg)
        self._closed = True
        end, done = self._pushed, 0
        while done < self.latency:
            n = min(self.max_block, self.latency - done)
            yield (self._step_hip(None, n, end) if m.backend == "hip" else self._step_torch(None, n, end))
            self._pushed += n
            done += n

    def flush(self):
        """Ends the clip: (B, 8, latency), the output samples that the pushes still owe.  Closes the stream."""
        pieces = list(self._drain())
        if pieces:
            return torch.cat(pieces, 2)
        w = self.mixer.input_conv.weight
        return w.new_zeros(self.batch_size, self.mixer.in_channels, 0)

    def _step_hip(self, x, N, t_end):
        dev, L = self._state.device, _lib.lib()
        y = torch.empty(self.batch_size, self.mixer.in_channels, N, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(L.mst_tcn_lookahead_push(self._handle.ptr, _lib.dptr(self._state), self._state.numel(), self.batch_size,
                                                self.max_block, self._pushed, t_end, _lib.dptr(x), N, _lib.dptr(y),
                                                _lib.stream_ptr(dev)), "mst_tcn_lookahead_push")
        return y

    def _step_torch(self, x, N, t_end):
        """The causal restatement's history tensors on the delayed timeline: ring r runs L_r samples behind the input, rows
        whose time is outside the clip are zeroed, and the two residuals are read at the lag of the row they are added to."""
        m, film, t0 = self.mixer, self._film_params, self._pushed
        w = m.input_conv.weight
        K, B = m.kernel_size, self.batch_size
        with torch.no_grad():
            if x is None:
                x = w.new_zeros(B, m.in_channels, N)
            if self._hist is None:
                self._hist = [x.new_zeros(B, m.hidden_channels, (K - 1) * 2 ** (i // 2)) for i in range(2 * m.num_blocks)]
                self._xdelay = x.new_zeros(B, m.in_channels, self.latency)

            def clip(v, lag):   # rows of this push at the times t0 - lag + i: zeros outside [0, t_end)
                lo = min(max(lag - t0, 0), N)
                hi = N if t_end is None else min(max(t_end - t0 + lag, 0), N)
                if lo > 0 or hi < N:
                    v = v.clone()
                    v[:, :, :lo] = 0
                    v[:, :, max(hi, lo):] = 0
                return v

            def conv(c, h, i):   # the causal convolution on (its history, the block); returns z for the delayed residual
                z = torch.cat([self._hist[i], h], dim=2)
                self._hist[i] = z[:, :, N:]
                return F.conv1d(z, c.conv.weight, c.conv.bias, dilation=c.conv.dilation), z

            lag = 0
            h = clip(m.input_conv(x), lag)
            for i, blk in enumerate(m.blocks):
                hist = (K - 1) * 2 ** i
                pad = 0 if m.causal else hist // 2
                g, z = conv(blk.conv1, h, 2 * i)
                res = z[:, :, hist - 2 * pad:hist - 2 * pad + N]   # h delayed by the two lags it skips
                g = blk.norm1(g)
                if m.use_film:
                    p = film[i]
                    g = clip(F.leaky_relu(p["gamma1"].unsqueeze(-1) * g + p["beta1"].unsqueeze(-1), negative_slope=0.2), lag + pad)
                    g = blk.norm2(conv(blk.conv2, g, 2 * i + 1)[0])
                    h = F.leaky_relu(p["gamma2"].unsqueeze(-1) * g + p["beta2"].unsqueeze(-1), negative_slope=0.2) + res
                else:
                    g = blk.norm2(conv(blk.conv2, clip(F.leaky_relu(g, negative_slope=0.2), lag + pad), 2 * i + 1)[0])
                    h = F.leaky_relu(g + res, negative_slope=0.2)
                lag += 2 * pad
                h = clip(h, lag)
            zx = torch.cat([self._xdelay, x], dim=2)
            self._xdelay = zx[:, :, N:]
            return clip(m.output_conv(h) + zx[:, :, :N], lag)


class _TCNTrainFn(torch.autograd.Function):
    """TCNMixer in train() mode on the HIP kernels: y = f(x, film, parameters), gradients of all of them."""

    @staticmethod
    def forward(ctx, mixer, x, film, *params):
        x = x.contiguous()
        y, save, h = mixer._train_forward(x, film, want_save=True)
        ctx.mixer, ctx.handle = mixer, h
        # the parameters are saved for autograd's version check: the backward reads the handle's copies of them
        ctx.save_for_backward(x, film, save, *params)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, film, save = ctx.saved_tensors[:3]
        mixer, h = ctx.mixer, ctx.handle
        dev = x.device
        B, _, T = x.shape
        nb, H, K = mixer.num_blocks, mixer.hidden_channels, mixer.kernel_size
        dy = dy.contiguous()
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
        g = dict(input_w=new(H, 8, 1), input_b=new(H), conv_w=new(nb, 2, H, H, K), conv_b=new(nb, 2, H), bn_w=new(nb, 2, H),
                 bn_b=new(nb, 2, H), output_w=new(8, H, 1), output_b=new(8))
        grads = _lib.TcnGrads(**{k: v.data_ptr() for k, v in g.items()})
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        dfilm = torch.empty_like(film) if film is not None and ctx.needs_input_grad[2] else None
        L = _lib.lib()
        with torch.cuda.device(dev):
            nws = L.mst_tcn_train_workspace_bytes(h.ptr, B, T)
            ws = torch.empty(nws, device=dev, dtype=torch.uint8)
            _lib.check(L.mst_tcn_backward(h.ptr, _lib.dptr(dy), _lib.dptr(x), _lib.dptr(film), B, T, _lib.dptr(save), save.numel(),
                                          C.byref(grads), _lib.dptr(dx), _lib.dptr(dfilm), _lib.dptr(ws), nws, _lib.stream_ptr(dev)),
                       "mst_tcn_backward")
        out = [g["input_w"], g["input_b"]]
        for i in range(nb):
            out += [g["conv_w"][i, 0], g["conv_b"][i, 0], g["conv_w"][i, 1], g["conv_b"][i, 1],
                    g["bn_w"][i, 0], g["bn_b"][i, 0], g["bn_w"][i, 1], g["bn_b"][i, 1]]
        return (None, dx, dfilm, *out, g["output_w"], g["output_b"])


def create_tcn_mixer(receptive_field_seconds=5.2, sample_rate=44100, use_film=False, hidden_channels=8, kernel_size=15,
                     causal=False):
    """TCNMixer whose receptive field covers `receptive_field_seconds` (block count clamped to 6..16)."""
    target = int(receptive_field_seconds * sample_rate)
    n = math.ceil(math.log2((target - 1) / (kernel_size - 1) + 1))
    n = max(6, min(n, 16))
    return TCNMixer(in_channels=8, hidden_channels=hidden_channels, num_blocks=n, kernel_size=kernel_size, causal=causal,
                    use_film=use_film)


def apply_style_transfer(tcn, film_generator, stems_input, target_embedding, input_embedding, device, block=None):
    """Processed stems and their mixture for one track (inference_e2e_style_transfer.py:124-177).  `block`: run the mixer
    through `forward_blockwise(block=block)` (whole songs: state independent of the length) in place of `forward`."""
    tcn.eval()
    film_generator.eval()
    with torch.no_grad():
        stems = {k: v.to(device) for k, v in stems_input.items()}
        x = torch.cat([stems[s] for s in STEM_ORDER], dim=0).unsqueeze(0)
        emb = torch.cat([input_embedding.unsqueeze(0), target_embedding.unsqueeze(0)], dim=1).to(device)
        film = film_generator(emb)
        y = tcn(x, film_params=film) if block is None else tcn.forward_blockwise(x, film_params=film, block=block)
        out ={s: y[0, 2 * i:2 * i + 2, :].cpu() for i, s in enumerate(STEM_ORDER)}
        mixture = sum(out.values())
    return {"processed_stems": out, "processed_mixture": mixture}


_FIT_OPTIMIZERS = ("adam", "adamw", "sgd")


def _fit_refusal(tcn, mixing_model, optimizer, sync):
    """Why `optimize_tcn_style_transfer` cannot run with these objects (None = it can); decided before anything touches a GPU."""
    if optimizer not in _FIT_OPTIMIZERS:
        return f"optimizer={optimizer!r}: 'adam' (default), 'adamw' or 'sgd'"
    if sync not in ("deferred", "step"):
        return f"sync={sync!r}: 'deferred' (default: no host synchronisation inside the loop) or 'step'"
    if mixing_model.training:
        return ("mixing_model is in train() mode; the fit differentiates the stems through a FROZEN encoder (eval-mode BatchNorm, "
                "no Dropout): call mixing_model.eval()")
    live = [n for n, q in mixing_model.named_parameters() if q.requires_grad]
    if live:
        return (f"{len(live)} parameters of mixing_model require grad (first: {live[0]}); the fit optimises the TCN alone: freeze "
                f"them with requires_grad_(False)")
    if getattr(mixing_model, "encoder_backend", None) != "hip" or getattr(mixing_model, "input_grad_backend", None) != "hip":
        return ("mixing_model must run its input gradient on the HIP kernels: encoder_backend='hip' with input_grad_backend='hip' "
                f"(got {getattr(mixing_model, 'encoder_backend', None)!r}, {getattr(mixing_model, 'input_grad_backend', None)!r})")
    if tcn.use_film:
        return "the fit optimises a mixer without FiLM (use_film=False), as the reference's does"
    return None


def optimize_tcn_style_transfer(tcn, stems_input, target_emb, mixing_model, feature_extractor, device, num_steps=200, lr=0.01,
                                verbose=True, *, optimizer="adam", sync="deferred"):
    """The reference's per-pair fit (inference/test_tcn_style_transfer.py:84-201; its optimiser choices grid_search_tcn.py:92-97):
    `num_steps` steps that move the TCN's parameters so that the embedding of the processed stems approaches `target_emb`, every
    step on the HIP kernels -- train-mode TCN forward and backward (`backend = "hip-train"`), the frozen `mixing_model`'s input
    gradient (it must be in eval() with every parameter frozen, `encoder_backend="hip"`, `input_grad_backend="hip"`;
    `feature_grad_backend` as the caller set it), `cosine_distance_loss` against the normalised target, and the step of
    `mst_amd.optim.Adam` / `AdamW` / `SGD(momentum=0.9)`.  The mixing features come from the deferred placeholder, i.e. from the
    encoder's own stage-A launch; `feature_extractor` is accepted for the reference's signature and not read.

    `sync="deferred"` makes no host synchronisation inside the loop: the distance history and the best output are kept on the
    device by `mst_keep_best` and read back once after the last step (`verbose` prints from the history then).  `sync="step"`
    reads the distance every step and tracks the best on the host, with the reference's live progress lines: the same kernels,
    so the same bits.  As in the reference, the output of step k is produced BEFORE update k, the first minimum wins, and
    `converged = best < 0.8 * distances[0]`.  The mixture is the sum of the best step's stems, formed once at the end.  The
    reference's `tcn_state` key (a shallow copy that aliases the live parameters; nobody reads it) is not reproduced, nor is its
    verbose-only extra forward before the loop.

    Returns {"processed_stems": {stem: (2, T) cpu}, "processed_mixture": (2, T) cpu, "distances": [float] * num_steps,
    "final_distance": float, "converged": bool}."""
    from . import optim as hip_optim
    from .loss import cosine_distance_loss
    from .mixing_utils import deferred_features
    why = _fit_refusal(tcn, mixing_model, optimizer, sync)
    if why:
        raise RuntimeError("optimize_tcn_style_transfer: " + why)
    if num_steps < 1:
        raise ValueError(f"num_steps must be at least 1, got {num_steps}")
    device = torch.device(device)
    target = F.normalize(target_emb.detach().to(device, torch.float32), p=2, dim=0).unsqueeze(0)
    x = torch.cat([stems_input[s] for s in STEM_ORDER], dim=0).unsqueeze(0).to(device).contiguous()   # (1, 8, T)
    tcn = tcn.to(device)
    tcn.backend = "hip-train"
    tcn.train()
    params = list(tcn.parameters())
    opt = {"adam": lambda: hip_optim.Adam(params, lr=lr), "adamw": lambda: hip_optim.AdamW(params, lr=lr),
           "sgd": lambda: hip_optim.SGD(params, lr=lr, momentum=0.9)}[optimizer]()
    feats = deferred_features(mixing_model.film_encoder.feature_dim).unsqueeze(0).to(device)
    deferred = sync == "deferred"
    if deferred:
        best = torch.full((), float("inf"), dtype=torch.float32, device=device)
        best_index = torch.full((), -1, dtype=torch.int32, device=device)
        history = torch.zeros(num_steps, dtype=torch.float32, device=device)
        best_y = torch.zeros_like(x)
    else:
        distances, best_distance, best_y = [], float("inf"), None

    def progress(step, distance, best_so_far):
        if verbose and (step % 10 == 0 or step == num_steps - 1):
            print(f"Step {step:3d}/{num_steps}: distance = {distance:.4f}, loss = {distance:.4f}, best = {best_so_far:.4f}")

    for step in range(num_steps):
        opt.zero_grad()
        y = tcn(x)
        emb = mixing_model({s: y[:, 2 * i:2 * i + 2] for i, s in enumerate(STEM_ORDER)}, feats)
        loss = cosine_distance_loss(emb, target)
        if deferred:
            hip_optim.keep_best(loss.detach(), best, best_index, history, step, [(y.detach(), best_y)])
        else:
            distance = loss.item()
            distances.append(distance)
            if distance < best_distance:
                best_distance, best_y = distance, y.detach().cpu()
        loss.backward()
        opt.step()
        if not deferred:
            progress(step, distance, best_distance)
    if deferred:
        distances = history.cpu().tolist()   # the one read-back
        best_distance, best_y = float(best.cpu()), best_y.cpu()
        running = float("inf")
        for step, d in enumerate(distances):
            running = d if d < running else running
            progress(step, d, running)
    if best_distance == float("inf"):
        raise RuntimeError("optimize_tcn_style_transfer: no step produced a distance below infinity (NaN in the stems, the target "
                           "or the encoder?)")
    stems = {s: best_y[0, 2 * i:2 * i + 2] for i, s in enumerate(STEM_ORDER)}
    return {"processed_stems": stems, "processed_mixture": sum(stems.values()), "distances": distances,
            "final_distance": best_distance, "converged": best_distance < distances[0] * 0.8}
