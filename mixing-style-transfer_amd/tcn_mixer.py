"""Stage C: the TCN mixer that turns a pair of mixing-style embeddings into processed stems (the reference's
`src/tcn_mixer.py`, driven by `inference/inference_e2e_style_transfer.py:124-177`).

Same class names, constructor arguments, defaults and `state_dict` keys as the reference, so a reference checkpoint's
`tcn_state_dict` / `film_generator_state_dict` loads with `strict=True`.  Two backends:

  * `backend = "hip"` (default): inference on the kernels of `csrc/tcn.hip` (exact fp32 MFMA).  Needs `eval()`, CUDA
    tensors, fp32 and no gradients; anything else RAISES and names the opt-in (no silent library path, no CPU fallback).
  * `backend = "torch"`: the plain module tree on PyTorch (any device, any dtype, autograd).  It is the opt-in for
    training and the arithmetic the tests pin to the reference.
"""
import ctypes as C
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

STEM_ORDER = ("vocals", "bass", "drums", "other")
_BACKENDS = ("hip", "torch")


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
        self._hip = None

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
        B = concat_embeddings.shape[0]
        if self.backend == "torch":
            return self.mlp(concat_embeddings).view(B, self.num_blocks, 4, self.hidden_channels)
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

    def _forward_hip(self, x, film, tap_blocks=()):
        """x (B, 8, T) cuda fp32, film (B, nb, 4, H) or None -> y, [hidden state after each block of tap_blocks]."""
        dev = x.device
        h = self._handle(dev)
        x = x.contiguous()
        B, _, T = x.shape
        H = self.hidden_channels
        y = torch.empty_like(x)
        taps_out = [torch.empty(B, H, T, device=dev, dtype=torch.float32) for _ in tap_blocks]
        if B == 0 or T == 0:
            return y, taps_out
        L = _lib.lib()
        with torch.cuda.device(dev):
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

    def forward(self, x, film_params=None):
        if self.use_film:
            if film_params is None:
                raise ValueError("film_params must be provided when use_film=True")
            if len(film_params) != self.num_blocks:
                raise ValueError(f"Expected {self.num_blocks} FiLM parameter dicts, got {len(film_params)}")
        if self.backend not in _BACKENDS:
            raise ValueError("backend must be 'hip' (default) or 'torch'")
        if self.backend == "torch":
            return self._forward_torch(x, film_params)
        fl = [p[k] for p in film_params for k in _FILM_KEYS] if self.use_film else []
        msg = _hip_refusal(self, "TCNMixer.forward", x, *fl)
        if msg:
            _raise_refusal(msg)
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"expected (B, {self.in_channels}, T) stems, got {tuple(x.shape)}")
        film = _packed_film(film_params, x.shape[0], self.num_blocks, self.hidden_channels) if self.use_film else None
        return self._forward_hip(x, film)[0]

    def process_stems_dict(self, stems_dict, film_params=None):
        stacked = torch.cat([stems_dict[s] for s in STEM_ORDER], dim=0).unsqueeze(0)
        out = self.forward(stacked, film_params=film_params).squeeze(0)
        return {s: out[2 * i:2 * i + 2, :] for i, s in enumerate(STEM_ORDER)}


def create_tcn_mixer(receptive_field_seconds=5.2, sample_rate=44100, use_film=False, hidden_channels=8, kernel_size=15,
                     causal=False):
    """TCNMixer whose receptive field covers `receptive_field_seconds` (block count clamped to 6..16)."""
    target = int(receptive_field_seconds * sample_rate)
    n = math.ceil(math.log2((target - 1) / (kernel_size - 1) + 1))
    n = max(6, min(n, 16))
    return TCNMixer(in_channels=8, hidden_channels=hidden_channels, num_blocks=n, kernel_size=kernel_size, causal=causal,
                    use_film=use_film)


def apply_style_transfer(tcn, film_generator, stems_input, target_embedding, input_embedding, device):
    """Processed stems and their mixture for one track (inference_e2e_style_transfer.py:124-177)."""
    tcn.eval()
    film_generator.eval()
    with torch.no_grad():
        stems = {k: v.to(device) for k, v in stems_input.items()}
        x = torch.cat([stems[s] for s in STEM_ORDER], dim=0).unsqueeze(0)
        emb = torch.cat([input_embedding.unsqueeze(0), target_embedding.unsqueeze(0)], dim=1).to(device)
        y = tcn(x, film_params=film_generator(emb))
        out = {s: y[0, 2 * i:2 * i + 2, :].cpu() for i, s in enumerate(STEM_ORDER)}
        mixture = sum(out.values())
    return {"processed_stems": out, "processed_mixture": mixture}
