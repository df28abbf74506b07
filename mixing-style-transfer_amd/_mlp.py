"""The three networks of the shape Linear -> act -> Dropout -> Linear -> act -> Dropout -> Linear that train in libmst.so
(csrc/head.hip): the FiLM MLP of MixingFeatureEncoder, the song-identity discriminator and the TCN FiLM generator.  One
autograd function drives all three; `Net` states what is particular to each."""
import ctypes as C
from typing import NamedTuple

import torch

from . import _lib


def _seed64():
    """A 62-bit seed from torch's CPU generator (reproducible under torch.manual_seed; no device work)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class Net(NamedTuple):
    dims: type             # the _lib structure classes
    weights: type
    grads: type
    forward: str           # the symbols: forward(dims, weights, x, B, *scalars, out, save, save_bytes, stream)
    backward: str          # backward(dims, weights, x, B, *scalars, dout, save, grads, [dx,] work, work_bytes, stream)
    save_bytes: str
    work_bytes: str
    fwd_scalars: str       # the scalar arguments behind B, of p1 p2 slope seed1 seed2
    bwd_scalars: str
    input_grad: bool       # whether the backward takes dx (NULL when the input needs no gradient)


FILM = Net(_lib.FilmDims, _lib.FilmPtrs, _lib.FilmPtrs, "mst_film_forward_train", "mst_film_backward", "mst_film_save_bytes",
           "mst_film_backward_workspace_bytes", "p1 seed1", "p1", False)
DISC = Net(_lib.DiscDims, _lib.DiscPtrs, _lib.DiscPtrs, "mst_disc_forward", "mst_disc_backward", "mst_disc_save_bytes",
           "mst_disc_backward_workspace_bytes", "p1 seed1 seed2", "p1 seed1 seed2", True)
TCN_FILM = Net(_lib.TcnFilmTrainDims, _lib.TcnFilmWeights, _lib.TcnFilmGrads, "mst_tcn_film_forward_train", "mst_tcn_film_backward",
               "mst_tcn_film_train_save_bytes", "mst_tcn_film_train_backward_workspace_bytes", "slope p1 seed1 p2 seed2",
               "slope p1 seed1 p2 seed2", True)


def mlp_dims(net, ws):
    """The dims structure of the six tensors (weight, bias) x 3 in state_dict layout."""
    return net.dims(ws[0].shape[1], ws[0].shape[0], ws[4].shape[0])


def mlp_ptrs(cls, tensors):
    return C.byref(cls(*[t.data_ptr() for t in tensors]))


def mlp_buffer(sym, dims, B, device):
    return torch.empty(getattr(_lib.lib(), sym)(C.byref(dims), B), dtype=torch.uint8, device=device)


def mlp_call(sym, device, *args):
    """One entry point on `device`'s current stream; tensors are passed as such (None = NULL)."""
    args = [_lib.dptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(device):
        _lib.check(getattr(_lib.lib(), sym)(*args, _lib.stream_ptr(device)), sym)


class _HipMLP(torch.autograd.Function):
    """`_HipMLP.apply(net, x, out_shape, p1, p2, slope, w0, b0, w3, b3, w6, b6)`: forward and backward of one of the three
    networks in libmst.so: fp32, deterministic, Dropout masks re-derived from (seed, element) instead of stored.  out_shape: the
    output is (B, *out_shape), None = (B, out_dim) (the generator's packed (nb, 4, H): autograd must know the tensor the mixer
    slices as this function's output, not as a view of it).  p1 / p2: the two Dropouts (0 = none; one seed is drawn per
    positive p, in this order); slope: the generator's LeakyReLU.  The input gets a gradient
    where the network has one (`net.input_grad`: not the FiLM MLP, whose features are data) and it is needed.  fp32 contiguous
    parameters are read by pointer, live; autograd's version check of the saved tensors covers the backward's second read."""

    @staticmethod
    def forward(ctx, net, x, out_shape, p1, p2, slope, *params):
        f = x.detach().contiguous().float()
        B = f.shape[0]
        ws = [t.detach().contiguous().float() for t in params]
        dims = mlp_dims(net, ws)
        scal = dict(p1=float(p1), p2=float(p2), slope=float(slope), seed1=_seed64() if p1 > 0.0 else 0,
                    seed2=_seed64() if p2 > 0.0 else 0)
        save = mlp_buffer(net.save_bytes, dims, B, f.device)
        out = torch.empty(B, *(out_shape or ws[4].shape[:1]), device=f.device)
        mlp_call(net.forward, f.device, C.byref(dims), mlp_ptrs(net.weights, ws), f, B, *[scal[k] for k in net.fwd_scalars.split()], out,
                 save, save.numel())
        ctx.cfg = (net, dims, scal)
        ctx.save_for_backward(f, save, *ws)
        return out

    @staticmethod
    def backward(ctx, dout):
        f, save, *ws = ctx.saved_tensors
        net, dims, scal = ctx.cfg
        B = f.shape[0]
        grads = [torch.empty_like(t) for t in ws]
        dx = torch.empty_like(f) if net.input_grad and ctx.needs_input_grad[1] else None
        work = mlp_buffer(net.work_bytes, dims, B, f.device)
        mlp_call(net.backward, f.device, C.byref(dims), mlp_ptrs(net.weights, ws), f, B, *[scal[k] for k in net.bwd_scalars.split()],
                 dout.contiguous().float(), save, mlp_ptrs(net.grads, grads), *((dx,) if net.input_grad else ()), work, work.numel())
        return (None, dx, None, None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[6:]))
