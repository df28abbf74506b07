"""InfoNCE loss with the reference semantics (src/loss.py:10-136), vectorised (no per-anchor host syncs) and
sharded: with torch.distributed initialised, embeddings and labels cross RCCL/xGMI in ONE packed all-gather and every
rank evaluates the (tiny) loss on the whole gathered batch -- no other collective in forward or backward
(SURVEY.md section 8e).  On CUDA/HIP tensors forward and backward run in libmst.so (`mst_infonce_forward/backward`);
CPU tensors (the gloo tests of the sharding logic) take the same formulas in torch ops.

MultiResolutionSTFTLoss is the cycle-consistency loss of the style-transfer trainer (src/loss.py:332-448): forward and the
gradient to the reconstructed audio in libmst.so (`mst_mrstft_forward/backward`), or `backend="torch"` on torch ops."""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F


class _AllGatherWithGrad(torch.autograd.Function):
    """all-gather of a (n, K) tensor; backward returns this rank's slice of the gradient of the gathered tensor.
    `reduce_grad=True` first all-reduces that gradient -- needed when every rank differentiates only ITS OWN rows of the
    loss, so that the local embeddings also receive the terms where they act as columns of other ranks' anchors.
    InfoNCELoss does not need it: every rank evaluates the whole (replicated) loss on the gathered batch."""

    @staticmethod
    def forward(ctx, x, reduce_grad):
        import torch.distributed as dist
        ws, ctx.rank, ctx.n, ctx.reduce_grad = dist.get_world_size(), dist.get_rank(), x.shape[0], reduce_grad
        out = torch.empty(ws * ctx.n, *x.shape[1:], dtype=x.dtype, device=x.device)
        dist.all_gather_into_tensor(out, x.contiguous())
        return out

    @staticmethod
    def backward(ctx, g):
        import torch.distributed as dist
        if ctx.reduce_grad:
            g = g.contiguous().clone()
            dist.all_reduce(g)
        return g[ctx.rank * ctx.n:(ctx.rank + 1) * ctx.n], None


def gather_embeddings(emb: torch.Tensor, labels: torch.Tensor, reduce_grad=True):
    """ONE all-gather over RCCL/xGMI of (N_local, D) fp32 embeddings with the int64 labels riding along as two extra
    fp32 columns (bit patterns; the collective only copies bytes) -> global embeddings and labels in rank order, plus
    the row offset of the local slice.  Differentiable w.r.t. `emb` (see _AllGatherWithGrad for `reduce_grad`)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return emb, labels, 0
    n, D = emb.shape
    bits = labels.to(torch.int64).contiguous().view(torch.float32).view(n, 2)
    packed = torch.cat([emb.float(), bits.to(emb.device)], dim=1)
    if emb.requires_grad:
        allp = _AllGatherWithGrad.apply(packed, reduce_grad)
    else:
        allp = torch.empty(dist.get_world_size() * n, D + 2, dtype=torch.float32, device=emb.device)
        dist.all_gather_into_tensor(allp, packed)
    all_l = allp[:, D:].detach().contiguous().view(torch.int64).view(-1).to(labels.dtype)
    return allp[:, :D], all_l, dist.get_rank() * n


def info_nce_rows(all_emb, all_labels, row0, rows, temperature):
    """Sum of -log(pos/(pos+neg+1e-8)) over local anchors [row0,row0+rows) that have a positive, and their count."""
    e = F.normalize(all_emb, dim=1)
    sim = e[row0:row0 + rows] @ e.T / temperature            # (rows, N)
    lab = all_labels
    same = lab[row0:row0 + rows, None] == lab[None, :]
    self_mask = torch.zeros_like(same)
    self_mask[torch.arange(rows, device=sim.device), torch.arange(row0, row0 + rows, device=sim.device)] = True
    ex = torch.exp(sim - sim.max(dim=1, keepdim=True)[0])
    pos = (ex * (same & ~self_mask)).sum(1)
    neg = (ex * (~same)).sum(1)
    keep = pos > 0
    li = -torch.log(pos / (pos + neg + 1e-8))
    return torch.where(keep, li, torch.zeros_like(li)).sum(), keep.sum()


def _infonce_ws(N, D, device):
    from . import _lib
    need = _lib.lib().mst_infonce_workspace_bytes(N, D)
    return torch.empty(need, dtype=torch.uint8, device=device), need


class _InfoNCERowsHip(torch.autograd.Function):
    """(sum of row losses, #valid rows) in libmst.so; backward = `mst_infonce_backward` (gradient for all N rows)."""

    @staticmethod
    def forward(ctx, all_emb, all_labels, row0, rows, temperature):
        from . import _lib
        e = all_emb.detach().contiguous().float()
        lab = all_labels.contiguous().to(torch.int64)
        N, D = e.shape
        ws, need = _infonce_ws(N, D, e.device)
        out = torch.empty(2, dtype=torch.float32, device=e.device)
        with torch.cuda.device(e.device):
            _lib.check(_lib.lib().mst_infonce_forward(_lib.dptr(e), _lib.dptr(lab), N, D, row0, rows, float(temperature),
                                                      _lib.dptr(out), _lib.dptr(ws), need, _lib.stream_ptr(e.device)),
                       "mst_infonce_forward")
        ctx.save_for_backward(e, lab)
        ctx.cfg = (row0, rows, float(temperature))
        ctx.mark_non_differentiable(out[1])
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_sum, _g_cnt):
        from . import _lib
        e, lab = ctx.saved_tensors
        row0, rows, temperature = ctx.cfg
        N, D = e.shape
        ws, need = _infonce_ws(N, D, e.device)
        grad = torch.empty_like(e)
        scale = g_sum.detach().reshape(1).float().contiguous()
        with torch.cuda.device(e.device):
            _lib.check(_lib.lib().mst_infonce_backward(_lib.dptr(e), _lib.dptr(lab), N, D, row0, rows, temperature,
                                                       _lib.dptr(scale), _lib.dptr(grad), _lib.dptr(ws), need,
                                                       _lib.stream_ptr(e.device)), "mst_infonce_backward")
        return grad, None, None, None, None


def info_nce_rows_hip(all_emb, all_labels, row0, rows, temperature):
    """Same as info_nce_rows, in libmst.so (`mst_infonce_forward` / `mst_infonce_backward`); differentiable."""
    return _InfoNCERowsHip.apply(all_emb, all_labels, row0, rows, temperature)


class InfoNCELoss(nn.Module):
    """Drop-in for reference InfoNCELoss(temperature)(embeddings (N, D), song_labels (N,)) -> scalar.

    `check`: how the reference's "No positive pairs found in batch!" guard (src/loss.py) is evaluated on the GPU path.
      "sync" (default)  -- as the reference: the count of anchors with a positive is read back and the RuntimeError raised before
                           the call returns.  One device -> host read per call: the host waits for the whole step and the GPU
                           idles for the launch latency of the next step's first kernels (~0.2 ms per step on this chip).
      "deferred"        -- the count goes to a pinned host word with an asynchronous copy; it is examined at the NEXT call (and
                           by `finish()`), by which time the next step's kernels are queued: the same RuntimeError, one call
                           later, no idle GPU.  The step without positives itself returns a zero loss with zero gradients
                           (sum 0 / max(count, 1)).  That step is NOT a no-op for the trainer's state: `optimizer.step()` on
                           zero gradients still applies weight decay and moves Adam's moments, and a training forward has
                           already updated the BatchNorm running statistics -- the model is one decay / momentum step past
                           the last good batch when the error surfaces.  `finish()` is therefore MANDATORY after the last
                           step of a loop and before every checkpoint (otherwise the last call's error is never raised);
                           the owed error of the previous call is raised at the top of the next call, before any of that
                           call's kernels are queued."""

    def __init__(self, temperature=0.1, gather=False, check="sync"):
        super().__init__()
        if check not in ("sync", "deferred"):
            raise ValueError("check must be 'sync' or 'deferred'")
        self.temperature = temperature
        self.gather = gather
        self.check = check
        self._pending = None   # (pinned count, event, message) of the previous call
        self.gather_events = None   # optional (start, end) torch.cuda.Event pair recorded around the all-gather (bench.py, N > 1)

    def finish(self):
        """Deferred mode: examine the last call's guard now (waits for that call's kernels); raises the RuntimeError it owes."""
        pend, self._pending = self._pending, None
        if pend is not None:
            flag, ev, msg = pend
            ev.synchronize()
            if flag.item() == 0:
                raise RuntimeError(msg)

    def forward(self, embeddings, song_labels):
        if self.check == "deferred" and embeddings.is_cuda:
            self.finish()   # the PREVIOUS call's guard, before this call queues anything (its kernels are at most one step behind)
        if self.gather:
            # sharded batch: one packed all-gather, then EVERY rank evaluates the whole loss on the gathered batch
            # (N^2 D flops: negligible next to the encoder).  No all-reduce in the forward, none in the backward:
            # the local slice of d loss / d all_embeddings is already complete, and the value is identical on all
            # ranks.  Parameter gradients must be SUMMED over ranks (each rank holds the part that flows through
            # its own clips).
            if self.gather_events is not None:
                self.gather_events[0].record()
            all_e, all_l, _ = gather_embeddings(embeddings, song_labels, reduce_grad=False)
            if self.gather_events is not None:
                self.gather_events[1].record()
            embeddings, song_labels = all_e, all_l
        rows_fn = info_nce_rows_hip if embeddings.is_cuda else info_nce_rows
        s, c = rows_fn(embeddings, song_labels, 0, embeddings.shape[0], self.temperature)
        if self.check == "deferred" and embeddings.is_cuda:
            bufs = self.__dict__.setdefault("_flags", [torch.zeros(1).pin_memory(), torch.zeros(1).pin_memory()])
            self._turn = 1 - getattr(self, "_turn", 0)
            flag = bufs[self._turn]
            flag.copy_(c.detach().reshape(1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (flag, ev, f"No positive pairs found in batch! Batch size: {embeddings.shape[0]}, "
                                       "This likely means each song only appears once in the batch.")
            return s / torch.clamp(c, min=1.0)
        if c.item() == 0:
            raise RuntimeError(
                f"No positive pairs found in batch! Batch size: {embeddings.shape[0]}, "
                f"Unique songs: {len(torch.unique(song_labels))}, "
                f"This likely means each song only appears once in the batch.")
        return s / c


def _raise_mrstft_refusal(msg):
    raise RuntimeError("MultiResolutionSTFTLoss: " + msg + "; backend='torch' runs the same loss on PyTorch ops (any device, "
                       "dtype, autograd to both arguments)")


class _MRSTFTHip(torch.autograd.Function):
    """(loss, components and norms) of `mst_mrstft_forward`; backward = `mst_mrstft_backward`, which recomputes the frames
    and multiplies by the incoming gradient on the device."""

    @staticmethod
    def forward(ctx, x, y, plan):
        from . import _lib
        T = x.shape[-1]
        xr = x.detach().reshape(-1, T).contiguous()
        yr = y.detach().reshape(-1, T).contiguous()
        out = plan.run_forward(xr, yr)
        ctx.save_for_backward(xr, yr, out)
        ctx.plan, ctx.shape = plan, x.shape
        rest = out[1:]   # components and norms
        ctx.mark_non_differentiable(rest)
        return out[0], rest

    @staticmethod
    def backward(ctx, g_loss, _g_out):
        from . import _lib
        xr, yr, out = ctx.saved_tensors
        plan = ctx.plan
        rows, T = xr.shape
        grad = torch.empty_like(xr)
        scale = g_loss.detach().reshape(1).float().contiguous()
        ws, need = plan.workspace(rows, T, xr.device)
        with torch.cuda.device(xr.device):
            _lib.check(_lib.lib().mst_mrstft_backward(_lib.dptr(xr), _lib.dptr(yr), rows, T, plan.n, plan.fft, plan.hop,
                                                      plan.window_ptrs(xr.device), plan.sc_weight, plan.log_weight,
                                                      _lib.dptr(out), _lib.dptr(scale), _lib.dptr(grad), _lib.dptr(ws), need,
                                                      _lib.stream_ptr(xr.device)), "mst_mrstft_backward")
        return grad.view(ctx.shape), None, None


class _MRSTFTPlan:
    """Host side of the HIP path: the resolution lists as C arrays and the fp32 window tables, built once on the host (as
    mixing_utils.hann_window for stage A) and uploaded once per device."""

    def __init__(self, fft_sizes, hop_sizes, sc_weight, log_weight):
        self.n = len(fft_sizes)
        self.fft_list = [int(v) for v in fft_sizes]
        self.fft = (C.c_int * self.n)(*self.fft_list)
        self.hop = (C.c_int * self.n)(*[int(v) for v in hop_sizes])
        self.sc_weight, self.log_weight = float(sc_weight), float(log_weight)
        self._windows = {}

    def window_ptrs(self, device):
        key = str(device)
        if key not in self._windows:
            tabs = [torch.hann_window(n).to(device) for n in self.fft_list]
            self._windows[key] = (tabs, (C.c_void_p * self.n)(*[t.data_ptr() for t in tabs]))
        return self._windows[key][1]

    def workspace(self, rows, T, device):
        from . import _lib
        need = _lib.lib().mst_mrstft_workspace_bytes(self.n, self.fft, self.hop, rows, T)
        return torch.empty(need, dtype=torch.uint8, device=device), need

    def run_forward(self, xr, yr):
        from . import _lib
        rows, T = xr.shape
        out = torch.empty(1 + 4 * self.n, dtype=torch.float32, device=xr.device)
        ws, need = self.workspace(rows, T, xr.device)
        with torch.cuda.device(xr.device):
            _lib.check(_lib.lib().mst_mrstft_forward(_lib.dptr(xr), _lib.dptr(yr), rows, T, self.n, self.fft, self.hop,
                                                     self.window_ptrs(xr.device), self.sc_weight, self.log_weight,
                                                     _lib.dptr(out), _lib.dptr(ws), need, _lib.stream_ptr(xr.device)),
                       "mst_mrstft_forward")
        return out


class MultiResolutionSTFTLoss(nn.Module):
    """Drop-in for the reference MultiResolutionSTFTLoss(fft_sizes, hop_sizes, win_sizes, window)(x, y) -> scalar, x and y
    (B, C, T) or (C, T): per resolution ||ym - xm||_F / (||ym||_F + 1e-8) + mean |log(xm + 1e-5) - log(ym + 1e-5)| of the
    STFT magnitudes (torch.stft defaults: center, reflect padding, one-sided; periodic Hann), averaged over resolutions.

    Keyword-only extensions (defaults = the reference): `sc_weight` / `log_weight` multiply the two terms;
    `backend="hip"` runs forward and the gradient to `x` in libmst.so (CUDA fp32, `y` without gradient, win == fft in
    {512, 1024, 2048}, hop in {n/8, n/4, n/2}, T > max(fft) // 2; anything else raises), `backend="torch"` is the plain
    restatement on torch ops.  Neither path synchronises with the host.

    `components(x, y)`: (n_resolutions, 2) unweighted (spectral convergence, log magnitude) terms, no graph."""

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[256, 512, 128], win_sizes=[1024, 2048, 512], window='hann', *,
                 sc_weight=1.0, log_weight=1.0, backend="hip"):
        super().__init__()
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if not (len(fft_sizes) == len(hop_sizes) == len(win_sizes)) or len(fft_sizes) < 1:
            raise ValueError("fft_sizes, hop_sizes and win_sizes need the same length, at least 1")
        self.fft_sizes = fft_sizes
        self.hop_sizes = hop_sizes
        self.win_sizes = win_sizes
        self.window = window
        self.sc_weight = sc_weight
        self.log_weight = log_weight
        self.backend = backend
        self._plan = None

    # ---- backend="torch": the reference's arithmetic, op for op
    def stft(self, x, fft_size, hop_size, win_size):
        if x.ndim == 2:
            x = x.unsqueeze(0)
        B, Cn, T = x.shape
        window_tensor = torch.hann_window(win_size, device=x.device)   # no dtype, as the reference: fp32 table also under float64
        return torch.stft(x.reshape(B * Cn, T), n_fft=fft_size, hop_length=hop_size, win_length=win_size, window=window_tensor,
                          return_complex=True)

    def spectral_convergence(self, x_mag, y_mag):
        return torch.norm(y_mag - x_mag, p='fro') / (torch.norm(y_mag, p='fro') + 1e-8)

    def log_stft_magnitude(self, x_mag, y_mag):
        return F.l1_loss(torch.log(x_mag + 1e-5), torch.log(y_mag + 1e-5))

    def _terms_torch(self, x, y):
        if self.window != 'hann':
            raise ValueError(f"window={self.window!r}: only 'hann' exists (the reference ignores the argument)")
        terms = []
        for fft_size, hop_size, win_size in zip(self.fft_sizes, self.hop_sizes, self.win_sizes):
            x_mag = torch.abs(self.stft(x, fft_size, hop_size, win_size))
            y_mag = torch.abs(self.stft(y, fft_size, hop_size, win_size))
            terms.append((self.spectral_convergence(x_mag, y_mag), self.log_stft_magnitude(x_mag, y_mag)))
        return terms

    # ---- backend="hip"
    def _hip_refusal(self, x, y):
        for name, t in (("x", x), ("y", y)):
            if not t.is_cuda:
                return f"the HIP backend needs CUDA tensors (there is no CPU fallback), got {name} on {t.device}"
            if t.dtype != torch.float32:
                return f"the HIP backend is fp32, got {name} of {t.dtype}"
        if x.shape != y.shape or x.dim() not in (2, 3):
            return f"the HIP backend needs x and y of one shape (B, C, T) or (C, T), got {tuple(x.shape)} and {tuple(y.shape)}"
        if x.device != y.device:
            return f"x on {x.device} and y on {y.device}"
        if torch.is_grad_enabled() and y.requires_grad:
            return "the HIP backend has no gradient to the target y (detach it)"
        if self.window != 'hann':
            return f"the HIP backend has the Hann window only, got window={self.window!r}"
        for n, h, w in zip(self.fft_sizes, self.hop_sizes, self.win_sizes):
            if w != n:
                return f"the HIP backend needs win_size == fft_size, got {w} and {n}"
            if n not in (512, 1024, 2048):
                return f"the HIP backend has fft_size 512, 1024 and 2048, got {n}"
            if h not in (n // 8, n // 4, n // 2):
                return f"the HIP backend needs hop_size in (n/8, n/4, n/2), got {h} for fft_size {n}"
        if len(self.fft_sizes) > 16:
            return f"the HIP backend takes up to 16 resolutions, got {len(self.fft_sizes)}"
        if x.shape[-1] <= max(self.fft_sizes) // 2:
            return f"the HIP backend needs T > max(fft_sizes) // 2 = {max(self.fft_sizes) // 2} samples, got T = {x.shape[-1]}"
        if x.numel() == 0:
            return "empty input"
        return None

    def _hip_plan(self):
        key = (tuple(self.fft_sizes), tuple(self.hop_sizes), float(self.sc_weight), float(self.log_weight))
        if self._plan is None or self._plan[0] != key:
            self._plan = (key, _MRSTFTPlan(self.fft_sizes, self.hop_sizes, self.sc_weight, self.log_weight))
        return self._plan[1]

    def _hip_out(self, x, y):
        msg = self._hip_refusal(x, y)
        if msg:
            _raise_mrstft_refusal(msg)
        return _MRSTFTHip.apply(x, y, self._hip_plan())

    def components(self, x, y):
        with torch.no_grad():
            if self.backend == "torch":
                return torch.stack([torch.stack(t) for t in self._terms_torch(x, y)])
            n = len(self.fft_sizes)
            return self._hip_out(x, y)[1][:2 * n].view(n, 2).clone()

    def forward(self, x, y):
        if self.backend == "hip":
            return self._hip_out(x, y)[0]
        total_loss = 0.0
        for sc_loss, log_mag_loss in self._terms_torch(x, y):
            if self.sc_weight == 1.0 and self.log_weight == 1.0:
                total_loss += sc_loss + log_mag_loss
            else:
                total_loss += self.sc_weight * sc_loss + self.log_weight * log_mag_loss
        return total_loss / len(self.fft_sizes)


class _CosDistHip(torch.autograd.Function):
    """mean_i (1 - cos(pred_i, target_i)) in libmst.so (`mst_cosdist_forward` / `mst_cosdist_backward`); gradient to `pred` only."""

    @staticmethod
    def forward(ctx, pred, target):
        from . import _lib
        p, t = pred.detach().contiguous(), target.detach().contiguous()
        K, D = p.shape
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        save = torch.empty(K, 3, dtype=torch.float32, device=p.device)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().mst_cosdist_forward(_lib.dptr(p), _lib.dptr(t), K, D, _lib.dptr(loss), _lib.dptr(save),
                                                      _lib.stream_ptr(p.device)), "mst_cosdist_forward")
        ctx.save_for_backward(p, t, save)
        return loss[0]

    @staticmethod
    def backward(ctx, g_loss):
        from . import _lib
        p, t, save = ctx.saved_tensors
        K, D = p.shape
        grad = torch.empty_like(p)
        g = g_loss.detach().reshape(1).float().contiguous()
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().mst_cosdist_backward(_lib.dptr(p), _lib.dptr(t), K, D, _lib.dptr(save), _lib.dptr(g), _lib.dptr(grad),
                                                       _lib.stream_ptr(p.device)), "mst_cosdist_backward")
        return grad, None


def cosine_distance_loss(pred, target, backend="hip"):
    """The adversarial branch's loss (reference src/train.py:199-202): mean over rows of 1 - cosine similarity of `pred` and
    `target` (K, D), both normalised as F.normalize does (norm clamped at 1e-12).  `backend="hip"`: forward and the gradient to
    `pred` in libmst.so (fp32 CUDA tensors, D <= 2048, `target` without gradient; anything else raises, naming the reason);
    `backend="torch"`: the reference's three lines on PyTorch ops (any device, dtype, autograd to both arguments)."""
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    if backend == "torch":
        pred_norm = F.normalize(pred, dim=1)
        target_norm = F.normalize(target, dim=1)
        return (1.0 - (pred_norm * target_norm).sum(dim=1)).mean()
    why = None
    for name, t in (("pred", pred), ("target", target)):
        if not t.is_cuda:
            why = f"the HIP backend needs CUDA tensors (there is no CPU fallback), got {name} on {t.device}"
        elif t.dtype != torch.float32:
            why = f"the HIP backend is fp32, got {name} of {t.dtype}"
        if why:
            break
    if why is None:
        if pred.dim() != 2 or pred.shape != target.shape or pred.device != target.device:
            why = f"the HIP backend needs pred and target of one shape (K, D) on one device, got {tuple(pred.shape)} and {tuple(target.shape)}"
        elif pred.shape[0] < 1 or not 1 <= pred.shape[1] <= 2048:
            why = f"the HIP backend takes K >= 1 rows of 1 <= D <= 2048, got {tuple(pred.shape)}"
        elif torch.is_grad_enabled() and target.requires_grad:
            why = "the HIP backend has no gradient to the target (detach it)"
    if why:
        raise RuntimeError("cosine_distance_loss: " + why + "; backend='torch' runs the same loss on PyTorch ops")
    return _CosDistHip.apply(pred, target)
