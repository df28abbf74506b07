"""Yardsticks of the frozen-encoder input gradient (tests/test_frozen_grad_{cpu,gpu}.py): the PyTorch modules on the host in
float64 / fp32 with their pre-pool activations, the max-pool DECISIONS (first maximum of a window, none if the maximum is
<= 0), the near-tie measure, and the float64 / fp32 RESTATEMENT of the backward pass with the decisions pinned:

    head autograd at a given pool_in -> dy2 = A2 * mask2 * d pool_in -> conv2d_input -> dy1 = A1 * mask1 * d pool1
    -> conv2d_input per band -> band sum.

A max-pool gradient is discontinuous where two candidates of a window tie, so a plain tolerance on the end-to-end gradient
either fails on a legitimate flip or is so wide that it hides real errors: decisions and arithmetic are tested separately."""
import torch
import torch.nn.functional as F

import cases

CASES = {"default": cases.CFG_DEFAULT, "baseline_sh": cases.CFG_BASELINE_SH}
SHAPES = [("default", 1, 20), ("default", 2, 45), ("default", 2, 83), ("default", 3, 122), ("baseline_sh", 2, 45),
          ("baseline_sh", 3, 122)]


def clip_samples(cfg, frames):
    return (frames - 1) * cfg["hop_length"] + 7


def side_inputs(B, embed_dim):
    """(feats (B, 64) = 2 randn, R (B, embed_dim) = randn) from one generator; the loss is (emb * R).sum()."""
    g = cases._g(21)
    return 2.0 * torch.randn(B, 64, generator=g), torch.randn(B, embed_dim, generator=g)


def torch_twin(cfg, state_dict, dtype):
    """The module with these parameters on the host, `encoder_backend="torch"`, eval mode, frozen, in `dtype`."""
    from mst_amd.model import MixingStyleEncoder
    m = MixingStyleEncoder(channels=8, feature_dim=64, encoder_backend="torch", **cfg)
    full = dict(m.state_dict())
    full.update({k: v.detach().cpu() for k, v in state_dict.items()})
    m.load_state_dict(full, strict=True)
    m = m.to(dtype).eval()
    for q in m.parameters():
        q.requires_grad_(False)
    return m


def geometry(cfg):
    sub = max(1, cfg["split_size"] // 10)
    return cases.n_subbands(cfg["n_mels"], cfg["split_size"], cfg["overlap"]), sub, cfg["split_size"] // sub


def affines(twin, feats):
    """A1 (B, ns, 32), A2 (B, ns, 64): slope of the folded eval affine, FiLM gamma * bn.weight / sqrt(running_var + eps)."""
    film = twin.film_encoder(feats.to(twin.film_encoder.film_head.weight.dtype))
    a1, a2 = [], []
    for i, c in enumerate(twin.audio_encoder.subnet_cnns):
        a1.append(film[f"gamma1_{i}"] * (c.bn1.weight / torch.sqrt(c.bn1.running_var + c.bn1.eps)))
        a2.append(film[f"gamma2_{i}"] * (c.bn2.weight / torch.sqrt(c.bn2.running_var + c.bn2.eps)))
    return torch.stack(a1, 1), torch.stack(a2, 1)


def tree(twin, logmel, feats, want_grad_R=None):
    """Forward of the twin with the pre-ReLU activations of both layers: dict z1 (B, ns, 32, R, Fr), pool1 (B, ns, 32, H1, W1),
    z2 (B, ns, 64, H1, W1), pool_in (B, C, W2), emb, A1, A2 -- and, with want_grad_R = R, `grad`: autograd's d logmel of
    (emb * R).sum()."""
    dt = twin.film_encoder.film_head.weight.dtype
    z = {}
    hooks = []
    for i, c in enumerate(twin.audio_encoder.subnet_cnns):
        hooks.append(c.film1.register_forward_hook(lambda m, a, out, i=i: z.__setitem__(("z1", i), out.detach())))
        hooks.append(c.film2.register_forward_hook(lambda m, a, out, i=i: z.__setitem__(("z2", i), out.detach())))
        hooks.append(c.dropout1.register_forward_hook(lambda m, a, out, i=i: z.__setitem__(("p1", i), out.detach())))
        hooks.append(c.dropout2.register_forward_hook(lambda m, a, out, i=i: z.__setitem__(("p2", i), out.detach())))
    lm = logmel.detach().to(dt).clone().requires_grad_(want_grad_R is not None)
    with torch.set_grad_enabled(want_grad_R is not None):
        emb = twin.forward_from_logmel(lm, feats.to(dt))
        grad = None
        if want_grad_R is not None:
            grad, = torch.autograd.grad((emb * want_grad_R.to(dt)).sum(), lm)
    for h in hooks:
        h.remove()
    ns = len(twin.audio_encoder.subnet_cnns)
    st = lambda k: torch.stack([z[(k, i)] for i in range(ns)], 1)
    p2 = st("p2")
    with torch.no_grad():
        A1, A2 = affines(twin, feats)
    return dict(z1=st("z1"), pool1=st("p1"), z2=st("z2"), pool_in=p2.reshape(p2.shape[0], -1, p2.shape[-1]), emb=emb.detach(),
                A1=A1, A2=A2, grad=grad)


def windows(z, kh, kw):
    """(..., H, W) -> (..., H // kh, W // kw, kh * kw): the pooling windows, positions in row-major order."""
    H, W = z.shape[-2:]
    hp, wp = H // kh, W // kw
    w = z[..., :hp * kh, :wp * kw].reshape(*z.shape[:-2], hp, kh, wp, kw)
    return w.transpose(-3, -2).reshape(*z.shape[:-2], hp, wp, kh * kw)


def decisions(z, kh, kw):
    """One-hot bool mask shaped like z: the FIRST maximum of every pooling window whose maximum is positive."""
    w = windows(z, kh, kw)
    m, am = w.max(dim=-1)   # (torch returns the first of several maxima)
    hot = F.one_hot(am, kh * kw).bool() & (m > 0)[..., None]
    return unwindow(hot, z.shape, kh, kw)


def unwindow(w, shape, kh, kw):
    """Inverse of `windows` into a zero tensor of `shape` (positions outside every window stay 0 / False)."""
    H, W = shape[-2:]
    hp, wp = H // kh, W // kw
    out = torch.zeros(shape, dtype=w.dtype)
    out[..., :hp * kh, :wp * kw] = w.reshape(*shape[:-2], hp, wp, kh, kw).transpose(-3, -2).reshape(*shape[:-2], hp * kh, wp * kw)
    return out


def picked_value(z, mask, kh, kw):
    """Per window: z at the mask's pick, 0 where the mask picks nothing."""
    return (windows(z, kh, kw) * windows(mask, kh, kw).to(z.dtype)).sum(-1)


def near_tie_share(z64, kh, kw, tau):
    """Share of windows whose decision an error below tau could change: the two largest values closer than tau (with a positive
    maximum), or the maximum within tau of 0."""
    w = windows(z64, kh, kw)
    top = w.topk(2, dim=-1).values
    t1, t2 = top[..., 0], top[..., 1]
    near = (t1.abs() < tau) | ((t1 > 0) & (t1 - t2 < tau))
    return float(near.double().mean()), int(near.numel())


def pool_shapes(cfg):
    ns, sub, H1 = geometry(cfg)
    return (sub, 5), (4, 4)


def pinned_gradient(twin, cfg, pool_in, A1, A2, mask1, mask2, R, frames):
    """The backward pass restated in the twin's dtype with the max-pool decisions given:
    pool_in (B, C, W2) -> head (autograd) -> d pool_in -> dy2 = A2 mask2 up(d pool_in) -> conv2d_input -> d pool1 ->
    dy1 = A1 mask1 up(d pool1) -> conv2d_input per band -> sum over the bands.  mask1 (B, ns, 32, R, Fr), mask2 (B, ns, 64, H1, W1)."""
    dt = twin.film_encoder.film_head.weight.dtype
    ns, sub, H1 = geometry(cfg)
    split, ov, M = cfg["split_size"], cfg["overlap"], cfg["n_mels"]
    B = pool_in.shape[0]
    W1 = frames // 5
    p = pool_in.detach().to(dt).clone().requires_grad_(True)
    with torch.enable_grad():
        emb = twin.audio_encoder.attention_pooling(p)
        dpool_in, = torch.autograd.grad((emb * R.to(dt)).sum(), p)
    FD, W2 = H1 // 4, W1 // 4
    d = dpool_in.reshape(B, ns, 64, FD, W2)
    up2 = torch.zeros(B, ns, 64, H1, W1, dtype=dt)
    up2[..., :4 * FD, :4 * W2] = d.repeat_interleave(4, -2).repeat_interleave(4, -1)
    dy2 = A2.to(dt)[..., None, None] * mask2.to(dt) * up2
    dlm = torch.zeros(B, 8, M, frames, dtype=dt)
    for i, c in enumerate(twin.audio_encoder.subnet_cnns):
        dp1 = torch.nn.grad.conv2d_input((B, 32, H1, W1), c.conv2.weight, dy2[:, i], padding=3)
        up1 = torch.zeros(B, 32, split, frames, dtype=dt)
        up1[..., :sub * H1, :5 * W1] = dp1.repeat_interleave(sub, -2).repeat_interleave(5, -1)
        dy1 = A1.to(dt)[:, i, :, None, None] * mask1[:, i].to(dt) * up1
        dlm[:, :, i * ov:i * ov + split] += torch.nn.grad.conv2d_input((B, 8, split, frames), c.conv1.weight, dy1, padding=3)
    return dlm


def normwise(a, ref):
    """max |a - ref| / max |ref|"""
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())
