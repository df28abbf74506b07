"""Seeded cases and helpers of the TCN training tests (data only, no reference code).

The cases are the smallest shapes at which the training kernels can still go wrong; each runs in seconds on the GPU and in
float64 on the CPU.  Inputs: cases.pcm_batch, a seeded FiLM tensor (gamma 1 +- 0.3, beta +- 0.3), a seeded uniform dy with
loss = sum(y * dy).  State dicts are cases_tcn.make_tcn_state_dict's.

The parity rule (per quantity group, LeakyReLU masks pinned): a LeakyReLU argument within rounding of zero takes slope 1 in
one precision and 0.2 in the other, so no fp32 implementation matches a free-running float64 run.  The float64 yardstick
therefore takes the masks of the fp32 run under test (`pinned`), and every group's maximum relative error (cases_tcn.max_rel)
must stay within 2 x the reference's own fp32-against-float64 error of that group in the fixture (e_ref)."""
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import cases
import cases_tcn as ct

CASES = {
    "t_st": dict(H=16, nb=6, K=15, causal=False, film=True, B=2, T=3001),        # trainer geometry, odd T
    "t_deep": dict(H=16, nb=14, K=15, causal=False, film=True, B=2, T=2500),     # dilations up to 8192 > T
    "t_causal": dict(H=16, nb=5, K=4, causal=True, film=True, B=2, T=2050),      # even kernel, one-sided padding
    "t_plain40": dict(H=40, nb=4, K=5, causal=False, film=False, B=2, T=1999),   # padded channels, activation after the sum
    "t_wide128": dict(H=128, nb=3, K=15, causal=False, film=True, B=1, T=1500),  # the split-channel instantiation
    "t_h8": dict(H=8, nb=4, K=15, causal=False, film=False, B=1, T=2000),        # H below one tile, B = 1
    # odd tile counts (the second half of the output channels has one tile fewer) and idle threads in the row reductions
    "t_odd72": dict(H=72, nb=3, K=7, causal=False, film=True, B=2, T=1201),      # HP = 80: 3 slots, 16 idle threads
    "t_w100": dict(H=100, nb=2, K=4, causal=True, film=False, B=2, T=1100),      # HP = 112: 2 slots, 32 idle, 12 padded channels
}
FILM_KEYS = ("gamma1", "beta1", "gamma2", "beta2")
# quantity groups of the parity rule (block conv biases are not among them: their gradient is mathematically zero)
GROUPS = ("y", "stats", "dx", "dfilm", "conv_w", "bn", "input_w", "input_b", "output_w", "output_b")


def fixture_path(name):
    return os.path.join(ct.GOLDEN, f"tcn_train_{name}.npz")


def film_tensor(c, seed=5100):
    """(B, nb, 4, H): gamma 1 +- 0.3, beta +- 0.3."""
    f = ct._u(cases._g(seed), (c["B"], c["nb"], 4, c["H"]), 0.3)
    f[:, :, 0::2] += 1.0
    return f


def film_dicts(film):
    return [{k: film[:, i, q] for q, k in enumerate(FILM_KEYS)} for i in range(film.shape[1])]


def dy_tensor(c, seed=5200):
    return ct._u(cases._g(seed), (c["B"], 8, c["T"]), 1.0)


def group_of(param_name):
    """Quantity group of a TCNMixer parameter; None for the block conv biases."""
    if param_name.startswith(("input_conv.", "output_conv.")):
        return param_name.replace("_conv.weight", "_w").replace("_conv.bias", "_b")
    if ".norm" in param_name:
        return "bn"
    return "conv_w" if param_name.endswith("conv.weight") else None


def sample(name, t, k=512):
    """The stored part of a gradient tensor: whole when small, else k seeded positions (flat, float64 numpy).  k = 512 per
    tensor keeps the 14-block case's fixture below the size limit of a committed file (28 conv weights)."""
    a = t.detach().cpu().double().numpy().ravel()
    if a.size <= k:
        return a
    return a[cases.sample_idx(a.size, k, seed=13 + sum(map(ord, name)))]


def dx_samples(dx):
    """The compared part of a (B, 8, T) input gradient: the first and last 128 samples of every channel and 4096 seeded
    positions of the rest, flat float64."""
    B, _, T = dx.shape
    d = dx.detach().cpu().double()
    mid = d[:, :, 128:T - 128].reshape(-1)[cases.sample_idx(B * 8 * (T - 256), 4096, seed=14)]
    return np.concatenate([d[:, :, :128].numpy().ravel(), d[:, :, T - 128:].numpy().ravel(), mid.numpy()])


class Recorder:
    """Stands in for the `F` a module tree sees: F.leaky_relu itself, noting the mask `argument > 0` of every call."""

    def __init__(self):
        self.masks = []

    def leaky_relu(self, x, negative_slope=0.01):
        self.masks.append((x > 0).detach())
        return F.leaky_relu(x, negative_slope=negative_slope)

    def stacked(self):
        return torch.stack(self.masks)   # (2 nb, B, H, T), the order of the calls = conv1, conv2 of block 0, 1, ...


class Pinned:
    """Stands in for `F` with the branch of every LeakyReLU imposed: where(mask, f, slope * f), masks in call order."""

    def __init__(self, masks):
        self.masks, self.i = masks, 0

    def leaky_relu(self, x, negative_slope=0.01):
        m = self.masks[self.i]
        self.i += 1
        return torch.where(m, x, negative_slope * x)


def run_tree(make_mixer, c, dtype):
    """One training step's forward and backward of a module tree (this project's with backend='torch', or the reference's)
    on the CPU.  Returns a dict: y, dx, dfilm, grads {parameter name: gradient}, bmean / bvar (2 nb, H) as seen at the
    BatchNorm inputs, rmean / rvar (2 nb, H) after the step, nbt."""
    tcn = make_mixer()
    tcn.load_state_dict(ct.make_tcn_state_dict(c), strict=True)
    tcn = tcn.to(dtype).train()
    x = cases.pcm_batch(c["B"], c["T"]).to(dtype).requires_grad_()
    film = film_tensor(c).to(dtype).requires_grad_() if c["film"] else None
    norms = [getattr(b, f"norm{l}") for b in tcn.blocks for l in (1, 2)]
    bmean, bvar = [], []

    def note(module, inputs, output):
        bmean.append(inputs[0].detach().mean((0, 2)))
        bvar.append(inputs[0].detach().var((0, 2), unbiased=False))

    hooks = [n.register_forward_hook(note) for n in norms]
    y = tcn(x, film_params=film_dicts(film) if c["film"] else None)
    for h in hooks:
        h.remove()
    (y * dy_tensor(c).to(dtype)).sum().backward()
    return SimpleNamespace(y=y.detach(), dx=x.grad, dfilm=film.grad if c["film"] else None,
                           grads={k: p.grad for k, p in tcn.named_parameters()}, bmean=torch.stack(bmean), bvar=torch.stack(bvar),
                           rmean=torch.stack([n.running_mean for n in norms]), rvar=torch.stack([n.running_var for n in norms]),
                           nbt=int(norms[0].num_batches_tracked))


def groups_of_run(r):
    """{group: flat float64 vector} of a run_tree-like result with WHOLE tensors, in a fixed order; and max |db| of the block
    conv biases."""
    cat = lambda ts: np.concatenate([t.detach().cpu().double().numpy().ravel() for t in ts])  # noqa: E731
    g = {"y": cat([r.y]), "stats": cat([r.bmean, r.bvar]), "dx": cat([r.dx])}
    if r.dfilm is not None:
        g["dfilm"] = cat([r.dfilm])
    for grp in ("conv_w", "bn", "input_w", "input_b", "output_w", "output_b"):
        g[grp] = cat([v for k, v in r.grads.items() if group_of(k) == grp])
    db = max(float(v.abs().max()) for k, v in r.grads.items() if group_of(k) is None)
    return g, db


def fixture_groups(g, bits):
    """{group: flat float64 vector} of the fixture's stored samples at `bits` (32 or 64)."""
    out = {"y": ct.golden_y(g, bits), "stats": np.concatenate([g[f"bmean{bits}"].ravel(), g[f"bvar{bits}"].ravel()]).astype(np.float64),
           "dx": g[f"dx{bits}"].astype(np.float64)}
    if f"dfilm{bits}" in g:
        out["dfilm"] = g[f"dfilm{bits}"].astype(np.float64).ravel()
    names = [str(k) for k in g["param_names"]]
    for grp in ("conv_w", "bn", "input_w", "input_b", "output_w", "output_b"):
        out[grp] = np.concatenate([g[f"g{bits}_{k}"].astype(np.float64).ravel() for k in names if group_of(k) == grp])
    return out


def sampled_groups(r):
    """groups_of_run on the fixture's sample positions (the order of fixture_groups)."""
    f = lambda t: t.detach().cpu().double().numpy().ravel()  # noqa: E731
    out = {"y": ct.flat_y(r.y), "stats": np.concatenate([f(r.bmean), f(r.bvar)]), "dx": dx_samples(r.dx)}
    if r.dfilm is not None:
        out["dfilm"] = f(r.dfilm)
    for grp in ("conv_w", "bn", "input_w", "input_b", "output_w", "output_b"):
        out[grp] = np.concatenate([sample(k, v) for k, v in r.grads.items() if group_of(k) == grp])
    return out


def e_ref(g):
    """{group: the reference's own fp32-against-float64 maximum relative error (masks pinned)} from a fixture."""
    a, b = fixture_groups(g, 32), fixture_groups(g, 64)
    return {k: ct.max_rel(a[k], b[k])[0] for k in a}


def unpack_masks(g, c):
    n = 2 * c["nb"] * c["B"] * c["H"] * c["T"]
    return torch.from_numpy(np.unpackbits(g["masks"])[:n].astype(bool)).view(2 * c["nb"], c["B"], c["H"], c["T"])
