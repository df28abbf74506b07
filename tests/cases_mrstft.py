"""Seeded inputs and sampling helpers of the MultiResolutionSTFTLoss tests (data only, no reference code).

y = cases.pcm_batch (integer-built PCM with silent stretches: 3-5 % of the target's bins are exactly zero);
x "near" = a reconstruction close to the target (the trainer's regime), x "far" = another clip's stems plus noise."""
import os

import numpy as np
import torch

import cases

GOLDEN = os.path.join(cases.ROOT, "tests", "golden", "mrstft.npz")

# the smallest shapes at which each part can go wrong
SHAPES = {
    "t1025": (3, 8, 1025),     # the minimum T: every 2048-point frame is mostly reflection, 3 frames
    "t2047": (1, 8, 2047),     # odd length, one short of a frame boundary
    "t6000": (2, 8, 6000),     # interior frames at all three resolutions
    "2d4096": (2, 4096),       # 2-D input
    "t44100": (2, 8, 44100),   # several workgroups: the number of partial sums
}
KINDS = ("near", "far")
TERMS = {"full": (1.0, 1.0), "sc": (1.0, 0.0), "log": (0.0, 1.0)}   # (sc_weight, log_weight)


def case_ids():
    return [f"{s}_{k}" for s in SHAPES for k in KINDS]


def make_xy(B, T, kind):
    """(B, 8, T) fp32 pair."""
    y = cases.pcm_batch(B, T)
    n = torch.randint(-2048, 2048, y.shape, generator=cases._g(5100), dtype=torch.int32).float() / 32768
    if kind == "near":
        x = 0.75 * y + 0.25 * torch.roll(y, 3, dims=2) + n / 32
    elif kind == "far":
        x = 0.5 * torch.roll(y, 1, dims=0).flip(1) + n / 8
    else:
        raise KeyError(kind)
    return x.contiguous(), y.contiguous()


def inputs(case):
    """(x, y) of a case id "<shape>_<kind>"."""
    sname, kind = case.rsplit("_", 1)
    shape = SHAPES[sname]
    if len(shape) == 2:   # (C, T): the first C channels of clip 0
        x, y = make_xy(1, shape[1], kind)
        return x[0, :shape[0]].contiguous(), y[0, :shape[0]].contiguous()
    return make_xy(shape[0], shape[2], kind)


def grad_samples(g):
    """The stored part of a gradient: the first 256 and last 256 samples of the first and of the last row (the reflected
    borders), and 1024 seeded positions anywhere, as one float64 vector."""
    g = np.asarray(g.detach().cpu().numpy() if hasattr(g, "detach") else g)
    g = g.reshape(-1, g.shape[-1])
    T = g.shape[1]
    edges = np.concatenate([g[r, :256] for r in (0, -1)] + [g[r, T - 256:] for r in (0, -1)])
    mid = g.reshape(-1)[cases.sample_idx(g.size, 1024, seed=21)]
    return np.concatenate([edges, mid])


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))
