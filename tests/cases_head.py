"""Seeded inputs, host references and comparison helpers of the edge-shape tests of the small training kernels
(tests/test_head_edges_gpu.py, tests/test_infonce_edges_gpu.py).  No kernel is called from here except `mst_dropout_mask`,
which makes the kernels' Dropout decisions explicit for the references.

References: the arithmetic of tests/test_head_gpu.py -- F.dropout -> AttentionPooling (src/model.py:118, :187-211) and
MixingFeatureEncoder's MLP (src/model.py:385-464) -- as torch functional ops on the CPU under autograd, evaluated twice: in
float64 (the yardstick) and in float32 (the reference's own fp32 result, which says how far ANY fp32 evaluation is from the
yardstick on these inputs)."""
import numpy as np
import torch
import torch.nn.functional as F

import parity
from cases_tcn import TwoTimesRule

HEAD_NAMES = ["d pool_in", "attention.0.weight", "attention.0.bias", "attention.2.weight", "attention.2.bias", "projection.0.weight",
              "projection.0.bias"]
FILM_NAMES = ["mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias", "film_head.weight", "film_head.bias"]


def _u(g, shape, scale):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def head_tensors(B, C, T, A, E, seed):
    """pool_in (a ReLU / max-pool output: non-negative with exact zeros), the six parameters in state_dict order at nn.Linear's
    init scale (attention.2.weight three times that: a peaky softmax, so that the scores matter) and the upstream gradient R."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, T, generator=g) * 0.7).relu_()
    ws = [_u(g, (A, C), C ** -0.5), _u(g, (A,), C ** -0.5), _u(g, (1, A), 3.0 * A ** -0.5), _u(g, (1,), A ** -0.5),
          _u(g, (E, C), C ** -0.5), _u(g, (E,), C ** -0.5)]
    R = torch.randn(B, E, generator=g)
    return x, ws, R


def film_tensors(B, Fd, H, O, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, Fd, generator=g) * 2.0
    ws = [_u(g, (H, Fd), Fd ** -0.5), _u(g, (H,), Fd ** -0.5), _u(g, (H, H), H ** -0.5), _u(g, (H,), H ** -0.5),
          _u(g, (O, H), H ** -0.5), _u(g, (O,), H ** -0.5)]
    R = torch.randn(B, O, generator=g)
    return f, ws, R


def next_seeds(n):
    """The seeds the autograd Functions will draw next (they take them from torch's CPU generator)."""
    st = torch.get_rng_state()
    out = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(n)]
    torch.set_rng_state(st)
    return out


def dropout_mask(p, seed, shape):
    """keep / (1 - p) of a Dropout(p) keyed by `seed`, float64 on the CPU; 1.0 without Dropout."""
    if p <= 0:
        return 1.0
    from mst_amd import _lib
    n = int(np.prod(shape))
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().mst_dropout_mask(float(p), int(seed), n, _lib.dptr(keep), _lib.stream_ptr(keep.device)), "mst_dropout_mask")
    return keep.view(*shape).cpu().double() / (1.0 - p)


def _cast(t, dtype):
    return t.to(dtype) if torch.is_tensor(t) else t


def head_reference(x, ws, R, m_in, m_out, dtype):
    """(embedding, [d pool_in, six parameter gradients]) of sum(embedding * R), on the CPU in `dtype`."""
    xl = x.detach().clone().to(dtype).requires_grad_(True)
    a0w, a0b, a2w, a2b, pw, pb = wl = [w.detach().clone().to(dtype).requires_grad_(True) for w in ws]
    xt = (xl * _cast(m_in, dtype)).transpose(1, 2)                       # (B, T, C)
    scores = F.linear(torch.tanh(F.linear(xt, a0w, a0b)), a2w, a2b)      # (B, T, 1)
    pooled = (xt * torch.softmax(scores, dim=1)).sum(dim=1)
    emb = torch.relu(F.linear(pooled, pw, pb)) * _cast(m_out, dtype)
    (emb * R.to(dtype)).sum().backward()
    return emb.detach(), [xl.grad] + [w.grad for w in wl]


def film_reference(f, ws, R, m, dtype):
    """(film, six parameter gradients, d feats) of sum(film * R), on the CPU in `dtype`."""
    fl = f.detach().clone().to(dtype).requires_grad_(True)
    w0, b0, w3, b3, wh, bh = wl = [w.detach().clone().to(dtype).requires_grad_(True) for w in ws]
    h1 = torch.relu(F.linear(fl, w0, b0)) * _cast(m, dtype)
    film = F.linear(torch.relu(F.linear(h1, w3, b3)), wh, bh)
    (film * R.to(dtype)).sum().backward()
    return film.detach(), [w.grad for w in wl], fl.grad


def normwise(got, ref64):
    a, r = got.detach().double().cpu(), ref64.detach().double().cpu()
    return (a - r).abs().max().item() / max(r.abs().max().item(), 1e-30)


class Checks:
    """One case's comparisons.  Every quantity goes through `cases_tcn.TwoTimesRule` (element-wise, against the fp32
    reference's own distance from float64 on the same elements; that also records both rows in the parity report) and has a
    norm-wise bar of its own.  Nothing asserts before `finish()`, so a failing case still prints every figure."""

    def __init__(self, family, case):
        self.family, self.case = family, case
        self.rule = TwoTimesRule(f"{family} {case}")
        self.rows, self.bad = [], []

    def add(self, name, got, ref32, ref64, bar, abs_floor=0.0):
        """bar: the norm-wise allowance, max|got - ref64| <= bar * max|ref64| + abs_floor."""
        got, ref32, ref64 = got.detach().cpu(), ref32.detach().cpu(), ref64.detach().cpu()
        assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
        assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
        self.rule.add(name, got, ref32, ref64)
        scale = ref64.abs().max().item()
        err = (got.double() - ref64).abs().max().item()
        self.rows.append((name, normwise(ref32, ref64), normwise(got, ref64), bar))
        if not err <= bar * scale + abs_floor:
            self.bad.append(f"{name}: max |d| {err:.3e} > {bar:.1e} * {scale:.3e} + {abs_floor:.0e}")

    def fail(self, msg):
        self.bad.append(msg)

    def finish(self):
        for name, nw32, nw, bar in self.rows:
            print(f"{self.family} {self.case} {name}: normwise ref fp32 {nw32:.3e}  under test {nw:.3e}  bar {bar:.1e}")
        if self.rows:
            parity.note(f"{self.family} {self.case} normwise", worst_of_bar=max(r[2] / r[3] for r in self.rows),
                        worst=max(r[2] for r in self.rows), worst_ref_fp32=max(r[1] for r in self.rows))
        try:
            self.rule.check()
        except AssertionError as e:
            self.bad.append(str(e))
        if self.rule.rows:
            e_ref = max(r[1] for r in self.rule.rows)
            parity.note(f"{self.family} {self.case} elementwise", worst_of_e_ref=max(r[2] for r in self.rule.rows) / max(e_ref, 1e-30),
                        allowed=2.0)
        assert not self.bad, "\n".join(self.bad)
