"""Shared by tests/test_tcn_film_train_gpu.py and tests/golden/make_golden_tcn_film_train.py: seeded weights and inputs of a
TCNFiLMGenerator, the module tree with the two Dropout masks imposed, and the parity rule of the generator's training kernels.

The rule, per quantity group (film, demb, each of the six parameter gradients): with e_ref the largest floored relative error
|d| / max(|ref64|, 0.01 max|ref64|) of the SAME tree in fp32 against float64, every element of the result under test is at most
2 e_ref max(|ref64|, 0.01 max|ref64|) + 1e-7 max|ref64| from float64 (fp32 against float64 can be exactly 0 on a small group)."""
import numpy as np
import torch

PARAMS = ("mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias", "mlp.6.weight", "mlp.6.bias")
GROUPS = ("film", "demb") + PARAMS
FIXTURE = dict(B=5, embed_dim=40, nb=3, H=8, seed=20250311)
MLP_HIDDEN = 512     # fixed by the reference's constructor
W3_SAMPLES = 512     # stored positions of the 512 x 512 gradient of mlp.3.weight


def make_inputs(B, embed_dim, nb, H, seed, std=0.05):
    """{state_dict key: fp32 tensor} (weights N(0, std), biases N(0, std): the module's own 0.01 / zero initialisation leaves film
    near zero), the embedding (B, embed_dim) and the cotangent R (B, nb, 4, H) of loss = sum(film * R)."""
    rng = np.random.default_rng(seed)
    out_dim = nb * 4 * H
    shapes = {"mlp.0.weight": (MLP_HIDDEN, embed_dim), "mlp.0.bias": (MLP_HIDDEN,), "mlp.3.weight": (MLP_HIDDEN, MLP_HIDDEN),
              "mlp.3.bias": (MLP_HIDDEN,), "mlp.6.weight": (out_dim, MLP_HIDDEN), "mlp.6.bias": (out_dim,)}
    sd = {k: torch.from_numpy((rng.standard_normal(s) * std).astype(np.float32)) for k, s in shapes.items()}
    emb = torch.from_numpy(rng.standard_normal((B, embed_dim)).astype(np.float32))
    R = torch.from_numpy(rng.standard_normal((B, nb, 4, H)).astype(np.float32))
    return sd, emb, R


def w3_positions():
    return np.random.default_rng(FIXTURE["seed"] + 1).choice(MLP_HIDDEN * MLP_HIDDEN, size=W3_SAMPLES, replace=False).astype(np.int64)


def run_tree(gen, emb, R, m1=None, m2=None):
    """Forward + backward of sum(film * R) through a generator's `mlp` with the Dropout modules replaced by the given scaled keep
    masks ((B, mlp_hidden), entries 0 or 1 / (1 - p); None = no Dropout).  `gen` is this project's module with backend='torch' or
    the reference's; dtype and device are the module's.  Returns {group: float64 numpy array}."""
    mlp = gen.mlp
    p = next(gen.parameters())
    for q in gen.parameters():
        q.grad = None
    x = emb.detach().to(p.device, p.dtype).clone().requires_grad_(True)
    h1 = mlp[1](mlp[0](x))
    h1 = h1 if m1 is None else h1 * m1.to(p.device, p.dtype)
    h2 = mlp[4](mlp[3](h1))
    h2 = h2 if m2 is None else h2 * m2.to(p.device, p.dtype)
    film = mlp[6](h2)
    (film * R.to(p.device, p.dtype).reshape(film.shape)).sum().backward()
    out = {"film": film.detach(), "demb": x.grad}
    out.update({k: q.grad for k, q in gen.named_parameters()})
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def floored(ref64):
    r = np.abs(np.asarray(ref64, dtype=np.float64))
    return np.maximum(r, max(0.01 * float(r.max()), 1e-300))


def rel_err(got, ref64):
    """max |got - ref64| / max(|ref64|, 0.01 max|ref64|)."""
    r = np.asarray(ref64, dtype=np.float64).ravel()
    return float((np.abs(np.asarray(got, dtype=np.float64).ravel() - r) / floored(r)).max())


def check_rule(tag, got, ref32, ref64, groups=GROUPS):
    """Prints kernels / e_ref per group and returns the groups that break the rule."""
    bad = []
    for k in groups:
        g, r32, r64 = (np.asarray(t[k], dtype=np.float64).ravel() for t in (got, ref32, ref64))
        e_ref, e = rel_err(r32, r64), rel_err(g, r64)
        bound = 2.0 * e_ref * floored(r64) + 1e-7 * float(np.abs(r64).max())
        worst = float((np.abs(g - r64) / bound).max()) if bound.min() > 0 else float("inf") if np.abs(g - r64).max() > 0 else 0.0
        print(f"{tag} {k}: kernels {e:.3e}  e_ref {e_ref:.3e}  kernels / e_ref {e / max(e_ref, 1e-30):.2f}  worst |d| / bound {worst:.3f}")
        if not worst <= 1.0:
            bad.append((k, e, e_ref, worst))
    return bad
