"""Seeded cases, state dicts and comparison helpers of the TCN mixer tests (data only, no reference code).

Everything random is built from torch.rand / torch.randint (integer draws scaled by powers of two or one IEEE division),
so the inputs and weights are bit-identical on every machine."""
import math
import os

import numpy as np
import torch

import cases

GOLDEN = os.path.join(cases.ROOT, "tests", "golden")

# name -> geometry.  B x T as run on the CPU with the reference when the fixture was written.
CASES = {
    "st_default": dict(H=16, nb=14, K=15, causal=False, film=True, B=2, T=40000),      # train_style_transfer.py defaults
    "loader_default": dict(H=16, nb=8, K=5, causal=False, film=True, B=2, T=20011),    # inference_e2e fallbacks, odd T
    "causal": dict(H=16, nb=14, K=15, causal=True, film=True, B=2, T=40000),
    "plain64": dict(H=64, nb=10, K=15, causal=False, film=False, B=2, T=20000),
    "wide128": dict(H=128, nb=14, K=15, causal=False, film=True, B=1, T=20000),        # class defaults
    "h8": dict(H=8, nb=14, K=15, causal=False, film=False, B=1, T=20000),              # create_tcn_mixer() default
}
EMBED = 1024          # 2 x embed_dim of the train_baseline.sh encoder
EMBED_WIDE = 1536     # 2 x the default encoder's, stored once (st_default)


def fixture_path(name):
    return os.path.join(GOLDEN, f"tcn_{name}.npz")


def mixer_kwargs(c):
    return dict(in_channels=8, hidden_channels=c["H"], num_blocks=c["nb"], kernel_size=c["K"], causal=c["causal"],
                use_film=c["film"])


def tap_blocks(c):
    return sorted({0, c["nb"] // 2, c["nb"] - 1})


def _u(g, shape, scale):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def make_tcn_state_dict(c, seed=4200):
    """Trained-looking TCNMixer state dict: non-trivial BN statistics, conv weights uniform +-1/sqrt(fan_in), and the
    OUTPUT conv at that scale too (at its 0.001 init y - x would be ~1e-3 and every comparison of y would pass on x)."""
    g = cases._g(seed)
    H, K = c["H"], c["K"]
    sd = {"input_conv.weight": _u(g, (H, 8, 1), 1 / math.sqrt(8)), "input_conv.bias": _u(g, (H,), 0.05)}
    for i in range(c["nb"]):
        for l in (1, 2):
            sd[f"blocks.{i}.conv{l}.conv.weight"] = _u(g, (H, H, K), 1 / math.sqrt(H * K))
            sd[f"blocks.{i}.conv{l}.conv.bias"] = _u(g, (H,), 0.05)
        for l in (1, 2):
            p = f"blocks.{i}.norm{l}."
            sd[p + "weight"] = 0.5 + torch.rand((H,), generator=g)
            sd[p + "bias"] = _u(g, (H,), 0.15)
            sd[p + "running_mean"] = _u(g, (H,), 0.15)
            sd[p + "running_var"] = 0.5 + torch.rand((H,), generator=g)
            sd[p + "num_batches_tracked"] = torch.tensor(100, dtype=torch.long)
    sd["output_conv.weight"] = _u(g, (8, H, 1), 1 / math.sqrt(H))
    sd["output_conv.bias"] = _u(g, (8,), 0.05)
    return sd


def make_film_state_dict(E, c, seed=4300):
    """TCNFiLMGenerator state dict at trained scale, the gamma biases shifted by +1."""
    g = cases._g(seed)
    nb, H = c["nb"], c["H"]
    sd = {}
    for k, (o, i) in (("0", (512, E)), ("3", (512, 512)), ("6", (nb * 4 * H, 512))):
        sd[f"mlp.{k}.weight"] = _u(g, (o, i), 1 / math.sqrt(i))
        sd[f"mlp.{k}.bias"] = _u(g, (o,), 0.05)
    b = sd["mlp.6.bias"].view(nb, 4, H)
    b[:, 0] += 1.0
    b[:, 2] += 1.0
    return sd


def embeddings(B, E, seed=4400):
    """(B, E) concatenated embeddings of about unit norm per half, integer-built."""
    n = torch.randint(-2048, 2048, (B, E), generator=cases._g(seed), dtype=torch.int32)
    return n.float() / 32768.0


def y_samples(y, c=None):
    """The compared part of a (B, 8, T) result: the first 512 and last 512 samples of every channel, (B, 8, 1024), and 4096
    seeded positions of the interior (B, 8, T - 1024), flat."""
    B, _, T = y.shape
    edges = torch.cat([y[:, :, :512], y[:, :, T - 512:]], dim=2)
    mid = y[:, :, 512:T - 512].reshape(-1)[cases.sample_idx(B * 8 * (T - 1024), 4096, seed=11)]
    return edges, mid


def flat_y(y):
    """y_samples as one float64 vector (the order of golden_y)."""
    e, m = y_samples(y.detach().cpu())
    return np.concatenate([e.double().numpy().ravel(), m.double().numpy().ravel()])


def golden_y(g, bits):
    return np.concatenate([g[f"ye{bits}"].astype(np.float64).ravel(), g[f"ym{bits}"].astype(np.float64).ravel()])


def hidden_idx(c, T=None, B=None):
    """2048 seeded flat positions of a (B, H, T) hidden state."""
    return cases.sample_idx((B or c["B"]) * c["H"] * (T or c["T"]), 2048, seed=12)


def max_rel(got, ref64, floor_frac=1e-2):
    """max |got - ref| / max(|ref|, floor_frac * max|ref|) and max|d| / max|ref| (the floor of tests/parity.py)."""
    a = np.asarray(got, dtype=np.float64).ravel()
    r = np.asarray(ref64, dtype=np.float64).ravel()
    d = np.abs(a - r)
    scale = float(np.abs(r).max())
    return float((d / np.maximum(np.abs(r), max(floor_frac * scale, 1e-30))).max()), float(d.max() / max(scale, 1e-30))


class TwoTimesRule:
    """The tolerance of the TCN tests.  For every compared quantity, the maximum relative error against the float64
    yardstick is taken for the reference's own fp32 result and for the result under test, on the same elements.  e_ref is
    the largest of the reference's maxima over the case's quantities; every maximum of the result under test must stay
    within 2 * e_ref (the rule of the log-mel and real-music tests), and norm-wise within 1e-4."""

    def __init__(self, case, report=True):
        # report: rows in the parity table of the GPU log; "summary": the case's e_ref / worst line only (a sweep with
        # dozens of quantities per case)
        self.case, self.rows, self.report = case, [], report

    def add(self, name, got, ref32, ref64):
        import parity
        if self.report is True:
            parity.record(f"tcn {self.case} {name} [ref fp32 vs f64]", ref32, ref64)
            parity.record(f"tcn {self.case} {name} [hip vs f64]", got, ref64)
        self.rows.append((name, max_rel(ref32, ref64)[0], *max_rel(got, ref64)))

    def check(self):
        import parity
        e_ref = max(r[1] for r in self.rows)
        if self.report:
            parity.note(f"tcn {self.case} 2x rule", e_ref=e_ref, worst=max(r[2] for r in self.rows),
                        worst_normwise=max(r[3] for r in self.rows))
        for name, e32, e, nw in self.rows:
            print(f"tcn {self.case} {name}: ref fp32 {e32:.3e}  under test {e:.3e}  normwise {nw:.3e}  (e_ref {e_ref:.3e})")
        bad = [(n, e, nw) for n, _, e, nw in self.rows if not (e <= 2 * e_ref and nw <= 1e-4)]
        assert not bad, f"{self.case}: beyond 2 x e_ref = {2 * e_ref:.3e} or 1e-4 norm-wise: {bad}"
