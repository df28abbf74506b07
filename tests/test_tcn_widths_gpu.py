"""GPU: every channel-tile instantiation of tcn_conv_kernel<NT, TT, SPLIT> (csrc/tcn.hip) in inference, and the clip
lengths around its time tiles.

NT = ceil(H / 16) selects the instantiation: NT 1, 2 -> TT 8; NT 3, 4 -> TT 4; NT 5..8 -> TT 4, SPLIT 2, where an odd NT
(5, 7: H in 65..80, 97..112) takes the ODD path -- the second half of the output channels has one tile fewer.  A wave's
time tile is 16 TT = 128 or 64 samples, a workgroup's 512, 256 or 128.

test_width_and_length_sweep: yardstick the float64 `backend="torch"` tree on the host CPUs (pinned to the reference by
tests/test_tcn_cpu.py), tolerance cases_tcn.TwoTimesRule with ONE rule per geometry over all lengths, so that e_ref is the
fp32 torch tree's error over several thousand elements and not over the 16 outputs of a T = 1 run.  Every element of y,
y - x and the hidden taps is compared.  The FiLM tensor is given directly (cases_tcn_train.film_tensor).  Measured e_ref:
4.6e-6 (h1), 1.1e-5 (w24) ... 2.9e-5 (w100); the kernels' worst 0.55 ... 1.09 of it (DESIGN 3.6 has the table).

test_zero_extended_mixer_gives_the_same_bits: a 12-channel mixer padded with zero channels to H' = 16 .. 128 runs on each
of the eight instantiations, its 12 channels in each of the H' / 16 tiles in turn, and must give the bits of the
12-channel one.  (With the channels in the first tile alone, every other tile's weights are zeros and a wrong value there
goes unseen.)  Derived from the code: a tap's partial sum is
one fmaf chain over the input channels in the same order for every NT, appended channels add exact zeros, `acc += part`
happens once per tap, the epilogue and the 1x1 kernels loop over HP with zeros appended; TT, SPLIT, EDGE and ODD change
which lane computes an element, not how."""
import pytest
import torch

import cases
import cases_tcn as ct
import cases_tcn_train as ctt
from test_tcn_gpu import hip_forward, torch_forward

pytestmark = pytest.mark.gpu

GEOMETRIES = {
    "w24": dict(H=24, nb=3, K=7, causal=False, film=True),       # NT = 2 with 8 padded channels
    "w32": dict(H=32, nb=3, K=6, causal=True, film=False),       # NT = 2 exact, even kernel, plain block
    "w48": dict(H=48, nb=3, K=15, causal=False, film=True),      # NT = 3
    "w72": dict(H=72, nb=3, K=15, causal=False, film=True),      # NT = 5: ODD, padded
    "w80": dict(H=80, nb=2, K=4, causal=True, film=False),       # NT = 5: ODD, exact, causal
    "w96": dict(H=96, nb=3, K=9, causal=False, film=True),       # NT = 6
    "w100": dict(H=100, nb=3, K=15, causal=False, film=False),   # NT = 7: ODD, 12 padded channels
    "w112": dict(H=112, nb=2, K=1, causal=False, film=True),     # NT = 7: ODD, exact, K = 1 (off0 = 0)
    "h1": dict(H=1, nb=1, K=3, causal=False, film=False),        # one channel, one block
    "deep16": dict(H=16, nb=16, K=15, causal=False, film=True),  # dilations up to 32768 >> T
    "deep16c": dict(H=16, nb=16, K=2, causal=True, film=True),   # the same, one-sided
}
# one sample below and above the 64- and 128-sample wave tiles; one above the 128-, 256- and 512-sample workgroup tiles;
# 1100: interior strips, so that the clamp-free path of NT <= 2 runs too
LENGTHS = (1, 63, 65, 127, 129, 257, 513, 1100)
EXTRA = {"w72": [(3, 257)]}   # blockIdx.y offsets of a third clip
FIRST_FAR_BLOCK = 11          # dilation 2048 > max(LENGTHS): every tap but one lies wholly outside the clip


def one_tap_state_dict(c):
    """The seeded state dict with, in blocks FIRST_FAR_BLOCK.., every tap zeroed except the one that can reach the clip at
    T <= 1100: the centre tap (non-causal) or the last (causal)."""
    assert 2 ** FIRST_FAR_BLOCK > max(LENGTHS)
    sd = ct.make_tcn_state_dict(c)
    keep = c["K"] - 1 if c["causal"] else (c["K"] - 1) // 2
    for i in range(FIRST_FAR_BLOCK, c["nb"]):
        for l in (1, 2):
            w = sd[f"blocks.{i}.conv{l}.conv.weight"]
            kept = w[:, :, keep].clone()
            w.zero_()
            w[:, :, keep] = kept
    return sd


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_width_and_length_sweep(name):
    geo = GEOMETRIES[name]
    rule = ct.TwoTimesRule(f"widths {name}", report="summary")
    for B, T in [(2, T) for T in LENGTHS] + EXTRA.get(name, []):
        c = dict(geo, B=B, T=T)
        x = cases.pcm_batch(B, T)
        film = ctt.film_tensor(c) if c["film"] else None
        blocks = ct.tap_blocks(c)
        y, _, hs = hip_forward(c, x, taps=blocks, film=film)
        y32, _, h32 = torch_forward(c, x, torch.float32, taps=blocks, film=film)
        y64, _, h64 = torch_forward(c, x, torch.float64, taps=blocks, film=film)
        x64 = x.double()
        tag = f"{B}x{T}"
        rule.add(f"y {tag}", y.numpy(), y32.numpy(), y64.numpy())
        rule.add(f"y-x {tag}", (y.double() - x64).numpy(), (y32.double() - x64).numpy(), (y64 - x64).numpy())
        for k, h, a, b in zip(blocks, hs, h32, h64):
            rule.add(f"h{k} {tag}", h.numpy(), a.numpy(), b.numpy())
        if c["nb"] > FIRST_FAR_BLOCK:
            y1, _, h1 = hip_forward(c, x, taps=blocks, film=film, sd=one_tap_state_dict(c))
            assert torch.equal(y1, y) and all(torch.equal(p, q) for p, q in zip(h1, hs)), \
                f"{name} {tag}: taps wholly outside the clip changed the result"
    rule.check()


# ---- zero-extended mixer -----------------------------------------------------------------------------------------------
BASE_H, BASE_B, BASE_T = 12, 2, 700
VARIANTS = {
    "film": dict(H=BASE_H, nb=4, K=15, causal=False, film=True, B=BASE_B, T=BASE_T),
    "plain": dict(H=BASE_H, nb=4, K=15, causal=False, film=False, B=BASE_B, T=BASE_T),
    "causal4": dict(H=BASE_H, nb=4, K=4, causal=True, film=True, B=BASE_B, T=BASE_T),
}
WIDE = (16, 32, 48, 64, 80, 96, 112, 128)   # NT = 1 .. 8


def zero_extended(sd, H, H2, at=0):
    """The state dict of the H2-channel mixer that computes what `sd`'s H-channel one does in its channels at .. at + H:
    every other conv weight, bias, BN bias / mean and input / output projection entry 0, BN weight / variance 1."""
    out = {}
    for k, v in sd.items():
        if v.dim() == 0:
            out[k] = v.clone()
            continue
        one = k.endswith(("norm1.weight", "norm2.weight", "running_var"))
        shape = tuple(H2 if n == H else n for n in v.shape)
        w = (torch.ones if one else torch.zeros)(shape, dtype=v.dtype)
        w[tuple(slice(at, at + H) if n == H else slice(0, n) for n in v.shape)] = v
        out[k] = w
    return out


_BASE = {}


def base_run(variant):
    if variant not in _BASE:
        c = VARIANTS[variant]
        x = cases.pcm_batch(c["B"], c["T"])
        film = ctt.film_tensor(c) if c["film"] else None
        y, _, hs = hip_forward(c, x, taps=range(c["nb"]), film=film)
        _BASE[variant] = (x, film, y, hs)
    return _BASE[variant]


@pytest.mark.parametrize("H2", WIDE)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_zero_extended_mixer_gives_the_same_bits(variant, H2):
    """The 12 channels sit at the start of each of the H' / 16 channel tiles in turn.  At the start of the first tile all
    other channels are appended; in a later tile they are also the only non-zero entries of that tile's weights, so that
    every output tile of every instantiation (the last one of the shorter half of an odd NT among them) carries values.
    A shift by a multiple of 16 keeps every MFMA's operands: lane group g supplies input channels 16 chunk + 4 g + s, and
    the chunks before add fma(0, 0, 0) to a partial sum that is still zero."""
    c = VARIANTS[variant]
    H = c["H"]
    assert H not in (1, 8, c["K"]) and H < min(WIDE)   # zero_extended tells the hidden axes from the 8 stem channels by their length
    x, film, y0, hs0 = base_run(variant)
    c2 = dict(c, H=H2)
    bad = []
    for at in range(0, H2, 16):
        film2 = None
        if film is not None:
            film2 = torch.zeros(c["B"], c["nb"], 4, H2)
            film2[..., at:at + H] = film
        y, _, hs = hip_forward(c2, x, taps=range(c["nb"]), film=film2, sd=zero_extended(ct.make_tcn_state_dict(c), H, H2, at))
        differing = [f"h{k}" for k, (h, h0) in enumerate(zip(hs, hs0)) if not torch.equal(h[:, at:at + H], h0)]
        nonzero = [f"h{k}" for k, h in enumerate(hs) if bool((h[:, :at] != 0).any() or (h[:, at + H:] != 0).any())]
        if not torch.equal(y, y0):
            differing.append("y")
        if differing or nonzero:
            bad.append(f"channels at {at}: {differing} differ from the {H}-channel mixer's; other channels not zero in {nonzero}")
    assert not bad, f"{variant} H' = {H2}: {bad}"
