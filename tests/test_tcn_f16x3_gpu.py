"""GPU: the TCN mixer's opt-in split-precision inference (TCNMixer.precision = "f16x3", csrc/tcn_f16x3.inc:
tcn_conv_f16x3_kernel<NT, TT, SPLIT> on the f16 MFMA, tcn_split_kernel, tcn_absmax_kernel, tcn_f16x3_weights_kernel).

Yardstick and tolerance are those of the fp32 kernels, unchanged: the float64 evaluation of the reference (fixtures) or
of the `backend="torch"` tree on the host CPUs, and cases_tcn.TwoTimesRule -- every maximum relative error <= 2 x e_ref
(e_ref: the fp32 torch tree's own error on the same elements) and <= 1e-4 norm-wise.  Nothing is widened for the mode.
Bit-equality tests (per-clip scale, clip order, stale fragments, the way back to fp32) compare the kernels with
themselves."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import cases
import cases_tcn as ct
import cases_tcn_train as ctt
from mst_amd import _lib
from test_tcn_gpu import build, torch_forward

pytestmark = pytest.mark.gpu


def f16_forward(c, x, E=ct.EMBED, taps=(), film=None, sd=None, precision="f16x3"):
    """test_tcn_gpu.hip_forward with TCNMixer.precision set."""
    tcn, gen = build(c, E, sd=sd, generator=film is None)
    tcn.precision = precision
    with torch.no_grad():
        if gen is not None:
            film = gen.film_tensor(ct.embeddings(x.shape[0], E).cuda())
        elif film is not None:
            film = film.cuda().contiguous()
        y, hs = tcn._forward_hip(x.cuda(), film, tuple(taps))
    torch.cuda.synchronize()
    assert _lib.lib().mst_tcn_get_precision(tcn._hip.ptr) == (1 if precision == "f16x3" else 0)
    return y.cpu(), None if film is None else film.cpu(), [h.cpu() for h in hs]


def add_all(rule, tag, x, blocks, got, ref32, ref64):
    """y, y - x and the hidden taps of one run into a TwoTimesRule; got / ref32 / ref64 = (y, taps)."""
    x64 = x.double()
    (y, hs), (y32, h32), (y64, h64) = got, ref32, ref64
    rule.add(f"y{tag}", y.numpy(), y32.numpy(), y64.numpy())
    rule.add(f"y-x{tag}", (y.double() - x64).numpy(), (y32.double() - x64).numpy(), (y64 - x64).numpy())
    for k, h, a, b in zip(blocks, hs, h32, h64):
        rule.add(f"h{k}{tag}", h.numpy(), a.numpy(), b.numpy())


# ---- 1. fixtures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ct.CASES))
def test_fixture_case_f16x3(name):
    c, g = ct.CASES[name], np.load(ct.fixture_path(name))
    x = cases.pcm_batch(c["B"], c["T"])
    blocks = ct.tap_blocks(c)
    y, film, hs = f16_forward(c, x, taps=blocks)
    xs, hi = ct.flat_y(x), ct.hidden_idx(c)
    rule = ct.TwoTimesRule(f"f16x3 {name}")
    rule.add("y", ct.flat_y(y), ct.golden_y(g, 32), ct.golden_y(g, 64))
    rule.add("y-x", ct.flat_y(y) - xs, ct.golden_y(g, 32) - xs, ct.golden_y(g, 64) - xs)
    for k, h in zip(blocks, hs):
        rule.add(f"h{k}", h.reshape(-1)[hi].numpy(), g[f"h{k}_32"], g[f"h{k}_64"])
    if c["film"]:
        rule.add("film", film.numpy(), g["film32"], g["film64"])
    rule.check()


# ---- 2. widths and lengths ---------------------------------------------------------------------------------------------
# H = 16 n: every output-tile count NT = 1..8 and every 32-channel chunk count 1..4 (odd NT: the upper half of the last
# chunk is padding); H in {1, 17, 40, 100}: padding in the 16 and the 32 granularity; K in {1, 15}; both paddings; both
# block types; 2 blocks, and 16 blocks with dilations far beyond the clip.
GEOMETRIES = {
    "w16": dict(H=16, nb=2, K=15, causal=False, film=True),
    "w32": dict(H=32, nb=2, K=15, causal=True, film=False),
    "w48": dict(H=48, nb=2, K=1, causal=False, film=True),
    "w64": dict(H=64, nb=2, K=15, causal=True, film=True),
    "w80": dict(H=80, nb=2, K=15, causal=False, film=False),
    "w96": dict(H=96, nb=2, K=15, causal=True, film=False),
    "w112": dict(H=112, nb=2, K=1, causal=True, film=True),
    "w128": dict(H=128, nb=2, K=15, causal=False, film=True),
    "h1": dict(H=1, nb=2, K=15, causal=False, film=False),
    "h17": dict(H=17, nb=2, K=15, causal=True, film=True),
    "h40": dict(H=40, nb=2, K=1, causal=False, film=False),
    "h100": dict(H=100, nb=2, K=15, causal=False, film=True),
    "deep16": dict(H=16, nb=16, K=15, causal=False, film=True),
}
LENGTHS = (1, 15, 16, 17, 64, 65, 1000)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_width_and_length_sweep_f16x3(name):
    """One rule per geometry over all lengths, as test_tcn_widths_gpu.test_width_and_length_sweep."""
    geo = GEOMETRIES[name]
    rule = ct.TwoTimesRule(f"f16x3 widths {name}", report="summary")
    for T in LENGTHS:
        c = dict(geo, B=2, T=T)
        x = cases.pcm_batch(2, T)
        film = ctt.film_tensor(c) if c["film"] else None
        blocks = ct.tap_blocks(c)
        y, _, hs = f16_forward(c, x, taps=blocks, film=film)
        y32, _, h32 = torch_forward(c, x, torch.float32, taps=blocks, film=film)
        y64, _, h64 = torch_forward(c, x, torch.float64, taps=blocks, film=film)
        add_all(rule, f" 2x{T}", x, blocks, (y, hs), (y32, h32), (y64, h64))
    rule.check()


# ---- 3. far dilations --------------------------------------------------------------------------------------------------
def test_far_dilations_f16x3():
    """st_default, 1 x 120 000 (> 114 688): all 15 taps of the d = 8192 block lie inside the clip.  Every element."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    c, T = ct.CASES["st_default"], 120000
    x = cases.pcm_batch(1, T)
    blocks = ct.tap_blocks(c)
    y, film, hs = f16_forward(c, x, taps=blocks)
    y32, film32, h32 = torch_forward(c, x, torch.float32, taps=blocks)
    y64, film64, h64 = torch_forward(c, x, torch.float64, taps=blocks)
    rule = ct.TwoTimesRule(f"f16x3 st_default 1x{T}")
    add_all(rule, "", x, blocks, (y, hs), (y32, h32), (y64, h64))
    rule.add("film", film.numpy(), film32.numpy(), film64.numpy())
    rule.check()


# ---- 4. range ----------------------------------------------------------------------------------------------------------
RANGE_CASE = dict(H=40, nb=4, K=15, causal=False, film=True, B=4, T=3000)


def test_range_scale_is_per_clip():
    """A full-scale clip, the same clip x 2^-14 and x 2^6, and an all-zero clip in one batch: each clip's result has the
    bits of that clip run alone (its scale is its own), and each is inside the rule against its own float64 result."""
    c = RANGE_CASE
    x0 = cases.pcm_batch(1, c["T"])[0]
    x = torch.stack([x0, x0 * 2.0 ** -14, x0 * 2.0 ** 6, torch.zeros_like(x0)])
    film = ctt.film_tensor(c)
    blocks = ct.tap_blocks(c)
    y, _, hs = f16_forward(c, x, taps=blocks, film=film)
    assert torch.isfinite(y).all()
    y32, _, h32 = torch_forward(c, x, torch.float32, taps=blocks, film=film)
    y64, _, h64 = torch_forward(c, x, torch.float64, taps=blocks, film=film)
    for b, tag in enumerate(("full scale", "x 2^-14", "x 2^6", "zeros")):
        s = slice(b, b + 1)
        ya, _, ha = f16_forward(dict(c, B=1), x[s], taps=blocks, film=film[s])
        assert torch.equal(ya, y[s]) and all(torch.equal(p, q[s]) for p, q in zip(ha, hs)), f"clip {b} ({tag}) depends on its batch"
        rule = ct.TwoTimesRule(f"f16x3 range {tag}", report="summary")
        add_all(rule, "", x[s], blocks, (y[s], [h[s] for h in hs]), (y32[s], [h[s] for h in h32]), (y64[s], [h[s] for h in h64]))
        rule.check()


# ---- 5. filters --------------------------------------------------------------------------------------------------------
def test_filter_rows_zero_tiny_and_large():
    """One output channel's filter all zero, one scaled by 2^-20 and one by 2^12, in both convolutions of a block."""
    c = dict(H=40, nb=3, K=15, causal=False, film=True, B=2, T=2000)
    sd = ct.make_tcn_state_dict(c)
    for l, (zero, tiny, large) in ((1, (3, 17, 38)), (2, (0, 21, 33))):
        w = sd[f"blocks.1.conv{l}.conv.weight"]
        w[zero] = 0.0
        w[tiny] *= 2.0 ** -20
        w[large] *= 2.0 ** 12
    x = cases.pcm_batch(c["B"], c["T"])
    film = ctt.film_tensor(c)
    blocks = ct.tap_blocks(c)
    y, _, hs = f16_forward(c, x, taps=blocks, film=film, sd=sd)
    assert torch.isfinite(y).all() and all(torch.isfinite(h).all() for h in hs)
    y32, _, h32 = torch_forward(c, x, torch.float32, taps=blocks, film=film, sd=sd)
    y64, _, h64 = torch_forward(c, x, torch.float64, taps=blocks, film=film, sd=sd)
    rule = ct.TwoTimesRule("f16x3 filter rows", report="summary")
    add_all(rule, "", x, blocks, (y, hs), (y32, h32), (y64, h64))
    rule.check()


# ---- 6. bits -----------------------------------------------------------------------------------------------------------
def test_bit_reproducible_and_clip_order():
    c = dict(H=72, nb=4, K=15, causal=False, film=True, B=3, T=2500)
    x = cases.pcm_batch(3, c["T"]) * torch.tensor([1.0, 0.125, 3.0]).view(3, 1, 1)
    film = ctt.film_tensor(c)
    y, _, hs = f16_forward(c, x, taps=(0, 3), film=film)
    y2, _, hs2 = f16_forward(c, x, taps=(0, 3), film=film)
    assert torch.equal(y, y2) and all(torch.equal(p, q) for p, q in zip(hs, hs2)), "two runs differ"
    for order in ([2, 1, 0], [1, 2, 0]):
        yp, _, hp = f16_forward(c, x[order], taps=(0, 3), film=film[order])
        assert torch.equal(yp, y[order]) and all(torch.equal(p, q[order]) for p, q in zip(hp, hs)), f"clip order {order} changed bits"


# ---- 7. stale fragments ------------------------------------------------------------------------------------------------
def test_fragments_follow_load_state_dict():
    c = ct.CASES["loader_default"]
    x = cases.pcm_batch(1, 9000).cuda()
    tcn, gen = build(c)
    tcn.precision = "f16x3"
    with torch.no_grad():
        params = gen(ct.embeddings(1, ct.EMBED).cuda())
        y0 = tcn(x, film_params=params)
        tcn.load_state_dict(ct.make_tcn_state_dict(c, seed=4201), strict=True)
        y1 = tcn(x, film_params=params)
        fresh, _ = build(c, sd=ct.make_tcn_state_dict(c, seed=4201))
        fresh.precision = "f16x3"
        assert not torch.equal(y1, y0) and torch.equal(fresh(x, film_params=params), y1)
        assert _lib.lib().mst_tcn_get_precision(tcn._hip.ptr) == 1


def test_fragments_follow_update_params():
    """C level: mst_tcn_update_params on a handle in the mode, then mst_tcn_forward, equals a fresh handle's result."""
    c = dict(H=40, nb=3, K=15, causal=False, film=True, B=2, T=1500)
    x = cases.pcm_batch(2, c["T"]).cuda()
    film = ctt.film_tensor(c).cuda()
    tcn, _ = build(c, generator=False)
    tcn.precision = "f16x3"
    new, _ = build(c, sd=ct.make_tcn_state_dict(c, seed=4201), generator=False)
    new.precision = "f16x3"
    with torch.no_grad():
        y0, _ = tcn._forward_hip(x, film)
        h = tcn._hip
        cat = lambda f: torch.stack([f(b, l).detach() for b in new.blocks for l in (1, 2)]).contiguous()  # noqa: E731
        keep = [new.input_conv.weight.detach(), new.input_conv.bias.detach(),
                cat(lambda b, l: getattr(b, f"conv{l}").conv.weight), cat(lambda b, l: getattr(b, f"conv{l}").conv.bias),
                cat(lambda b, l: getattr(b, f"norm{l}").weight), cat(lambda b, l: getattr(b, f"norm{l}").bias),
                cat(lambda b, l: getattr(b, f"norm{l}").running_mean), cat(lambda b, l: getattr(b, f"norm{l}").running_var),
                new.output_conv.weight.detach(), new.output_conv.bias.detach()]
        w = _lib.TcnWeights(*[C.c_void_p(t.data_ptr()) for t in keep])
        dev = x.device
        _lib.check(_lib.lib().mst_tcn_update_params(h.ptr, C.byref(w), _lib.stream_ptr(dev)), "mst_tcn_update_params")
        y1, _ = tcn._forward_hip(x, film, handle=h)
        y_new, _ = new._forward_hip(x, film)
    assert _lib.lib().mst_tcn_get_precision(h.ptr) == 1
    assert not torch.equal(y1, y0) and torch.equal(y1, y_new)


# ---- 8. default path untouched -----------------------------------------------------------------------------------------
def test_switching_back_gives_the_fp32_bits():
    c = ct.CASES["plain64"]
    x = cases.pcm_batch(1, 5000).cuda()
    tcn, _ = build(c)
    never, _ = build(c)
    L = _lib.lib()
    with torch.no_grad():
        y_fp32 = never(x)
        tcn.precision = "f16x3"
        y_f16 = tcn(x)
        h = tcn._hip
        assert L.mst_tcn_get_precision(h.ptr) == 1 and L.mst_tcn_get_precision(never._hip.ptr) == 0
        assert not torch.equal(y_f16, y_fp32)   # the mode ran other arithmetic
        small, big = (L.mst_tcn_workspace_bytes(q.ptr, 1, 5000) for q in (never._hip, h))
        assert big == small + 2 * 5000 * 64 * 2 + 256   # two f16 planes [T][HP32] and the absmax array
        tcn.precision = "fp32"
        assert torch.equal(tcn(x), y_fp32) and tcn._hip is h and L.mst_tcn_get_precision(h.ptr) == 0
    assert L.mst_tcn_set_precision(h.ptr, 2, None) != 0 and b"unknown mode" in L.mst_last_error()
    assert L.mst_tcn_get_precision(h.ptr) == 0


# ---- 9. example --------------------------------------------------------------------------------------------------------
def test_example_tcn_precision_flag():
    spec = importlib.util.spec_from_file_location("style_transfer_example", os.path.join(cases.ROOT, "examples", "style_transfer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--seconds", "1", "--tcn-precision", "f16x3"])
    ref = mod.main(["--seconds", "1"])
    assert torch.isfinite(out["processed_mixture"]).all()
    d = float((out["processed_mixture"] - ref["processed_mixture"]).abs().max()) / float(ref["processed_mixture"].abs().max())
    assert d <= 1e-4, d
