"""GPU: block-wise streaming of a causal TCN mixer (csrc/tcn_stream.inc, mst_tcn_stream_*, TCNMixer.stream).

The acceptance criterion needs no tolerance: with zero-initialised history the pushes concatenated are the offline
`mixer(x, film)` result BIT FOR BIT, whatever the block sizes.  Every output element is the same chain in both kernels (per
tap a partial sum in channel order, `acc += part` once per tap, the folded epilogue), whichever lane or tile computes it,
and the history before the stream's start is stored zeros where the offline kernel selects zeros or skips the tap."""
import numpy as np
import pytest
import torch

import cases
import cases_tcn as ct
import cases_tcn_stream as cs
import cases_tcn_train as ctt
from mst_amd import _lib

pytestmark = pytest.mark.gpu

# H, blocks, K, FiLM: one geometry per channel-tile instantiation NT = ceil(H / 16) of the convolution kernel
GEOMETRIES = {1: (1, 1, 2, False), 16: (16, 3, 15, True), 24: (24, 3, 4, False), 48: (48, 3, 15, True), 64: (64, 2, 6, False),
              72: (72, 3, 15, True), 96: (96, 2, 9, True), 100: (100, 3, 15, False), 128: (128, 2, 15, True)}
SMALL = cs.case(16, 3, 15, True)
DEEP = dict(ct.CASES["causal"])
_cache = {}


def offline(H):
    """(case, mixer, film, x, offline y) of a geometry, computed once."""
    if H not in _cache:
        c = cs.case(*GEOMETRIES[H])
        m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(c["B"], c["T"]).cuda()
        with torch.no_grad():
            _cache[H] = (c, m, film, x, m(x, film_params=film))
    return _cache[H]


@pytest.mark.parametrize("sched", ["a", "b", "c"])
@pytest.mark.parametrize("H", list(GEOMETRIES))
def test_bit_equal_to_offline_every_instantiation(H, sched):
    c, m, film, x, want = offline(H)
    sizes = cs.schedule(sched, c["T"])
    with torch.no_grad():
        got = cs.run(m.stream(batch_size=c["B"], max_block=max(sizes), film_params=film), x, sizes)
    assert torch.equal(got, want), f"max |d| = {float((got - want).abs().max()):.3e}"
    assert float((want - x).abs().max()) > 1e-2


@pytest.mark.parametrize("H", list(GEOMETRIES))
def test_bit_equal_on_every_time_tile(H):
    """A push is spread over the chip: a wave owns 16, 32 or the offline kernel's 64 / 128 samples, by the number of waves the
    push has (mst_tcn_stream_samples_per_wave).  With B = 2 every push above runs the 16-sample tile; 256 streams and blocks of
    700, 150, 50 and 30 samples run all three of every channel-tile instantiation."""
    c = cs.case(*GEOMETRIES[H], B=256)
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(2, c["T"]).repeat(128, 1, 1).cuda()
    x[2:] *= torch.linspace(0.25, 1.0, 254, device="cuda").view(-1, 1, 1)      # (254 further clips: scaled copies of the two)
    sizes = cs.walk(c["T"], (700, 150, 50, 30), then="cycle")
    h = m._handle(torch.device("cuda", torch.cuda.current_device()))
    tiles = {_lib.lib().mst_tcn_stream_samples_per_wave(h.ptr, c["B"], n) for n in sizes}
    assert tiles == {16, 32, 128 if H <= 32 else 64}, tiles
    with torch.no_grad():
        want = m(x, film_params=film)
        got = cs.run(m.stream(batch_size=c["B"], max_block=max(sizes), film_params=film), x, sizes)
    assert torch.equal(got, want), f"max |d| = {float((got - want).abs().max()):.3e}"


def test_deep_fixture_in_blocks_of_4096():
    """The `causal` fixture (16 channels, 14 blocks, K = 15, FiLM from the generator, 2 x 40 000) pushed in blocks of 4096:
    the offline bits, and inside the fixture's TwoTimesRule with the stream's y in the place of the offline one."""
    import test_tcn_gpu as base
    c, g = DEEP, np.load(ct.fixture_path("causal"))
    x = cases.pcm_batch(c["B"], c["T"])
    blocks = ct.tap_blocks(c)
    tcn, gen = base.build(c)
    with torch.no_grad():
        film = gen.film_tensor(ct.embeddings(c["B"], ct.EMBED).cuda())
        want, hs = tcn._forward_hip(x.cuda(), film, tuple(blocks))
        got = cs.run(tcn.stream(batch_size=c["B"], max_block=4096, film_params=ctt.film_dicts(film)), x.cuda(),
                     cs.walk(c["T"], (), then=4096))
    assert torch.equal(got, want)
    xs, hi = ct.flat_y(x), ct.hidden_idx(c)
    rule = ct.TwoTimesRule("causal, streamed", report=False)
    rule.add("y", ct.flat_y(got), ct.golden_y(g, 32), ct.golden_y(g, 64))
    rule.add("y-x", ct.flat_y(got) - xs, ct.golden_y(g, 32) - xs, ct.golden_y(g, 64) - xs)
    for k, h in zip(blocks, hs):   # the case's other quantities, from the offline call: they set e_ref as in test_fixture_case
        rule.add(f"h{k}", h.cpu().reshape(-1)[hi].numpy(), g[f"h{k}_32"], g[f"h{k}_64"])
    rule.add("film", film.cpu().numpy(), g["film32"], g["film64"])
    rule.check()


def test_top_dilation_ring_wrap():
    """260 000 samples, more than twice the 114 688 rows of history of block 13, so the largest ring (131 072 rows at
    max_block = 16 384) wraps; 106 pushes of 1 ... 16 384 samples."""
    c = dict(DEEP, B=1, T=260000)
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(1, 260000).cuda()
    sizes = cs.walk(c["T"], cs.WRAP_CYCLE, then="cycle")
    assert len(sizes) == 106 and max(sizes) == 16384
    with torch.no_grad():
        want = m(x, film_params=film)
        got = cs.run(m.stream(batch_size=1, max_block=16384, film_params=film), x, sizes)
    assert torch.equal(got, want), f"max |d| = {float((got - want).abs().max()):.3e}"


def test_position_invariance():
    """Ring offsets are taken from a 64-bit position: starting at 2^40 + 12345 gives the bits of starting at 0."""
    c, m, film, x, want = offline(16)
    sizes = cs.schedule("b", c["T"])
    with torch.no_grad():
        s = m.stream(batch_size=c["B"], max_block=max(sizes), film_params=film)
        s.reset(position=2 ** 40 + 12345)
        got = cs.run(s, x, sizes)
    assert s.position == 2 ** 40 + 12345 + c["T"]
    assert torch.equal(got, want)


def test_independence_of_clips_and_of_streams():
    c, m, film, x, want = offline(16)
    sizes = cs.schedule("b", c["T"])
    with torch.no_grad():
        for b in range(c["B"]):   # a clip alone, B = 1
            fb = [{k: v[b:b + 1] for k, v in p.items()} for p in film]
            alone = cs.run(m.stream(batch_size=1, max_block=max(sizes), film_params=fb), x[b:b + 1], sizes)
            assert torch.equal(alone[0], want[b]), f"clip {b} depends on its batch"
        # two streams of one mixer, pushed alternately, on different inputs and schedules
        x2 = x.flip(0).contiguous()
        want2 = m(x2, film_params=film)
        s1 = m.stream(batch_size=c["B"], max_block=c["T"], film_params=film)
        s2 = m.stream(batch_size=c["B"], max_block=c["T"], film_params=film)
        o1, o2, t1, t2 = [], [], 0, 0
        for n1, n2 in zip(cs.schedule("b", c["T"]), cs.walk(c["T"], (), then=c["T"] // 9 + 1)):
            o1.append(s1.push(x[:, :, t1:t1 + n1]))
            o2.append(s2.push(x2[:, :, t2:t2 + n2]))
            t1, t2 = t1 + n1, t2 + n2
        assert t1 == t2 == c["T"]
    assert torch.equal(torch.cat(o1, 2), want) and torch.equal(torch.cat(o2, 2), want2)


def test_reset():
    c, m, film, x, want = offline(16)
    other = cs.film(c, "cuda", seed=5101)
    sizes = cs.schedule("b", c["T"])
    with torch.no_grad():
        s = m.stream(batch_size=c["B"], max_block=max(sizes), film_params=film)
        first = cs.run(s, x, sizes)
        s.reset()
        assert s.position == 0 and torch.equal(cs.run(s, x, sizes), first) and torch.equal(first, want)
        s.reset(film_params=other)
        want_other = m(x, film_params=other)
        assert torch.equal(cs.run(s, x, sizes), want_other) and not torch.equal(want_other, want)


def test_state_accounting_and_abi_refusals():
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    err = lambda: L.mst_last_error().decode()  # noqa: E731
    for H, B, max_block in ((16, 1, 16384), (128, 2, 128), (100, 3, 1)):
        c = dict(DEEP, H=H)
        h = cs.mixer(c, "cuda")._handle(dev)
        HP, K, nb = (H + 15) // 16 * 16, c["K"], c["nb"]
        floor = B * nb * 4 * HP * 4 + 2 * (K - 1) * (2 ** nb - 1) * HP * 4 * B
        n = L.mst_tcn_stream_state_bytes(h.ptr, B, max_block)
        print(f"H={H} B={B} max_block={max_block}: state {n} B, history alone {floor} B")
        assert n >= floor + 2 * nb * max_block * HP * 4 * B and L.mst_tcn_stream_workspace_bytes(h.ptr, B, max_block) > 0
    m = cs.mixer(SMALL, "cuda")
    h = m._handle(dev)
    for B, max_block, word in ((0, 64, "B must be"), (65536, 64, "B must be"), (1, 0, "max_block"), (1, 1 << 27, "2^31")):
        assert L.mst_tcn_stream_state_bytes(h.ptr, B, max_block) == 0 and word in err(), (B, max_block, err())
        assert L.mst_tcn_stream_workspace_bytes(h.ptr, B, max_block) == 0 and word in err()
    nc = cs.mixer(cs.case(16, 3, 15, True, causal=False), "cuda")._handle(dev)
    assert L.mst_tcn_stream_state_bytes(nc.ptr, 1, 64) == 0 and "causal" in err() and "mst_tcn_forward" in err()
    _lib.check(L.mst_tcn_set_precision(h.ptr, 1, None), "mst_tcn_set_precision")
    assert L.mst_tcn_stream_state_bytes(h.ptr, 1, 64) == 0 and "mst_tcn_set_precision(MST_TCN_FP32)" in err()
    _lib.check(L.mst_tcn_set_precision(h.ptr, 0, None), "mst_tcn_set_precision")
    # reset / push: every refusal comes before anything is launched
    n = L.mst_tcn_stream_state_bytes(h.ptr, 1, 64)
    state = torch.empty(n, dtype=torch.uint8, device="cuda")
    work = torch.empty(L.mst_tcn_stream_workspace_bytes(h.ptr, 1, 64), dtype=torch.uint8, device="cuda")
    film = torch.ones(1, 3, 4, 16, device="cuda")
    x = torch.zeros(1, 8, 64, device="cuda")
    y = torch.empty_like(x)
    p = _lib.dptr
    assert L.mst_tcn_stream_reset(h.ptr, p(state), n, 1, 64, None, None) != 0 and "film" in err()
    assert L.mst_tcn_stream_reset(h.ptr, p(state), n - 1, 1, 64, p(film), None) != 0 and "state" in err()
    assert L.mst_tcn_stream_reset(h.ptr, p(state), n, 1, 64, p(film), None) == 0
    push = lambda nbytes, t0, N, wbytes: L.mst_tcn_stream_push(h.ptr, p(state), nbytes, 1, 64, t0, p(x), N, p(y), p(work), wbytes, None)  # noqa: E731
    assert push(n, 0, 0, work.numel()) != 0 and "N must be" in err()
    assert push(n, 0, 65, work.numel()) != 0 and "N must be" in err()
    assert push(n, -1, 64, work.numel()) != 0 and "t0" in err()
    assert push(n - 1, 0, 64, work.numel()) != 0 and "state" in err()
    assert push(n, 0, 64, 0) != 0 and "workspace" in err()
    assert push(n, 0, 64, work.numel()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()


def test_python_refusals():
    c, B = SMALL, SMALL["B"]
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(B, 300).cuda()   # its own: the test edits them
    with torch.no_grad():
        nc = cs.mixer(cs.case(16, 3, 15, True, causal=False), "cuda")
        with pytest.raises(RuntimeError, match="causal.*look.*TCNMixer.forward"):
            nc.stream(batch_size=B, film_params=film)
        s = m.stream(batch_size=B, max_block=256, film_params=film)
        m.train()
        with pytest.raises(RuntimeError, match=r"train\(\) mode.*backend='torch'"):
            s.push(x[:, :, :64])
        with pytest.raises(RuntimeError, match=r"train\(\) mode"):
            m.stream(batch_size=B, film_params=film)
        m.eval()
        m.precision = "f16x3"
        try:
            with pytest.raises(RuntimeError, match="f16x3.*precision='fp32'"):
                s.push(x[:, :, :64])
            with pytest.raises(RuntimeError, match="f16x3.*precision='fp32'"):
                m.stream(batch_size=B, film_params=film)
        finally:
            m.precision = "fp32"
        with pytest.raises(ValueError, match="max_block=256"):
            s.push(x[:, :, :0])
        with pytest.raises(ValueError, match="max_block=256"):
            s.push(x[:, :, :257])
        with pytest.raises(ValueError, match=f"batch_size={B}"):
            s.push(x[:1, :, :64])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.push(x[:, :, :64].cpu())
        with pytest.raises(RuntimeError, match="fp32"):
            s.push(x[:, :, :64].double())
        assert s.position == 0
        first = s.push(x[:, :, :64])
        m.output_conv.bias.add_(0.25)            # the parameter's _version moves
        with pytest.raises(RuntimeError, match=r"changed.*reset\(\)"):
            s.push(x[:, :, 64:128])
        s.reset()
        assert torch.allclose(s.push(x[:, :, :64]), first + 0.25, rtol=0, atol=1e-6)
    with pytest.raises(RuntimeError, match="no_grad"):   # gradients are not built
        s.push(x[:, :, 64:128].clone().requires_grad_(True))
