"""GPU: fixed-latency block-wise streaming of a non-causal TCN mixer (csrc/tcn_lookahead.inc, mst_tcn_lookahead_*,
TCNMixer.lookahead_stream, TCNMixer.forward_blockwise).

The acceptance criterion needs no tolerance: the pushes and the flush, without the first `latency` samples, are the offline
`mixer(x, film)` result BIT FOR BIT, whatever the block sizes and the clip's length.  Every output element is the chain of
the offline kernel (per tap a partial sum in channel order, `acc += part` once per tap, the folded epilogue) on the same
operands, and the rows of every layer outside the clip are stored zeros where the offline kernel selects zeros or skips
the tap -- at the clip's start and at its end."""
import numpy as np
import pytest
import torch

import cases
import cases_tcn as ct
import cases_tcn_lookahead as cl
import cases_tcn_stream as cs
import cases_tcn_train as ctt
from mst_amd import _lib

pytestmark = pytest.mark.gpu

SMALL = cl.case(16, 3, 15, True)
DEEP = dict(ct.CASES["st_default"])
_cache = {}


def offline(H):
    """(case, mixer, film, x, offline y) of a geometry, computed once."""
    if H not in _cache:
        c = cl.case(*cl.GEOMETRIES[H])
        m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(c["B"], c["T"]).cuda()
        with torch.no_grad():
            _cache[H] = (c, m, film, x, m(x, film_params=film))
    return _cache[H]


def diff(got, want):
    return f"max |d| = {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("sched", ["a", "b", "c"])
@pytest.mark.parametrize("H", list(cl.GEOMETRIES))
def test_bit_equal_to_offline_every_instantiation(H, sched):
    c, m, film, x, want = offline(H)
    sizes = cs.schedule(sched, c["T"])
    with torch.no_grad():
        s = m.lookahead_stream(batch_size=c["B"], max_block=1100, film_params=film)
        assert s.latency == cl.latency(c) > 0
        got = cl.run(s, x, sizes)
    assert torch.equal(got, want), diff(got, want)
    assert float((want - x).abs().max()) > 1e-2


@pytest.mark.parametrize("H", list(cl.GEOMETRIES))
def test_bit_equal_on_every_time_tile(H):
    """256 streams and blocks of 700, 150, 50 and 30 samples run the 16-, 32- and 64 / 128-sample tiles of every channel-tile
    instantiation (mst_tcn_stream_samples_per_wave), as in test_tcn_stream_gpu."""
    c = cl.case(*cl.GEOMETRIES[H], B=256)
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(2, c["T"]).repeat(128, 1, 1).cuda()
    x[2:] *= torch.linspace(0.25, 1.0, 254, device="cuda").view(-1, 1, 1)
    sizes = cs.walk(c["T"], (700, 150, 50, 30), then="cycle")
    h = m._handle(torch.device("cuda", torch.cuda.current_device()))
    tiles = {_lib.lib().mst_tcn_stream_samples_per_wave(h.ptr, c["B"], n) for n in sizes}
    assert tiles == {16, 32, 128 if H <= 32 else 64}, tiles
    with torch.no_grad():
        want = m(x, film_params=film)
        got = cl.run(m.lookahead_stream(batch_size=c["B"], max_block=max(sizes), film_params=film), x, sizes)
    assert torch.equal(got, want), diff(got, want)


@pytest.mark.parametrize("max_block", cl.FLUSH_BLOCKS)
@pytest.mark.parametrize("T", cl.SHORT_T)
def test_clip_lengths_around_the_latency(T, max_block):
    """Latency 98: clips shorter than, as long as and up to twice as long as the latency, in single-sample pushes and in the
    fewest pushes max_block allows (one push at max_block = 4096); flush() drains in pieces of max_block = 1, 64, 4096."""
    c, m, film, x, _ = offline(16)
    x = x[:, :, 300:300 + T].contiguous()
    with torch.no_grad():
        want = m(x, film_params=film)
        for sizes in (cs.walk(T, (), then=max_block), [1] * T):
            s = m.lookahead_stream(batch_size=c["B"], max_block=max_block, film_params=film)
            got = cl.run(s, x, sizes)
            assert s.position == T
            assert got.shape == want.shape and torch.equal(got, want), (T, max_block, len(sizes), diff(got, want))


def test_deep_fixture_in_blocks_of_4096():
    """The `st_default` fixture (16 channels, 14 blocks, K = 15, non-causal, FiLM from the generator, 2 x 40 000; latency
    229 362 > T) pushed in blocks of 4096: the offline bits, and inside the fixture's TwoTimesRule with the stream's y."""
    import test_tcn_gpu as base
    c, g = DEEP, np.load(ct.fixture_path("st_default"))
    x = cases.pcm_batch(c["B"], c["T"])
    blocks = ct.tap_blocks(c)
    tcn, gen = base.build(c)
    with torch.no_grad():
        film = gen.film_tensor(ct.embeddings(c["B"], ct.EMBED).cuda())
        want, hs = tcn._forward_hip(x.cuda(), film, tuple(blocks))
        s = tcn.lookahead_stream(batch_size=c["B"], max_block=4096, film_params=ctt.film_dicts(film))
        assert s.latency == 229362 > c["T"]
        got = cl.run(s, x.cuda(), cs.walk(c["T"], (), then=4096))
    assert torch.equal(got, want), diff(got, want)
    xs, hi = ct.flat_y(x), ct.hidden_idx(c)
    rule = ct.TwoTimesRule("st_default, streamed", report=False)
    rule.add("y", ct.flat_y(got), ct.golden_y(g, 32), ct.golden_y(g, 64))
    rule.add("y-x", ct.flat_y(got) - xs, ct.golden_y(g, 32) - xs, ct.golden_y(g, 64) - xs)
    for k, h in zip(blocks, hs):
        rule.add(f"h{k}", h.cpu().reshape(-1)[hi].numpy(), g[f"h{k}_32"], g[f"h{k}_64"])
    rule.add("film", film.cpu().numpy(), g["film32"], g["film64"])
    rule.check()


def test_ring_wrap():
    """300 000 samples in WRAP_CYCLE: with the 229 362 drained samples the stream runs 529 362 samples, so the block-13 ring
    (131 072 rows at max_block = 16 384) and the x delay ring (262 144 columns) both wrap."""
    c = dict(DEEP, B=1, T=300000)
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(1, 300000).cuda()
    sizes = cs.walk(c["T"], cs.WRAP_CYCLE, then="cycle")
    assert max(sizes) == 16384
    with torch.no_grad():
        want = m(x, film_params=film)
        got = cl.run(m.lookahead_stream(batch_size=1, max_block=16384, film_params=film), x, sizes)
    assert torch.equal(got, want), diff(got, want)


def test_large_start_position():
    c, m, film, x, want = offline(16)
    sizes = cs.schedule("b", c["T"])
    with torch.no_grad():
        s = m.lookahead_stream(batch_size=c["B"], max_block=max(sizes), film_params=film)
        s.reset(position=2 ** 40 + 12345)
        got = cl.run(s, x, sizes)
    assert s.position == 2 ** 40 + 12345 + c["T"]
    assert torch.equal(got, want), diff(got, want)


def test_stream_lifecycle():
    """Clips alone against clips in a batch; two interleaved streams of one mixer; reset after flush."""
    c, m, film, x, want = offline(16)
    sizes = cs.schedule("b", c["T"])
    with torch.no_grad():
        for b in range(c["B"]):
            fb = [{k: v[b:b + 1] for k, v in p.items()} for p in film]
            alone = cl.run(m.lookahead_stream(batch_size=1, max_block=max(sizes), film_params=fb), x[b:b + 1], sizes)
            assert torch.equal(alone[0], want[b]), f"clip {b} depends on its batch"
        x2 = x.flip(0).contiguous()
        want2 = m(x2, film_params=film)
        s1 = m.lookahead_stream(batch_size=c["B"], max_block=c["T"], film_params=film)
        s2 = m.lookahead_stream(batch_size=c["B"], max_block=c["T"], film_params=film)
        o1, o2, t1, t2 = [], [], 0, 0
        for n1, n2 in zip(cs.schedule("b", c["T"]), cs.walk(c["T"], (), then=c["T"] // 9 + 1)):
            o1.append(s1.push(x[:, :, t1:t1 + n1]))
            o2.append(s2.push(x2[:, :, t2:t2 + n2]))
            t1, t2 = t1 + n1, t2 + n2
        assert t1 == t2 == c["T"]
        o1.append(s1.flush()), o2.append(s2.flush())
        assert torch.equal(torch.cat(o1, 2)[:, :, s1.latency:], want) and torch.equal(torch.cat(o2, 2)[:, :, s2.latency:], want2)
        # a closed stream refuses, reset() reopens it and reproduces the first run; new FiLM on reset
        with pytest.raises(RuntimeError, match=r"flush\(\).*reset\(\)"):
            s1.push(x[:, :, :10])
        with pytest.raises(RuntimeError, match=r"flush\(\).*reset\(\)"):
            s1.flush()
        s1.reset()
        assert s1.position == 0 and torch.equal(cl.run(s1, x, sizes), want)
        other = cs.film(c, "cuda", seed=5101)
        s1.reset(film_params=other)
        want_other = m(x, film_params=other)
        assert torch.equal(cl.run(s1, x, sizes), want_other) and not torch.equal(want_other, want)


def test_causal_mixer_through_the_lookahead_api():
    c = cs.case(16, 3, 15, True)
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(c["B"], c["T"]).cuda()
    sizes = cs.schedule("b", c["T"])
    with torch.no_grad():
        want = cs.run(m.stream(batch_size=c["B"], max_block=max(sizes), film_params=film), x, sizes)
        s = m.lookahead_stream(batch_size=c["B"], max_block=max(sizes), film_params=film)
        assert s.latency == 0
        pushes = cs.run(s, x, sizes)
        tail = s.flush()
        assert tail.shape == (c["B"], 8, 0)
        assert torch.equal(pushes, want) and torch.equal(want, m(x, film_params=film))


@pytest.mark.parametrize("causal", [False, True])
def test_forward_blockwise(causal):
    c = cl.case(16, 3, 15, True, T=5000, causal=causal)
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(c["B"], c["T"]).cuda()
    with torch.no_grad():
        want = m(x, film_params=film)
        got = m.forward_blockwise(x, film_params=film, block=512)
    assert got.shape == want.shape and torch.equal(got, want), diff(got, want)


def test_beyond_the_offline_limit():
    """H = 128 (2 blocks, K = 15, latency 42) on a clip of 2^31 / 128 + 70 000 samples, which the offline forward refuses.
    Three windows of 4096 samples -- the start, across sample 2^31 / 128, the end -- against the offline forward of the
    window with 42 samples of context either side (cut at the clip's ends): a sample's receptive field is 42 samples each
    way, so inside the window the context clip computes the whole clip's chains on the whole clip's operands."""
    c = cl.case(128, 2, 15, True, B=1)
    lat, limit = cl.latency(c), 2 ** 31 // 128
    T = limit + 70000
    assert lat == 42
    m, film = cs.mixer(c, "cuda"), cs.film(c, "cuda")
    short = cases.pcm_batch(1, 70001).cuda()
    x = short.repeat(1, 1, T // 70001 + 1)[:, :, :T].contiguous()
    x *= torch.linspace(0.5, 1.0, T, device="cuda")
    with torch.no_grad():
        with pytest.raises(Exception, match="2\\^31"):
            m(x, film_params=film)
        got = m.forward_blockwise(x, film_params=film, block=16384)
        assert got.shape == x.shape
        for a in (0, limit - 2048, T - 4096):
            b = a + 4096
            lo, hi = max(a - lat, 0), min(b + lat, T)
            want = m(x[:, :, lo:hi].contiguous(), film_params=film)[:, :, a - lo:a - lo + 4096]
            assert torch.equal(got[:, :, a:b], want), (a, diff(got[:, :, a:b], want))
    assert float((got[:, :, -4096:] - x[:, :, -4096:]).abs().max()) > 1e-3


def test_state_accounting_and_abi_refusals():
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    err = lambda: L.mst_last_error().decode()  # noqa: E731
    deep = cs.mixer(dict(DEEP, B=1), "cuda")._handle(dev)
    assert L.mst_tcn_lookahead_latency(deep.ptr) == 229362
    n = L.mst_tcn_lookahead_state_bytes(deep.ptr, 1, 4096)
    print(f"st_default, B = 1, max_block = 4096: state {n} B")
    # the x delay ring: 262 144 columns of 8 floats on top of the causal layout's rings (14 * 15 - 1 rows of history ... )
    assert n >= 262144 * 8 * 4 + 2 * 14 * (2 ** 14 - 1) * 16 * 4
    m = cs.mixer(SMALL, "cuda")
    h = m._handle(dev)
    assert L.mst_tcn_lookahead_latency(h.ptr) == 98
    assert L.mst_tcn_lookahead_latency(None) == -1 and "NULL" in err()
    causal = cs.mixer(cs.case(16, 3, 15, True), "cuda")._handle(dev)
    assert L.mst_tcn_lookahead_latency(causal.ptr) == 0 and L.mst_tcn_lookahead_state_bytes(causal.ptr, 1, 64) > 0
    assert L.mst_tcn_lookahead_state_bytes(None, 1, 64) == 0 and "NULL" in err()
    for B, max_block, word in ((0, 64, "B must be"), (65536, 64, "B must be"), (1, 0, "max_block"), (1, 1 << 27, "2^31")):
        assert L.mst_tcn_lookahead_state_bytes(h.ptr, B, max_block) == 0 and word in err(), (B, max_block, err())
    _lib.check(L.mst_tcn_set_precision(h.ptr, 1, None), "mst_tcn_set_precision")
    assert L.mst_tcn_lookahead_state_bytes(h.ptr, 1, 64) == 0 and "mst_tcn_set_precision(MST_TCN_FP32)" in err()
    _lib.check(L.mst_tcn_set_precision(h.ptr, 0, None), "mst_tcn_set_precision")
    # the causal entry points still refuse a non-causal mixer, and now name the new one
    assert L.mst_tcn_stream_state_bytes(h.ptr, 1, 64) == 0 and "causal" in err() and "mst_tcn_forward" in err()
    assert "mst_tcn_lookahead_push" in err()
    # reset / push: every refusal comes before anything is launched
    n = L.mst_tcn_lookahead_state_bytes(h.ptr, 1, 64)
    state = torch.empty(n, dtype=torch.uint8, device="cuda")
    film = torch.ones(1, 3, 4, 16, device="cuda")
    x = torch.zeros(1, 8, 64, device="cuda")
    y = torch.empty_like(x)
    p = _lib.dptr
    assert L.mst_tcn_lookahead_reset(h.ptr, None, n, 1, 64, p(film), None) != 0 and "NULL" in err()
    assert L.mst_tcn_lookahead_reset(h.ptr, p(state), n, 1, 64, None, None) != 0 and "film" in err()
    assert L.mst_tcn_lookahead_reset(h.ptr, p(state), n - 1, 1, 64, p(film), None) != 0 and "state" in err()
    assert L.mst_tcn_lookahead_reset(h.ptr, p(state), n, 1, 64, p(film), None) == 0
    push = lambda nbytes, t0, t_end, xx, N, yy=y: L.mst_tcn_lookahead_push(h.ptr, p(state), nbytes, 1, 64, t0, t_end, p(xx), N, p(yy), None)  # noqa: E731
    assert push(n, 0, -1, x, 0) != 0 and "N must be" in err()
    assert push(n, 0, -1, x, 65) != 0 and "N must be" in err()
    assert push(n, -1, -1, x, 64) != 0 and "t0" in err()
    assert push(n - 1, 0, -1, x, 64) != 0 and "state" in err()
    assert push(n, 0, -1, None, 64) != 0 and "needs x" in err()
    assert push(n, 0, -1, x, 64, None) != 0 and "NULL" in err()
    assert push(n, 63, 64, None, 64) != 0 and "t0 >= t_end" in err()
    assert L.mst_tcn_lookahead_push(h.ptr, None, n, 1, 64, 0, -1, p(x), 64, p(y), None) != 0 and "NULL" in err()
    assert push(n, 0, -1, x, 64) == 0
    assert push(n, 64, 64, None, 64) == 0      # a drain push takes NULL
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()


def test_python_refusals():
    c, B = SMALL, SMALL["B"]
    m, film, x = cs.mixer(c, "cuda"), cs.film(c, "cuda"), cases.pcm_batch(B, 300).cuda()   # its own: the test edits them
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="causal.*look.*TCNMixer.forward.*lookahead_stream"):
            m.stream(batch_size=B, film_params=film)
        s = m.lookahead_stream(batch_size=B, max_block=256, film_params=film)
        assert s.latency == 98 and s.state_bytes > 0 and s.position == 0
        m.train()
        with pytest.raises(RuntimeError, match=r"train\(\) mode.*backend='torch'"):
            s.push(x[:, :, :64])
        with pytest.raises(RuntimeError, match=r"train\(\) mode"):
            m.lookahead_stream(batch_size=B, film_params=film)
        m.eval()
        m.backend = "hip-train"
        with pytest.raises(RuntimeError, match="hip-train.*inference"):
            s.push(x[:, :, :64])
        with pytest.raises(RuntimeError, match="hip-train.*inference"):
            m.lookahead_stream(batch_size=B, film_params=film)
        m.backend = "hip"
        m.precision = "f16x3"
        try:
            with pytest.raises(RuntimeError, match="f16x3.*precision='fp32'"):
                s.push(x[:, :, :64])
            with pytest.raises(RuntimeError, match="f16x3.*precision='fp32'"):
                m.lookahead_stream(batch_size=B, film_params=film)
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
        first = torch.cat([s.push(x[:, :, :64]), s.flush()], 2)[:, :, 98:]
        s.reset()
        s.push(x[:, :, :64])
        m.output_conv.bias.add_(0.25)            # the parameter's _version moves
        with pytest.raises(RuntimeError, match=r"changed.*reset\(\)"):
            s.push(x[:, :, 64:128])
        with pytest.raises(RuntimeError, match=r"changed.*reset\(\)"):
            s.flush()
        s.reset()
        again = torch.cat([s.push(x[:, :, :64]), s.flush()], 2)[:, :, 98:]
        assert torch.allclose(again, first + 0.25, rtol=0, atol=1e-6)
        s.reset()
    with pytest.raises(RuntimeError, match="no_grad"):   # gradients are not built
        s.push(x[:, :, 64:128].clone().requires_grad_(True))
