"""CPU: TCNMixer.lookahead_stream / TCNLookaheadStream / forward_blockwise on backend="torch" -- the state logic of
fixed-latency streaming of a non-causal mixer.

Every layer runs ((K-1)*d)//2 samples behind its input, rows of every layer outside the clip are zeros, the two residuals
are delayed by the lag they skip, and flush() drains the last `latency` samples, so the pushes and the flush without the
first `latency` samples must be the whole-clip forward whatever the block sizes.  In float64 the two differ by torch's
summation order alone; the bound is test_tcn_stream_cpu's 1e-12 of max|y|: far below any state error, which shows at 1e-3
or above."""
import pytest
import torch

import cases
import cases_tcn_lookahead as cl
import cases_tcn_stream as cs

BOUND = 1e-12


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def build(c):
    m, film = cs.mixer(c, "cpu", torch.float64, "torch"), cs.film(c, "cpu", torch.float64)
    x = cases.pcm_batch(c["B"], c["T"]).double()
    with torch.no_grad():
        whole = m(x, film_params=film)
    return m, film, x, whole


@pytest.mark.parametrize("sched", ["a", "b", "c"])
@pytest.mark.parametrize("c", [cl.case(12, 4, 5, False, B=2, T=1100), cl.case(16, 3, 15, True, B=2, T=1100)],
                         ids=["h12_plain", "h16_film"])
def test_stream_equals_whole_clip_float64(c, sched):
    m, film, x, whole = build(c)
    sizes = cs.schedule(sched, c["T"])
    s = m.lookahead_stream(batch_size=c["B"], max_block=max(sizes), film_params=film)
    assert s.latency == cl.latency(c) == (c["K"] - 1) * (2 ** c["nb"] - 1) and s.state_bytes == 0
    got = cl.run(s, x, sizes)
    e = rel(got, whole)
    print(f"lookahead stream vs whole clip, float64, {len(sizes)} pushes: {e:.2e} of max|y|")
    assert got.shape == whole.shape and got.dtype == torch.float64
    assert e <= BOUND
    assert float((whole - x).abs().max()) > 1e-2   # the mixer does something: y is not x
    assert s.position == c["T"]


def test_deep_mixer_latency_exceeds_the_clip():
    """14 blocks, K = 15: latency 229 362 against a clip of 6000 samples, pushed in blocks of 4096."""
    c = cl.case(16, 14, 15, True, B=1, T=6000)
    m, film, x, whole = build(c)
    s = m.lookahead_stream(batch_size=1, max_block=65536, film_params=film)
    assert s.latency == 229362
    got = cl.run(s, x, cs.walk(6000, (), then=4096))
    assert rel(got, whole) <= BOUND


@pytest.mark.parametrize("max_block", cl.FLUSH_BLOCKS)
@pytest.mark.parametrize("T", cl.SHORT_T)
def test_clip_lengths_around_the_latency(T, max_block):
    c = cl.case(16, 3, 15, True, B=2, T=T)
    m, film, x, whole = build(c)
    for sizes in (cs.walk(T, (), then=max_block), [1] * T):
        s = m.lookahead_stream(batch_size=2, max_block=max_block, film_params=film)
        assert s.latency == 98
        got = cl.run(s, x, sizes)
        assert got.shape == whole.shape and rel(got, whole) <= BOUND, (T, max_block, len(sizes))


@pytest.mark.parametrize("causal", [False, True])
def test_forward_blockwise(causal):
    c = cl.case(16, 3, 15, True, B=2, T=5000, causal=causal)
    m, film, x, whole = build(c)
    with torch.no_grad():
        for block in (512, 5000, 65536):
            got = m.forward_blockwise(x, film_params=film, block=block)
            assert got.shape == whole.shape and rel(got, whole) <= BOUND
        short = m.forward_blockwise(x[:, :, :50], film_params=film, block=7)    # T < latency
        assert rel(short, m(x[:, :, :50], film_params=film)) <= BOUND
    with pytest.raises(ValueError, match="block must be positive"):
        m.forward_blockwise(x, film_params=film, block=0)
    with pytest.raises(ValueError, match="stems"):
        m.forward_blockwise(x[:, :7], film_params=film)


def test_causal_mixer_has_latency_zero():
    c = cl.case(12, 4, 4, False, B=2, T=700, causal=True)
    m, film, x, whole = build(c)
    sizes = cs.schedule("b", 700)
    s = m.lookahead_stream(batch_size=2, max_block=700)
    assert s.latency == 0
    pushes = cs.run(s, x, sizes)
    assert s.flush().shape == (2, 8, 0)
    assert torch.equal(pushes, cs.run(m.stream(batch_size=2, max_block=700), x, sizes)) and rel(pushes, whole) <= BOUND


def test_lifecycle_position_and_block_checks():
    c = cl.case(12, 4, 5, False, B=2, T=300)
    m, film, x, whole = build(c)
    s = m.lookahead_stream(batch_size=2, max_block=128)
    assert s.position == 0 and s.max_block == 128 and s.batch_size == 2 and s.latency == 60
    assert s.push(x[:, :, :100]).shape == (2, 8, 100) and s.position == 100
    for bad, word in ((x[:, :, :0], "max_block"), (x[:, :, :129], "max_block"), (x[:1, :, :10], "batch_size"), (x[:, :7, :10], "stems")):
        with pytest.raises(ValueError, match=word):
            s.push(bad)
    assert s.position == 100   # a refused push moves nothing
    assert s.flush().shape == (2, 8, 60) and s.position == 100
    with pytest.raises(RuntimeError, match=r"flush\(\).*reset\(\)"):
        s.push(x[:, :, :10])
    with pytest.raises(RuntimeError, match=r"flush\(\).*reset\(\)"):
        s.flush()
    s.reset(position=2 ** 40 + 12345)          # the result does not depend on the position
    sizes = cs.walk(300, (), then=77)
    first = cl.run(s, x, sizes)
    assert s.position == 2 ** 40 + 12345 + 300 and rel(first, whole) <= BOUND
    s.reset()
    assert s.position == 0 and torch.equal(cl.run(s, x, sizes), first)
    with pytest.raises(ValueError, match="negative"):
        s.reset(position=-1)
    with pytest.raises(ValueError, match="positive"):
        m.lookahead_stream(batch_size=0)
    with pytest.raises(ValueError, match="use_film=False"):
        m.lookahead_stream(film_params=[{}] * 4)
    s.reset()
    s.push(x[:, :, :50])
    with torch.no_grad():
        m.output_conv.bias.add_(0.25)
    with pytest.raises(RuntimeError, match=r"changed.*reset\(\)"):
        s.push(x[:, :, 50:100])
    with pytest.raises(RuntimeError, match=r"changed.*reset\(\)"):
        s.flush()
    s.reset()
    with torch.no_grad():
        assert rel(cl.run(s, x, sizes), m(x)) <= BOUND


def test_reset_takes_new_film():
    c = cl.case(16, 3, 15, True, B=2, T=700)
    m, film, x, whole = build(c)
    other = cs.film(c, "cpu", torch.float64, seed=5101)
    sizes = cs.schedule("b", 700)
    s = m.lookahead_stream(batch_size=2, max_block=700, film_params=film)
    first = cl.run(s, x, sizes)
    s.reset(film_params=other)
    with torch.no_grad():
        want = m(x, film_params=other)
    got = cl.run(s, x, sizes)
    assert rel(got, want) <= BOUND and rel(got, first) > 1e-3
    with pytest.raises(ValueError, match="film_params"):
        m.lookahead_stream(batch_size=2)       # a FiLM mixer without FiLM parameters


def test_refusals_of_every_backend():
    noncausal = cs.mixer(cl.case(12, 4, 5, False), "cpu", torch.float32, "torch")
    for backend in ("torch", "hip"):           # the causal stream still refuses a non-causal mixer, and names the new entry
        noncausal.backend = backend
        with pytest.raises(RuntimeError, match="causal.*look.*TCNMixer.forward.*lookahead_stream"):
            noncausal.stream()
    m = noncausal
    m.backend = "hip-train"
    with pytest.raises(RuntimeError, match="hip-train.*inference"):
        m.lookahead_stream()
    m.backend = "torch"
    s = m.lookahead_stream()
    m.backend = "hip-train"
    with pytest.raises(RuntimeError, match="hip-train"):
        s.push(torch.zeros(1, 8, 16))
    with pytest.raises(RuntimeError, match="hip-train"):
        s.flush()
    m.backend = "torch"
    m.train()
    with pytest.raises(RuntimeError, match=r"train\(\) mode"):
        s.push(torch.zeros(1, 8, 16))
    with pytest.raises(RuntimeError, match=r"train\(\) mode"):
        m.lookahead_stream()
    m.eval()
    assert s.push(torch.zeros(1, 8, 16)).shape == (1, 8, 16)
    m.backend = "hip"                          # a CPU mixer has no HIP stream, and no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.lookahead_stream()
    with pytest.raises(RuntimeError, match="changed.*reset"):   # the backend is part of what a stream binds
        s.push(torch.zeros(1, 8, 16))
    m.backend = "nonsense"
    with pytest.raises(ValueError, match="backend must be"):
        m.lookahead_stream()


def test_apply_style_transfer_block():
    """`block=` routes the mixer through forward_blockwise: the same stems as the whole-clip call."""
    from mst_amd import tcn_mixer as tm
    c = cl.case(16, 3, 15, True, B=1, T=3000)
    m = cs.mixer(c, "cpu", torch.float64, "torch")
    gen = tm.TCNFiLMGenerator(embed_dim=64, num_blocks=3, hidden_channels=16).double()
    gen.backend = "torch"
    x = cases.pcm_batch(1, 3000)[0].double()
    stems = {s: x[2 * i:2 * i + 2] for i, s in enumerate(tm.STEM_ORDER)}
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(32, generator=g).double(), torch.randn(32, generator=g).double()
    whole = tm.apply_style_transfer(m, gen, stems, a, b, "cpu")
    blocks = tm.apply_style_transfer(m, gen, stems, a, b, "cpu", block=700)
    for k in tm.STEM_ORDER:
        assert rel(blocks["processed_stems"][k], whole["processed_stems"][k]) <= BOUND
    assert rel(blocks["processed_mixture"], whole["processed_mixture"]) <= BOUND
    assert float((whole["processed_stems"]["vocals"] - stems["vocals"]).abs().max()) > 1e-3
