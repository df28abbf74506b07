"""CPU: TCNMixer.stream / TCNStream on backend="torch" -- the state logic of block-wise streaming.

Each dilated convolution keeps the last (K-1)*d samples of its own input, zeros at the start, so the pushes concatenated
must be the whole-clip forward whatever the block sizes.  In float64 the two differ by torch's summation order alone
(measured 1.0e-15 and 1.9e-16 of max|y| on the two geometries below); the bound is 1e-12 of max|y|: three decades above
that and far below any state error, which shows at 1e-3 or above."""
import pytest
import torch

import cases
import cases_tcn_stream as cs

BOUND = 1e-12


def whole_and_stream(c, sizes, max_block):
    m, film = cs.mixer(c, "cpu", torch.float64, "torch"), cs.film(c, "cpu", torch.float64)
    x = cases.pcm_batch(c["B"], c["T"]).double()
    with torch.no_grad():
        whole = m(x, film_params=film)
    s = m.stream(batch_size=c["B"], max_block=max_block, film_params=film)
    return m, film, x, whole, s, cs.run(s, x, sizes)


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("c,sizes,max_block", [
    (cs.case(12, 4, 4, False, B=2, T=3000), cs.schedule("b", 3000), 3000),
    (cs.case(16, 14, 15, True, B=1, T=20000), cs.walk(20000, (), then=4096), 4096),
], ids=["h12_plain_edges", "h16_deep_film_4096"])
def test_stream_equals_whole_clip_float64(c, sizes, max_block):
    _, _, x, whole, s, got = whole_and_stream(c, sizes, max_block)
    e = rel(got, whole)
    print(f"stream vs whole clip, float64, {len(sizes)} pushes: {e:.2e} of max|y|")
    assert got.shape == whole.shape and got.dtype == torch.float64
    assert e <= BOUND
    assert float((whole - x).abs().max()) > 1e-2   # the mixer does something: y is not x
    assert s.position == c["T"]


def test_position_bookkeeping_and_block_checks():
    c = cs.case(12, 4, 4, False, B=2, T=300)
    m = cs.mixer(c, "cpu", torch.float64, "torch")
    x = cases.pcm_batch(2, 300).double()
    s = m.stream(batch_size=2, max_block=128)
    assert s.position == 0 and s.max_block == 128 and s.batch_size == 2
    assert s.push(x[:, :, :100]).shape == (2, 8, 100) and s.position == 100
    s.push(x[:, :, 100:228])
    assert s.position == 228
    for bad, word in ((x[:, :, :0], "max_block"), (x[:, :, :129], "max_block"), (x[:1, :, :10], "batch_size"), (x[:, :7, :10], "stems")):
        with pytest.raises(ValueError, match=word):
            s.push(bad)
    assert s.position == 228   # a refused push moves nothing
    s.reset(position=5000)
    assert s.position == 5000
    s.push(x[:, :, :7])
    assert s.position == 5007
    with pytest.raises(ValueError, match="negative"):
        s.reset(position=-1)
    with pytest.raises(ValueError, match="positive"):
        m.stream(batch_size=0)
    with pytest.raises(ValueError, match="use_film=False"):
        m.stream(film_params=[{}] * 4)


def test_reset_semantics():
    c = cs.case(16, 3, 15, True, B=2, T=700)
    m = cs.mixer(c, "cpu", torch.float64, "torch")
    film, other = cs.film(c, "cpu", torch.float64), cs.film(c, "cpu", torch.float64, seed=5101)
    x = cases.pcm_batch(2, 700).double()
    sizes = cs.schedule("b", 700)
    s = m.stream(batch_size=2, max_block=700, film_params=film)
    first = cs.run(s, x, sizes)
    s.reset()                                  # zero history, the same FiLM
    assert s.position == 0 and torch.equal(cs.run(s, x, sizes), first)
    s.reset(position=2 ** 40 + 12345)          # the result does not depend on the position
    assert torch.equal(cs.run(s, x, sizes), first) and s.position == 2 ** 40 + 12345 + 700
    s.reset(film_params=other)
    with torch.no_grad():
        want = m(x, film_params=other)
    got = cs.run(s, x, sizes)
    assert rel(got, want) <= BOUND and rel(got, first) > 1e-3
    with pytest.raises(ValueError, match="film_params"):
        m.stream(batch_size=2)                 # a FiLM mixer without FiLM parameters


def test_push_after_a_parameter_changed_names_reset():
    c = cs.case(12, 4, 4, False, B=1, T=200)
    m = cs.mixer(c, "cpu", torch.float64, "torch")
    x = cases.pcm_batch(1, 200).double()
    s = m.stream(max_block=200)
    s.push(x[:, :, :50])
    with torch.no_grad():
        m.output_conv.bias.add_(0.25)
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        s.push(x[:, :, 50:])
    s.reset()
    with torch.no_grad():
        assert rel(s.push(x), m(x)) <= BOUND


def test_refusals_of_every_backend():
    noncausal = cs.mixer(cs.case(12, 4, 5, False, causal=False), "cpu", torch.float32, "torch")
    for backend in ("torch", "hip"):
        noncausal.backend = backend
        with pytest.raises(RuntimeError, match="causal.*look.*TCNMixer.forward"):
            noncausal.stream()
    m = cs.mixer(cs.case(12, 4, 4, False), "cpu", torch.float32, "hip-train")
    with pytest.raises(RuntimeError, match="hip-train.*inference"):
        m.stream()
    m.backend = "torch"
    s = m.stream()
    m.backend = "hip-train"
    with pytest.raises(RuntimeError, match="hip-train"):
        s.push(torch.zeros(1, 8, 16))
    m.backend = "torch"
    m.train()
    with pytest.raises(RuntimeError, match=r"train\(\) mode"):
        s.push(torch.zeros(1, 8, 16))
    with pytest.raises(RuntimeError, match=r"train\(\) mode"):
        m.stream()
    m.eval()
    assert s.push(torch.zeros(1, 8, 16)).shape == (1, 8, 16)
    m.backend = "hip"                          # a CPU mixer has no HIP stream, and no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.stream()
