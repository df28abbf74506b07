"""GPU parity of the augmentation chain (csrc/aug.hip) where a clip is cut into pieces: chunk (32), wave (2048) and segment
(16 384) edges of the IIR chain, overlap-save block (512) and shift (D = L - 1 - L / 2) edges of the reverb, misaligned bases,
impulse responses of other lengths, silent clips and stems, and a clip of more segments than one look-back tile holds.
Decisions are explicit (tests/cases_aug.py); the reference is the oracle's arithmetic for those decisions, and the input
conditions of every case are asserted on the CPU in tests/test_aug_cases_cpu.py.  No element is left out of a comparison."""
import pytest
import torch

import cases
import cases_aug as ca
from oracle import mel as omel

pytestmark = pytest.mark.gpu


def augmenter():
    from mst_amd.mixing_utils import AudioAugmenter
    return AudioAugmenter(ca.SR)


def run(specs, x, aug=None):
    """The decisions on a packed contiguous (aligned) copy of x, in place -> CPU tensor."""
    aug = aug or augmenter()
    y = x.cuda().clone()
    clips, irs = ca.fill_clips(specs, aug)
    aug._apply(y, clips, irs)
    torch.cuda.synchronize()
    return y.cpu()


def run_case(name):
    specs, x, silent = ca.case(name)
    return specs, x, silent, ca.reference(name), run(specs, x)


# ---- (a) chain lengths on and next to chunk, wave and segment edges -------------------------------------------------
@pytest.mark.parametrize("T", ca.CHAIN_T)
def test_chain_lengths(T):
    specs, x, _, ref, y = run_case(f"a-T{T}")
    ca.assert_close(y, ref, **ca.TOL_CHAIN, what=f"(a) T={T}")
    assert torch.equal(y[:, 6:8], x[:, 6:8]), "a stem without a decision was written"


# ---- (b) all 8 combinations of tilt / compressor / low-pass, orders 2 and 4 ----------------------------------------
@pytest.mark.parametrize("T", (16385, 33))
def test_every_effect_combination(T):
    specs, x, _, ref, y = run_case(f"b-T{T}")
    assert not specs[0].stems[0].any and torch.equal(y[0, 0:2], x[0, 0:2])
    ca.assert_close(y, ref, **ca.TOL_CHAIN, what=f"(b) T={T}")


# ---- (c) T % 4 == 0 on a base that is not 16-byte aligned -----------------------------------------------------------
def _misaligned(x):
    """x (1, 8, T) -> (buffer, view of it that starts 4 bytes in and holds x)."""
    n = x.numel()
    buf = torch.full((n + 8,), 7.0, device="cuda")
    view = buf[1:1 + n].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return buf, view


def _untouched(buf, n):
    return bool((buf[0] == 7.0).item()) and bool((buf[1 + n:] == 7.0).all().item())


@pytest.mark.parametrize("name", ("c-chain", "c-reverb"))
def test_aligned_length_on_a_misaligned_base(name):
    specs, x, _, ref, y0 = run_case(name)
    ca.assert_close(y0, ref, **(ca.TOL_REVERB if specs[0].reverb else ca.TOL_CHAIN), what=f"({name}) aligned")
    aug, n = augmenter(), x.numel()
    clips, irs = ca.fill_clips(specs, aug)
    xa = x.cuda()
    assert xa.data_ptr() % 16 == 0
    # in place on the misaligned view
    buf, v = _misaligned(xa)
    aug._apply(v, clips, irs)
    assert torch.equal(v.cpu(), y0) and _untouched(buf, n)
    # aligned source -> misaligned destination
    buf, v = _misaligned(torch.full_like(xa, float("nan")))
    aug._apply(v, clips, irs, src=xa)
    assert torch.equal(v.cpu(), y0) and _untouched(buf, n) and torch.equal(xa.cpu(), x)
    # misaligned source -> aligned destination
    buf, v = _misaligned(xa)
    dst = torch.full_like(xa, float("nan"))
    aug._apply(dst, clips, irs, src=v)
    assert torch.equal(dst.cpu(), y0) and _untouched(buf, n) and torch.equal(v.cpu(), x)


# ---- (d) strided and out-of-place variants at an edge ---------------------------------------------------------------
@pytest.mark.parametrize("T", (16385, 31))
def test_packed_strided_in_place_variant_at_an_edge(T):
    x = torch.stack([cases.synth_clip(c, T) for c in range(7)], 0).cuda()
    aug = augmenter()
    torch.manual_seed(21)
    dec = aug.draw_decisions(3)
    ref8 = omel.stems_dict_to_tensor(aug.augment_stems(omel.tensor_to_stems_dict(x[0::3]), decisions=dec))
    y = x.clone()
    aug.augment_packed_(y[0::3], decisions=dec)
    torch.cuda.synchronize()
    assert torch.equal(y[0::3], ref8)
    for b in (1, 2, 4, 5):
        assert torch.equal(y[b], x[b])
    assert not torch.equal(y[0], x[0])


@pytest.mark.parametrize("T", (16385, 31))
def test_out_of_place_variant_at_an_edge(T):
    from mst_amd import _lib
    x = torch.stack([cases.synth_clip(c, T) for c in range(7)], 0).cuda()
    keep = x.clone()
    aug = augmenter()
    torch.manual_seed(21)
    dec = aug.draw_decisions(3)
    ref = x.clone()
    aug.augment_packed_(ref[0::3], decisions=dec)
    y = torch.full_like(x, float("nan"))
    aug.augment_packed_(y[0::3], decisions=dec, src=x[0::3])
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "src was written"
    assert torch.equal(y[0::3], ref[0::3])
    assert bool(torch.isnan(y[1]).all()), "clips between the strided ones were touched"
    clips = (_lib.AugClip * 2)()   # no decision at all: a plain copy
    for b in range(2):
        for i in range(4):
            clips[b].stem[i].gain = 1.0
    z = torch.full((2, 8, T), float("nan"), device="cuda")
    aug.augment_packed_(z, decisions=(clips, [None, None], [{}, {}]), src=x[1:3])
    torch.cuda.synchronize()
    assert torch.equal(z, x[1:3])


# ---- (e) reverb: clip lengths around the block size and the shift D, L = 22050 --------------------------------------
@pytest.mark.parametrize("T", ca.REVERB_T)
def test_reverb_lengths_mode1(T):
    specs, x, _, ref, y = run_case(f"e-mode1-T{T}")
    ca.assert_close(y, ref, **ca.TOL_REVERB, what=f"(e) mode 1 T={T}")


@pytest.mark.parametrize("T", ca.REVERB_T)
def test_reverb_lengths_mode2(T):
    x, ref, nxt = ca.mode2_case(T, 100 + T)
    torch.manual_seed(100 + T)
    y = augmenter().apply_reverb(x.cuda()).cpu()
    assert float(torch.rand(1)) == nxt, "apply_reverb consumed the generator differently from the reference"
    ca.assert_close(y, ref, **ca.TOL_REVERB2, what=f"(e) mode 2 T={T}")


# ---- (f) impulse responses of other lengths -------------------------------------------------------------------------
@pytest.mark.parametrize("L", ca.IR_L)
@pytest.mark.parametrize("T", ca.IR_T)
def test_impulse_response_lengths(T, L):
    specs, x, _, ref, y = run_case(f"f-T{T}-L{L}")
    ca.assert_close(y, ref, **ca.TOL_REVERB, what=f"(f) T={T} L={L}")


def test_apply_reverb_with_another_decay():
    x, ref, nxt = ca.mode2_case(4099, 77, decay=0.1)
    torch.manual_seed(77)
    y = augmenter().apply_reverb(x.cuda(), decay=0.1).cpu()
    assert float(torch.rand(1)) == nxt, "apply_reverb(decay=0.1) consumed the generator differently from oaug.make_ir"
    ca.assert_close(y, ref, **ca.TOL_REVERB2, what="(f) apply_reverb(decay=0.1) T=4099 L=4410")


# ---- (g) reverb on, off and on silence in one batch -----------------------------------------------------------------
def test_reverb_batch_edges():
    specs, x, _, ref, y = run_case("g-batch")
    ca.assert_close(y[0:1], ref[0:1], **ca.TOL_REVERB, what="(g) clip 0, reverb on")
    ca.assert_close(y[1:2], ref[1:2], **ca.TOL_CHAIN, what="(g) clip 1, reverb off")
    assert torch.equal(y[1:2], run([specs[1]], x[1:2])), "a clip without reverb differs from its chain-only result"
    assert torch.equal(y[2], torch.zeros_like(y[2])), "reverb of a silent clip is not exactly zero"


def test_reverb_silent_stem_among_live_ones():
    specs, x, silent, ref, y = run_case("g-silent-stem")
    assert torch.equal(y[0, 4:6], torch.zeros_like(y[0, 4:6])), "a silent stem must receive exactly 0 + rev * 0"
    ca.assert_close(y, ref, **ca.TOL_REVERB, what="(g) silent stem")


# ---- (h) more segments than one look-back tile holds ----------------------------------------------------------------
def test_long_clip_beyond_one_lookback_tile():
    """257 segments + 33 samples: the look-back of the last segments folds 2 tiles of 256 aggregates (biquads) and 3 tiles of
    128 (the 4th-order low-pass).  The last segments on their own as well: an error there must not drown in 4 M samples."""
    specs, x, _, ref, y = run_case("h-long")
    assert torch.equal(y[:, 4:8], x[:, 4:8])
    assert not bool(torch.isnan(y).any()), "a look-back wait timed out"
    ca.assert_close(y[:, 0:4], ref[:, 0:4], **ca.TOL_CHAIN, what="(h) whole clip")
    for k0 in (128, 129, 256, 257):   # first segments of the second and third tile, and the last two
        ca.assert_close(y[:, 0:4, k0 * ca.SEG:(k0 + 1) * ca.SEG], ref[:, 0:4, k0 * ca.SEG:(k0 + 1) * ca.SEG], **ca.TOL_CHAIN,
                        what=f"(h) segment {k0}")
