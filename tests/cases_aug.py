"""Explicit augmentation decisions and their expected output (data + the oracle's arithmetic; no GPU needed).

A `Clip` says, per stem, which effects run and with which settings -- no coin is thrown.  `fill_clips` writes it into the
`mst_aug_clip` array the C ABI takes; `expected` computes what `oracle/augment.py` computes for those decisions, by calling
the oracle's own functions in the oracle's order, so the GPU edge tests (tests/test_aug_edges_gpu.py) compare the kernels with
the same arithmetic the seeded parity tests do, at lengths and settings a seeded draw never reaches."""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import cases  # noqa: F401  (puts the repository root on sys.path)
from oracle import augment as oaug

SR = 44100
SEG = 16384   # aug.hip: samples per workgroup (kFS); a thread owns 32 of them (kFL), a wave 2048


def gain_of_db(db: float) -> float:
    """The float32 factor the oracle multiplies with for a gain of `db` dB (augment.py: `10 ** (gdb / 20)`, gdb float32 (1,))."""
    return float((10 ** (torch.tensor([db], dtype=torch.float32) / 20)).item())


@dataclass(frozen=True)
class Stem:
    gain: float = 1.0                               # linear, a float32 value (gain_of_db)
    tilt: Optional[str] = None                      # None | "high" | "low"
    compress: Optional[Tuple[float, float]] = None  # None | (threshold dB, ratio)
    bw: Optional[Tuple[int, float]] = None          # None | (order 2 or 4, cutoff Hz)

    @property
    def any(self):
        return self.gain != 1.0 or self.tilt is not None or self.compress is not None or self.bw is not None


@dataclass(frozen=True)
class Clip:
    stems: Tuple[Stem, Stem, Stem, Stem] = (Stem(), Stem(), Stem(), Stem())
    reverb: int = 0                                 # 0 off | 1 mix reverb + energy redistribution | 2 plain reverb of stem 0
    ir: Optional[torch.Tensor] = None               # (L,) float32, when reverb != 0


DEFAULT_COMP = (-20.0, 4.0)


def clip_from_trace(trace) -> Clip:
    """The decision trace of `oaug.augment_stems` as a Clip."""
    stems = []
    for name in oaug.STEMS:
        t = trace[name]
        stems.append(Stem(gain=gain_of_db(t["gain_db"]) if "gain_db" in t else 1.0, tilt=t.get("tilt"),
                          compress=DEFAULT_COMP if t.get("comp") else None, bw=(4, t["cutoff"]) if "cutoff" in t else None))
    ir = trace.get("reverb_ir")
    return Clip(tuple(stems), 1 if ir is not None else 0, ir)


def fill_clips(specs, aug=None):
    """[Clip] -> (`_lib.AugClip` array, [ir | None]): what `AudioAugmenter._apply` / `augment_packed_(decisions=...)` take.
    Order 2 is ONE low-pass section (scipy's butter), order 4 the augmenter's closed-form two sections."""
    from mst_amd import _lib
    from mst_amd.mixing_utils import AudioAugmenter
    aug = aug or AudioAugmenter(SR)
    clips = (_lib.AugClip * len(specs))()
    for c, spec in zip(clips, specs):
        for st, s in zip(c.stem, spec.stems):
            st.gain = s.gain
            if s.tilt is not None:
                st.tilt = 1
                st.tilt_sos[:] = (aug._butter(2, 2000, "high") if s.tilt == "high" else aug._butter(2, 500, "low"))[0].tolist()
            if s.compress is not None:
                if tuple(s.compress) == DEFAULT_COMP:
                    st.compress = 1
                else:
                    st.compress, st.comp_threshold_db, st.comp_ratio = 2, float(s.compress[0]), float(s.compress[1])
            if s.bw is not None:
                order, fc = s.bw
                sos = aug._butter4_low(fc) if order == 4 else aug._butter(2, fc, "low")
                assert sos.shape == (order // 2, 6)
                st.bw_sections = sos.shape[0]
                st.bw_sos[:6 * sos.shape[0]] = sos.reshape(-1).tolist()
        c.reverb = spec.reverb
        assert (spec.reverb != 0) == (spec.ir is not None)
    return clips, [s.ir for s in specs]


def _chain(x2, s: Stem, comp_in=None):
    """One stem (2, T) through the oracle's chain; comp_in: list that receives the compressor's input."""
    x = x2.clone()
    if s.gain != 1.0:
        x = x * torch.tensor([s.gain], dtype=torch.float32)
    if s.tilt is not None:
        x = oaug._sosfilt32(oaug.tilt_sos(s.tilt == "high", SR), x)
    if s.compress is not None:
        if comp_in is not None:
            comp_in.append(x)
        x = oaug.compress(x, *s.compress)
    if s.bw is not None:
        x = oaug.lowpass(x, s.bw[1], SR, order=s.bw[0])
    return x


def expected(specs, x, comp_inputs=None):
    """x (B, 8, T) float32 CPU -> the (B, 8, T) the oracle's arithmetic gives for these decisions.
    comp_inputs: dict that receives {(clip, stem): compressor input} for the input conditions."""
    out = []
    for b, spec in enumerate(specs):
        stems = {}
        for i, name in enumerate(oaug.STEMS):
            sink = [] if comp_inputs is not None else None
            stems[name] = _chain(x[b, 2 * i:2 * i + 2], spec.stems[i], sink)
            if sink:
                comp_inputs[(b, i)] = sink[0]
        if spec.reverb == 1:
            stems = oaug.reverb_redistribute(stems, spec.ir)
        elif spec.reverb == 2:
            stems["vocals"] = oaug.reverb(stems["vocals"], spec.ir)
        out.append(torch.cat([stems[n] for n in oaug.STEMS], 0))
    return torch.stack(out, 0)


def expected_f64(specs, x):
    """The same chain in float64 throughout (float64 sosfilt without the oracle's `.float()`, float64 compressor and
    convolution): the yardstick for the oracle's own float32 error."""
    from scipy.signal import butter, sosfilt
    out = []
    for b, spec in enumerate(specs):
        stems = []
        for i, s in enumerate(spec.stems):
            v = x[b, 2 * i:2 * i + 2].double() * float(s.gain)
            if s.tilt is not None:
                v = torch.from_numpy(sosfilt(oaug.tilt_sos(s.tilt == "high", SR), v.numpy(), axis=-1))
            if s.compress is not None:
                v = oaug.compress(v, *s.compress)
            if s.bw is not None:
                v = torch.from_numpy(sosfilt(butter(s.bw[0], s.bw[1], btype="low", fs=SR, output="sos"), v.numpy(), axis=-1))
            stems.append(v)
        if spec.reverb == 1:
            stems = list(oaug.reverb_redistribute(dict(enumerate(stems)), spec.ir.double()).values())
        elif spec.reverb == 2:
            stems[0] = oaug.reverb(stems[0], spec.ir.double())
        out.append(torch.cat(stems, 0))
    return torch.stack(out, 0)


def edge_input(B, T, seed=0):
    """(B, 8, T): seeded noise of amplitude 0.3 plus unit impulses on both sides of every segment boundary (the state a segment
    hands to the next is then large against the tolerances), signs alternating over the channels.  The first sample of every
    channel is fixed -- 0.9 left, -0.02 right -- so that even a one-sample clip has a compressor input on each side of a threshold."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = 0.3 * torch.randn(B, 8, T, generator=g)
    sign = torch.tensor([1.0, -1.0, -1.0, 1.0, 1.0, 1.0, -1.0, -1.0])
    for n in range(SEG, T + 1, SEG):
        x[:, :, n - 1] += sign
        if n < T:
            x[:, :, n] -= 0.75 * sign
    x[:, 0::2, 0] = 0.9
    x[:, 1::2, 0] = -0.02
    return x


def make_ir(L, seed=0, decay_samples=None):
    """A seeded (L,) impulse response shaped like the reference's: exponentially decaying noise * 0.1."""
    g = torch.Generator().manual_seed(2000 + seed)
    t = torch.arange(L, dtype=torch.float32) / float(decay_samples or max(L / 4.0, 1.0))
    return torch.exp(-t) * torch.randn(L, generator=g) * 0.1


def check_conditions(specs, x, ref, silent=()):
    """The input conditions of the edge tests, from the reference alone: every compressor sees at least 5 % of its input on
    each side of its threshold, and no channel of the expected output is all zero except those listed in `silent`
    ((clip, channel) pairs), which must be."""
    comp = {}
    expected(specs, x, comp)
    for (b, i), v in comp.items():
        thr = specs[b].stems[i].compress[0]
        above = float((20 * torch.log10(v.abs() + 1e-8) > thr).float().mean())
        assert 0.05 <= above <= 0.95, f"clip {b} stem {i}: {above:.3f} of the compressor's input above {thr} dB"
    for b in range(ref.shape[0]):
        for c in range(8):
            zero = not bool(ref[b, c].any())
            assert zero == ((b, c) in silent), f"clip {b} channel {c}: all zero = {zero}"


def worst(y, ref, rtol, atol):
    """max over ALL elements of |y - ref| / (atol + rtol |ref|)  (<= 1 passes; NaN or inf anywhere fails), and the max |y - ref|."""
    y, ref = y.double(), ref.double()
    assert y.shape == ref.shape
    d = (y - ref).abs()
    q = d / (atol + rtol * ref.abs())
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))
    return (float(q.max()), float(d.max())) if q.numel() else (0.0, 0.0)


def assert_close(y, ref, rtol, atol, what=""):
    q, d = worst(y, ref, rtol, atol)
    print(f"[aug-edge] {what}: worst |err| / tol = {q:.3f}, max |err| = {d:.3e}")
    assert q <= 1.0, f"{what}: worst |err| / (atol + rtol |ref|) = {q:.3f} (max |err| {d:.3e}, rtol {rtol}, atol {atol})"
    return q


# ---------------------------------------------------------------------------------------------------------------
# The cases of tests/test_aug_edges_gpu.py: name -> (decisions, input, channels expected to be all zero).  Kept here so that
# tests/test_aug_cases_cpu.py can check their input conditions without a GPU; built and referenced once per process.
# ---------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402

TOL_CHAIN = dict(rtol=1e-5, atol=1e-6)     # filters and compressor, no reverb (test_aug_loss_gpu.py::test_single_effects)
TOL_REVERB = dict(rtol=1e-4, atol=2e-5)    # anything with reverb (test_aug_loss_gpu.py::close)
TOL_REVERB2 = dict(rtol=1e-4, atol=1e-5)   # plain reverb, mode 2 (test_single_effects)

CHAIN_T = (1, 3, 31, 32, 33, 2047, 2048, 2049, 16383, 16384, 16385, 32768, 49153)
REVERB_T = (1, 511, 512, 513, 1024, 11023, 11024, 11025, 12288)      # L = 22050: D = 11024
IR_T, IR_L = (4096, 4099), (1, 2, 511, 512, 513, 1025, 4410, 44100)
LONG_T = 257 * SEG + 33

STEMS_A = (Stem(gain=gain_of_db(-9.0), tilt="high", compress=DEFAULT_COMP, bw=(4, 4000.0)),
           Stem(gain=gain_of_db(9.0), tilt="low", bw=(2, 11999.0)),
           Stem(compress=(-12.0, 2.0)),
           Stem())
STEMS_LONG = (Stem(tilt="high", compress=DEFAULT_COMP, bw=(4, 4000.0)), Stem(bw=(2, 6000.0)), Stem(), Stem())
ENERGY_SCALE = torch.tensor([1.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.1, 0.1])[:, None]   # four stems, four energies


def _stems_combo(b):
    """Stem k = 4 b + i of (b): tilt iff k & 1, compressor iff k & 2, low-pass iff k & 4 -- all 8 combinations over two clips;
    gain alternates 1.0 / another value, the low-pass order 2 / 4, the tilt high / low, the compressor default / parametric (stem 3, behind
    the 500 Hz tilt, with a threshold low enough to be crossed)."""
    out = []
    for k in range(4 * b, 4 * b + 4):
        out.append(Stem(gain=1.0 if k % 2 == 0 else gain_of_db(-6.0 if k < 4 else 4.5),
                        tilt=(None if not k & 1 else "high" if k & 4 else "low"),
                        compress=(None if not k & 2 else DEFAULT_COMP if k & 4 else (-36.0, 3.0) if k & 1 else (-12.0, 2.0)),
                        bw=(None if not k & 4 else (2 if k % 2 == 0 else 4, 5000.0 + 700.0 * k))))
    return tuple(out)


def _reverb_input(T, seed):
    return edge_input(1, T, seed) * ENERGY_SCALE


def _builders():
    c = {}
    for T in CHAIN_T:
        c[f"a-T{T}"] = lambda T=T: ([Clip(STEMS_A)], edge_input(1, T, 1), ())
    for T in (16385, 33):
        c[f"b-T{T}"] = lambda T=T: ([Clip(_stems_combo(0)), Clip(_stems_combo(1))], edge_input(2, T, 2), ())
    c["c-chain"] = lambda: ([Clip(STEMS_A)], edge_input(1, 32768, 3), ())
    c["c-reverb"] = lambda: ([Clip(STEMS_A, 1, make_ir(22050, 3, 5512))], edge_input(1, 32768, 3), ())
    for T in REVERB_T:
        c[f"e-mode1-T{T}"] = lambda T=T: ([Clip(reverb=1, ir=make_ir(22050, T, 5512))], _reverb_input(T, 4), ())
    for T in IR_T:
        for L in IR_L:
            c[f"f-T{T}-L{L}"] = lambda T=T, L=L: ([Clip((Stem(), Stem(gain=gain_of_db(3.0), tilt="low"), Stem(), Stem()), 1,
                                                        make_ir(L, L))], _reverb_input(T, 5), ())
    ir = make_ir(1025, 6)

    def g_batch():
        x = edge_input(3, SEG + 1, 6)
        x[2] = 0.0
        return [Clip(STEMS_A, 1, ir), Clip(STEMS_A), Clip(reverb=1, ir=ir)], x, tuple((2, ch) for ch in range(8))

    def g_stem():
        x = _reverb_input(SEG + 1, 7)
        x[0, 4:6] = 0.0
        return [Clip((STEMS_A[0], STEMS_A[1], Stem(), Stem()), 1, ir)], x, ((0, 4), (0, 5))
    c["g-batch"], c["g-silent-stem"] = g_batch, g_stem
    c["h-long"] = lambda: ([Clip(STEMS_LONG)], edge_input(1, LONG_T, 8), ())
    return c


CASE_NAMES = tuple(_builders())


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (decisions [Clip], input (B, 8, T), silent channels); shared: do not modify."""
    return _builders()[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The expected (B, 8, T) of case(name); shared: do not modify."""
    specs, x, _ = case(name)
    return expected(specs, x)


def mode2_case(T, seed, decay=0.5):
    """Plain `apply_reverb(audio, decay)` under torch.manual_seed(seed): (audio (2, T), expected (2, T), the float the global
    generator yields next -- the RNG consumption of the reference's impulse-response draw)."""
    x = edge_input(1, T, 9)[0, 0:2].clone()
    torch.manual_seed(seed)
    ir = oaug.make_ir(SR, decay)
    nxt = float(torch.rand(1))
    return x, oaug.reverb(x, ir), nxt
