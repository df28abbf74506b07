"""TCN mixer forward: HIP-event time of the kernels (csrc/tcn.hip) against the same module's `backend="torch"` tree on
PyTorch-ROCm / MIOpen, alternating in one process so both see the same machine state.

    python scripts/probe_tcn.py [--out profiles/tcn_probe.json] [--repeats 3] [--window 0.5] [--only 0,3]

Per geometry (H, blocks, K, B, T): ms per forward (median and spread over repeats of a >= `window` s timed loop),
algorithmic flop (2*nb*2*H^2*K + 2*2*8*H per sample) and executed flop (padded channels, minus the taps whose strip lies
wholly outside the clip for a wave's tile -- the rule of tcn_conv_kernel), algorithmic bytes (fp32 activations layer by
layer: per block conv1 read + write, conv2 read + residual read + write; plus the two projections), the bounding floor
(fp32 MFMA 157.3 TF/s or HBM 8 TB/s, whichever is larger) and the fraction of it reached, the torch time and the ratio.

    python scripts/probe_tcn.py --f16x3 [--out profiles/tcn_f16x3_probe.json] [--repeats 5]

The opt-in split-precision mode (TCNMixer.precision = "f16x3", csrc/tcn_f16x3.inc) at the wide mixer (H = 128, B = 1, 10 s)
and the trainer's (H = 16, B = 8): fp32 kernels, f16x3 kernels and the torch tree alternate in ONE process; per mode the
repeats, median, min and max; the f16 MFMA flop executed by the three products (padded to 32 input channels) as a fraction
of the 2.5 PFLOP/s data-sheet peak; the distance of the f16x3 y from the fp32 kernels' (element-wise, floor 1 % of the
maximum, and norm-wise); and whether the f16x3 median lies below the fp32 minimum."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import cases_tcn as ct  # noqa: E402
from mst_amd import tcn_mixer as tm  # noqa: E402

GEOMETRIES = [(16, 14, 15, 8, 441000), (64, 10, 15, 2, 441000), (128, 14, 15, 1, 441000), (16, 8, 5, 8, 441000)]
MFMA_F32_FLOPS, HBM_BYTES = 157.3e12, 8.0e12
MFMA_F16_FLOPS = 2.5e15          # data sheet, dense f16
F16X3_GEOMETRIES = (2, 0)        # wide128 1 x 10 s; st_default 8 x 10 s


def flop_counts(H, nb, K, B, T, causal=False):
    HP = (H + 15) // 16 * 16
    tile = 16 * (8 if HP <= 32 else 4)          # samples per wave (launch table of csrc/tcn.hip)
    alg = B * T * (2 * nb * 2 * H * H * K + 2 * 2 * 8 * H)
    ntile = (T + tile - 1) // tile
    t0 = torch.arange(ntile, dtype=torch.int64) * tile
    strips = 0
    for k in range(nb):
        d = 2 ** k
        off0 = -(K - 1) * d if causal else -((K - 1) * d // 2)
        for tap in range(K):
            ts = t0 + off0 + tap * d
            strips += int(((ts < T) & (ts + tile > 0)).sum())
    exe = B * (2 * strips * tile * 2 * HP * HP + T * 2 * 2 * 8 * HP)
    byt = B * T * 4 * (nb * 5 * H + 2 * H + 3 * 8)
    return alg, exe, byt


def timed(fn, window):
    """ms per call over a loop of >= window seconds (HIP events), after one call to size the loop."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(2, int(window * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def stats(v):
    return dict(repeats=v, median=sorted(v)[len(v) // 2], min=min(v), max=max(v))


def main_f16x3(a):
    rows = []
    for gi in F16X3_GEOMETRIES:
        H, nb, K, B, T = GEOMETRIES[gi]
        c = dict(H=H, nb=nb, K=K, causal=False, film=True, B=B, T=T)
        tcn = tm.TCNMixer(**ct.mixer_kwargs(c))
        tcn.load_state_dict(ct.make_tcn_state_dict(c))
        gen = tm.TCNFiLMGenerator(embed_dim=ct.EMBED, num_blocks=nb, hidden_channels=H)
        gen.load_state_dict(ct.make_film_state_dict(ct.EMBED, c))
        tcn, gen = tcn.cuda().eval(), gen.cuda().eval()
        x = cases.pcm_batch(1, T).cuda().expand(B, 8, T).contiguous()
        with torch.no_grad():
            params = gen(ct.embeddings(B, ct.EMBED).cuda())

            def run(backend, precision):
                def fn():
                    tcn.backend, tcn.precision = backend, precision
                    try:
                        return tcn(x, film_params=params)
                    finally:
                        tcn.backend, tcn.precision = "hip", "fp32"
                return fn
            modes = dict(fp32=run("hip", "fp32"), f16x3=run("hip", "f16x3"), torch=run("torch", "fp32"))
            y = {k: fn().double() for k, fn in modes.items()}   # warm-up of all three
            ref = y["fp32"]
            d = (y["f16x3"] - ref).abs()
            scale = float(ref.abs().max())
            dist = dict(elementwise_max_rel=float((d / ref.abs().clamp(min=1e-2 * scale)).max()), normwise=float(d.max()) / scale,
                        torch_vs_fp32_normwise=float((y["torch"] - ref).abs().max()) / scale)
            del y, ref, d
            ms = {k: [] for k in modes}
            for _ in range(a.repeats):
                for k, fn in modes.items():   # alternating: every mode sees the same machine state
                    ms[k].append(timed(fn, a.window)[0])
        HP, HP32 = (H + 15) // 16 * 16, (H + 31) // 32 * 32
        alg, exe32, _ = flop_counts(H, nb, K, B, T)
        proj = B * T * 2 * 2 * 8 * HP
        exe16 = (exe32 - proj) * 3 * HP32 // HP
        st = {k: stats(v) for k, v in ms.items()}
        row = dict(H=H, num_blocks=nb, kernel_size=K, B=B, T=T, ms=st, algorithmic_flop=alg, executed_f16_mfma_flop=exe16,
                   f16x3_fraction_of_f16_peak=exe16 / (st["f16x3"]["median"] * 1e-3) / MFMA_F16_FLOPS,
                   fp32_fraction_of_fp32_peak=(exe32 - proj) / (st["fp32"]["median"] * 1e-3) / MFMA_F32_FLOPS,
                   fp32_median_over_f16x3_median=st["fp32"]["median"] / st["f16x3"]["median"],
                   torch_median_over_f16x3_median=st["torch"]["median"] / st["f16x3"]["median"],
                   f16x3_median_below_fp32_min=st["f16x3"]["median"] < st["fp32"]["min"], y_f16x3_vs_fp32=dist)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del tcn, gen, x, params
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"), window_s=a.window,
               peaks=dict(f16_mfma_flops=MFMA_F16_FLOPS, fp32_mfma_flops=MFMA_F32_FLOPS), geometries=rows)
    path = a.out or os.path.join(ROOT, "profiles", "tcn_f16x3_probe.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/tcn_probe.json, with --f16x3 profiles/tcn_f16x3_probe.json")
    ap.add_argument("--f16x3", action="store_true", help="fp32 kernels, f16x3 kernels and the torch tree at the mode's two shapes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-torch", action="store_true", help="kernels only (for a rocprofv3 kernel table)")
    a = ap.parse_args()
    if a.f16x3:
        return main_f16x3(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "tcn_probe.json")
    pick = [int(i) for i in a.only.split(",")] if a.only else range(len(GEOMETRIES))
    rows = []
    for gi in pick:
        H, nb, K, B, T = GEOMETRIES[gi]
        c = dict(H=H, nb=nb, K=K, causal=False, film=True, B=B, T=T)
        tcn = tm.TCNMixer(**ct.mixer_kwargs(c))
        tcn.load_state_dict(ct.make_tcn_state_dict(c))
        gen = tm.TCNFiLMGenerator(embed_dim=ct.EMBED, num_blocks=nb, hidden_channels=H)
        gen.load_state_dict(ct.make_film_state_dict(ct.EMBED, c))
        tcn, gen = tcn.cuda().eval(), gen.cuda().eval()
        x = cases.pcm_batch(1, T).cuda().expand(B, 8, T).contiguous()
        emb = ct.embeddings(B, ct.EMBED).cuda()
        with torch.no_grad():
            params = gen(emb)
            run_hip = lambda: tcn(x, film_params=params)  # noqa: E731

            def run_torch():
                tcn.backend = "torch"
                try:
                    return tcn(x, film_params=params)
                finally:
                    tcn.backend = "hip"
            y = run_hip()
            diff = None
            if not a.no_torch:
                yt = run_torch()                      # warm-up of both (MIOpen picks its kernels here)
                diff = float((y - yt).abs().max() / yt.abs().max())
                del yt
            del y
            hip, tor = [], []
            for _ in range(a.repeats):
                hip.append(timed(run_hip, a.window)[0])
                if not a.no_torch:
                    tor.append(timed(run_torch, a.window)[0])
        alg, exe, byt = flop_counts(H, nb, K, B, T)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        ms = med(hip)
        floor_mfma, floor_hbm = alg / MFMA_F32_FLOPS * 1e3, byt / HBM_BYTES * 1e3
        row = dict(H=H, num_blocks=nb, kernel_size=K, B=B, T=T, hip_ms=ms, hip_ms_repeats=hip,
                   hip_spread=(max(hip) - min(hip)) / ms, algorithmic_flop=alg, executed_flop=exe, algorithmic_bytes=byt,
                   tflops_algorithmic=alg / ms / 1e9, tflops_executed=exe / ms / 1e9,
                   floor_ms=max(floor_mfma, floor_hbm), floor_bound="fp32 MFMA" if floor_mfma >= floor_hbm else "HBM",
                   floor_mfma_ms=floor_mfma, floor_hbm_ms=floor_hbm, fraction_of_floor=max(floor_mfma, floor_hbm) / ms)
        if tor:
            mt = med(tor)
            row.update(torch_ms=mt, torch_ms_repeats=tor, torch_spread=(max(tor) - min(tor)) / mt, torch_over_hip=mt / ms,
                       max_diff_rel_to_max=diff)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del tcn, gen, x, params
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"),
               peaks=dict(fp32_mfma_flops=MFMA_F32_FLOPS, hbm_bytes_per_s=HBM_BYTES), geometries=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
