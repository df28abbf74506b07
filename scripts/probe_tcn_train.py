"""TCN mixer training step (train-mode forward + full backward): HIP-event time of `backend="hip-train"` (csrc/tcn_train.inc)
against the same module's `backend="torch"` tree under PyTorch-ROCm autograd, alternating in one process.

    python scripts/probe_tcn_train.py [--out profiles/tcn_train_probe.json] [--repeats 3] [--window 0.5] [--only 0]

Per geometry (H, blocks, K, B, T): ms per forward + backward of loss = sum(y * dy) (median and spread over repeats of a
>= `window` s timed loop), the algorithmic flop (3 x the forward's: convolution, input gradient, weight gradient), the
executed flop (padded channels; forward and input gradient skip a tap per wave tile as tcn_conv_kernel does, the weight
gradient per wave chunk as tcn_wgrad_kernel does), the arithmetic floor (3 x the forward's fp32-MFMA floor, 157.3 TF/s)
and the saved bytes of the step."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import cases  # noqa: E402
import cases_tcn as ct  # noqa: E402
import cases_tcn_train as ctt  # noqa: E402
from mst_amd import tcn_mixer as tm  # noqa: E402
from probe_tcn import MFMA_F32_FLOPS, flop_counts, timed  # noqa: E402

GEOMETRIES = [(16, 14, 15, 8, 441000), (128, 14, 15, 1, 441000)]   # the trainer's defaults; the class defaults
ROWS_WAVE = 512   # kRowsWave of csrc/tcn_train.inc


def wgrad_executed(H, nb, K, B, T):
    HP = (H + 15) // 16 * 16
    t0 = torch.arange((T + ROWS_WAVE - 1) // ROWS_WAVE, dtype=torch.int64) * ROWS_WAVE
    rows = (torch.clamp(t0 + ROWS_WAVE, max=T) - t0 + 3) // 4 * 4
    total = 0
    for k in range(nb):
        d = 2 ** k
        off0 = -((K - 1) * d // 2)
        for tap in range(K):
            s0 = t0 + off0 + tap * d
            total += int((rows * ((s0 < T) & (s0 + rows > 0))).sum())
    return B * 2 * total * 2 * HP * HP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcn_train_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-torch", action="store_true", help="kernels only (for a rocprofv3 kernel table)")
    a = ap.parse_args()
    pick = [int(i) for i in a.only.split(",")] if a.only else range(len(GEOMETRIES))
    rows = []
    for gi in pick:
        H, nb, K, B, T = GEOMETRIES[gi]
        c = dict(H=H, nb=nb, K=K, causal=False, film=True, B=B, T=T)
        tcn = tm.TCNMixer(**ct.mixer_kwargs(c))
        tcn.load_state_dict(ct.make_tcn_state_dict(c))
        tcn = tcn.cuda().train()
        x = cases.pcm_batch(1, T).cuda().expand(B, 8, T).contiguous().requires_grad_()
        film = ctt.film_tensor(c).cuda().requires_grad_()
        dy = ctt.dy_tensor(dict(B=1, T=T)).cuda().expand(B, 8, T).contiguous()

        def step(backend):
            tcn.backend = backend
            x.grad = film.grad = None
            tcn.zero_grad(set_to_none=True)
            y = tcn(x, film_params=ctt.film_dicts(film))
            y.backward(dy)
            return y.detach(), x.grad

        y, dx = step("hip-train")
        diff = None
        if not a.no_torch:
            yt, dxt = step("torch")                  # warm-up of both (MIOpen picks its kernels here)
            diff = dict(y=float((y - yt).abs().max() / yt.abs().max()), dx=float((dx - dxt).abs().max() / dxt.abs().max()))
            del yt, dxt
        del y, dx
        hip, tor = [], []
        for _ in range(a.repeats):
            hip.append(timed(lambda: step("hip-train"), a.window)[0])
            if not a.no_torch:
                tor.append(timed(lambda: step("torch"), a.window)[0])
        alg, exe, _ = flop_counts(H, nb, K, B, T)
        conv_exe = exe - B * T * 2 * 2 * 8 * ((H + 15) // 16 * 16)
        alg3, exe3 = 3 * alg, 2 * conv_exe + wgrad_executed(H, nb, K, B, T) + 3 * (exe - conv_exe)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        ms = med(hip)
        HP = (H + 15) // 16 * 16
        row = dict(H=H, num_blocks=nb, kernel_size=K, B=B, T=T, hip_ms=ms, hip_ms_repeats=hip, hip_spread=(max(hip) - min(hip)) / ms,
                   algorithmic_flop=alg3, executed_flop=exe3, tflops_algorithmic=alg3 / ms / 1e9, tflops_executed=exe3 / ms / 1e9,
                   floor_mfma_ms=alg3 / MFMA_F32_FLOPS * 1e3, fraction_of_floor=alg3 / MFMA_F32_FLOPS * 1e3 / ms,
                   saved_bytes=B * T * (3 * nb + 1) * HP * 4)
        if tor:
            mt = med(tor)
            row.update(torch_ms=mt, torch_ms_repeats=tor, torch_spread=(max(tor) - min(tor)) / mt, torch_over_hip=mt / ms,
                       max_diff_rel_to_max=diff)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del tcn, x, film, dy
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"),
               peaks=dict(fp32_mfma_flops=MFMA_F32_FLOPS), geometries=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
