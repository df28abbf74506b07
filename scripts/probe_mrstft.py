"""MultiResolutionSTFTLoss: HIP-event time of the kernels (csrc/mrstft.hip) against the same class's `backend="torch"`
(torch.stft on PyTorch-ROCm), alternating in one process so both see the same machine state.

    python scripts/probe_mrstft.py [--out profiles/mrstft_probe.json] [--repeats 3] [--window 0.5]

Per batch (B x 8 x T): ms of the forward and of forward + backward (median and spread over repeats of a >= `window` s timed
loop) for both backends, the ratio, and the HBM floor the kernels are reported against: x and y read once per resolution
and pass (forward; forward + the recomputing backward), grad_x written once."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases_mrstft as cm  # noqa: E402
from mst_amd.loss import MultiResolutionSTFTLoss  # noqa: E402

BATCHES = [(8, 441000), (2, 441000)]   # the trainer's batch, and the contract size of the tests
HBM_BYTES = 8.0e12


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
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrstft_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    for B, T in BATCHES:
        x1, y1 = cm.make_xy(1, T, "near")
        x = x1.cuda().expand(B, 8, T).contiguous().requires_grad_(True)
        y = y1.cuda().expand(B, 8, T).contiguous()
        mods = {"hip": MultiResolutionSTFTLoss(), "torch": MultiResolutionSTFTLoss(backend="torch")}
        n_res = len(mods["hip"].fft_sizes)

        def fwd(m):
            with torch.no_grad():
                return m(x, y)

        def fwd_bwd(m):
            x.grad = None
            m(x, y).backward()

        vals = {k: fwd(m).item() for k, m in mods.items()}   # warm-up of both
        for m in mods.values():
            fwd_bwd(m)
        t = {(k, w): [] for k in mods for w in ("fwd", "fwd_bwd")}
        for _ in range(a.repeats):
            for k, m in mods.items():
                t[k, "fwd"].append(timed(lambda: fwd(m), a.window))
                t[k, "fwd_bwd"].append(timed(lambda: fwd_bwd(m), a.window))
        elems = B * 8 * T
        floor_fwd = n_res * 2 * elems * 4 / HBM_BYTES * 1e3
        floor_fb = (2 * n_res * 2 * elems * 4 + elems * 4) / HBM_BYTES * 1e3
        row = dict(B=B, C=8, T=T, loss_hip=vals["hip"], loss_torch=vals["torch"], floor_hbm_fwd_ms=floor_fwd,
                   floor_hbm_fwd_bwd_ms=floor_fb)
        for (k, w), v in t.items():
            row[f"{k}_{w}_ms"] = med(v)
            row[f"{k}_{w}_ms_repeats"] = v
            row[f"{k}_{w}_spread"] = (max(v) - min(v)) / med(v)
        row["torch_over_hip_fwd"] = row["torch_fwd_ms"] / row["hip_fwd_ms"]
        row["torch_over_hip_fwd_bwd"] = row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
        row["fraction_of_floor_fwd"] = floor_fwd / row["hip_fwd_ms"]
        row["fraction_of_floor_fwd_bwd"] = floor_fb / row["hip_fwd_bwd_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"),
               peaks=dict(hbm_bytes_per_s=HBM_BYTES), batches=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
