"""Adversarial branch (GRL -> SongIdentityDiscriminator -> cosine-distance loss), forward + backward: HIP-event time and launch
count of `backend="hip"` (csrc/head.hip) against the same modules' `backend="torch"` on PyTorch-ROCm, alternating in one
process so both see the same machine state.

    python scripts/probe_adv.py [--out profiles/adv_probe.json] [--repeats 5] [--window 0.3]

Two shapes: the package default (K = 48 valid rows, 768 -> 512 -> 512) and the reference's train_baseline.sh (K = 200,
512 -> 512 -> 512), train mode with Dropout 0.3.  Per shape and backend: ms per forward + backward (median and spread over
repeats of a >= `window` s timed loop after a warm-up call) and the number of kernel launches of one forward + backward
(torch.profiler's device events).  The arithmetic is tiny (0.2 GFLOP at K = 200): what is measured is launch count and latency."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mst_amd.grl import GradientReversalLayer  # noqa: E402
from mst_amd.loss import cosine_distance_loss  # noqa: E402
from mst_amd.model import SongIdentityDiscriminator  # noqa: E402

SHAPES = [dict(name="default", K=48, in_dim=768, hidden=512, out_dim=512),
          dict(name="train_baseline.sh", K=200, in_dim=512, hidden=512, out_dim=512)]


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


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    return len(names), sorted(set(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adv_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    rows = []
    for sh in SHAPES:
        torch.manual_seed(0)
        disc = SongIdentityDiscriminator(sh["in_dim"], sh["hidden"], sh["out_dim"], dropout=0.3).cuda().train()
        grl = GradientReversalLayer(0.5)
        emb = torch.randn(sh["K"], sh["in_dim"], device="cuda", requires_grad=True)
        target = torch.randn(sh["K"], sh["out_dim"], device="cuda")

        def step(backend):
            disc.backend = backend
            emb.grad = None
            for q in disc.parameters():
                q.grad = None
            loss = cosine_distance_loss(disc(grl(emb)), target, backend=backend)
            loss.backward()
            return loss

        row = dict(sh)
        torch.manual_seed(1)
        l_hip = step("hip")
        g_hip = emb.grad.clone()
        disc.eval()     # Dropout off: the two backends compute the same function
        l_hip, l_tor = step("hip").item(), step("torch").item()
        disc.train()
        row["loss_hip_eval"], row["loss_torch_eval"] = l_hip, l_tor
        assert torch.isfinite(g_hip).all()
        ms = {"hip": [], "torch": []}
        for _ in range(a.repeats):
            for backend in ("hip", "torch"):
                ms[backend].append(timed(lambda: step(backend), a.window))
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        for backend in ("hip", "torch"):
            m = med(ms[backend])
            row[f"{backend}_ms"], row[f"{backend}_ms_repeats"], row[f"{backend}_spread"] = m, ms[backend], (max(ms[backend]) - min(ms[backend])) / m
            try:
                row[f"{backend}_launches"], row[f"{backend}_kernels"] = count_launches(lambda: step(backend))
            except Exception as e:     # the profiler is optional: the timings stand without it
                row[f"{backend}_launches"], row[f"{backend}_kernels"] = None, [f"profiler unavailable: {e}"]
        row["torch_over_hip"] = row["torch_ms"] / row["hip_ms"]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_kernels")}), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, when=time.strftime("%Y-%m-%d"),
               what="GRL + discriminator + cosine-distance loss, forward + backward, train mode, Dropout 0.3", shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
