"""TCNFiLMGenerator in training, forward + backward of sum(film * R): HIP-event time and launch count of
`backend="hip", train_backend="hip"` (csrc/head.hip) against the same module's `backend="torch"` on PyTorch-ROCm, alternating
in one process so both see the same machine state.

    python scripts/probe_tcn_film_train.py [--out profiles/tcn_film_train_probe.json] [--repeats 3] [--window 0.5]

Two shapes of the style-transfer trainer: B = 8, embed_dim 1024, 14 blocks, H = 16 (out_dim 896) and H = 128 (out_dim 7168),
train mode with the module's Dropout 0.1.  Per shape and backend: ms per forward + backward (median and spread over repeats of a
>= `window` s timed loop after a warm-up call) and the number of kernel launches of one forward + backward (torch.profiler's
device events).  The arithmetic is tiny: what is measured is launch count and latency.  Every shape runs in a child process
of its own under `timeout`; the first one that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(name="H16", B=8, embed_dim=1024, num_blocks=14, hidden_channels=16),
          dict(name="H128", B=8, embed_dim=1024, num_blocks=14, hidden_channels=128)]
CHILD_TIMEOUT_S = 180


def timed(fn, window):
    """ms per call over a loop of >= window seconds (HIP events), after one call to size the loop."""
    import torch
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
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    return len(names), sorted(set(names))


def run_shape(sh, repeats, window):
    import torch
    from mst_amd.tcn_mixer import TCNFiLMGenerator
    torch.manual_seed(0)
    gen = TCNFiLMGenerator(embed_dim=sh["embed_dim"], num_blocks=sh["num_blocks"], hidden_channels=sh["hidden_channels"]).cuda().train()
    gen.train_backend = "hip"
    emb = torch.randn(sh["B"], sh["embed_dim"], device="cuda")     # from torch.no_grad() in the trainer: no gradient
    R = torch.randn(sh["B"], sh["num_blocks"], 4, sh["hidden_channels"], device="cuda")

    def step(backend):
        gen.backend = backend
        for q in gen.parameters():
            q.grad = None
        film = gen.film_tensor(emb)
        (film * R).sum().backward()
        return film

    row = dict(sh)
    gen.eval()     # Dropout off: the two backends compute the same function
    f_hip, f_tor = step("hip").detach(), step("torch").detach()
    gen.train()
    row["max_abs_diff_eval"], row["max_abs_film_eval"] = float((f_hip - f_tor).abs().max()), float(f_tor.abs().max())
    ms = {"hip": [], "torch": []}
    for _ in range(repeats):
        for backend in ("hip", "torch"):
            ms[backend].append(timed(lambda: step(backend), window))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for backend in ("hip", "torch"):
        m = med(ms[backend])
        row[f"{backend}_ms"], row[f"{backend}_ms_repeats"], row[f"{backend}_spread"] = m, ms[backend], (max(ms[backend]) - min(ms[backend])) / m
        try:
            row[f"{backend}_launches"], row[f"{backend}_kernels"] = count_launches(lambda: step(backend))
        except Exception as e:     # the profiler is optional: the timings stand without it
            row[f"{backend}_launches"], row[f"{backend}_kernels"] = None, [f"profiler unavailable: {e}"]
    row["torch_over_hip"] = row["torch_ms"] / row["hip_ms"]
    row["device"], row["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcn_film_train_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shape", default=None, help="(child) run this shape alone and print its row")
    a = ap.parse_args()
    if a.shape is not None:
        print("ROW " + json.dumps(run_shape(next(s for s in SHAPES if s["name"] == a.shape), a.repeats, a.window)), flush=True)
        return
    rows = []
    for sh in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--shape", sh["name"],
                            "--repeats", str(a.repeats), "--window", str(a.window)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"shape {sh['name']} failed (exit {r.returncode}); nothing further is started\n" + r.stdout[-2000:] + r.stderr[-4000:])
        row = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("ROW "))[4:])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_kernels")}), flush=True)
    out = dict(device=rows[0].pop("device"), torch=rows[0].pop("torch_version"), when=time.strftime("%Y-%m-%d"),
               what="TCNFiLMGenerator forward + backward of sum(film * R), train mode, Dropout 0.1, embedding without gradient", shapes=rows)
    for row in rows[1:]:
        row.pop("device"), row.pop("torch_version")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
