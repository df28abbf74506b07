"""The optimiser tail (clip_grad_norm_ + AdamW step) on csrc/optim.hip against PyTorch's own, and the per-pair fit loop with and
without its per-step host synchronisation: HIP-event time and launch count, alternating in one process so every arm sees the same
machine state.

    python scripts/probe_optim.py [--out profiles/optim_probe.json] [--repeats 3] [--window 0.5]

Parameter sets: (a) `encoder` = the default MixingStyleEncoder, (b) `mixer` = the 16-channel, 14-block FiLM TCNMixer plus its
TCNFiLMGenerator (two clip calls, one optimiser, as examples/train_tcn_mixer.py).  Arms: `hip` = mst_amd.optim.clip_grad_norm_ +
mst_amd.optim.AdamW; `foreach` / `fused` = torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True / fused=True).  Per
arm: ms per clip + step (median and spread over repeats of a >= `window` s timed loop after a warm-up call) and the number of
kernel launches of one clip + step (torch.profiler's device events).  Gradients are fixed random tensors; after the first clip
their norm is max_norm, so every later call takes the same path in every arm.
`fit` = optimize_tcn_style_transfer, 200 steps on a one-second clip (hidden 8, 6 blocks, kernel 15, default encoder): wall ms per
step with sync="deferred" against sync="step".
Every set runs in a child process of its own under `timeout`; the first one that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = ("encoder", "mixer", "fit")
CHILD_TIMEOUT_S = 240
FIT_STEPS = 200


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


def median(v):
    return sorted(v)[len(v) // 2]


def param_lists(which):
    """[[parameters of one clip call], ...] of the set, on the GPU."""
    import torch
    torch.manual_seed(0)
    if which == "encoder":
        from mst_amd.model import MixingStyleEncoder
        return [list(MixingStyleEncoder().cuda().parameters())]
    from mst_amd.tcn_mixer import TCNFiLMGenerator, TCNMixer
    tcn = TCNMixer(hidden_channels=16, num_blocks=14, kernel_size=15, use_film=True).cuda()
    gen = TCNFiLMGenerator(embed_dim=1024, num_blocks=14, hidden_channels=16).cuda()
    return [list(tcn.parameters()), list(gen.parameters())]


def run_tail(which, repeats, window):
    import torch
    from mst_amd import optim as hip_optim
    arms = {}
    for arm in ("hip", "foreach", "fused"):
        lists = param_lists(which)
        g = torch.Generator(device="cuda").manual_seed(1)
        for p in (p for ps in lists for p in ps):
            p.grad = 1e-2 * torch.randn(p.shape, device="cuda", generator=g)
        flat = [p for ps in lists for p in ps]
        if arm == "hip":
            opt, clip = hip_optim.AdamW(flat, lr=1e-4, weight_decay=1e-4), hip_optim.clip_grad_norm_
        else:
            opt, clip = torch.optim.AdamW(flat, lr=1e-4, weight_decay=1e-4, **{arm: True}), torch.nn.utils.clip_grad_norm_

        def tail(lists=lists, opt=opt, clip=clip):
            for ps in lists:
                clip(ps, 1.0)
            opt.step()
        arms[arm] = tail
    row = dict(set=which, tensors=sum(len(ps) for ps in param_lists(which)),
               elements=sum(p.numel() for ps in param_lists(which) for p in ps))
    ms = {arm: [] for arm in arms}
    for _ in range(repeats):
        for arm, fn in arms.items():
            ms[arm].append(timed(fn, window))
    for arm, fn in arms.items():
        m = median(ms[arm])
        row[f"{arm}_ms"], row[f"{arm}_ms_repeats"], row[f"{arm}_spread"] = m, ms[arm], (max(ms[arm]) - min(ms[arm])) / m
        try:
            row[f"{arm}_launches"], row[f"{arm}_kernels"] = count_launches(fn)
        except Exception as e:     # the profiler is optional: the timings stand without it
            row[f"{arm}_launches"], row[f"{arm}_kernels"] = None, [f"profiler unavailable: {e}"]
    row["foreach_over_hip"], row["fused_over_hip"] = row["foreach_ms"] / row["hip_ms"], row["fused_ms"] / row["hip_ms"]
    return row


def run_fit(repeats):
    import torch
    from mst_amd.mixing_utils import STEMS
    from mst_amd.model import MixingStyleEncoder
    from mst_amd.synth import synth_batch
    from mst_amd.tcn_mixer import TCNMixer, optimize_tcn_style_transfer
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    enc = MixingStyleEncoder(embed_dim=512, feature_dim=64, encoder_backend="hip").to(dev).eval()
    for q in enc.parameters():
        q.requires_grad_(False)
    enc.input_grad_backend = "hip"
    x = synth_batch(1, 44100)[0]
    stems = {s: x[2 * i:2 * i + 2] for i, s in enumerate(STEMS)}
    target = torch.nn.functional.normalize(torch.randn(512), dim=0)

    def fit(sync, steps=FIT_STEPS):
        torch.manual_seed(1)
        tcn = TCNMixer(hidden_channels=8, num_blocks=6, kernel_size=15, use_film=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = optimize_tcn_style_transfer(tcn, stems, target, enc, None, dev, num_steps=steps, lr=0.01, verbose=False, sync=sync)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps, out

    fit("deferred", 5), fit("step", 5)   # warm-up: handles, tables, allocator
    ms, outs = {"deferred": [], "step": []}, {}
    for _ in range(repeats):
        for sync in ms:
            t, outs[sync] = fit(sync)
            ms[sync].append(t)
    row = dict(set="fit", steps=FIT_STEPS, samples=44100, same_distances=outs["deferred"]["distances"] == outs["step"]["distances"],
               first_distance=outs["deferred"]["distances"][0], best_distance=outs["deferred"]["final_distance"])
    for sync, v in ms.items():
        row[f"{sync}_wall_ms_per_step"], row[f"{sync}_wall_ms_repeats"] = median(v), v
    row["step_over_deferred"] = row["step_wall_ms_per_step"] / row["deferred_wall_ms_per_step"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--set", default=None, choices=SETS, help="(child) run this set alone and print its row")
    a = ap.parse_args()
    if a.set is not None:
        import torch
        row = run_fit(a.repeats) if a.set == "fit" else run_tail(a.set, a.repeats, a.window)
        row["device"], row["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
        print("ROW " + json.dumps(row), flush=True)
        return
    rows = []
    for which in SETS:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--set", which,
                            "--repeats", str(a.repeats), "--window", str(a.window)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"set {which} failed (exit {r.returncode}); nothing further is started\n" + r.stdout[-2000:] + r.stderr[-4000:])
        row = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("ROW "))[4:])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_kernels")}), flush=True)
    out = dict(device=rows[0]["device"], torch=rows[0]["torch_version"], when=time.strftime("%Y-%m-%d"),
               what="clip_grad_norm_ + AdamW step per parameter set (HIP events), and the per-pair fit loop's wall time per step", sets=rows)
    for row in rows:
        row.pop("device"), row.pop("torch_version")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
