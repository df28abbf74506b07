"""Block-wise streaming of a causal TCN mixer (TCNMixer.stream, csrc/tcn_stream.inc): time per push against the block's
duration, against the offline forward's time per sample, and against the same TCNStream on backend="torch" (PyTorch-ROCm).

    python scripts/probe_tcn_stream.py [--out profiles/tcn_stream_probe.json] [--repeats 3] [--window 0.5]

Mixers (H, blocks, K) = (16, 14, 15) and (128, 14, 15), causal, FiLM, seeded weights; B = 1 and 8 streams; blocks of 128, 512,
2048 and 16 384 samples (max_block = the block).  Per (mixer, B, block) and arm (`hip`, `torch`): ms per push = HIP-event time
of a loop of >= `window` s of pushes of one fixed block after a warm-up push, `repeats` times with the arms alternating in one
process; median and spread (max - min over the median).  `realtime_x` = the block's duration at 44.1 kHz over the median.
`offline`: mst_tcn_forward (TCNMixer.forward) on 10 s clips of the same mixer and B, ms per call and ns per sample and stream;
`stream_over_offline` = time per sample of the pushes over that: the throughput cost of streaming.  `samples_per_wave`: the time
tile the convolution kernel ran (mst_tcn_stream_samples_per_wave).  The stream keeps running
through the loop (its position grows), so every push sees warm rings.  Every mixer runs in a child process of its own under
`timeout`; the first one that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIXERS = {"h16": (16, 14, 15), "h128": (128, 14, 15)}
BATCHES = (1, 8)
BLOCKS = (128, 512, 2048, 16384)
OFFLINE_T = 441000
SAMPLE_RATE = 44100
CHILD_TIMEOUT_S = 420


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


def median(v):
    return sorted(v)[len(v) // 2]


def stats(v):
    m = median(v)
    return dict(ms=m, ms_repeats=v, spread=(max(v) - min(v)) / m)


def run_mixer(name, repeats, window):
    import copy

    import torch
    from mst_amd import _lib
    from mst_amd.tcn_mixer import TCNMixer
    H, nb, K = MIXERS[name]
    torch.manual_seed(0)
    hip = TCNMixer(hidden_channels=H, num_blocks=nb, kernel_size=K, causal=True, use_film=True)
    with torch.no_grad():
        hip.output_conv.weight.mul_(100.0)   # (the 0.001 init would leave y = x to three digits)
    hip = hip.cuda().eval()
    ref = copy.deepcopy(hip)
    ref.backend = "torch"
    rows = []
    with torch.no_grad():
        for B in BATCHES:
            g = torch.Generator(device="cuda").manual_seed(1)
            film_t = 1.0 + 0.3 * (2 * torch.rand(B, nb, 4, H, device="cuda", generator=g) - 1)
            film = [{k: film_t[:, i, q] for q, k in enumerate(("gamma1", "beta1", "gamma2", "beta2"))} for i in range(nb)]
            xl = 0.5 * (2 * torch.rand(B, 8, OFFLINE_T, device="cuda", generator=g) - 1)
            hip(xl, film_params=film)        # warm-up of the shape
            off = stats([timed(lambda: hip(xl, film_params=film), window) for _ in range(repeats)])
            off_ns = 1e6 * off["ms"] / OFFLINE_T / B
            rows.append(dict(mixer=name, H=H, blocks=nb, K=K, B=B, arm="offline", T=OFFLINE_T, ns_per_sample_and_stream=off_ns, **off))
            for N in BLOCKS:
                x = xl[:, :, :N].contiguous()
                arms = {"hip": hip.stream(batch_size=B, max_block=N, film_params=film),
                        "torch": ref.stream(batch_size=B, max_block=N, film_params=film)}
                same = float((arms["hip"].push(x) - arms["torch"].push(x)).abs().max())   # warm-up, and the arms agree
                tile = _lib.lib().mst_tcn_stream_samples_per_wave(arms["hip"]._handle.ptr, B, N)
                ms = {arm: [] for arm in arms}
                for _ in range(repeats):
                    for arm, s in arms.items():
                        ms[arm].append(timed(lambda s=s: s.push(x), window))
                audio_ms = 1e3 * N / SAMPLE_RATE
                for arm in arms:
                    st = stats(ms[arm])
                    rows.append(dict(mixer=name, H=H, blocks=nb, K=K, B=B, arm=arm, block=N, block_ms_at_44k1=audio_ms,
                                     realtime_x=audio_ms / st["ms"], ns_per_sample_and_stream=1e6 * st["ms"] / N / B,
                                     stream_over_offline=1e6 * st["ms"] / N / B / off_ns, first_push_max_abs_diff_hip_torch=same,
                                     state_mib=arms[arm].state_bytes / 2 ** 20, launches_per_push=2 * nb + 2 if arm == "hip" else None,
                                     samples_per_wave=tile if arm == "hip" else None,
                                     **st))
                del arms
                print(f"{name} B={B} block={N} done", file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcn_stream_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--mixer", default=None, choices=list(MIXERS), help="(child) run this mixer alone and print its rows")
    a = ap.parse_args()
    if a.mixer is not None:
        import torch
        rows = run_mixer(a.mixer, a.repeats, a.window)
        print("ROWS " + json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rows=rows)), flush=True)
        return
    rows, meta = [], {}
    for name in MIXERS:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--mixer", name,
                            "--repeats", str(a.repeats), "--window", str(a.window)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:   # (the child's stderr, with its progress lines, goes straight through)
            sys.exit(f"mixer {name} failed (exit {r.returncode}); nothing further is started\n" + r.stdout[-2000:])
        got = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("ROWS "))[5:])
        meta = dict(device=got["device"], torch=got["torch"])
        rows += got["rows"]
        for row in got["rows"]:
            print(json.dumps({k: v for k, v in row.items() if k != "ms_repeats"}), flush=True)
    out = dict(**meta, when=time.strftime("%Y-%m-%d"), sample_rate=SAMPLE_RATE, repeats=a.repeats, window_s=a.window,
               what="ms per TCNStream.push (HIP events, median of repeats, arms alternating) per mixer, B and block; offline = "
                    "TCNMixer.forward on 10 s clips", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
