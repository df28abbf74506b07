"""Fixed-latency streaming of a non-causal TCN mixer (TCNMixer.lookahead_stream, csrc/tcn_lookahead.inc): time per push next
to the causal stream's on the same geometry, and TCNMixer.forward_blockwise of a 10 s clip against the offline forward.

    python scripts/probe_tcn_lookahead.py [--out profiles/tcn_lookahead_probe.json] [--repeats 3] [--window 0.5]

The method of probe_tcn_stream.py.  Mixers (H, blocks, K) = (16, 14, 15) and (128, 14, 15), FiLM, seeded weights, once causal
and once not; B = 1 and 8 streams; blocks of 128, 512, 2048 and 16 384 samples (max_block = the block).  Per (mixer, B, block)
and arm (`causal` = TCNStream.push, `lookahead` = TCNLookaheadStream.push): ms per push = HIP-event time of a loop of >= `window`
s of pushes of one fixed block after a warm-up push, `repeats` times with the arms alternating in one process; median and
spread (max - min over the median).  The lookahead stream is moved past its latency before it is timed (its sample counter
is set to latency + block), so every row of every layer is inside the clip and no tile takes the all-zero shortcut: the steady
state of a long stream.  `blockwise`: forward_blockwise(block = 65 536) of a 10 s clip, B = 1, against the offline forward of
the same non-causal mixer, alternating, ms per call.  Every mixer runs in a child process of its own under `timeout`; the first
one that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_tcn_stream import BATCHES, BLOCKS, MIXERS, OFFLINE_T, SAMPLE_RATE, stats, timed  # noqa: E402

CHILD_TIMEOUT_S = 420
BLOCKWISE_BLOCK = 65536


def run_mixer(name, repeats, window):
    import torch
    from mst_amd.tcn_mixer import TCNMixer
    H, nb, K = MIXERS[name]
    mixers = {}
    for arm, causal in (("causal", True), ("lookahead", False)):
        torch.manual_seed(0)
        m = TCNMixer(hidden_channels=H, num_blocks=nb, kernel_size=K, causal=causal, use_film=True)
        with torch.no_grad():
            m.output_conv.weight.mul_(100.0)   # (the 0.001 init would leave y = x to three digits)
        mixers[arm] = m.cuda().eval()
    rows = []
    with torch.no_grad():
        for B in BATCHES:
            g = torch.Generator(device="cuda").manual_seed(1)
            film_t = 1.0 + 0.3 * (2 * torch.rand(B, nb, 4, H, device="cuda", generator=g) - 1)
            film = [{k: film_t[:, i, q] for q, k in enumerate(("gamma1", "beta1", "gamma2", "beta2"))} for i in range(nb)]
            xl = 0.5 * (2 * torch.rand(B, 8, OFFLINE_T, device="cuda", generator=g) - 1)
            for N in BLOCKS:
                x = xl[:, :, :N].contiguous()
                arms = {"causal": mixers["causal"].stream(batch_size=B, max_block=N, film_params=film),
                        "lookahead": mixers["lookahead"].lookahead_stream(batch_size=B, max_block=N, film_params=film)}
                for s in arms.values():
                    s.push(x)                                   # warm-up
                arms["lookahead"]._pushed = arms["lookahead"].latency + N   # steady state: every row is inside the clip
                ms = {arm: [] for arm in arms}
                for _ in range(repeats):
                    for arm, s in arms.items():
                        ms[arm].append(timed(lambda s=s: s.push(x), window))
                for arm, s in arms.items():
                    st = stats(ms[arm])
                    rows.append(dict(kind="push", mixer=name, H=H, blocks=nb, K=K, B=B, arm=arm, block=N,
                                     block_ms_at_44k1=1e3 * N / SAMPLE_RATE, realtime_x=1e3 * N / SAMPLE_RATE / st["ms"],
                                     latency_samples=getattr(s, "latency", 0), state_mib=s.state_bytes / 2 ** 20, **st))
                rows.append(dict(kind="push_ratio", mixer=name, B=B, block=N,
                                 lookahead_over_causal=stats(ms["lookahead"])["ms"] / stats(ms["causal"])["ms"]))
                del arms
                print(f"{name} B={B} block={N} done", file=sys.stderr, flush=True)
        # the long-clip path: one 10 s clip in blocks against the offline forward of the same mixer
        m = mixers["lookahead"]
        film1 = [{k: v[:1] for k, v in p.items()} for p in film]
        x1 = xl[:1].contiguous()
        same = bool(torch.equal(m.forward_blockwise(x1, film_params=film1, block=BLOCKWISE_BLOCK), m(x1, film_params=film1)))
        fns = {"offline": lambda: m(x1, film_params=film1),
               "blockwise": lambda: m.forward_blockwise(x1, film_params=film1, block=BLOCKWISE_BLOCK)}
        ms = {arm: [] for arm in fns}
        for _ in range(repeats):
            for arm, fn in fns.items():
                ms[arm].append(timed(fn, window))
        for arm in fns:
            rows.append(dict(kind="blockwise", mixer=name, H=H, blocks=nb, K=K, B=1, arm=arm, T=OFFLINE_T,
                             block=BLOCKWISE_BLOCK if arm == "blockwise" else None, bit_equal_to_offline=same, **stats(ms[arm])))
        rows.append(dict(kind="blockwise_ratio", mixer=name, T=OFFLINE_T,
                         blockwise_over_offline=stats(ms["blockwise"])["ms"] / stats(ms["offline"])["ms"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcn_lookahead_probe.json"))
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
               what="ms per push (HIP events, median of repeats, arms alternating) of TCNLookaheadStream next to TCNStream per "
                    "mixer, B and block; blockwise = TCNMixer.forward_blockwise of a 10 s clip against TCNMixer.forward", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
