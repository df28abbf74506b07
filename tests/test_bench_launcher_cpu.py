"""CPU: `python bench.py --gpus N` starts its own N ranks (driver contract) -- rehearsed on gloo with MST_BENCH_DRYRUN=1
(no kernels, labelled as a dry run), plus the refusal paths: a world size that differs from --gpus never prints a line; and
the clip sample --dump-outputs writes when the outputs exceed its budget."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True, text=True,
                          timeout=300)


def test_gpus_n_spawns_n_ranks_and_prints_one_line():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"], MST_BENCH_DRYRUN="1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world"] == 2 and out["rccl_ranks_seen"] == 2 and out["dry_run"] is True
    assert out["steps"] == 3 and out["value"] == 0.0 and "DRY RUN" in out["metric"]


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "4", "--steps", "1"], MST_BENCH_DRYRUN="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 3 and "WORLD_SIZE=1" in r.stderr and not r.stdout.strip()


def test_too_few_gpus_is_refused_before_any_rank_starts():
    r = _run(["--gpus", "64", "--steps", "1"])          # no dry run: the device count is checked first
    assert r.returncode == 2 and "GPU(s) visible" in r.stderr and not r.stdout.strip()


def test_dump_outputs_keeps_the_same_seeded_clips_within_its_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch

    import bench
    emb, feats = torch.randn(50, 8), torch.randn(50, 2)
    monkeypatch.setattr(bench, "DUMP_BYTES", 20 * 40)   # room for 20 of the 50 clips (40 bytes per clip)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"embeddings": emb, "features": feats}, {"loss": torch.tensor(1.5)})
    e, f = np.load(tmp_path / "a" / "embeddings.npy"), np.load(tmp_path / "a" / "features.npy")
    assert e.shape == (20, 8) and f.shape == (20, 2) and e.dtype == f.dtype == np.float32
    rows = [int(np.flatnonzero((emb.numpy() == r).all(1))[0]) for r in e]
    assert rows == sorted(set(rows)) and np.array_equal(f, feats.numpy()[rows])     # the same clips in every array
    assert np.array_equal(e, np.load(tmp_path / "b" / "embeddings.npy")) and float(np.load(tmp_path / "a" / "loss.npy")) == 1.5
