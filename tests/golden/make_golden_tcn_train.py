"""Writes tests/golden/tcn_train_<case>.npz from the UNMODIFIED reference (its `src/tcn_mixer.py`) in train() mode.

    python tests/golden/make_golden_tcn_train.py [REFERENCE_SRC] [--cases NAME ...]
                                                  # REFERENCE_SRC default: the directory make_golden.py reads
                                                  # --cases: write these fixtures only (default: all of them)

Runs only where the reference checkout exists; the tests read the fixtures, never the reference.  Per case
(tests/cases_tcn_train.CASES) one forward + backward of loss = sum(y * dy) in fp32 and in float64.  The fp32 run notes the
mask `argument > 0` of every F.leaky_relu call (the `F` name the reference's module sees is replaced at run time by
cases_tcn_train.Recorder); the float64 run has those masks imposed (cases_tcn_train.Pinned), because a LeakyReLU argument
within rounding of zero otherwise takes another branch in the other precision.  Arrays and name lists only:
  masks                    np.packbits of the (2 nb, B, H, T) masks
  ye / ym {32,64}          y at cases_tcn.y_samples' positions
  dx {32,64}               dx at cases_tcn_train.dx_samples' positions
  param_names, g{32,64}_<name>   every parameter gradient at cases_tcn_train.sample's positions (whole when small)
  dfilm{32,64}             (B, nb, 4, H)
  bmean / bvar {32,64}     batch mean and biased variance at every BatchNorm input, (2 nb, H)
  rmean / rvar {32,64}, nbt     running statistics and num_batches_tracked after the step
  db32_max                 max |gradient| of the block conv biases in fp32 (mathematically zero: rounding noise)
Prints the reference's fp32-against-float64 error per quantity group (the e_ref of the parity rule)."""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def arguments():
    """([REFERENCE_SRC], [case names after --cases])."""
    args = sys.argv[1:]
    at = args.index("--cases") if "--cases" in args else len(args)
    return args[:at], args[at + 1:]


def reference_src():
    if arguments()[0]:
        return arguments()[0][0]
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "make_golden.py")).read()
    return re.search(r'sys\.path\.insert\(0, "([^"]*/src)"\)', text).group(1)


sys.path.insert(0, reference_src())

import cases_tcn as ct  # noqa: E402
import cases_tcn_train as ctt  # noqa: E402
with contextlib.redirect_stdout(io.StringIO()):
    import tcn_mixer as ref  # noqa: E402  (reference)


def run(c, dtype, namespace):
    def make():
        with contextlib.redirect_stdout(io.StringIO()):
            return ref.TCNMixer(**ct.mixer_kwargs(c))
    real = ref.F
    ref.F = namespace
    try:
        return ctt.run_tree(make, c, dtype)
    finally:
        ref.F = real


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    names = arguments()[1] or list(ctt.CASES)
    unknown = [n for n in names if n not in ctt.CASES]
    if unknown:
        sys.exit(f"no such case: {unknown}; cases: {list(ctt.CASES)}")
    for name in names:
        c = ctt.CASES[name]
        t0 = time.time()
        rec = ctt.Recorder()
        r32 = run(c, torch.float32, rec)
        masks = rec.stacked()
        r64 = run(c, torch.float64, ctt.Pinned(masks))
        free = ctt.Recorder()
        run(c, torch.float64, free)
        flips = int((free.stacked() != masks).sum())
        out = {"masks": np.packbits(masks.numpy()), "param_names": np.array(list(r32.grads.keys())), "nbt": np.array(r32.nbt)}
        for bits, r in ((32, r32), (64, r64)):
            (out[f"ye{bits}"], out[f"ym{bits}"]) = [t.numpy() for t in ct.y_samples(r.y)]
            out[f"dx{bits}"] = ctt.dx_samples(r.dx).astype(np.float32 if bits == 32 else np.float64)
            for k, v in r.grads.items():
                out[f"g{bits}_{k}"] = ctt.sample(k, v).astype(np.float32 if bits == 32 else np.float64)
            if c["film"]:
                out[f"dfilm{bits}"] = r.dfilm.numpy()
            for k in ("bmean", "bvar", "rmean", "rvar"):
                out[f"{k}{bits}"] = getattr(r, k).numpy()
        out["db32_max"] = np.array(ctt.groups_of_run(r32)[1])
        np.savez_compressed(ctt.fixture_path(name), **out)
        g = np.load(ctt.fixture_path(name))
        e = ctt.e_ref(g)
        print(f"{name}: {time.time() - t0:.1f} s, {os.path.getsize(ctt.fixture_path(name)) / 1024:.0f} KiB, masks differing from the "
              f"free float64 run {flips}, max|db| fp32 {float(out['db32_max']):.2e} (float64 {ctt.groups_of_run(r64)[1]:.1e}), "
              f"e_ref: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()), flush=True)


if __name__ == "__main__":
    main()
