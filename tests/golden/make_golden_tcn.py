"""Writes tests/golden/tcn_<case>.npz from the UNMODIFIED reference (its `src/tcn_mixer.py`), fp32 and float64.

    python tests/golden/make_golden_tcn.py [REFERENCE_SRC]     # default: the directory make_golden.py reads

Runs only where the reference checkout exists (the build container); the tests read the fixtures, never the reference.
One file per case (tests/cases_tcn.CASES) so that each stays far below the size limit of a committed file.  Arrays and
name lists only:
  keys / shapes       state-dict key list and shapes of TCNMixer (tcn_*) and TCNFiLMGenerator (film_*)
  x_checksum          [sum, sum of squares] of the seeded input (cases.pcm_batch)
  film32 / film64     (B, nb, 4, H) FiLM parameters for E = 1024 (film cases; st_default also E = 1536 as film1536_*)
  ye32 / ye64         (B, 8, 1024): y at the first 512 and last 512 samples of every channel   } cases_tcn.y_samples
  ym32 / ym64         y at 4096 seeded positions of the interior                               }
  h{blk}_32 / _64     hidden state after blocks 0, nb//2, nb-1 at cases_tcn.hidden_idx (2048 flat positions of (B, H, T))
"""
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


def reference_src():
    """The reference's src/ directory: the argument, or the one tests/golden/make_golden.py names."""
    if len(sys.argv) > 1:
        return sys.argv[1]
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "make_golden.py")).read()
    return re.search(r'sys\.path\.insert\(0, "([^"]*/src)"\)', text).group(1)


sys.path.insert(0, reference_src())

import cases  # noqa: E402
import cases_tcn as ct  # noqa: E402
with contextlib.redirect_stdout(io.StringIO()):
    import tcn_mixer as ref  # noqa: E402  (reference)


def run(c, dtype, E):
    with contextlib.redirect_stdout(io.StringIO()):
        tcn = ref.TCNMixer(**ct.mixer_kwargs(c))
    tcn.load_state_dict(ct.make_tcn_state_dict(c), strict=True)
    tcn = tcn.to(dtype).eval()
    x = cases.pcm_batch(c["B"], c["T"]).to(dtype)
    film, params = None, None
    if c["film"]:
        gen = ref.TCNFiLMGenerator(embed_dim=E, num_blocks=c["nb"], hidden_channels=c["H"])
        gen.load_state_dict(ct.make_film_state_dict(E, c), strict=True)
        gen = gen.to(dtype).eval()
        with torch.no_grad():
            params = gen(ct.embeddings(c["B"], E).to(dtype))
        film = torch.stack([torch.stack([p[k] for k in ("gamma1", "beta1", "gamma2", "beta2")], 1) for p in params], 1)
    hidden = {}
    hooks = [tcn.blocks[k].register_forward_hook(lambda m, i, o, k=k: hidden.__setitem__(k, o)) for k in ct.tap_blocks(c)]
    with torch.no_grad():
        y = tcn(x, film_params=params)
    for h in hooks:
        h.remove()
    return tcn, x, film, y, hidden


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for name, c in ct.CASES.items():
        t0 = time.time()
        out = {}
        tcn, x, film32, y32, h32 = run(c, torch.float32, ct.EMBED)
        _, _, film64, y64, h64 = run(c, torch.float64, ct.EMBED)
        sd = tcn.state_dict()
        out["tcn_keys"] = np.array(list(sd.keys()))
        out["tcn_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        if c["film"]:
            fsd = ct.make_film_state_dict(ct.EMBED, c)
            out["film_keys"] = np.array(list(fsd.keys()))
            out["film_shapes"] = np.array([",".join(map(str, v.shape)) for v in fsd.values()])
            out["film32"], out["film64"] = film32.numpy(), film64.numpy()
            if name == "st_default":
                out["film1536_32"] = run(c, torch.float32, ct.EMBED_WIDE)[2].numpy()
                out["film1536_64"] = run(c, torch.float64, ct.EMBED_WIDE)[2].numpy()
        out["x_checksum"] = np.array(cases.checksum(x))
        out["receptive_field"] = np.array(tcn.receptive_field)
        (e32, m32), (e64, m64), (xe, xm) = ct.y_samples(y32), ct.y_samples(y64), ct.y_samples(x.double())
        out["ye32"], out["ym32"], out["ye64"], out["ym64"] = e32.numpy(), m32.numpy(), e64.numpy(), m64.numpy()
        cat = lambda a, b: np.concatenate([np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()])  # noqa: E731
        ya32, ya64, xa = cat(e32, m32), cat(e64, m64), cat(xe, xm)
        hi = ct.hidden_idx(c)
        for k in ct.tap_blocks(c):
            out[f"h{k}_32"], out[f"h{k}_64"] = h32[k].reshape(-1)[hi].numpy(), h64[k].reshape(-1)[hi].numpy()
        np.savez(ct.fixture_path(name), **out)
        dyx = (y64 - x.double()).abs().max().item()
        rows = [("y", ct.max_rel(ya32, ya64)[0]), ("y-x", ct.max_rel(ya32 - xa, ya64 - xa)[0])]
        rows += [(f"h{k}", ct.max_rel(out[f"h{k}_32"], out[f"h{k}_64"])[0]) for k in ct.tap_blocks(c)]
        if c["film"]:
            rows.append(("film", ct.max_rel(out["film32"], out["film64"])[0]))
        print(f"{name}: {time.time() - t0:.1f} s, {os.path.getsize(ct.fixture_path(name)) / 1024:.0f} KiB, max|x| {x.abs().max():.3f}, "
              f"max|y-x| {dyx:.3f}, reference fp32 vs f64: " + ", ".join(f"{n} {v:.2e}" for n, v in rows), flush=True)


if __name__ == "__main__":
    main()
