"""Writes tests/golden/tcn_film_train.npz from the UNMODIFIED reference TCNFiLMGenerator (its `src/tcn_mixer.py:148-216`).

    python tests/golden/make_golden_tcn_film_train.py [REFERENCE_SRC]      # default: the directory make_golden.py reads

Runs only where the reference checkout exists; the tests read the fixture, never the reference.  The generator in eval() mode
with gradients (Dropout off: masks are not reproducible across implementations), once in fp32 and once in float64, at
cases_tcn_film_train.FIXTURE (embed_dim 40, 3 blocks, H = 8, B = 5): forward() -> the list of dicts, stacked back into film
(B, nb, 4, H), loss = sum(film * R), backward.  Weights (std 0.05, non-zero biases), embedding and R come from
cases_tcn_film_train.make_inputs and are regenerated from the seed by the test, not stored.  Arrays only:
  f32.<group> / f64.<group>   film, demb and the six parameter gradients; mlp.3.weight at cases_tcn_film_train.w3_positions()"""
import contextlib
import io
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_src():
    if sys.argv[1:]:
        return sys.argv[1]
    text = open(os.path.join(HERE, "make_golden.py")).read()
    return re.search(r'sys\.path\.insert\(0, "([^"]*/src)"\)', text).group(1)


sys.path.insert(0, reference_src())

import cases_tcn_film_train as cf  # noqa: E402
with contextlib.redirect_stdout(io.StringIO()):
    import tcn_mixer as ref  # noqa: E402  (reference)


def main():
    c = cf.FIXTURE
    sd, emb, R = cf.make_inputs(c["B"], c["embed_dim"], c["nb"], c["H"], c["seed"])
    pos = cf.w3_positions()
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        gen = ref.TCNFiLMGenerator(embed_dim=c["embed_dim"], num_blocks=c["nb"], hidden_channels=c["H"])
        gen.load_state_dict(sd, strict=True)
        gen = gen.to(dt).eval()
        x = emb.to(dt).clone().requires_grad_(True)
        dicts = gen(x)
        film = torch.stack([torch.stack([d[k] for k in ("gamma1", "beta1", "gamma2", "beta2")], 1) for d in dicts], 1)
        (film * R.to(dt)).sum().backward()
        out[f"{tag}.film"], out[f"{tag}.demb"] = film.detach().numpy(), x.grad.numpy()
        for k, q in gen.named_parameters():
            out[f"{tag}.{k}"] = q.grad.numpy().ravel()[pos] if k == "mlp.3.weight" else q.grad.numpy()
    path = os.path.join(HERE, "tcn_film_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k in cf.GROUPS:
        print(f"e_ref {k}: {cf.rel_err(out[f'f32.{k}'], out[f'f64.{k}'].astype(np.float64)):.3e}")


if __name__ == "__main__":
    main()
