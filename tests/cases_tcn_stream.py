"""Schedules and builders of the TCN streaming tests (test_tcn_stream_cpu.py, test_tcn_stream_gpu.py): data only."""
import torch

import cases_tcn as ct
import cases_tcn_train as ctt
from mst_amd import tcn_mixer as tm

# a block edge one sample either side of the 64- and 128-sample wave tiles, blocks shorter and longer than the history
EDGES = (1, 63, 64, 65, 127, 128, 129, 257)
WRAP_CYCLE = EDGES + (512, 4096, 16384, 10007)


def case(H, nb, K, film, B=2, T=1100, causal=True):
    return dict(H=H, nb=nb, K=K, causal=causal, film=film, B=B, T=T)


def walk(T, sizes, then=None):
    """Block sizes that sum to T: `sizes` once, then `then` repeated (default: one block with the rest); or, with
    then="cycle", `sizes` over and over.  The last block is cut to what is left."""
    out, left = [], T
    seq = list(sizes)
    while left > 0:
        if not seq:
            seq = list(sizes) if then == "cycle" else [then or left]
        n = min(seq.pop(0), left)
        out.append(n)
        left -= n
    return out


def schedule(name, T):
    return {"a": [T], "b": walk(T, EDGES), "c": walk(T, (1,) * 70, then=103)}[name]


def mixer(c, device, dtype=torch.float32, backend="hip", seed=4200):
    m = tm.TCNMixer(**ct.mixer_kwargs(c))
    m.load_state_dict(ct.make_tcn_state_dict(c, seed=seed), strict=True)
    m = m.to(device=device, dtype=dtype).eval()
    m.backend = backend
    return m


def film(c, device, dtype=torch.float32, seed=5100):
    """The FiLM dicts of a seeded (B, nb, 4, H) tensor, or None for a plain mixer."""
    return ctt.film_dicts(ctt.film_tensor(c, seed=seed).to(device=device, dtype=dtype)) if c["film"] else None


def run(stream, x, sizes):
    """The pushes of x cut into `sizes`, concatenated."""
    out, t = [], 0
    for n in sizes:
        out.append(stream.push(x[:, :, t:t + n]))
        t += n
    assert t == x.shape[2]
    return torch.cat(out, 2)
