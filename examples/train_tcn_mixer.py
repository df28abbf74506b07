"""Minimal training loop of the style-transfer stage on the MI355X path: the TCN mixer trains on the HIP kernels
(`tcn.backend = "hip-train"`: train-mode forward and full backward in libmst.so), the FiLM generator on PyTorch
(`gen.backend = "torch"`: three small GEMMs, its gradient arrives through the FiLM tensors), the loss is the HIP
MultiResolutionSTFTLoss.

    python examples/train_tcn_mixer.py --steps 100 --seconds 10 --batch-size 8

What a step does (the reference's src/train_style_transfer.py:255-317 with its cycle term :228-242): synthetic stem pairs
(input stems, and the same stems under another fixed "mix": per-stem gains and a short smoothing filter), fixed random
embeddings for the two styles,

    out   = tcn(input, film(input_emb, target_emb))
    cycle = tcn(out, film(target_emb, input_emb))
    loss  = MRSTFT(out, target) + lambda_cycle * MRSTFT(cycle, input)

AdamW, and the reference's two clip_grad_norm_ calls.  The reference's style term -- the cosine distance between the
frozen encoder's embedding of `out` and the target embedding -- is NOT part of this loop: the gradient of the encoder with
respect to its input waveform does not exist on the HIP path yet, so the supervised MRSTFT term stands in for it.
The same seed prints the same losses: every kernel of the step has a fixed summation order."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mst_amd.loss import MultiResolutionSTFTLoss  # noqa: E402
from mst_amd.synth import synth_batch  # noqa: E402
from mst_amd.tcn_mixer import TCNFiLMGenerator, TCNMixer  # noqa: E402


def other_mix(x):
    """The target of a pair: the input stems under another mix -- per-channel gains, drums smoothed by a 3-tap filter."""
    gains = torch.tensor([1.4, 1.4, 0.6, 0.6, 1.2, 1.2, 0.8, 0.8], device=x.device).view(1, 8, 1)
    y = x * gains
    d = y[:, 4:6]
    y[:, 4:6] = 0.5 * d + 0.25 * (torch.roll(d, 1, -1) + torch.roll(d, -1, -1))
    return y


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=14)
    ap.add_argument("--kernel-size", type=int, default=15)
    ap.add_argument("--embed-dim", type=int, default=512)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--lambda-cycle", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_tcn_mixer.py needs a GPU (backend='hip-train' has no CPU fallback)")
    torch.manual_seed(a.seed)
    dev = torch.device("cuda", 0)
    tcn = TCNMixer(hidden_channels=a.hidden, num_blocks=a.blocks, kernel_size=a.kernel_size, use_film=True).to(dev).train()
    gen = TCNFiLMGenerator(embed_dim=2 * a.embed_dim, num_blocks=a.blocks, hidden_channels=a.hidden).to(dev).train()
    tcn.backend, gen.backend = "hip-train", "torch"
    mrstft = MultiResolutionSTFTLoss()
    opt = torch.optim.AdamW(list(tcn.parameters()) + list(gen.parameters()), lr=a.lr)

    x = synth_batch(a.batch_size, int(a.seconds * 44100)).to(dev)
    target = other_mix(x)
    g = torch.Generator().manual_seed(a.seed + 1)
    emb_in = torch.nn.functional.normalize(torch.randn(a.batch_size, a.embed_dim, generator=g), dim=1).to(dev)
    emb_tg = torch.nn.functional.normalize(torch.randn(a.batch_size, a.embed_dim, generator=g), dim=1).to(dev)

    for step in range(1, a.steps + 1):
        opt.zero_grad()
        out = tcn(x, film_params=gen(torch.cat([emb_in, emb_tg], dim=1)))
        fit = mrstft(out, target)
        cycle = mrstft(tcn(out, film_params=gen(torch.cat([emb_tg, emb_in], dim=1))), x)
        loss = fit + a.lambda_cycle * cycle
        loss.backward()
        torch.nn.utils.clip_grad_norm_(tcn.parameters(), max_norm=1.0)
        torch.nn.utils.clip_grad_norm_(gen.parameters(), max_norm=1.0)
        opt.step()
        print(f"step {step} loss {loss.item():.6f} (target {fit.item():.6f}, cycle {cycle.item():.6f})", flush=True)


if __name__ == "__main__":
    main()
