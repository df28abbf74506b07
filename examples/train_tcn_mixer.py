"""Minimal training loop of the style-transfer stage on the MI355X path: the TCN mixer trains on the HIP kernels
(`tcn.backend = "hip-train"`: train-mode forward and full backward in libmst.so), the loss is the HIP
MultiResolutionSTFTLoss, and the FiLM generator, whose gradient arrives through the FiLM tensors, runs on PyTorch
(`--film-generator torch`, the default: `gen.backend = "torch"`, three small library GEMMs) or on the HIP kernels as well
(`--film-generator hip`: `gen.backend = "hip"` with `gen.train_backend = "hip"`, train-mode forward and full backward in
libmst.so; the step then has no PyTorch module and no library GEMM in it).

    python examples/train_tcn_mixer.py --steps 100 --seconds 10 --batch-size 8

What a step does (the reference's src/train_style_transfer.py:255-317 with its cycle term :228-242): synthetic stem pairs
(input stems, and the same stems under another fixed "mix": per-stem gains and a short smoothing filter), fixed random
embeddings for the two styles,

    out   = tcn(input, film(input_emb, target_emb))
    cycle = tcn(out, film(target_emb, input_emb))
    loss  = MRSTFT(out, target) + lambda_cycle * MRSTFT(cycle, input)

AdamW, and the reference's two clip_grad_norm_ calls: torch.optim / torch.nn.utils by default (`--optimizer torch`), or the
kernels of csrc/optim.hip (`--optimizer hip`: `mst_amd.optim.AdamW` and `mst_amd.optim.clip_grad_norm_`, three launches per
clip and two per step whatever the number of tensors, the clip's norm summed in double in a fixed order).

`--style-weight W` (default 0: the loop above, unchanged) adds the reference's style term (:192-224),

    loss += W * cosine_distance_loss(encoder(out_stems, deferred_features), encoder(target_stems, deferred_features))

through a FROZEN MixingStyleEncoder in eval mode (`--encoder-checkpoint`, else randomly initialised).  The gradient reaches
the TCN through the encoder's input waveform: stage A (STFT -> mel -> log) forward and backward in HIP, the conv trunk on
PyTorch-ROCm autograd (`--style-encoder torch`, the default: `encoder_backend="torch"`) or in HIP as well
(`--style-encoder hip`: `encoder_backend="hip"` with `input_grad_backend="hip"`, the frozen encoder's input gradient on
hand-written kernels).  The mixing features of `out` condition the encoder as constants by default (`--style-features
const`); `--style-features grad` differentiates them too, as the reference does (it extracts the output's features with
gradients): `feature_grad_backend="hip"`, stage A's feature gradient fused with the log-mel's.
With W = 0 the same seed prints the same losses: every kernel of the step has a fixed summation order (with
`--film-generator torch` that leans on the GEMM library repeating itself; with `hip` the order is the project's own)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mst_amd.loss import MultiResolutionSTFTLoss, cosine_distance_loss  # noqa: E402
from mst_amd.mixing_utils import STEMS, deferred_features  # noqa: E402
from mst_amd.model import MixingStyleEncoder  # noqa: E402
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
    ap.add_argument("--style-weight", type=float, default=0.0,
                    help="weight of the style term 1 - cos(encoder(out), encoder(target)) through the frozen encoder (0 = off)")
    ap.add_argument("--encoder-checkpoint", default=None,
                    help="MixingStyleEncoder checkpoint (a state_dict, or a dict holding 'model_state_dict'); default: random weights")
    ap.add_argument("--style-encoder", choices=("torch", "hip"), default="torch",
                    help="conv trunk of the style term's encoder: PyTorch-ROCm autograd, or the hand-written HIP input gradient")
    ap.add_argument("--style-features", choices=("const", "grad"), default="const",
                    help="mixing features of the style term: constants (default), or differentiated as the reference does "
                         "(feature_grad_backend='hip': the second path from the waveform to the embedding)")
    ap.add_argument("--film-generator", choices=("torch", "hip"), default="torch",
                    help="the FiLM generator's training step: PyTorch-ROCm modules, or the hand-written HIP forward and backward")
    ap.add_argument("--optimizer", choices=("torch", "hip"), default="torch",
                    help="AdamW and the two clip_grad_norm_ calls: torch.optim / torch.nn.utils, or the hand-written HIP kernels")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_tcn_mixer.py needs a GPU (backend='hip-train' has no CPU fallback)")
    torch.manual_seed(a.seed)
    dev = torch.device("cuda", 0)
    tcn = TCNMixer(hidden_channels=a.hidden, num_blocks=a.blocks, kernel_size=a.kernel_size, use_film=True).to(dev).train()
    gen = TCNFiLMGenerator(embed_dim=2 * a.embed_dim, num_blocks=a.blocks, hidden_channels=a.hidden).to(dev).train()
    tcn.backend, gen.backend = "hip-train", "torch"
    if a.film_generator == "hip":
        gen.backend, gen.train_backend = "hip", "hip"
    mrstft = MultiResolutionSTFTLoss()
    AdamW, clip_grad_norm_ = torch.optim.AdamW, torch.nn.utils.clip_grad_norm_
    if a.optimizer == "hip":
        from mst_amd.optim import AdamW, clip_grad_norm_
    opt = AdamW(list(tcn.parameters()) + list(gen.parameters()), lr=a.lr)

    x = synth_batch(a.batch_size, int(a.seconds * 44100)).to(dev)
    target = other_mix(x)
    g = torch.Generator().manual_seed(a.seed + 1)
    emb_in = torch.nn.functional.normalize(torch.randn(a.batch_size, a.embed_dim, generator=g), dim=1).to(dev)
    emb_tg = torch.nn.functional.normalize(torch.randn(a.batch_size, a.embed_dim, generator=g), dim=1).to(dev)

    encoder = style_target = None
    if a.style_weight > 0:   # (after everything above: the W = 0 loop draws the same random numbers as before)
        as_stems = lambda t: {s: t[:, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}
        feats = deferred_features(64).expand(a.batch_size, 64).to(dev)   # filled on the device from the encoder's own stage-A launch
        encoder = MixingStyleEncoder(embed_dim=a.embed_dim, feature_dim=64, encoder_backend=a.style_encoder)
        if a.style_encoder == "hip":
            encoder.input_grad_backend = "hip"
        if a.style_features == "grad":
            encoder.feature_grad_backend = "hip"
        if a.encoder_checkpoint:
            sd = torch.load(a.encoder_checkpoint, map_location="cpu")
            encoder.load_state_dict(sd.get("model_state_dict", sd))
        encoder = encoder.to(dev).eval()
        for q in encoder.parameters():
            q.requires_grad_(False)
        with torch.no_grad():
            style_target = encoder(as_stems(target), feats)

    for step in range(1, a.steps + 1):
        opt.zero_grad()
        out = tcn(x, film_params=gen(torch.cat([emb_in, emb_tg], dim=1)))
        fit = mrstft(out, target)
        cycle = mrstft(tcn(out, film_params=gen(torch.cat([emb_tg, emb_in], dim=1))), x)
        loss = fit + a.lambda_cycle * cycle
        if encoder is not None:
            style = cosine_distance_loss(encoder(as_stems(out), feats), style_target)
            loss = loss + a.style_weight * style
        loss.backward()
        clip_grad_norm_(tcn.parameters(), max_norm=1.0)
        clip_grad_norm_(gen.parameters(), max_norm=1.0)
        opt.step()
        extra = f", style {style.item():.6f}" if encoder is not None else ""
        print(f"step {step} loss {loss.item():.6f} (target {fit.item():.6f}, cycle {cycle.item():.6f}{extra})", flush=True)


if __name__ == "__main__":
    main()
