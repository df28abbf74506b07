"""Mixing style transfer end to end on the MI355X path -- what the reference's
inference/inference_e2e_style_transfer.py does once the stems are separated:

    input stems, target stems -> MixingFeatureExtractor + MixingStyleEncoder (HIP)  -> two embeddings
                              -> TCNFiLMGenerator (HIP)  -> FiLM parameters of every block
                              -> TCNMixer (HIP)          -> processed stems, processed mixture
                              -> embedding of the result -> cosine distance to the target, before and after

    python examples/style_transfer.py                       # two seeded synthetic clips, seeded weights
    python examples/style_transfer.py --tcn_checkpoint ckpt.pt --encoder_checkpoint enc.pt --seconds 10
    python examples/style_transfer.py --tcn-precision f16x3 # the mixer's convolutions in split precision on the f16 MFMA
    python examples/style_transfer.py --cycle               # + the cycle-consistency distance of the trainer (no gradient step)

--tcn_checkpoint is the reference's format (train_style_transfer.py): a dict with `tcn_state_dict`,
`film_generator_state_dict` and optionally `hidden_channels`, `num_blocks`, `kernel_size`, `causal` (defaults 16, 8, 5,
False as in the reference's loader).  Without it the mixer has seeded weights: the numbers then only show the data path.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mst_amd.loss import MultiResolutionSTFTLoss  # noqa: E402
from mst_amd.mixing_utils import STEMS, deferred_features  # noqa: E402
from mst_amd.model import MixingStyleEncoder  # noqa: E402
from mst_amd.synth import synth_batch  # noqa: E402
from mst_amd.tcn_mixer import TCNFiLMGenerator, TCNMixer, apply_style_transfer  # noqa: E402


def embed(encoder, clip, device):
    """(8, T) stems -> embedding, through the reference's call contract (features filled by stage A)."""
    stems = {s: clip[None, 2 * i:2 * i + 2].to(device) for i, s in enumerate(STEMS)}
    with torch.no_grad():
        return encoder(stems, deferred_features(64)[None].to(device))[0]


def distance(a, b):
    return float(1.0 - F.cosine_similarity(a[None], b[None]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tcn_checkpoint", default=None)
    ap.add_argument("--encoder_checkpoint", default=None, help="state_dict of MixingStyleEncoder (reference format)")
    ap.add_argument("--backend", choices=["hip", "torch"], default="hip")
    ap.add_argument("--tcn-precision", choices=["fp32", "f16x3"], default="fp32",
                    help="TCNMixer.precision of the hip backend: f16x3 = split-precision inference on the f16 MFMA (pays on wide mixers)")
    ap.add_argument("--cycle", action="store_true",
                    help="also send the processed stems back (style of the input) and print the MR-STFT distance to the input stems")
    a = ap.parse_args(argv)
    device = torch.device("cuda")
    torch.manual_seed(a.seed)

    encoder = MixingStyleEncoder(feature_dim=64)
    if a.encoder_checkpoint:
        sd = torch.load(a.encoder_checkpoint, map_location="cpu")
        encoder.load_state_dict(sd.get("model_state_dict", sd))
    encoder = encoder.to(device).eval()

    x = synth_batch(2, int(a.seconds * 44100))            # clip 0: input, clip 1: target style
    e_in, e_tgt = embed(encoder, x[0], device), embed(encoder, x[1], device)

    ck = torch.load(a.tcn_checkpoint, map_location="cpu", weights_only=False) if a.tcn_checkpoint else {}
    H, nb = ck.get("hidden_channels", 16), ck.get("num_blocks", 8)
    tcn = TCNMixer(in_channels=8, hidden_channels=H, num_blocks=nb, kernel_size=ck.get("kernel_size", 5),
                   causal=ck.get("causal", False), use_film=True)
    gen = TCNFiLMGenerator(embed_dim=2 * e_in.shape[0], num_blocks=nb, hidden_channels=H)
    if ck:
        tcn.load_state_dict(ck["tcn_state_dict"])
        gen.load_state_dict(ck["film_generator_state_dict"])
    tcn, gen = tcn.to(device), gen.to(device)
    tcn.backend = gen.backend = a.backend
    tcn.precision = a.tcn_precision

    stems_in = {s: x[0, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}
    out = apply_style_transfer(tcn, gen, stems_in, e_tgt, e_in, device)
    y = torch.cat([out["processed_stems"][s] for s in STEMS], 0)
    e_out = embed(encoder, y, device)
    print(f"TCN: {nb} blocks, {H} channels, receptive field {tcn.receptive_field} samples, backend {a.backend}, precision {a.tcn_precision}")
    print(f"processed mixture {tuple(out['processed_mixture'].shape)}, max |y - x| = {float((y - x[0]).abs().max()):.4f}")
    print(f"cosine distance to the target: input {distance(e_in, e_tgt):.4f} -> processed {distance(e_out, e_tgt):.4f}")
    if a.cycle:   # train_style_transfer.py:228-239: output -> reconstructed input, MultiResolutionSTFTLoss(reconstructed, input)
        back = apply_style_transfer(tcn, gen, {s: y[2 * i:2 * i + 2] for i, s in enumerate(STEMS)}, e_in, e_out, device)
        rec = torch.cat([back["processed_stems"][s] for s in STEMS], 0).to(device)
        crit = MultiResolutionSTFTLoss(backend=a.backend)
        with torch.no_grad():
            cyc, comp = float(crit(rec, x[0].to(device))), crit.components(rec, x[0].to(device)).cpu()
        out["cycle_loss"] = cyc
        print(f"cycle MR-STFT distance input -> target style -> input style: {cyc:.4f}  (per resolution sc / log: "
              + ", ".join(f"{n}: {c[0]:.3f} / {c[1]:.3f}" for n, c in zip(crit.fft_sizes, comp.tolist())) + ")")
    return out


if __name__ == "__main__":
    main()
