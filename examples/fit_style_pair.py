"""The per-pair fit of the style-transfer stage on the MI355X path (the reference's own inference method,
inference/test_tcn_style_transfer.py): optimise a small TCN mixer on ONE clip so that the embedding of its processed stems
approaches the embedding of a target mix, every step on hand-written HIP kernels and, with `--sync deferred` (default), without a
host synchronisation inside the loop.

    python examples/fit_style_pair.py --steps 200 --seconds 2

A synthetic pair: input stems, and the same stems under another fixed mix (the target).  The frozen MixingStyleEncoder is
randomly initialised unless `--encoder-checkpoint` names a state_dict (or a dict holding 'model_state_dict').  Prints the
distance to the target's embedding before the fit, the best distance the fit reached, and the distance recomputed from the
returned stems."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mst_amd.loss import cosine_distance_loss  # noqa: E402
from mst_amd.mixing_utils import STEMS, deferred_features  # noqa: E402
from mst_amd.model import MixingStyleEncoder  # noqa: E402
from mst_amd.synth import synth_batch  # noqa: E402
from mst_amd.tcn_mixer import TCNMixer, optimize_tcn_style_transfer  # noqa: E402
from train_tcn_mixer import other_mix  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--hidden", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--kernel-size", type=int, default=15)
    ap.add_argument("--embed-dim", type=int, default=512)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--optimizer", choices=("adam", "adamw", "sgd"), default="adam")
    ap.add_argument("--sync", choices=("deferred", "step"), default="deferred",
                    help="deferred: history and best output stay on the device until the end; step: the reference's per-step read-back")
    ap.add_argument("--style-features", choices=("const", "grad"), default="const",
                    help="mixing features of the processed stems: constants, or differentiated as the reference does")
    ap.add_argument("--encoder-checkpoint", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fit_style_pair.py needs a GPU (the fit runs on HIP kernels; there is no CPU fallback)")
    torch.manual_seed(a.seed)
    dev = torch.device("cuda", 0)
    encoder = MixingStyleEncoder(embed_dim=a.embed_dim, feature_dim=64, encoder_backend="hip")
    if a.encoder_checkpoint:
        sd = torch.load(a.encoder_checkpoint, map_location="cpu")
        encoder.load_state_dict(sd.get("model_state_dict", sd))
    encoder = encoder.to(dev).eval()
    for q in encoder.parameters():
        q.requires_grad_(False)
    encoder.input_grad_backend = "hip"
    if a.style_features == "grad":
        encoder.feature_grad_backend = "hip"
    tcn = TCNMixer(hidden_channels=a.hidden, num_blocks=a.blocks, kernel_size=a.kernel_size, use_film=False)

    x = synth_batch(1, int(a.seconds * 44100)).to(dev)
    target = other_mix(x)
    as_stems = lambda t: {s: t[:, 2 * i:2 * i + 2] for i, s in enumerate(STEMS)}  # noqa: E731
    feats = deferred_features(64).unsqueeze(0).to(dev)
    with torch.no_grad():
        target_emb = encoder(as_stems(target), feats)
        before = float(cosine_distance_loss(encoder(as_stems(x), feats), target_emb))
    t0 = time.perf_counter()
    out = optimize_tcn_style_transfer(tcn, {s: v[0] for s, v in as_stems(x).items()}, target_emb[0], encoder, None, dev,
                                      num_steps=a.steps, lr=a.lr, verbose=not a.quiet, optimizer=a.optimizer, sync=a.sync)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    y = torch.cat([out["processed_stems"][s] for s in STEMS], dim=0).unsqueeze(0).to(dev)
    with torch.no_grad():
        after = float(cosine_distance_loss(encoder(as_stems(y), feats), target_emb))
    print(f"distance to the target: input {before:.6f}, best of {a.steps} steps {out['final_distance']:.6f} "
          f"(eval-mode re-embedding of the returned stems {after:.6f}), converged {out['converged']}, "
          f"{1e3 * wall / a.steps:.2f} ms per step ({a.sync})", flush=True)
    return out


if __name__ == "__main__":
    main()
