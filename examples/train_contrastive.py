"""Minimal contrastive training loop on the MI355X path -- what the reference's src/train.py:223-332 does per step,
with this package's drop-ins:

    PCM shards -> PcmShardDataset / pcm_collate_fn (fork'd DataLoader workers, int16, pinned)
               -> DeviceStager (async H2D, overlapped)
               -> stage A in HIP: 64-d mixing features + log-mel straight from the int16 batch
               -> MixingStyleEncoder (train mode: PyTorch-ROCm autograd for the encoder; eval mode: all HIP)
               -> InfoNCELoss (forward and backward in HIP)
               -> AdamW

    python examples/train_contrastive.py --shards /data/shards --steps 100 --batch-size 24

With --synthetic N the script first writes N synthetic tracks as shards into --shards (no dataset needed).

--use_adversarial adds the reference's adversarial branch (src/train.py:130-204, :258-275): the embeddings of the clips whose
shard path appears in --song_id_cache_path (a .pt with `embeddings` (M, D) and `track_paths`, src/train.py:534-536) go through
GradientReversalLayer -> SongIdentityDiscriminator -> cosine-distance loss against the cached song-identity embedding, and
`adv_lambda * loss_adversarial` is added to the contrastive loss.  Discriminator and loss run in libmst.so (csrc/head.hip).
--checkpoint PATH writes the reference's checkpoint dictionary (src/train.py:34-52) after the last step.
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mst_amd import ingest  # noqa: E402
from mst_amd.grl import GradientReversalLayer, compute_adversarial_lambda, compute_grl_lambda  # noqa: E402
from mst_amd.loss import InfoNCELoss, cosine_distance_loss  # noqa: E402
from mst_amd.mixing_utils import deferred_features  # noqa: E402
from mst_amd.model import MixingStyleEncoder, SongIdentityDiscriminator  # noqa: E402
from mst_amd.synth import synth_clip  # noqa: E402


def write_synthetic_shards(path, n_tracks, seconds, sr):
    os.makedirs(path, exist_ok=True)
    for i in range(n_tracks):
        ingest.write_pcm_shard(os.path.join(path, f"track{i:04d}.pcm16"), synth_clip(1000 + i, int(seconds * sr), sr), sr)


def adversarial_loss(emb, paths, discriminator, grl_layer, song_id_embeddings, song_id_lookup, noise):
    """src/train.py:166-202 on one batch: rows whose track has a cached song-identity embedding -> (optional noise) -> GRL ->
    discriminator -> mean cosine distance to that embedding.  None when no row of the batch is in the cache."""
    rows = [(i, song_id_lookup[p]) for i, p in enumerate(paths) if p in song_id_lookup]
    if not rows:
        return None
    valid = torch.tensor([r[0] for r in rows], dtype=torch.long, device=emb.device)
    target = song_id_embeddings[torch.tensor([r[1] for r in rows], dtype=torch.long, device=emb.device)]
    x = emb[valid]
    if noise > 0.0:
        x = x + torch.randn_like(x) * noise
    return cosine_distance_loss(discriminator(grl_layer(x)), target)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", required=True)
    ap.add_argument("--synthetic", type=int, default=0, help="write this many synthetic tracks into --shards first")
    ap.add_argument("--track-seconds", type=float, default=25.0)
    ap.add_argument("--clip-seconds", type=float, default=10.0)
    ap.add_argument("--batch-size", type=int, default=24, help="songs per batch (2 segments each)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--workers", type=int, default=0)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--train-backend", choices=["hip", "torch"], default="hip",
                    help="hip: conv trunk forward + backward in libmst.so (default); torch: PyTorch-ROCm autograd")
    ap.add_argument("--train-precision", choices=["fp32", "f16x3", "f16"], default="fp32",
                    help="precision of the hand-written conv trunk: fp32 = exact fp32 MFMA; f16x3 = 3-term split-precision f16, "
                         "fp32-equivalent gradients at about twice the speed; f16 = float16 operands with fp32 accumulation (the "
                         "arithmetic of the reference's --use_amp step)")
    ap.add_argument("--small-nets", choices=["hip", "torch"], default="hip",
                    help="pooling head and FiLM MLP of the training step: hand-written forward / backward (csrc/head.hip) or the nn.Modules")
    # the adversarial branch: names and defaults of the reference's src/params.py:77-97 (the cache path has no default here)
    ap.add_argument("--use_adversarial", action="store_true", default=False,
                    help="adversarial training that removes song identity from the embedding")
    ap.add_argument("--adversarial_lambda", type=float, default=1.0, help="final weight of the adversarial loss")
    ap.add_argument("--initial_adversarial_lambda", type=float, default=0.0,
                    help="initial weight of the adversarial loss, ramps linearly up to --adversarial_lambda")
    ap.add_argument("--adversarial_warmup_steps", type=int, default=2000, help="steps before the adversarial schedules start")
    ap.add_argument("--fixed_grl_lambda", type=float, default=None,
                    help="constant gradient-reversal strength instead of the DANN schedule")
    ap.add_argument("--song_id_cache_path", type=str, default=None,
                    help=".pt file with `embeddings` (M, D) and `track_paths` (the shard paths), required by --use_adversarial")
    ap.add_argument("--discriminator_hidden_dim", type=int, default=512)
    ap.add_argument("--discriminator_dropout", type=float, default=0.3)
    ap.add_argument("--discriminator_lr", type=float, default=None,
                    help="learning rate of a separate discriminator optimizer; default: one optimizer, the encoder's rate")
    ap.add_argument("--discriminator_noise", type=float, default=0.0,
                    help="standard deviation of Gaussian noise added to the embeddings in front of the discriminator")
    ap.add_argument("--discriminator-backend", choices=["hip", "torch"], default="hip",
                    help="discriminator and cosine loss: hand-written forward / backward (csrc/head.hip) or PyTorch ops")
    ap.add_argument("--checkpoint", type=str, default=None, help="write a checkpoint here after the last step")
    ap.add_argument("--optimizer", choices=["torch", "hip"], default="torch",
                    help="AdamW of torch.optim, or of mst_amd.optim (csrc/optim.hip: two launches per step, same state_dict keys)")
    a = ap.parse_args(argv)
    if a.use_adversarial and not a.song_id_cache_path:
        ap.error("--use_adversarial needs --song_id_cache_path")
    sr = 44100
    if a.synthetic:
        write_synthetic_shards(a.shards, a.synthetic, a.track_seconds, sr)
    torch.manual_seed(a.seed)
    np.random.seed(a.seed)
    dev = torch.device("cuda")
    ds = ingest.PcmShardDataset(a.shards, clip_duration=a.clip_seconds, sample_rate=sr, num_segments=2)
    dl = DataLoader(ds, batch_size=a.batch_size, shuffle=True, drop_last=True, num_workers=a.workers,
                    collate_fn=ingest.pcm_collate_fn, pin_memory=True)
    model = MixingStyleEncoder(sr, 1024, 256, 128, 20, 10, 8, 768, feature_dim=64).to(dev).train()
    model.train_backend = a.train_backend
    model.train_precision = a.train_precision
    model.small_nets_backend = a.small_nets
    deferred = torch.stack([deferred_features(64)] * (2 * a.batch_size)).to(dev)   # what the Dataset's feature slot carries
    crit = InfoNCELoss(0.1)   # (check="deferred" would drop the per-step read-back of the guard; this loop reads loss.item() anyway)
    discriminator = grl_layer = song_id_embeddings = song_id_lookup = disc_opt = None
    if a.use_adversarial:   # src/train.py:526-541, :563-609
        cache = torch.load(a.song_id_cache_path, map_location="cpu")
        song_id_embeddings = cache["embeddings"].to(dev).float()
        song_id_lookup = {path: idx for idx, path in enumerate(cache["track_paths"])}
        discriminator = SongIdentityDiscriminator(input_dim=768, hidden_dim=a.discriminator_hidden_dim,
                                                  output_dim=song_id_embeddings.shape[1], dropout=a.discriminator_dropout).to(dev).train()
        discriminator.backend = a.discriminator_backend
        grl_layer = GradientReversalLayer(init_lambda=0.0).to(dev)
        print(f"adversarial: {song_id_embeddings.shape[0]} song-identity embeddings of dimension {song_id_embeddings.shape[1]}, "
              f"{sum(q.numel() for q in discriminator.parameters()):,} discriminator parameters", flush=True)
    AdamW = torch.optim.AdamW
    if a.optimizer == "hip":
        from mst_amd.optim import AdamW
    if a.use_adversarial and a.discriminator_lr is not None:
        opt = AdamW(model.parameters(), lr=a.lr)
        disc_opt = AdamW(discriminator.parameters(), lr=a.discriminator_lr)
    elif a.use_adversarial:
        opt = AdamW(list(model.parameters()) + list(discriminator.parameters()), lr=a.lr)
    else:
        opt = AdamW(model.parameters(), lr=a.lr)
    stager = ingest.DeviceStager((2 * a.batch_size, 8, ds.clip_samples), torch.int16, dev)
    losses, step = [], 0
    it = iter(dl)
    stems, labels, paths = next(it)
    fut, lab = stager.submit(stems), labels
    adv_losses = []
    while step < a.steps:
        x = fut.get()
        cur_lab, cur_paths = lab.to(dev, non_blocking=True), paths
        try:                                   # stage the next batch while this one is on the GPU
            stems, labels, paths = next(it)
        except StopIteration:
            it = iter(dl)
            stems, labels, paths = next(it)
        nxt, lab = stager.submit(stems), labels
        # the reference trainer's call (src/train.py:253) with the Dataset's deferred feature rows: ONE stage-A launch inside
        # yields the features and the log-mel, in the layout the training trunk reads
        emb = model(ingest.stems_views(x), deferred[:x.shape[0]])
        stager.release(fut)
        loss = crit(emb, cur_lab)
        if a.use_adversarial:   # src/train.py:153-164, :258-275 (the step counter is this loop's)
            grl_lambda = a.fixed_grl_lambda if a.fixed_grl_lambda is not None else \
                compute_grl_lambda(step, a.steps, a.adversarial_warmup_steps)
            grl_layer.set_lambda(grl_lambda)
            loss_adv = adversarial_loss(emb, cur_paths, discriminator, grl_layer, song_id_embeddings, song_id_lookup,
                                        a.discriminator_noise)
            adv_lambda = compute_adversarial_lambda(step, a.steps, a.adversarial_warmup_steps, a.initial_adversarial_lambda,
                                                    a.adversarial_lambda)
            if loss_adv is None:
                print("WARNING: no clip of this batch has a song-identity embedding", flush=True)
                loss_adv = torch.zeros((), device=dev)
            else:
                loss = loss + adv_lambda * loss_adv
        opt.zero_grad(set_to_none=True)
        if disc_opt is not None:
            disc_opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if disc_opt is not None:
            disc_opt.step()
        losses.append(loss.item())
        step += 1
        fut = nxt
        if a.use_adversarial:
            adv_losses.append(loss_adv.item())
            if step % 10 == 0 or step == a.steps:
                print(f"step {step}: loss {losses[-1]:.4f} adversarial {adv_losses[-1]:.4f} grl_lambda {grl_lambda:.4f} "
                      f"adv_lambda {adv_lambda:.4f}", flush=True)
        elif step % 10 == 0 or step == a.steps:
            print(f"step {step}: loss {losses[-1]:.4f}", flush=True)
    if a.checkpoint:   # the reference's checkpoint dictionary (src/train.py:34-52)
        ckpt = {"epoch": 0, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict(), "loss": losses[-1]}
        if discriminator is not None:
            ckpt["discriminator_state_dict"] = discriminator.state_dict()
        if disc_opt is not None:
            ckpt["disc_optimizer_state_dict"] = disc_opt.state_dict()
        os.makedirs(os.path.dirname(os.path.abspath(a.checkpoint)), exist_ok=True)
        torch.save(ckpt, a.checkpoint)
        print(f"checkpoint saved to {a.checkpoint}", flush=True)
    return losses


if __name__ == "__main__":
    main()
