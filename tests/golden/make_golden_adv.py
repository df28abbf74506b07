"""Generate tests/golden/adversarial.npz by running the REFERENCE's own adversarial branch in the build container.

Usage (build container only; the reference tree does not exist on the GPU box):
    python tests/golden/make_golden_adv.py

Imports /root/reference/src/{grl,model}.py unmodified (with the stand-in `torchaudio` of oracle/torchaudio_standin on sys.path,
as make_golden.py does) and evaluates what src/train.py:182-202 computes -- index-select of the valid rows, GradientReversalLayer,
SongIdentityDiscriminator, cosine-distance loss -- and its backward pass, once in fp32 and once in float64, in eval mode
(Dropout off: masks are not reproducible across implementations).  Small on purpose: in / hidden / out = 96 / 80 / 48, K = 7
valid of N = 10 rows, GRL lambda 0.37.  Also the two schedules of src/grl.py at a handful of steps.  Arrays and name lists only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle", "torchaudio_standin"))
sys.path.insert(0, "/root/reference/src")

import grl as ref_grl  # noqa: E402      (reference)
import model as ref_model  # noqa: E402  (reference)

IN, HID, OUT, N, LAM = 96, 80, 48, 10, 0.37
VALID = [0, 2, 3, 5, 6, 8, 9]
STEPS = [0, 1999, 2000, 2001, 6000, 10000, 12000]
TOTAL, WARMUP = 10000, 2000


def main():
    out = {}
    rng = np.random.default_rng(20240607)
    disc = ref_model.SongIdentityDiscriminator(input_dim=IN, hidden_dim=HID, output_dim=OUT, dropout=0.3).eval()
    keys = list(disc.state_dict().keys())
    out["state_dict_keys"] = np.array(keys)
    out["state_dict_shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in disc.state_dict().values()], dtype=np.int64)
    sd = {}
    for k, v in disc.state_dict().items():   # fp32 values: the float64 run starts from exactly the same numbers
        fan_in = v.shape[1] if v.dim() == 2 else v.shape[0]
        sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * (1.5 / np.sqrt(fan_in))).astype(np.float32))
        out[f"weight.{k}"] = sd[k].numpy()
    emb = torch.from_numpy(rng.standard_normal((N, IN)).astype(np.float32))
    target = torch.from_numpy(rng.standard_normal((len(VALID), OUT)).astype(np.float32))
    out["embeddings"], out["targets"], out["valid_indices"], out["grl_lambda"] = emb.numpy(), target.numpy(), np.array(VALID), np.array(LAM)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        d = ref_model.SongIdentityDiscriminator(input_dim=IN, hidden_dim=HID, output_dim=OUT, dropout=0.3).to(dt).eval()
        d.load_state_dict({k: v.to(dt) for k, v in sd.items()}, strict=True)
        layer = ref_grl.GradientReversalLayer(init_lambda=0.0)
        layer.set_lambda(LAM)
        e = emb.detach().to(dt).clone().requires_grad_(True)
        valid = e[torch.tensor(VALID, dtype=torch.long)]                      # train.py:182-183
        pred = d(layer(valid))                                                # train.py:192-193
        pred_norm = torch.nn.functional.normalize(pred, dim=1)                # train.py:199-202
        target_norm = torch.nn.functional.normalize(target.to(dt), dim=1)
        loss = (1.0 - (pred_norm * target_norm).sum(dim=1)).mean()
        loss.backward()
        out[f"{tag}.pred"] = pred.detach().numpy()
        out[f"{tag}.loss"] = np.array(loss.item(), dtype=pred.detach().numpy().dtype)
        out[f"{tag}.grad_embeddings"] = e.grad.numpy()
        for k, q in d.named_parameters():
            out[f"{tag}.grad.{k}"] = q.grad.numpy()
    out["schedule.steps"] = np.array(STEPS)
    out["schedule.total_warmup"] = np.array([TOTAL, WARMUP])
    out["schedule.grl"] = np.array([float(ref_grl.compute_grl_lambda(s, TOTAL, WARMUP)) for s in STEPS])
    out["schedule.adv_0_1"] = np.array([float(ref_grl.compute_adversarial_lambda(s, TOTAL, WARMUP, 0.0, 1.0)) for s in STEPS])
    out["schedule.adv_02_05"] = np.array([float(ref_grl.compute_adversarial_lambda(s, TOTAL, WARMUP, 0.2, 0.5)) for s in STEPS])
    path = os.path.join(HERE, "adversarial.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
