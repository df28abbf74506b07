"""Mixing style transfer on audio as it arrives: a CAUSAL FiLM mixer pushed through a clip block by block.

    input stems, target stems -> MixingStyleEncoder (HIP) -> two embeddings -> TCNFiLMGenerator (HIP) -> FiLM, ONCE per song
    next --block samples      -> TCNStream.push (HIP, csrc/tcn_stream.inc)  -> the next --block processed samples

The blocks concatenated are compared with the whole-clip `mixer(x, film_params)` by torch.equal: on the HIP backend the
streamed result is the offline one bit for bit, whatever --block is.  Prints milliseconds per block next to the block's
duration at 44.1 kHz; exits non-zero if the equality fails.

    python examples/stream_style_transfer.py                        # seeded synthetic clips, seeded weights, 512-sample blocks
    python examples/stream_style_transfer.py --block 128 --seconds 10
    python examples/stream_style_transfer.py --tcn_checkpoint ckpt.pt   # the reference's format, trained with causal=True
    python examples/stream_style_transfer.py --lookahead                # a NON-CAUSAL mixer, with a fixed latency
    python examples/stream_style_transfer.py --lookahead --tcn_checkpoint ckpt.pt   # the reference's default: causal=False

--lookahead streams a non-causal mixer through TCNLookaheadStream (csrc/tcn_lookahead.inc): every push returns the samples
that lie `latency` = (K-1) * (2^blocks - 1) samples back, flush() drains the rest at the end of the clip, and the pushes and the
flush without their first `latency` samples are compared with the whole-clip forward in the same way.

Without --tcn_checkpoint the mixer has seeded weights (14 blocks, 16 channels, K = 15: the trainer's defaults).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mst_amd.mixing_utils import STEMS, deferred_features  # noqa: E402
from mst_amd.model import MixingStyleEncoder  # noqa: E402
from mst_amd.synth import synth_batch  # noqa: E402
from mst_amd.tcn_mixer import TCNFiLMGenerator, TCNMixer  # noqa: E402


def embed(encoder, clip, device):
    stems = {s: clip[None, 2 * i:2 * i + 2].to(device) for i, s in enumerate(STEMS)}
    with torch.no_grad():
        return encoder(stems, deferred_features(64)[None].to(device))[0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--block", type=int, default=512, help="samples per push")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tcn_checkpoint", default=None)
    ap.add_argument("--encoder_checkpoint", default=None, help="state_dict of MixingStyleEncoder (reference format)")
    ap.add_argument("--backend", choices=["hip", "torch"], default="hip")
    ap.add_argument("--lookahead", action="store_true", help="a non-causal mixer on the fixed-latency stream (TCNMixer.lookahead_stream)")
    a = ap.parse_args(argv)
    device = torch.device("cuda")
    torch.manual_seed(a.seed)

    encoder = MixingStyleEncoder(feature_dim=64)
    if a.encoder_checkpoint:
        sd = torch.load(a.encoder_checkpoint, map_location="cpu")
        encoder.load_state_dict(sd.get("model_state_dict", sd))
    encoder = encoder.to(device).eval()
    clips = synth_batch(2, int(a.seconds * 44100))        # clip 0: input, clip 1: target style
    e_in, e_tgt = embed(encoder, clips[0], device), embed(encoder, clips[1], device)

    ck = torch.load(a.tcn_checkpoint, map_location="cpu", weights_only=False) if a.tcn_checkpoint else {}
    causal = ck.get("causal", False) if ck else not a.lookahead
    if not causal and not a.lookahead:
        sys.exit("stream_style_transfer: the checkpoint's mixer is not causal (it looks ahead); --lookahead streams it with a fixed "
                 "latency, examples/style_transfer.py runs it on whole clips")
    H, nb, K = ck.get("hidden_channels", 16), ck.get("num_blocks", 14), ck.get("kernel_size", 15)
    tcn = TCNMixer(in_channels=8, hidden_channels=H, num_blocks=nb, kernel_size=K, causal=causal, use_film=True)
    gen = TCNFiLMGenerator(embed_dim=2 * e_in.shape[0], num_blocks=nb, hidden_channels=H)
    if ck:
        tcn.load_state_dict(ck["tcn_state_dict"])
        gen.load_state_dict(ck["film_generator_state_dict"])
    else:
        with torch.no_grad():
            tcn.output_conv.weight.mul_(100.0)            # from its 0.001 init to trained size: y - x is then not ~1e-3
    tcn, gen = tcn.to(device).eval(), gen.to(device).eval()
    tcn.backend = gen.backend = a.backend

    x = clips[0][None].to(device)
    T = x.shape[2]
    with torch.no_grad():
        film = gen(torch.cat([e_in, e_tgt])[None])        # constant for the whole song
        whole = tcn(x, film_params=film)
        make = tcn.lookahead_stream if a.lookahead else tcn.stream
        stream = make(batch_size=1, max_block=a.block, film_params=film)
        latency = stream.latency if a.lookahead else 0
        for t in range(0, min(T, 4 * a.block), a.block):  # warm-up, then from zero history
            stream.push(x[:, :, t:t + a.block])
        stream.reset()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        start.record()
        for t in range(0, T, a.block):
            out.append(stream.push(x[:, :, t:t + a.block]))
        stop.record()
        tail = [stream.flush()] if a.lookahead else []    # the end of the clip: the last `latency` samples
        torch.cuda.synchronize()
    y = torch.cat(out + tail, 2)[:, :, latency:]
    per_block, audio = start.elapsed_time(stop) / len(out), 1000.0 * a.block / 44100
    # bit equality is a property of the HIP kernels; torch picks its summation order by length, so there: to fp32 rounding
    same = torch.equal(y, whole) if a.backend == "hip" else float((y - whole).abs().max()) <= 1e-5 * float(whole.abs().max())
    print(f"TCN: {'causal' if causal else 'non-causal'}, {nb} blocks, {H} channels, K = {K}, receptive field {tcn.receptive_field} samples, backend {a.backend}")
    print(f"{len(out)} pushes of {a.block} samples: {per_block:.3f} ms per block, a block lasts {audio:.3f} ms at 44.1 kHz "
          f"({audio / per_block:.1f} x real time), state {stream.state_bytes / 2 ** 20:.1f} MiB")
    if a.lookahead:
        print(f"latency {latency} samples = {1000.0 * latency / 44100:.1f} ms at 44.1 kHz (every push returns the samples that far back; "
              f"flush() drained the last {latency})")
    print(f"streamed == whole clip: {same}   max |y - x| = {float((y - x).abs().max()):.4f}")
    if not same:
        print(f"max |streamed - whole| = {float((y - whole).abs().max()):.3e}")
        sys.exit(1)
    return {"ms_per_block": per_block, "equal": same}


if __name__ == "__main__":
    main()
