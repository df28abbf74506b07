"""GPU: the adversarial branch in libmst.so (csrc/head.hip: `mst_disc_forward`, `mst_disc_backward`, `mst_cosdist_forward`,
`mst_cosdist_backward`) and the Python layer over it (SongIdentityDiscriminator, mst_amd.grl, cosine_distance_loss).

Oracle of the kernels: the SAME arithmetic in FLOAT64 with autograd -- the reference's network structure (src/model.py:545-587)
with the two Dropout masks the kernels derive made explicit through `mst_dropout_mask`, and the three loss lines of
src/train.py:199-202.  Bars are those of tests/test_head_gpu.py (it is the same GEMM kernel with shorter sums, at most 2048
products against 6192 there): 2e-5 of the tensor's maximum for pred and dx, 5e-5 for the weight and bias gradients.
The fixture case pins the whole chain (index-select, GRL, discriminator, loss, backward) to the reference's own float64 values
of tests/golden/adversarial.npz.  The contract tests restate the adversarial lines of src/train.py on this package."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adversarial.npz")


def _mask(p, seed, shape):
    from mst_amd import _lib
    n = int(np.prod(shape))
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().mst_dropout_mask(float(p), int(seed), n, _lib.dptr(keep), _lib.stream_ptr(keep.device)), "mst_dropout_mask")
    return keep.view(*shape).double() / (1.0 - p)


def _close(a, ref, tol, name):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.abs().max().item()
    err = (a - ref).abs().max().item()
    print(f"{name}: max |d| {err:.3e} vs scale {scale:.3e} (bar {tol:.0e})")
    assert err <= tol * max(scale, 1e-30), f"{name}: max |d| {err:.3e} vs scale {scale:.3e}"


def _seeds(n):
    """The seeds the autograd Functions will draw next (they take them from torch's CPU generator)."""
    st = torch.get_rng_state()
    out = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(n)]
    torch.set_rng_state(st)
    return out


def _params(d):
    n = d.network
    return [n[0].weight, n[0].bias, n[3].weight, n[3].bias, n[6].weight, n[6].bias]


def _oracle(d, x, R, m1, m2):
    """float64 autograd of the reference structure with explicit masks -> (pred, [dx, six parameter gradients])"""
    from mst_amd.model import SongIdentityDiscriminator
    n = d.network
    d64 = SongIdentityDiscriminator(n[0].in_features, n[0].out_features, n[6].out_features).cuda().double()
    d64.load_state_dict({k: v.double() for k, v in d.state_dict().items()})
    n64 = d64.network
    x64 = x.double().requires_grad_(True)
    h1 = torch.relu(n64[0](x64)) * m1
    h2 = torch.relu(n64[3](h1)) * m2
    ref = n64[6](h2)
    (ref * R.double()).sum().backward()
    return ref, [x64.grad] + [q.grad for q in _params(d64)]


DISC_CASES = [(1, 768, 512, 512, 0.0),      # a single valid row
              (10, 768, 512, 512, 0.3),     # the default
              (67, 100, 72, 40, 0.3),       # M crosses a 64-row tile; no dimension a multiple of 16 or of the 32-wide K chunk
              (200, 512, 512, 512, 0.0)]    # train_baseline.sh
NAMES = ["dx", "network.0.weight", "network.0.bias", "network.3.weight", "network.3.bias", "network.6.weight", "network.6.bias"]


@pytest.mark.parametrize("B,I,H,O,p", DISC_CASES)
def test_discriminator_forward_backward(B, I, H, O, p):
    from mst_amd.model import SongIdentityDiscriminator
    torch.manual_seed(B * 1000 + I)
    d = SongIdentityDiscriminator(I, H, O, dropout=p).cuda().train()
    x = torch.randn(B, I, device="cuda")
    R = torch.randn(B, O, device="cuda")
    ps = _params(d)

    def run():
        torch.manual_seed(99)
        for q in ps:
            q.grad = None
        xg = x.clone().requires_grad_(True)
        pred = d(xg)
        (pred * R).sum().backward()
        return pred.detach(), [xg.grad.clone()] + [q.grad.clone() for q in ps]

    torch.manual_seed(99)
    s1, s2 = _seeds(2) if p > 0 else (0, 0)
    pred, got = run()
    m1 = _mask(p, s1, (B, H)) if p > 0 else 1.0
    m2 = _mask(p, s2, (B, H)) if p > 0 else 1.0
    ref, want = _oracle(d, x, R, m1, m2)
    _close(pred, ref, 2e-5, "pred")
    if p > 0:
        assert not torch.equal(m1, m2)
        for m in (m1, m2):
            keep = (m > 0).double().mean().item()
            assert abs(keep - (1 - p)) <= 4 * (p * (1 - p) / (B * H)) ** 0.5, keep
    for g, r, n in zip(got, want, NAMES):
        _close(g, r, 2e-5 if n == "dx" else 5e-5, n)
    # determinism: the same seed gives the same bits
    pred2, got2 = run()
    assert torch.equal(pred, pred2) and torch.equal(got[0], got2[0]) and torch.equal(got[1], got2[1])
    # a detached input (the discriminator trains alone): dx is skipped, the parameter gradients are the same bits
    torch.manual_seed(99)
    for q in ps:
        q.grad = None
    (d(x) * R).sum().backward()
    assert all(torch.equal(q.grad, g) for q, g in zip(ps, got[1:]))
    # eval mode is the Dropout-free forward
    if p > 0:
        d.eval()
        ref_eval = _oracle(d, x, R, 1.0, 1.0)[0]
        with torch.no_grad():
            _close(d(x), ref_eval, 2e-5, "pred (eval)")


@pytest.mark.parametrize("B,I,H,O,p", [(67, 100, 72, 40, 0.3), (3, 768, 512, 512, 0.0)])
def test_discriminator_forward_without_save_buffer(B, I, H, O, p):
    """`save == NULL` (no backward will follow): the scratch-free kernel computes the same function with the same masks."""
    from mst_amd import _lib
    from mst_amd.model import SongIdentityDiscriminator
    torch.manual_seed(5 + B)
    d = SongIdentityDiscriminator(I, H, O, dropout=p).cuda()
    x = torch.randn(B, I, device="cuda")
    s1, s2 = (1234567891011, 98765432123) if p > 0 else (0, 0)
    dims = _lib.DiscDims(I, H, O)
    wp = _lib.DiscPtrs(*[q.data_ptr() for q in _params(d)])
    pred = torch.empty(B, O, device="cuda")
    L = _lib.lib()
    _lib.check(L.mst_disc_forward(C.byref(dims), C.byref(wp), _lib.dptr(x), B, p, s1, s2, _lib.dptr(pred), None, 0,
                                  _lib.stream_ptr(x.device)), "mst_disc_forward")
    m1 = _mask(p, s1, (B, H)) if p > 0 else 1.0
    m2 = _mask(p, s2, (B, H)) if p > 0 else 1.0
    ref, _ = _oracle(d, x, torch.zeros(B, O, device="cuda"), m1, m2)
    _close(pred, ref, 2e-5, "pred (no save buffer)")
    save = torch.empty(L.mst_disc_save_bytes(C.byref(dims), B), dtype=torch.uint8, device="cuda")
    pred2 = torch.empty(B, O, device="cuda")
    _lib.check(L.mst_disc_forward(C.byref(dims), C.byref(wp), _lib.dptr(x), B, p, s1, s2, _lib.dptr(pred2), _lib.dptr(save), save.numel(),
                                  _lib.stream_ptr(x.device)), "mst_disc_forward")
    _close(pred2, ref, 2e-5, "pred (save buffer)")


def test_discriminator_refusals():
    from mst_amd import _lib
    from mst_amd.model import SongIdentityDiscriminator
    L = _lib.lib()
    x = torch.zeros(4, 64, device="cuda")
    d = SongIdentityDiscriminator(64, 32, 16).cuda()
    wp = _lib.DiscPtrs(*[q.data_ptr() for q in _params(d)])
    pred = torch.empty(4, 16, device="cuda")
    for dims, B in ((_lib.DiscDims(64, 2049, 16), 4), (_lib.DiscDims(0, 32, 16), 4), (_lib.DiscDims(64, 32, 4096), 4),
                    (_lib.DiscDims(64, 32, 16), 0)):
        rc = L.mst_disc_forward(C.byref(dims), C.byref(wp), _lib.dptr(x), B, 0.0, 0, 0, _lib.dptr(pred), None, 0, _lib.stream_ptr(x.device))
        assert rc == -1 and b"mst_disc_forward" in L.mst_last_error()
        assert L.mst_disc_save_bytes(C.byref(dims), B) == 0
    with pytest.raises(RuntimeError, match="fp32"):
        d(x.half())
    with pytest.raises(RuntimeError, match="2048"):
        SongIdentityDiscriminator(64, 2304, 16).cuda()(x)
    with pytest.raises(RuntimeError, match="input_dim"):
        d(torch.zeros(4, 63, device="cuda"))
    d.backend = "torch"
    assert d(x).shape == (4, 16)
    d.backend = "hip"
    with torch.autocast("cuda", dtype=torch.float16):     # src/train.py:251-267: the modules run under autocast
        assert d(x).dtype == torch.float16
    assert d(x.view(2, 2, 64)).shape == (2, 2, 16)


def _cos_ref(pred, target, g):
    p64 = pred.double().requires_grad_(True)
    pred_norm = torch.nn.functional.normalize(p64, dim=1)                 # src/train.py:199-202
    target_norm = torch.nn.functional.normalize(target.double(), dim=1)
    cosine_sim = (pred_norm * target_norm).sum(dim=1)
    loss = (1.0 - cosine_sim).mean()
    (loss * g).backward()
    return loss.detach(), p64.grad


@pytest.mark.parametrize("K,D,zero_row", [(1, 48, False), (7, 48, False), (200, 48, False), (1, 512, False), (7, 512, False),
                                          (200, 512, False), (7, 48, True), (300, 100, True)])
def test_cosine_distance_loss(K, D, zero_row):
    from mst_amd.loss import cosine_distance_loss
    torch.manual_seed(K * 7 + D)
    pred = (torch.randn(K, D, device="cuda") * 3.0)
    target = torch.randn(K, D, device="cuda")
    if zero_row:
        target[K // 2] = 0.0
    g = 0.7

    def run():
        pg = pred.clone().requires_grad_(True)
        loss = cosine_distance_loss(pg, target)
        (loss * g).backward()
        return loss.detach(), pg.grad

    loss, grad = run()
    ref_loss, ref_grad = _cos_ref(pred, target, g)
    _close(loss, ref_loss, 2e-5, "loss")
    _close(grad, ref_grad, 2e-5, "dpred")
    if zero_row:
        assert not grad[K // 2].any()     # loss 1, zero gradient
    loss2, grad2 = run()
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    with pytest.raises(RuntimeError, match="detach"):
        cosine_distance_loss(pred, target.clone().requires_grad_(True))
    # backend="torch" is the same function
    _close(cosine_distance_loss(pred, target, backend="torch"), ref_loss, 2e-5, "loss (torch)")


def test_cosine_distance_loss_zero_prediction_row_follows_the_clamp():
    """|p_i| <= eps: F.normalize divides by eps, so the row's gradient is -(g / K) t^_i / eps (and its loss term is 1)."""
    from mst_amd.loss import cosine_distance_loss
    torch.manual_seed(3)
    K, D = 5, 48
    pred = torch.randn(K, D, device="cuda")
    pred[2] = 0.0
    target = torch.randn(K, D, device="cuda")
    pg = pred.clone().requires_grad_(True)
    loss = cosine_distance_loss(pg, target)
    loss.backward()
    ref_loss, ref_grad = _cos_ref(pred, target, 1.0)
    _close(loss, ref_loss, 2e-5, "loss")
    rest = [0, 1, 3, 4]
    _close(pg.grad[rest], ref_grad[rest], 2e-5, "dpred (rows with a norm)")
    _close(pg.grad[2], ref_grad[2], 2e-5, "dpred (zero row)")
    want = -(1.0 / K) * torch.nn.functional.normalize(target[2].double(), dim=0) / 1e-12
    _close(pg.grad[2], want, 2e-5, "dpred (zero row, closed form)")


def test_fixture_case_against_the_reference_float64_values():
    """The reference's own chain (src/train.py:182-202 on src/grl.py and src/model.py:545-587; tests/golden/make_golden_adv.py)
    on the GPU: the kernels are at most 2x as far from the reference's float64 values as the reference's own fp32 run is, plus
    1e-7 of the tensor's maximum (fp32 against float64 on 96-term sums can be exactly 0 on some elements)."""
    from mst_amd.grl import GradientReversalLayer
    from mst_amd.loss import cosine_distance_loss
    from mst_amd.model import SongIdentityDiscriminator
    gold = np.load(GOLDEN)
    d = SongIdentityDiscriminator(input_dim=96, hidden_dim=80, output_dim=48, dropout=0.3)
    d.load_state_dict({k: torch.from_numpy(gold[f"weight.{k}"]) for k in gold["state_dict_keys"]}, strict=True)
    d = d.cuda().eval()
    layer = GradientReversalLayer(init_lambda=0.0)
    layer.set_lambda(float(gold["grl_lambda"]))
    e = torch.from_numpy(gold["embeddings"]).cuda().requires_grad_(True)
    target = torch.from_numpy(gold["targets"]).cuda()
    valid = e[torch.from_numpy(gold["valid_indices"]).long().cuda()]
    pred = d(layer(valid))
    loss = cosine_distance_loss(pred, target)
    loss.backward()
    got = {"pred": pred, "loss": loss, "grad_embeddings": e.grad}
    got.update({f"grad.{k}": q.grad for k, q in d.named_parameters()})
    bad = []
    for k, v in got.items():
        f64, f32 = gold[f"f64.{k}"].astype(np.float64), gold[f"f32.{k}"].astype(np.float64)
        mine = v.detach().double().cpu().numpy()
        own = np.abs(f32 - f64).max()
        err = np.abs(mine - f64).max()
        bar = 2.0 * own + 1e-7 * np.abs(f64).max()
        print(f"fixture {k}: kernels {err:.3e}, reference fp32 {own:.3e}, bar {bar:.3e}, max {np.abs(f64).max():.3e}")
        if not err <= bar:
            bad.append((k, err, bar))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# src/train.py's adversarial lines, restated on this package with the import swaps only
# ---------------------------------------------------------------------------------------------------------------------
def compute_adversarial_loss(mixing_embeddings, track_dirs, discriminator, grl_layer, song_id_embeddings, song_id_lookup,
                             global_step, total_steps, args, device):                      # train.py:130-204
    import torch.nn as nn
    from mst_amd.grl import compute_grl_lambda
    if args.fixed_grl_lambda is not None:
        lambda_param = args.fixed_grl_lambda
    else:
        lambda_param = compute_grl_lambda(current_step=global_step, total_steps=total_steps,
                                          warmup_steps=args.adversarial_warmup_steps)
    grl_layer.set_lambda(lambda_param)
    valid_indices = []
    target_song_ids = []
    for i, track_dir in enumerate(track_dirs):
        if track_dir in song_id_lookup:
            valid_indices.append(i)
            embedding_idx = song_id_lookup[track_dir]
            target_song_ids.append(song_id_embeddings[embedding_idx])
    if len(valid_indices) == 0:
        return torch.tensor(0.0, device=device, requires_grad=True), lambda_param
    valid_indices = torch.tensor(valid_indices, dtype=torch.long, device=device)
    mixing_emb_valid = mixing_embeddings[valid_indices]
    target_song_id = torch.stack(target_song_ids, dim=0).to(device)
    if args.discriminator_noise > 0.0:
        noise = torch.randn_like(mixing_emb_valid) * args.discriminator_noise
        mixing_emb_valid = mixing_emb_valid + noise
    grl_output = grl_layer(mixing_emb_valid)
    predicted_song_id = discriminator(grl_output)
    pred_norm = nn.functional.normalize(predicted_song_id, dim=1)
    target_norm = nn.functional.normalize(target_song_id, dim=1)
    cosine_sim = (pred_norm * target_norm).sum(dim=1)
    loss = (1.0 - cosine_sim).mean()
    return loss, lambda_param


@pytest.mark.parametrize("noise,disc_lr", [(0.0, None), (0.01, 1e-4)])
def test_reference_adversarial_step_runs_unchanged(tmp_path, noise, disc_lr):
    # ---- the import swaps; everything below follows src/train.py
    from mst_amd.data import FMABaselineDataset, baseline_collate_fn
    from mst_amd.grl import GradientReversalLayer, compute_adversarial_lambda
    from mst_amd.loss import InfoNCELoss
    from mst_amd.model import MixingStyleEncoder, SongIdentityDiscriminator

    class args:   # src/params.py defaults, clip shortened to the toy tracks
        separated_path = cases.write_toy_tracks(str(tmp_path))
        clip_duration, sample_rate, n_fft, hop_length, n_mels = 0.25, 44100, 1024, 256, 128
        band_split_size, band_overlap, encoder_dim = 20, 10, 768
        batch_size, num_workers, learning_rate, weight_decay, temperature, num_epochs = 5, 2, 1e-4, 0.01, 0.1, 2
        use_adversarial = True
        adversarial_lambda, initial_adversarial_lambda, adversarial_warmup_steps = 1.0, 1.0, 2000     # adv_lambda = 1
        fixed_grl_lambda = 0.5
        discriminator_hidden_dim, discriminator_dropout = 512, 0.3
        discriminator_lr, discriminator_noise = disc_lr, noise
        song_id_cache_path = str(tmp_path / "song_identity_embeddings.pt")

    device = torch.device("cuda")
    torch.manual_seed(42)
    np.random.seed(42)
    full_dataset = FMABaselineDataset(separated_path=args.separated_path, clip_duration=args.clip_duration,
                                      sample_rate=args.sample_rate, n_fft=args.n_fft, hop_length=args.hop_length, n_mels=args.n_mels,
                                      num_segments=2, min_audio_duration=25.0)
    train_dataloader = DataLoader(full_dataset, batch_size=args.batch_size, shuffle=True, num_workers=args.num_workers,
                                  collate_fn=baseline_collate_fn, pin_memory=False, prefetch_factor=2, persistent_workers=False,
                                  multiprocessing_context='fork')
    # a song-id cache with all but one of the track dirs: the valid-index filter has something to drop
    cached = sorted(full_dataset.track_dirs)[1:]
    assert len(cached) == len(full_dataset) - 1 == 4
    torch.save({"embeddings": torch.randn(len(cached), 512, generator=torch.Generator().manual_seed(11)), "track_paths": cached},
               args.song_id_cache_path)
    cache = torch.load(args.song_id_cache_path, map_location='cpu')                       # train.py:534-536
    song_id_embeddings = cache['embeddings'].to(device)
    song_id_lookup = {path: idx for idx, path in enumerate(cache['track_paths'])}
    model = MixingStyleEncoder(sample_rate=args.sample_rate, n_fft=args.n_fft, hop_length=args.hop_length, n_mels=args.n_mels,
                               split_size=args.band_split_size, overlap=args.band_overlap, channels=8, embed_dim=args.encoder_dim,
                               feature_dim=full_dataset[0][1][0].shape[0]).to(device)
    discriminator = SongIdentityDiscriminator(                                            # train.py:563-609
        input_dim=args.encoder_dim, hidden_dim=args.discriminator_hidden_dim, output_dim=song_id_embeddings.shape[1],
        dropout=args.discriminator_dropout).to(device)
    grl_layer = GradientReversalLayer(init_lambda=0.0).to(device)
    disc_optimizer = None
    if args.use_adversarial and args.discriminator_lr is not None:
        optimizer = torch.optim.AdamW(model.parameters(), lr=args.learning_rate, weight_decay=args.weight_decay)
        disc_optimizer = torch.optim.AdamW(discriminator.parameters(), lr=args.discriminator_lr, weight_decay=args.weight_decay)
    elif args.use_adversarial:
        parameters = list(model.parameters()) + list(discriminator.parameters())
        optimizer = torch.optim.AdamW(parameters, lr=args.learning_rate, weight_decay=args.weight_decay)
    steps_per_epoch = len(train_dataloader)
    total_steps = args.num_epochs * steps_per_epoch
    criterion = InfoNCELoss(temperature=args.temperature)
    before = {k: v.detach().clone() for k, v in list(model.named_parameters()) + [("disc." + k, v) for k, v in discriminator.named_parameters()]}

    def forward_losses(stems_dict, mixing_features, song_labels, track_dirs, global_step, seed):      # train.py:299-321
        torch.manual_seed(seed)     # the model's Dropout seeds come from the CPU generator: the same masks for every evaluation of a batch
        embeddings = model(stems_dict, mixing_features)
        loss_contrastive = criterion(embeddings, song_labels)
        loss_adversarial = torch.tensor(0.0, device=device)
        adv_lambda = 0.0
        if args.use_adversarial and track_dirs is not None:
            loss_adversarial, grl_lambda = compute_adversarial_loss(embeddings, track_dirs, discriminator, grl_layer, song_id_embeddings,
                                                                    song_id_lookup, global_step, total_steps, args, device)
            adv_lambda = compute_adversarial_lambda(global_step, total_steps, args.adversarial_warmup_steps,
                                                    args.initial_adversarial_lambda, args.adversarial_lambda)
        loss = loss_contrastive + adv_lambda * loss_adversarial if args.use_adversarial else loss_contrastive
        return loss, loss_contrastive, loss_adversarial, adv_lambda

    def zero():
        optimizer.zero_grad()
        if disc_optimizer is not None:
            disc_optimizer.zero_grad()

    def enc_grads():
        return {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}

    model.train()
    discriminator.train()
    losses = []
    for epoch in range(args.num_epochs):
        for batch_idx, batch_data in enumerate(train_dataloader):
            stems_dict, mixing_features, song_labels, track_dirs = batch_data
            stems_dict = {k: v.to(device) for k, v in stems_dict.items()}
            mixing_features = mixing_features.to(device)
            song_labels = song_labels.to(device)
            global_step = epoch * steps_per_epoch + batch_idx
            assert len(track_dirs) == 10 and sum(t in song_id_lookup for t in track_dirs) == 8
            if epoch == 0:
                # the contrastive-only step on this batch ...
                zero()
                args.use_adversarial = False
                forward_losses(stems_dict, mixing_features, song_labels, track_dirs, global_step, 1234)[0].backward()
                args.use_adversarial = True
                g_con = enc_grads()
                assert all(q.grad is None for q in discriminator.parameters())
                # ... is what a reversal strength of 0 leaves of the adversarial step for the encoder, bit for bit, while the
                # discriminator still learns
                zero()
                args.fixed_grl_lambda = 0.0
                forward_losses(stems_dict, mixing_features, song_labels, track_dirs, global_step, 1234)[0].backward()
                args.fixed_grl_lambda = 0.5
                g_zero = enc_grads()
                assert g_zero.keys() == g_con.keys() and all(torch.equal(g_zero[k], g_con[k]) for k in g_con)
                assert all(q.grad is not None and bool(q.grad.any()) for q in discriminator.parameters())
            zero()                                                                         # train.py:246-248
            loss, loss_contrastive, loss_adversarial, adv_lambda = forward_losses(stems_dict, mixing_features, song_labels, track_dirs,
                                                                                  global_step, 1234)
            assert adv_lambda == 1.0 and grl_layer.lambda_param == 0.5
            loss.backward()                                                                # train.py:323-326
            if epoch == 0:
                g_adv = enc_grads()
                assert any(not torch.equal(g_adv[k], g_con[k]) for k in g_con)
                assert not torch.equal(g_adv["audio_encoder.attention_pooling.projection.0.weight"],
                                       g_con["audio_encoder.attention_pooling.projection.0.weight"])
            optimizer.step()
            if disc_optimizer is not None:
                disc_optimizer.step()
            losses.append((loss.detach().item(), loss_contrastive.detach().item(), loss_adversarial.detach().item()))
    assert len(losses) == 2 and np.isfinite(np.array(losses)).all(), losses
    assert all(0.0 <= l[2] <= 2.0 for l in losses), losses
    after = dict(list(model.named_parameters()) + [("disc." + k, v) for k, v in discriminator.named_parameters()])
    moved = [k for k, v in after.items() if not torch.equal(v.detach(), before[k])]
    assert sum(k.startswith("disc.") for k in moved) == 6, moved
    assert len(moved) > 0.9 * len(before), f"only {len(moved)} of {len(before)} parameters changed"
    assert len(model._warned) == 0, model._warned

    # ---- checkpoint with the discriminator (train.py:34-52, :95-97)
    path = str(tmp_path / "checkpoint.pt")
    checkpoint_dict = {'epoch': 1, 'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(),
                       'loss': losses[-1][0], 'discriminator_state_dict': discriminator.state_dict()}
    if disc_optimizer is not None:
        checkpoint_dict['disc_optimizer_state_dict'] = disc_optimizer.state_dict()
    torch.save(checkpoint_dict, path)
    checkpoint = torch.load(path, map_location='cpu')
    fresh = SongIdentityDiscriminator(input_dim=args.encoder_dim, hidden_dim=args.discriminator_hidden_dim,
                                      output_dim=song_id_embeddings.shape[1], dropout=args.discriminator_dropout)
    fresh.load_state_dict(checkpoint['discriminator_state_dict'], strict=True)
    for k, v in discriminator.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v.cpu()), k


def test_example_runs_the_adversarial_branch(tmp_path):
    """examples/train_contrastive.py --use_adversarial, a few steps on toy shards in a fresh child process."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import glob
    import train_contrastive as tc
    shards = str(tmp_path / "shards")
    tc.write_synthetic_shards(shards, 4, 3.0, 44100)
    paths = sorted(glob.glob(os.path.join(shards, "*.pcm16")))
    assert len(paths) == 4
    cache, ckpt = str(tmp_path / "song_ids.pt"), str(tmp_path / "out" / "last.pt")
    torch.save({"embeddings": torch.randn(3, 512, generator=torch.Generator().manual_seed(1)), "track_paths": paths[:3]}, cache)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "train_contrastive.py"), "--shards", shards,
           "--clip-seconds", "1.0", "--batch-size", "4", "--steps", "4", "--use_adversarial", "--song_id_cache_path", cache,
           "--fixed_grl_lambda", "0.5", "--adversarial_warmup_steps", "0", "--initial_adversarial_lambda", "0.5",
           "--discriminator_lr", "1e-4", "--checkpoint", ckpt]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.findall(r"step 4: loss (\S+) adversarial (\S+) grl_lambda (\S+) adv_lambda (\S+)", r.stdout)
    assert len(m) == 1, r.stdout
    loss, adv, grl_lambda, adv_lambda = (float(v) for v in m[0])
    assert math.isfinite(loss) and math.isfinite(adv) and 0.0 <= adv <= 2.0
    assert grl_lambda == 0.5 and 0.5 < adv_lambda <= 1.0
    ck = torch.load(ckpt, map_location="cpu")
    assert sorted(ck["discriminator_state_dict"]) == sorted(f"network.{i}.{n}" for i in (0, 3, 6) for n in ("weight", "bias"))
    assert "disc_optimizer_state_dict" in ck and ck["discriminator_state_dict"]["network.6.weight"].shape == (512, 512)
