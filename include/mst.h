/*
 * mst.h -- C ABI of libmst.so: MI355X (gfx950) kernels for the contrastive data path of
 * barry-mir/mixing-style-transfer (waveform stems -> [augment] -> STFT -> mel -> 64-d mixing
 * features -> FiLM band-split CNN encoder -> embedding -> InfoNCE), and of its consumer, the TCN mixer of the
 * style-transfer stage (embeddings -> FiLM generator -> dilated residual Conv1d stack on the stems; inference).
 *
 * The reference is 100 % Python and has no FFI; the drop-in boundary is its Python call
 * contract.  Each entry point below names the reference code whose
 * arithmetic it replaces (paths relative to the reference repo).  The Python mirror of the
 * reference classes (mixing-style-transfer_amd/{mixing_utils,model,loss,data}.py) binds these
 * through ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; all `dev` pointers are HIP device pointers owned by the caller
 *     (PyTorch), all `host` pointers are ordinary host memory read during the call only;
 *   - every function returns 0 on success, a negative MST_E* code otherwise, and never throws;
 *     mst_last_error() returns a thread-local description of the last failure;
 *   - the library allocates device memory only inside plan/encoder handles (constant tables and
 *     weights); per-call scratch is a caller-provided workspace (query the size first);
 *   - launches are asynchronous on the given `hipStream_t` (passed as void*; NULL = default
 *     stream), never synchronise, and are safe to capture into a hipGraph;
 *   - handles are immutable after creation and may be shared by concurrent streams as long as
 *     each in-flight call has its own workspace.
 */
#ifndef MST_H_
#define MST_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MST_ABI_VERSION 1

#define MST_OK 0
#define MST_EINVAL (-1)   /* bad argument (shape, NULL pointer, unsupported n_fft ...) */
#define MST_ENOMEM (-2)   /* workspace too small / device allocation failed          */
#define MST_EHIP (-3)     /* a HIP runtime call or kernel launch failed               */

int mst_version(void);
const char* mst_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Stage A: STFT -> mel -> log-mel + mixing features.
 * Replaces: torchaudio MelSpectrogram as called at src/mixing_utils.py:159,280 and
 * src/model.py:58-65; MixingFeatureExtractor.extract_all_features src/mixing_utils.py:71-105
 * (extract_dynamics :107-139, extract_spectral :141-236, extract_stereo :238-268,
 * extract_masking :270-309, compute_loudness :311-318, _flatten_features :320-357).
 * ------------------------------------------------------------------------------------------ */
typedef struct mst_plan mst_plan;

/* window: host [n_fft] analysis window (periodic Hann in the reference);
 * fb:     host [n_fft/2+1][n_mels] row-major mel filterbank exactly as the host framework built
 *         it (torchaudio melscale_fbanks, fp32); each mel band must have contiguous support.
 * detailed_bins: 0 = reference default (5 spectral features/stem, feature_dim 64);
 *         n>0 = use_detailed_spectral mode with n_spectral_bins=n (feature_dim 4*(9+n+2)+8).
 * n_fft in {512,1024,2048}; n_mels <= 256; hop >= 1.                                    */
int mst_plan_create(mst_plan** out, int sample_rate, int n_fft, int hop, int n_mels,
                    const float* window, const float* fb, int detailed_bins);
void mst_plan_destroy(mst_plan* plan);
int mst_plan_frames(const mst_plan* plan, int T);      /* 1 + T / hop (center=True)            */
int mst_plan_feature_dim(const mst_plan* plan);
size_t mst_melfeat_workspace_bytes(const mst_plan* plan, int B, int T);

/* stems:  dev [B][8][T] fp32, channel order vocals L,R, bass L,R, drums L,R, other L,R.
 * logmel: dev [B][8][n_mels][frames] fp32 = log(mel + 1e-10)  (may be NULL: features only)
 * feats:  dev [B][feature_dim] fp32 in the reference's sorted-key layout (may be NULL)
 * Requires T > n_fft/2 (reflect padding), same as torch.stft.                               */
int mst_melfeat_forward(const mst_plan* plan, const float* stems, int B, int T, float* logmel,
                        float* feats, void* workspace, size_t workspace_bytes, void* stream);
/* Same, for the four separate tensors that baseline_collate_fn (src/data.py:291-328) returns:
 * stems4[s] = dev [B][2][T] for s = vocals, bass, drums, other; clip_stride = floats between consecutive
 * clips of one stem (2*T for contiguous (B,2,T) tensors, 8*T for views of a packed [B][8][T] tensor). */
int mst_melfeat_forward_stems(const mst_plan* plan, const float* const stems4[4], long long clip_stride,
                              int B, int T, float* logmel, float* feats, void* workspace,
                              size_t workspace_bytes, void* stream);
/* Same two entry points for int16 PCM stems (the ingest format of SURVEY.md section 8 f2: pre-decoded PCM
 * shards, half the PCIe and HBM bytes of fp32; the reference decodes `{stem}.mp3` to float at
 * src/data.py:169-199).  Samples are converted in-kernel as float(s) * 2^-15 (exact), so the outputs are
 * bit-identical to the fp32 entry points run on that conversion.  clip_stride is in samples.            */
int mst_melfeat_forward_pcm16(const mst_plan* plan, const int16_t* stems, int B, int T, float* logmel,
                              float* feats, void* workspace, size_t workspace_bytes, void* stream);
int mst_melfeat_forward_stems_pcm16(const mst_plan* plan, const int16_t* const stems4[4], long long clip_stride,
                                    int B, int T, float* logmel, float* feats, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* Log-mel layouts.  MST_LOGMEL_REF is the reference's tensor (what MelSpectrogramPreprocessor.forward returns,
 * src/model.py:41-67).  The two channel-minor layouts are the ENCODER-INTERNAL forms: conv1 reads 8-channel patches, and a
 * (frame, band) holding its 8 channels contiguously (32 bytes fp32; 16 + 16 bytes as float16 high / low parts, x = hi + lo to
 * 22 significant bits) lets stage A write whole 128-byte lines once and conv1 load 256-byte runs per frame; the float16
 * form is what the f16 / split-precision convolutions (mst_encoder_set_precision) consume without any conversion pass.  */
#define MST_LOGMEL_REF 0   /* dev [B][8][n_mels][frames] fp32                                            */
#define MST_LOGMEL_CM32 1  /* dev [B][frames][n_mels][8] fp32, 16-byte aligned                           */
#define MST_LOGMEL_CM16 2  /* dev [B][frames][n_mels][8] float16, twice: high parts and low parts        */
/* 1 if stage A writes `layout` directly for this plan (the sliding-window kernels: n_fft 1024 / hop 256 and n_fft 2048 /
 * hop 512), else 0: ask for MST_LOGMEL_REF then.                                                                      */
int mst_plan_layout_supported(const mst_plan* plan, int layout);
typedef struct mst_melfeat_io {
  const void* stems4[4];  /* dev, per stem [B][2][T]: fp32, or int16 PCM when pcm16 != 0 (as the entry points above) */
  long long clip_stride;  /* samples between consecutive clips of one stem                                          */
  int32_t pcm16;
  int32_t layout;         /* MST_LOGMEL_*: layout of `logmel`                                                        */
  void* logmel;           /* dev, may be NULL (features only)                                                        */
  void* logmel_lo;        /* dev, MST_LOGMEL_CM16 only: the low parts; NULL = write the high parts alone (plain f16) */
  uint32_t* absmax;       /* optional dev [B]: max |log-mel| of every clip as float bits (zeroed by the call) -- the    */
                          /* range bound of the float16 convolutions, so that no separate pass reads the log-mel      */
  float* feats;           /* dev [B][feature_dim], may be NULL                                                       */
} mst_melfeat_io;
/* The same launch as mst_melfeat_forward_stems[_pcm16] with the log-mel in any of the layouts above.                  */
int mst_melfeat_forward_io(const mst_plan* plan, const mst_melfeat_io* io, int B, int T, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage B: FiLM MLP + band-split Conv2D/BN/FiLM/ReLU/MaxPool x2 + attention pooling (eval).
 * Replaces: MixingFeatureEncoder.forward src/model.py:410-464, SubSpectrogramCNN.forward
 * :127-157 (x n_subbands, loop :345-362), concat/view :332-367, AttentionPooling.forward
 * :187-211.  BatchNorm uses running statistics, Dropout is identity (model.eval()).
 * ------------------------------------------------------------------------------------------ */
typedef struct mst_encoder mst_encoder;

typedef struct mst_encoder_config {
  int32_t n_mels, split_size, overlap, n_subbands;
  int32_t feature_dim, embed_dim;
  int32_t film_hidden;  /* 256: feature_mlp width        (src/model.py:385-408) */
  int32_t attn_hidden;  /* 256: attention hidden width   (src/model.py:284-288) */
  float bn_eps;         /* 1e-5                                                   */
} mst_encoder_config;

/* All pointers: host fp32, tensors exactly as in the reference state_dict.                   */
typedef struct mst_encoder_weights {
  /* per sub-band i: audio_encoder.subnet_cnns.{i}.* , concatenated over i                    */
  const float* conv1_w;  /* [n_sub][32][8][7][7]  */
  const float* conv1_b;  /* [n_sub][32]           */
  const float* bn1_w, *bn1_b, *bn1_mean, *bn1_var; /* [n_sub][32] */
  const float* conv2_w;  /* [n_sub][64][32][7][7] */
  const float* conv2_b;  /* [n_sub][64]           */
  const float* bn2_w, *bn2_b, *bn2_mean, *bn2_var; /* [n_sub][64] */
  /* film_encoder.* */
  const float* mlp0_w, *mlp0_b;   /* feature_mlp.0  [H][feature_dim], [H] */
  const float* mlp3_w, *mlp3_b;   /* feature_mlp.3  [H][H], [H]           */
  const float* head_w, *head_b;   /* film_head      [n_sub*192][H], [n_sub*192] */
  /* audio_encoder.attention_pooling.* ; C = 64*n_sub*freq_dim */
  const float* att0_w, *att0_b;   /* attention.0   [A][C], [A] */
  const float* att2_w, *att2_b;   /* attention.2   [1][A], [1] */
  const float* proj_w, *proj_b;   /* projection.0  [E][C], [E] */
} mst_encoder_weights;

/* Optional device outputs for intermediate activations (parity tests); any may be NULL.      */
typedef struct mst_encoder_taps {
  float* film;     /* dev [B][n_sub*192]                      */
  float* pool1;    /* dev [B][n_sub][32][H1][W1]              */
  float* pool_in;  /* dev [B][64*n_sub*freq_dim][W2]  (input of attention pooling) */
  void* events[6]; /* optional hipEvent_t recorded on the stream: [0] start, [1] after FiLM MLP, [2] after conv1,
                      [3] after conv2, [4] after attention scores, [5] end (per-kernel timing for bench.py) */
} mst_encoder_taps;

int mst_encoder_create(mst_encoder** out, const mst_encoder_config* cfg,
                       const mst_encoder_weights* w);
void mst_encoder_destroy(mst_encoder* enc);
/* Optional: mode 1 runs conv1, mode 2 conv1 and conv2, on the f16 matrix cores with 3-term split precision
 * (x = xh + xl, w = wh + wl; xh*wh + xh*wl + xl*wh, fp32 accumulate; per-product error ~2^-22).  conv2's f16 input is
 * range-scaled per (clip, sub-band) by an exact power of two derived on the device from a bound on conv1's output
 * (||w||_1 * max|log-mel| through the folded affine), so no activation magnitude overflows f16 and nothing is refused.  Mode 3 runs both convolutions with plain f16 operands (xh * wh only, fp32 accumulate):
 * the arithmetic of the reference's `--use_amp` autocast convolutions (src/train.py:251-253), ~1e-3 of fp32.
 * 0 (default) = exact fp32 MFMA.  Call before mst_encoder_workspace_bytes. */
int mst_encoder_set_precision(mst_encoder* enc, int conv1_f16x3);
size_t mst_encoder_workspace_bytes(const mst_encoder* enc, int B, int frames);
/* logmel: dev [B][8][n_mels][frames]; feats: dev [B][feature_dim]; emb: dev [B][embed_dim]  */
int mst_encoder_forward(const mst_encoder* enc, const float* logmel, int frames, const float* feats,
                        int B, float* emb, const mst_encoder_taps* taps, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The same forward with the log-mel in one of the encoder-internal channel-minor layouts that stage A writes directly
 * (MST_LOGMEL_*, mst_melfeat_forward_io): MST_LOGMEL_CM32 for the exact-fp32 conv1 (20-mel sub-bands, or an even
 * split_size below 20), MST_LOGMEL_CM16 (high + low float16 planes; the plain-f16 mode 3 reads the high parts only) for
 * the f16 / split-precision modes of mst_encoder_set_precision.  mst_encoder_layout_supported answers for the encoder's
 * CURRENT precision mode.  absmax: stage A's per-clip max |log-mel| (float bits) -- required with MST_LOGMEL_CM16 in the
 * modes that run conv2 on float16 as well (2, 3), optional otherwise (it saves the pass that derives it).          */
typedef struct mst_logmel_in {
  int32_t layout;          /* MST_LOGMEL_*                                     */
  int32_t pad_;
  const void* data;        /* dev: the log-mel (MST_LOGMEL_CM16: high parts)   */
  const void* lo;          /* dev: MST_LOGMEL_CM16 low parts, else NULL        */
  const uint32_t* absmax;  /* dev [B] or NULL                                  */
} mst_logmel_in;
int mst_encoder_layout_supported(const mst_encoder* enc, int layout);
int mst_encoder_forward_in(const mst_encoder* enc, const mst_logmel_in* logmel, int frames, const float* feats,
                           int B, float* emb, const mst_encoder_taps* taps, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Training forward (first half): the same network with train-mode BatchNorm -- batch statistics over
 * (B, H, W) per (sub-band, channel), biased variance, as nn.BatchNorm2d in training mode (src/model.py:107-125 under
 * model.train()) -- and Dropout as identity (pass p = 0 modules; dropout masks are the caller's business until the
 * backward kernels land).  The raw convolution outputs are kept in the workspace in accumulator order for the
 * backward pass.  taps (all optional, device): film / pool1 / pool_in as above; bn1 [n_sub][32][2], bn2 [n_sub][64][2]
 * = (batch mean, 1/sqrt(biased var + eps)) -- the caller updates its running statistics from them.
 * Needs the default 20-mel sub-bands.  Workspace: mst_encoder_train_workspace_bytes (3.6 GB + 1.1 GB of saved
 * activations at 72 clips of 10 s).                                                                           */
typedef struct mst_encoder_train_taps {
  float* film;
  float* pool1;
  float* pool_in;
  float* bn1;
  float* bn2;
  const float* film_in; /* optional INPUT dev [B][n_sub*192]: FiLM parameters from the caller's own MLP (then feats may
                           be NULL); emb may be NULL as well: stop at pool_in, the caller runs its own pooling head */
  const unsigned char* drop1_mask; /* optional INPUT dev, layout of pool1: Dropout keep-mask after the first pooling
                                      (src/model.py:118: Dropout(0.3)); pool1 = mask ? pooled * drop1_scale : 0 */
  float drop1_scale;               /* 1 / (1 - p) */
  /* Data-parallel training with CROSS-RANK BatchNorm statistics (what the single-process reference computes on
   * the whole batch, src/model.py:107-125 under src/train.py:211).  phase 0 (default): the whole forward.  Otherwise the
   * forward runs in three calls with the same arguments -- 1: FiLM + conv1 raw output and its statistics; 2: BatchNorm 1 +
   * FiLM + pooling + conv2 raw output and its statistics; 3: BatchNorm 2 + FiLM + pooling + head -- and between the calls
   * the caller SUMS the statistics accumulators over its ranks (mst_encoder_train_stats_buffer: 64-bit integers, so the sum
   * is exact and order-independent).  The buffer's last word pair carries the CLIP COUNT: every phased call writes this
   * rank's B there, the all-reduce turns it into the global count, and the BatchNorm kernels divide by it -- ranks may hold
   * different numbers of clips (a ragged last batch).  count_scale: kept for ABI compatibility, ignored by the phased calls
   * (phase 0 normalises by B).                                                                                            */
  int phase;
  double count_scale;
  /* Dropout drawn BY the kernel (instead of drop1_mask): with drop1_mask_out != NULL and 0 < drop1_p < 1 the first-pooling
   * epilogue keeps element o iff philox2x32-10(drop1_seed, o) >= drop1_p * 2^32, scales the kept ones by 1 / (1 - p) and
   * writes the keep-mask (uint8, layout of pool1) to drop1_mask_out -- pass that buffer to mst_encoder_train_conv2_dgrad.  */
  unsigned char* drop1_mask_out;
  uint64_t drop1_seed;
  float drop1_p;
} mst_encoder_train_taps;
size_t mst_encoder_train_workspace_bytes(const mst_encoder* enc, int B, int frames);
/* Where the statistics accumulators of conv layer 1 or 2 sit inside the training workspace: byte offset and number of
 * int64 words ([n_sub][C][2 sums][2 words], then 2 words whose first is the rank's clip count -- sum them all).  The forward (sum y, sum y^2) and the backward pass (sum dz, sum dz * zhat)
 * use the same words; all-reduce them with SUM between the phases.  Returns 0 on success.                          */
int mst_encoder_train_stats_buffer(const mst_encoder* enc, int layer, int B, int frames, size_t* offset_bytes,
                                   size_t* n_int64);
int mst_encoder_forward_train(const mst_encoder* enc, const float* logmel, int frames, const float* feats, int B,
                              float* emb, const mst_encoder_train_taps* taps, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The same with a described log-mel (mst_logmel_in, above).  The float16 training modes (mst_encoder_set_train_precision 1, 2)
 * read stage A's MST_LOGMEL_CM16 planes directly -- no fp32 -> float16 conversion while staging, no pass for the per-clip
 * maximum (absmax is required with that layout); the fp32 mode takes MST_LOGMEL_REF only.
 * mst_encoder_train_layout_supported answers for the CURRENT training precision.  The weight gradient of conv1
 * (mst_encoder_train_conv1_wgrad_in) must be given the same log-mel.                                                  */
int mst_encoder_train_layout_supported(const mst_encoder* enc, int layout);
int mst_encoder_forward_train_in(const mst_encoder* enc, const mst_logmel_in* logmel, int frames, const float* feats, int B,
                                 float* emb, const mst_encoder_train_taps* taps, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Operand precision of the TRAINING kernels (all six entry points below and mst_encoder_forward_train).
 * 0 (default): exact fp32 MFMA.  1: float16 operands, fp32 accumulation -- the arithmetic of the reference's `--use_amp`
 * step (autocast + GradScaler, src/train.py:251-262, src/params.py:71; BASELINE configs[4]): both operands of every
 * convolution-shaped product are rounded to f16 (forward y = conv(f16 x, f16 w); input gradient conv^T(f16 dy, f16 w);
 * weight gradient corr(f16 x, f16 dy)) and the convolution outputs are STORED as f16 (as autocast's are; BatchNorm's batch
 * statistics are those of the stored values); the BatchNorm / FiLM / pooling arithmetic, their backward, all reductions and
 * the master weights stay fp32.  Every rounded tensor is first multiplied by an exact power of two chosen on the device (weights per
 * output channel; pool1 and the stored conv outputs per band from bounds on their values; the gradients by one factor per backward pass from
 * max |d pool_in| -- the internal equivalent of the reference's loss scale) and the factor is divided out in fp32, so neither
 * f16's ceiling nor its subnormals are reached; no host synchronisation.  Needs 20-mel sub-bands.
 * 2: the same kernels with THREE-TERM SPLIT PRECISION -- every operand is a pair hi + lo of float16 (22 significant bits),
 * a product is lo*hi + hi*lo + hi*hi in three MFMAs, fp32 accumulation: results equivalent to the fp32 kernels (tested at
 * their bar) at a third of the f16 matrix rate, i.e. ~5x the fp32 rate.
 * In modes 1 and 2 the `dy` of mst_encoder_train_backward_apply(layer 2) and the `dy2` of mst_encoder_train_conv2_dgrad are
 * a float16 buffer [n_sub][B][H1][W1][64] (channel-minor; mode 2: [2][n_sub][B][H1][W1][64], low parts second; pass it
 * through), layer 1's dy must be NULL, and d pool_in must be contiguous.
 * Call before mst_encoder_train_workspace_bytes and mst_encoder_update_trunk_params.                              */
int mst_encoder_set_train_precision(mst_encoder* enc, int mode);

/* Refresh the convolution / BatchNorm parameters of the TRAINING kernels from device tensors (concatenated over the
 * sub-bands, reference state_dict shapes) -- once per optimizer step; re-swizzles the MFMA weight fragments on the
 * device.  The eval-only tables (folded running statistics, FiLM / pooling-head weights) are NOT refreshed: call
 * mst_encoder_update_params before evaluating after training.                                                    */
int mst_encoder_update_trunk_params(mst_encoder* enc, const float* conv1_w, const float* conv1_b, const float* bn1_w,
                                    const float* bn1_b, const float* conv2_w, const float* conv2_b,
                                    const float* bn2_w, const float* bn2_b, void* stream);

/* Running statistics of BatchNorm layer 1 / 2 after mst_encoder_forward_train, as nn.BatchNorm2d updates them in training mode
 * (src/model.py:107-125): running = (1 - momentum) running + momentum batch (unbiased batch variance), num_batches_tracked += 1.
 * running_mean / running_var: dev [n_sub][C] (the sub-bands' buffers stacked), num_batches_tracked: dev int64 [n_sub];
 * reads the batch statistics the forward left in `workspace` (same buffer, B, frames); cross_rank != 0: the element count is taken
 * from the summed clip-count word of the statistics buffer (mst_encoder_train_stats_buffer), i.e. the GLOBAL batch.  One launch. */
int mst_encoder_train_update_running_stats(const mst_encoder* enc, int layer, int B, int frames, float* running_mean,
                                           float* running_var, long long* num_batches_tracked, float momentum, int cross_rank,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* Device-side refresh of EVERY parameter table of an existing encoder -- what a trainer calls before a validation pass after
 * optimizer steps (src/train.py:388-427 follows :292-296): `w` has mst_encoder_create's fields, but every pointer is a DEVICE
 * tensor in state_dict layout (the sub-band tensors stacked over the bands).  Fragment swizzles, the eval BatchNorm fold, the
 * float16 fragments with their power-of-two pre-scales, transposes and copies all run as kernels on `stream`: no host
 * round trip, no synchronisation, no allocation.  mst_encoder_create runs this same call on device copies of its host
 * arrays, so a refreshed handle holds the bits a fresh one would.  The configuration (shapes) must be the one the
 * encoder was created with.                                                                                           */
int mst_encoder_update_params(mst_encoder* enc, const mst_encoder_weights* device_weights, void* stream);

/* Backward of max-pool / ReLU / FiLM / BatchNorm(batch statistics) of conv layer 1 or 2, from the activations that
 * mst_encoder_forward_train left in `workspace` (same buffer, same B and frames).
 * dpool: gradient of the pooled activation; element (clip, band, ch, r, c) at
 *        dpool[clip*dp_clip + band*dp_band + ch*dp_ch + r*cols + c]   (layer 1: pool1 10 x W1; layer 2: pool_in 2 x W2).
 * dy:    out, gradient of the convolution output, [n_sub][B][C][rows][cols] (per band a contiguous NCHW tensor: the
 *        operand of a library convolution weight / input gradient); layer 1 only: NULL = keep it in the workspace in
 *        accumulator order for mst_encoder_train_conv1_wgrad.
 * dfilm: [B][n_sub*192], the layer's gamma / beta slots are ACCUMULATED (+=): zero it once per step.
 * dbn:   out [2][n_sub][C]: the plane of d BatchNorm weight, then the plane of d BatchNorm bias (each is the stacked
 *        gradient tensor of its parameter family).                                                               */
int mst_encoder_train_backward_apply(const mst_encoder* enc, int layer, int B, int frames, const float* dpool,
                                     long long dp_clip, long long dp_band, long long dp_ch, float* dy, float* dfilm,
                                     float* dbn, void* workspace, size_t workspace_bytes, void* stream);
/* The same in phases, for cross-rank BatchNorm statistics (see mst_encoder_train_taps::phase): 0 = everything (the call
 * above); 1 = (f16 training modes, layer 2) max |d pool_in| of this rank into the scale word -- all-reduce it with MAX
 * (mst_encoder_train_scale_buffer), so that every rank derives the same internal loss scale; 2 = pass A, the sums over this
 * rank's clips -- all-reduce the layer's statistics buffer with SUM; 3 = pass B and the outputs.  count_scale as above.  */
int mst_encoder_train_backward_apply_phase(const mst_encoder* enc, int layer, int B, int frames, const float* dpool,
                                           long long dp_clip, long long dp_band, long long dp_ch, float* dy, float* dfilm,
                                           float* dbn, void* workspace, size_t workspace_bytes, void* stream, int phase,
                                           double count_scale);
/* f16 training modes: byte offset inside the workspace of the 32-bit word that holds max |d pool_in| as a float bit pattern
 * (non-negative floats order like unsigned integers: all-reduce with MAX on int32).  Returns non-zero in fp32 mode.     */
int mst_encoder_train_scale_buffer(const mst_encoder* enc, int B, int frames, size_t* offset_bytes);

/* conv1 weight gradient, hand-written fp32-MFMA GEMM over positions.  Call after
 * mst_encoder_train_backward_apply(layer 1) with dy == NULL: that variant leaves d(conv1 output) in the workspace, in
 * place of the saved activation, in accumulator order (the operand layout of this kernel).
 * dw: out dev [n_sub][32][8][7][7] (zeroed here).  The bias gradient of a convolution that feeds a batch-statistics
 * BatchNorm is identically zero and is not computed.                                                            */
int mst_encoder_train_conv1_wgrad(const mst_encoder* enc, const float* logmel, int B, int frames, float* dw,
                                  void* workspace, size_t workspace_bytes, void* stream);
int mst_encoder_train_conv1_wgrad_in(const mst_encoder* enc, const mst_logmel_in* logmel, int B, int frames, float* dw,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* conv2 weight gradient, same scheme (dy of layer 2 is always left in the workspace in accumulator order by
 * mst_encoder_train_backward_apply(layer 2), next to the NCHW copy it returns).
 * pool1: dev [B][n_sub][32][H1][W1], the (dropped-out) input of conv2 as the training forward produced it.
 *        NULL in the float16 training modes: the operand is taken from the float16 pool1 planes the training forward left in
 *        the workspace (the bits the fp32 tensor would be rounded to); mst_encoder_forward_train then writes the fp32 pool1
 *        only when taps->pool1 asks for it.
 * dw:    out dev [n_sub][64][32][7][7] (zeroed here).                                                           */
int mst_encoder_train_conv2_wgrad(const mst_encoder* enc, const float* pool1, int B, int frames, float* dw,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* conv2 input gradient: the chunked fp32-MFMA convolution kernel run on d(conv2 output) with the transposed, flipped
 * weights (64 -> 32 channels), Dropout keep-mask applied on the way out.
 * dy2:    dev [n_sub][B][64][H1][W1]  (the NCHW-per-band tensor mst_encoder_train_backward_apply(layer 2) returns).
 * dpool1: out dev [B][n_sub][32][H1][W1] = gradient of pool1 (feed it to backward_apply(layer 1)).
 * drop1_mask / drop1_scale: as in mst_encoder_train_taps (NULL: no dropout).                                      */
int mst_encoder_train_conv2_dgrad(const mst_encoder* enc, const float* dy2, int B, int frames, float* dpool1,
                                  const unsigned char* drop1_mask, float drop1_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frozen encoder: the gradient of the embedding to the LOG-MEL through an encoder whose parameters are constants
 * (eval-mode BatchNorm with the running statistics, no Dropout, FiLM from constant mixing features) -- the style term of
 * the style-transfer trainer.  fp32 only; first-pool heights 1 and 2 (split_size < 30) and frames >= 20, as the training
 * kernels; anything else returns an error naming the reason.  Nothing is allocated after handle creation; everything
 * runs on the caller's stream without host synchronisation.  The handle's tables follow mst_encoder_create /
 * mst_encoder_update_params (the eval handle's refresh).
 *
 * mst_encoder_forward_frozen: the eval-mode forward (same embedding as mst_encoder_forward within the forward tolerance;
 *   other kernels) that KEEPS the raw convolution outputs and the eval affines in `workspace` for the calls below.  One
 *   workspace per forward pass that is still to be differentiated; the backward calls read it and leave it intact, so a
 *   pass may be differentiated any number of times.  logmel: dev [B][8][n_mels][frames] (MST_LOGMEL_REF).  emb may be NULL
 *   (the caller runs its own head on taps->pool_in).  taps (optional): film, pool1, pool_in; events are ignored.
 * mst_encoder_frozen_backward_apply: backward of max-pool -> ReLU -> affine of conv layer 1 or 2:
 *   dy[band][B][C][rows][cols] = A(clip, band, ch) * dpool at the first arg-max (row-major) of every pooling window whose
 *   maximum is positive, 0 elsewhere.  dpool: layer 1 [B][n_sub][32][H1][W1], layer 2 [B][64*n_sub*freq_dim][W2], given by
 *   its clip / band / channel strides in floats (rows are the pooled width apart).  No FiLM gradient here: see
 *   mst_encoder_frozen_film_grad.
 * mst_encoder_frozen_film_grad: the gradient to the FiLM tensor of conv layer 1 or 2 from the same dpool (for a caller that
 *   differentiates the mixing features): with z = gamma u + beta, u = BN_eval(conv + bias) from the raw output and the
 *   running statistics (no division by gamma) and df the pool / ReLU-routed cotangent, dgamma = sum df u, dbeta = sum df.
 *   dfilm: dev [B][n_sub*192], per band [gamma1(32) beta1(32) gamma2(64) beta2(64)]; a call WRITES its layer's slots and
 *   leaves the other layer's alone.  Fixed-order sums (order-independent accumulators): bit-reproducible.
 * conv2 input gradient: mst_encoder_train_conv2_dgrad with drop1_mask = NULL.
 * mst_encoder_conv1_dgrad: dy1 dev [n_sub][B][32][split_size][frames] -> dlogmel dev [B][8][n_mels][frames]: per band
 *   the 7x7 convolution with the transposed, flipped conv1 weights on the band's own rows (exact-fp32 MFMA), then the
 *   bands that hold a mel row added in ascending band order by one thread per element (no atomics: bit-reproducible, a
 *   clip's result does not depend on its batch neighbours); mel rows no band covers get exact zeros.                    */
size_t mst_encoder_frozen_workspace_bytes(const mst_encoder* enc, int B, int frames);
int mst_encoder_forward_frozen(const mst_encoder* enc, const float* logmel, int frames, const float* feats, int B, float* emb,
                               const mst_encoder_taps* taps, void* workspace, size_t workspace_bytes, void* stream);
int mst_encoder_frozen_backward_apply(const mst_encoder* enc, int layer, int B, int frames, const float* dpool,
                                      long long dp_clip, long long dp_band, long long dp_ch, float* dy, void* workspace,
                                      size_t workspace_bytes, void* stream);
int mst_encoder_frozen_film_grad(const mst_encoder* enc, int layer, int B, int frames, const float* dpool,
                                 long long dp_clip, long long dp_band, long long dp_ch, float* dfilm, void* workspace,
                                 size_t workspace_bytes, void* stream);
int mst_encoder_conv1_dgrad(const mst_encoder* enc, const float* dy1, int B, int frames, float* dlogmel, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Augmentation chain.  Replaces AudioAugmenter.augment_stems src/mixing_utils.py:376-419 and
 * apply_spectral_tilt :421-433, apply_compression :435-447, apply_bandwidth_limit :449-456,
 * apply_reverb :458-479.  Every random decision is drawn by the HOST in the reference's order
 * with the reference's RNG (torch CPU generator) and passed in; the kernels are deterministic.
 * ------------------------------------------------------------------------------------------ */
typedef struct mst_aug_stem {
  float gain;          /* linear gain, 1.0f = none             (:389-392)                   */
  int32_t tilt;        /* 0 none, 1 section in tilt_sos        (:421-433)                   */
  int32_t compress;    /* 0 none; 1: the reference's default 4:1 above -20 dB; 2: comp_threshold_db / comp_ratio (:435-447) */
  int32_t bw_sections; /* 0 none, else #biquads in bw_sos (2)  (:449-456)                   */
  double tilt_sos[6];  /* scipy.signal.butter(..., output='sos') rows b0 b1 b2 a0 a1 a2     */
  double bw_sos[12];
  float comp_threshold_db; /* compress == 2: apply_compression(audio, threshold, ratio), threshold in dB ... */
  float comp_ratio;        /* ... and ratio > 0                                               */
} mst_aug_stem;

typedef struct mst_aug_clip {
  mst_aug_stem stem[4];
  int32_t reverb;      /* 0/1: reverb of the summed mix, redistributed (:404-417)           */
  int32_t pad_;
} mst_aug_clip;

size_t mst_aug_workspace_bytes(int B, int T, int ir_len);
/* stems_inout: dev [B][8][T] modified in place; decisions: host [B];
 * reverb_ir:   dev [B][ir_len] (rows of clips with reverb==0 are ignored; may be NULL if none).
 * Any T >= 1 and any ir_len >= 1 (shorter or longer than T): no limit on the number of 16 384-sample segments of a clip;
 * the index arithmetic holds for T <= 2^24.                                                                          */
int mst_aug_apply(const mst_aug_clip* decisions, int B, int T, float* stems_inout,
                  const float* reverb_ir, int ir_len, void* workspace, size_t workspace_bytes,
                  void* stream);

/* The same on clips that sit `clip_stride` floats apart (>= 8 * T; each clip's 8 channels contiguous): e.g. the
 * negatives of a triplet batch, every third clip of the batch tensor, augmented where they stand.               */
int mst_aug_apply_strided(const mst_aug_clip* decisions, int B, int T, float* stems_inout, long long clip_stride,
                          const float* reverb_ir, int ir_len, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Out of place: stems_out[b] = augment(src[b]) -- the reference's `stems.clone()` (src/mixing_utils.py:386) folded into the
 * first pass over the audio instead of a copy before it.  src: dev, B clips `src_stride` floats apart, never written; stems_out:
 * dev, B clips `clip_stride` floats apart, every sample written (a stem without a decision is copied).  The address ranges of
 * src and stems_out must be disjoint (MST_EINVAL otherwise); src == stems_out with equal strides is mst_aug_apply_strided.  */
int mst_aug_apply_from(const mst_aug_clip* decisions, int B, int T, const float* src, long long src_stride,
                       float* stems_out, long long clip_stride, const float* reverb_ir, int ir_len,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training forward / backward of the two small networks around the convolution trunk, fp32, deterministic
 * (fixed-order reductions, no atomics), Dropout masks never stored -- a keep decision is a pure function of
 * (seed, element index), Philox-2x32-10, re-derived by every kernel that needs it; p = 0 switches a Dropout off.
 * All weight / gradient pointers are DEVICE tensors in state_dict layout (row-major nn.Linear weights [out][in]).
 *
 * Attention-pooling head = the reference's  F.dropout -> AttentionPooling  (src/model.py:118 for the Dropout in front,
 * :187-211):  xd = Dropout_in(pool_in);  a = softmax_t(att2 . tanh(att0 xd_t + b0) + b2);  pooled = sum_t a_t xd_t;
 * emb = Dropout_out(ReLU(proj pooled + bp)).     pool_in: dev [B][channels][frames];  emb: dev [B][embed_dim].
 * `save` (mst_head_save_bytes) carries the activations the backward needs and must stay untouched until then.
 * mst_head_backward: demb [B][embed_dim] -> the six parameter gradients (overwritten) and dpool_in [B][channels][frames].
 * ------------------------------------------------------------------------------------------ */
typedef struct mst_head_dims { int32_t channels, frames, attn_hidden, embed_dim; } mst_head_dims;   /* attn_hidden <= 256, channels <= 3072 */
typedef struct mst_head_weights {
  const float *att0_w, *att0_b;   /* attention.0   [A][C], [A] */
  const float *att2_w, *att2_b;   /* attention.2   [1][A], [1] */
  const float *proj_w, *proj_b;   /* projection.0  [E][C], [E] */
} mst_head_weights;
typedef struct mst_head_grads { float *att0_w, *att0_b, *att2_w, *att2_b, *proj_w, *proj_b; } mst_head_grads;
size_t mst_head_save_bytes(const mst_head_dims* dims, int B, float drop_in_p);   /* (holds Dropout_in(pool_in) when drop_in_p > 0) */
size_t mst_head_backward_workspace_bytes(const mst_head_dims* dims, int B);
int mst_head_forward_train(const mst_head_dims* dims, const mst_head_weights* w, const float* pool_in, int B, float drop_in_p,
                           uint64_t drop_in_seed, float drop_out_p, uint64_t drop_out_seed, float* emb, void* save,
                           size_t save_bytes, void* stream);
int mst_head_backward(const mst_head_dims* dims, const mst_head_weights* w, const float* pool_in, int B, float drop_in_p,
                      uint64_t drop_in_seed, float drop_out_p, uint64_t drop_out_seed, const float* demb, const void* save,
                      const mst_head_grads* grads, float* dpool_in, void* workspace, size_t workspace_bytes, void* stream);

/* The keep mask those Dropouts use, materialised: keep[i] = 1 iff element i (row-major index in the dropped tensor) survives
 * Dropout(p) under `seed`; survivors are scaled by 1 / (1 - p).  For tests and for callers that want the mask itself.   */
int mst_dropout_mask(float p, uint64_t seed, long long n, unsigned char* keep, void* stream);

/* FiLM MLP = MixingFeatureEncoder.forward (src/model.py:410-464) in training mode:
 * film = head(ReLU(mlp3(Dropout(ReLU(mlp0 feats)))));  feats: dev [B][feature_dim];  film: dev [B][out_dim] (n_sub * 192).
 * mst_film_backward: dfilm [B][out_dim] -> the six parameter gradients (overwritten); the features get no gradient here
 * (mst_film_input_grad below: eval mode).                                                                               */
typedef struct mst_film_dims { int32_t feature_dim, hidden, out_dim; } mst_film_dims;                /* feature_dim, hidden <= 2048 */
typedef struct mst_film_weights {
  const float *mlp0_w, *mlp0_b;   /* feature_mlp.0 [H][Fd], [H] */
  const float *mlp3_w, *mlp3_b;   /* feature_mlp.3 [H][H], [H]  */
  const float *head_w, *head_b;   /* film_head     [O][H], [O]  */
} mst_film_weights;
typedef struct mst_film_grads { float *mlp0_w, *mlp0_b, *mlp3_w, *mlp3_b, *head_w, *head_b; } mst_film_grads;
size_t mst_film_save_bytes(const mst_film_dims* dims, int B);
size_t mst_film_backward_workspace_bytes(const mst_film_dims* dims, int B);
int mst_film_forward_train(const mst_film_dims* dims, const mst_film_weights* w, const float* feats, int B, float drop_p,
                           uint64_t drop_seed, float* film, void* save, size_t save_bytes, void* stream);
int mst_film_backward(const mst_film_dims* dims, const mst_film_weights* w, const float* feats, int B, float drop_p,
                      const float* dfilm, const void* save, const mst_film_grads* grads, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Gradient to the INPUT of the FiLM MLP, eval mode (no Dropout): dfilm [B][out_dim] -> dfeats [B][feature_dim] (overwritten)
 * through head -> ReLU -> mlp3 -> ReLU -> mlp0; the hidden activations are recomputed from feats.  Fixed-order split sums. */
size_t mst_film_input_grad_workspace_bytes(const mst_film_dims* dims, int B);
int mst_film_input_grad(const mst_film_dims* dims, const mst_film_weights* w, const float* feats, int B, const float* dfilm,
                        float* dfeats, void* workspace, size_t workspace_bytes, void* stream);

/* Song-identity discriminator of the adversarial branch = SongIdentityDiscriminator.forward (src/model.py:545-587):
 * h1 = Dropout(ReLU(w0 x + b0));  h2 = Dropout(ReLU(w3 h1 + b3));  pred = w6 h2 + b6.   x: dev [B][in_dim];  pred: dev [B][out_dim].
 * Both Dropouts use drop_p (0 = eval mode / no dropout); the keep decision of element m * hidden + n of h1 / h2 is that of
 * mst_dropout_mask under seed1 / seed2.  `save` (mst_disc_save_bytes) carries the activations to the backward; NULL when no
 * backward will follow (a row-per-workgroup kernel then computes the same function without any scratch).
 * mst_disc_backward: dpred [B][out_dim] -> the six parameter gradients (overwritten) and dx [B][in_dim]; dx == NULL skips the
 * input gradient (a caller that trains the discriminator alone).  Every dimension 1..2048, B >= 1.                          */
typedef struct mst_disc_dims { int32_t in_dim, hidden, out_dim; } mst_disc_dims;
typedef struct mst_disc_weights {
  const float *w0, *b0;   /* network.0 [H][in_dim], [H] */
  const float *w3, *b3;   /* network.3 [H][H], [H]      */
  const float *w6, *b6;   /* network.6 [O][H], [O]      */
} mst_disc_weights;
typedef struct mst_disc_grads { float *w0, *b0, *w3, *b3, *w6, *b6; } mst_disc_grads;
size_t mst_disc_save_bytes(const mst_disc_dims* dims, int B);
size_t mst_disc_backward_workspace_bytes(const mst_disc_dims* dims, int B);
int mst_disc_forward(const mst_disc_dims* dims, const mst_disc_weights* w, const float* x, int B, float drop_p, uint64_t seed1,
                     uint64_t seed2, float* pred, void* save, size_t save_bytes, void* stream);
int mst_disc_backward(const mst_disc_dims* dims, const mst_disc_weights* w, const float* x, int B, float drop_p, uint64_t seed1,
                      uint64_t seed2, const float* dpred, const void* save, const mst_disc_grads* grads, float* dx,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Cosine-distance loss of the adversarial branch (src/train.py:199-202):
 * loss = mean_i (1 - p_i . t_i / (max(|p_i|, 1e-12) max(|t_i|, 1e-12))).   pred, target: dev [K][D], K >= 1, 1 <= D <= 2048.
 * loss: dev [1];  save: dev [K][3] = (p.p, t.t, p.t) per row, taken back by the backward.  Rows are summed in index order by
 * one workgroup: bit-reproducible, no host synchronisation.
 * mst_cosdist_backward: dpred [K][D] = dloss * d loss / d pred with F.normalize's clamp (a row with |p_i| <= 1e-12 gets
 * -(dloss / K) t^_i / 1e-12; an all-zero target row gets zeros); dloss: dev [1].  The target gets no gradient.              */
int mst_cosdist_forward(const float* pred, const float* target, int K, int D, float* loss, float* save, void* stream);
int mst_cosdist_backward(const float* pred, const float* target, int K, int D, const float* save, const float* dloss,
                         float* dpred, void* stream);

/* ------------------------------------------------------------------------------------------
 * InfoNCE forward on (gathered) embeddings.  Replaces InfoNCELoss.forward src/loss.py:31-136.
 * emb: dev [N][D] fp32; labels: dev [N] int64; anchors [row0,row0+rows) are the local rows.
 * out: dev [2] = { sum over valid local anchors of -log(pos/(pos+neg+1e-8)), #valid anchors }.
 * ------------------------------------------------------------------------------------------ */
size_t mst_infonce_workspace_bytes(int N, int D);
int mst_infonce_forward(const float* emb, const int64_t* labels, int N, int D, int row0, int rows,
                        float temperature, float* out, void* workspace, size_t workspace_bytes,
                        void* stream);
/* Backward of the same sum (what autograd derives for src/loss.py:110-136):
 * grad: dev [N][D], overwritten with  (*scale) * d( sum over valid local anchors of loss_i ) / d emb  for ALL N rows
 *       (rows of other ranks receive the terms where they act as columns; the caller all-reduces and slices).
 * scale: dev [1] (the upstream gradient, e.g. 1/#valid anchors) or NULL for 1.  Same workspace size as forward. */
int mst_infonce_backward(const float* emb, const int64_t* labels, int N, int D, int row0, int rows,
                         float temperature, const float* scale, float* grad, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage C loss: multi-resolution STFT loss of the style-transfer trainer, forward and the gradient to x.
 * Replaces: MultiResolutionSTFTLoss.forward src/loss.py:332-448 (torch.stft center=True / reflect, periodic Hann,
 * magnitudes, spectral convergence + mean |log(xm + 1e-5) - log(ym + 1e-5)| per resolution, mean over resolutions).
 * x, y: dev fp32 [rows][T], rows = B * C.  fft[], hop[]: host, n_res entries; fft in {512, 1024, 2048} (window length
 * = fft), hop in {fft/8, fft/4, fft/2}, T > max(fft) / 2.  windows: host array of n_res DEVICE pointers, windows[r] =
 * fp32 [fft[r]] (built by the caller on the host; never re-derived on the device).
 * out: dev fp32 [1 + 4 n_res] = { loss, (sc, log) x n_res unweighted, (||ym - xm||_F, ||ym||_F) x n_res }; the backward
 * pass takes it back as fwd_out.  Bit-reproducible (no floating-point atomics), stream-ordered, no host sync.
 * ------------------------------------------------------------------------------------------ */
size_t mst_mrstft_workspace_bytes(int n_res, const int* fft, const int* hop, int rows, int T);
int mst_mrstft_forward(const float* x, const float* y, int rows, int T, int n_res, const int* fft, const int* hop,
                       const float* const* windows, float sc_weight, float log_weight, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
/* grad_x: dev [rows][T] = grad_scale * d loss / d x (every element written).  grad_scale: dev [1] (the upstream
 * gradient) or NULL for 1.  Recomputes the frames: needs x, y and the forward's out, not its workspace contents.  */
int mst_mrstft_backward(const float* x, const float* y, int rows, int T, int n_res, const int* fft, const int* hop,
                        const float* const* windows, float sc_weight, float log_weight, const float* fwd_out,
                        const float* grad_scale, float* grad_x, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage A backward: the gradient of the log-mel front end to the waveform (what the style term of the style-transfer
 * trainer, src/train_style_transfer.py:192-224, needs from the frozen encoder's first stage).
 * For L = log(mel + 1e-10), mel[m,f] = sum_k fb[k,m] |X[k,f]|^2, X = stft(x) (center / reflect, periodic Hann,
 * one-sided, F = 1 + T / hop frames) and a cotangent g on L:  grad_x = adjoint STFT of 2 dP X,
 * dP[k,f] = sum_m fb[k,m] g[m,f] / (mel[m,f] + 1e-10), mel recomputed with the frames (nothing of the forward is kept).
 * x: dev fp32 [rows][T]; grad_logmel: dev fp32 [rows][n_mels][F] (MST_LOGMEL_REF with rows = B * 8).
 * n_fft in {1024, 2048}, hop in {n_fft/8, n_fft/4, n_fft/2}, n_mels <= 256, T > n_fft / 2.  window: dev fp32 [n_fft].
 * The filterbank enters as a per-bin band table built by the caller on the host: band dev int32 [n_fft/2 + 1][2] =
 * (first mel index, count), band_weight dev fp32 [n_fft/2 + 1][MST_LOGMEL_BAND_MAX] = fb[k][first], fb[k][first + 1];
 * band_width = the widest count of the table: more than MST_LOGMEL_BAND_MAX is refused (MST_EINVAL), never truncated.
 * mel_ranges: dev int32 [n_mels][4] = (start, count) of the run of bins whose FIRST mel is m, (start, count) of the run
 * whose SECOND mel is m -- the transposed view of `band`, for the mel sums (triangular filters: each is one run of bins;
 * the caller checks that its table has this form).
 * grad_x: dev [rows][T], every element written (accumulate = 0) or added to (accumulate != 0).
 * Bit-reproducible (fixed-order overlap-add, no floating-point atomics), stream-ordered, no host sync, no allocation.
 * ------------------------------------------------------------------------------------------ */
#define MST_LOGMEL_BAND_MAX 2
size_t mst_logmel_backward_workspace_bytes(int rows);
int mst_logmel_backward(const float* x, const float* grad_logmel, int rows, int T, int n_fft, int hop, int n_mels,
                        const float* window, const int32_t* band, const float* band_weight, int band_width,
                        const int32_t* mel_ranges, float* grad_x, int accumulate, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage A backward, second path: the gradient of the MIXING FEATURES to the waveform (the reference extracts the features
 * of the mixer's output with gradients: src/train_style_transfer.py:204-215).  Basic 64-feature layout only; of those the
 * reference differentiates 24: per stem block o in {0 bass, 15 drums, 34 other, 49 vocals} rms L/R (o, o+1), crest L/R
 * (o+2, o+3), rel_loudness (o+6), and the masking features 30..33; every other entry of grad_feats is ignored.
 * x: dev fp32 [B][8][T] packed (rows vL vR bL bR dL dR oL oR); grad_feats, feats: dev fp32 [B][64], feats = the forward's
 * values: an entry with |feats| >= 100 (clamped) or NaN passes no gradient.  grad_logmel: NULL, or dev fp32
 * [B*8][n_mels][F] -- the log-mel cotangent of the same backward, which then rides in the SAME adjoint pass
 * (w = g_L / (mel + 1e-10) + g_P).  Tables and parameter limits as mst_logmel_backward.
 * A channel with sum x^2 == 0 gets exact zeros from its own rms / crest / loudness terms (the reference: NaN).
 * grad_x: dev [B][8][T], written (accumulate = 0) or added to.  After the call the first B*8*n_mels*F floats of the
 * workspace hold the recomputed mel power [B*8][n_mels][F].
 * Bit-reproducible (fixed summation order, no floating-point atomics), a clip's result does not depend on its batch
 * neighbours; stream-ordered, no host sync, no allocation.  Returns MST_EINVAL naming the reason for anything else.
 * ------------------------------------------------------------------------------------------ */
size_t mst_melfeat_backward_workspace_bytes(int B, int T, int n_fft, int hop, int n_mels);
int mst_melfeat_backward(const float* x, const float* grad_feats, const float* feats, const float* grad_logmel, int B, int T,
                         int n_fft, int hop, int n_mels, int feature_dim, const float* window, const int32_t* band,
                         const float* band_weight, int band_width, const int32_t* mel_ranges, float* grad_x, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage C: TCN mixer (eval) -- the style-transfer stage that consumes the embeddings.
 * Replaces: TCNMixer.forward src/tcn_mixer.py:285-321 (input 1x1 conv, num_blocks residual blocks with dilation
 * 2^i, output 1x1 conv + x), ResidualBlock.forward :82-90, FiLMResidualBlock.forward :119-145, CausalConv1d :16-36,
 * NonCausalConv1d :39-57, TCNFiLMGenerator.forward :186-216, as driven by
 * inference/inference_e2e_style_transfer.py:124-177.  BatchNorm1d uses running statistics, Dropout is identity,
 * LeakyReLU slope 0.2.  Exact fp32 (fp32 MFMA).  Padding is zeros of each layer's own input.
 * Geometry: in_channels == 8, hidden_channels <= 128 (padded inside the handle to a multiple of 16 with zero
 * weights: exact), kernel_size <= 15 (odd unless causal), num_blocks <= 16.
 * ------------------------------------------------------------------------------------------ */
typedef struct mst_tcn mst_tcn;           /* mixer          */
typedef struct mst_tcn_film mst_tcn_film; /* FiLM generator */
typedef struct mst_tcn_config {
  int32_t in_channels, hidden_channels, num_blocks, kernel_size;
  int32_t causal;   /* 0: symmetric padding ((K-1)*d)/2; 1: (K-1)*d zeros on the left only                     */
  int32_t use_film; /* 0: ResidualBlock (activation after the residual sum); 1: FiLMResidualBlock (before it)  */
  float bn_eps;
} mst_tcn_config;
/* host fp32, the state_dict tensors; per-block tensors stacked over (block, layer = conv1/norm1, conv2/norm2). */
typedef struct mst_tcn_weights {
  const float *input_w, *input_b;   /* input_conv  [H][8][1], [H]                                   */
  const float *conv_w, *conv_b;     /* blocks.{i}.conv{1,2}.conv  [nb][2][H][H][K], [nb][2][H]      */
  const float *bn_w, *bn_b, *bn_mean, *bn_var; /* blocks.{i}.norm{1,2}  [nb][2][H] each             */
  const float *output_w, *output_b; /* output_conv [8][H][1], [8]                                   */
} mst_tcn_weights;
/* optional: the hidden state after chosen blocks in the reference's layout, for the tests */
typedef struct mst_tcn_taps {
  int32_t n;        /* 0..4 */
  int32_t block[4]; /* block index whose output is copied                    */
  float* h[4];      /* dev [B][H][T] each                                    */
} mst_tcn_taps;
typedef struct mst_tcn_film_weights { const float *mlp0_w, *mlp0_b, *mlp3_w, *mlp3_b, *mlp6_w, *mlp6_b; } mst_tcn_film_weights;

int mst_tcn_create(mst_tcn** out, const mst_tcn_config* cfg, const mst_tcn_weights* w);
void mst_tcn_destroy(mst_tcn* tcn);
/* 0 (and mst_last_error) when the shape is refused: H_padded * T must stay below 2^31 per clip, B <= 65535. */
size_t mst_tcn_workspace_bytes(const mst_tcn* tcn, int B, long long T);
/* x, y: dev [B][8][T] fp32 (y may not alias x).  film: dev [B][num_blocks][4][H] = gamma1, beta1, gamma2, beta2 per
 * block (what mst_tcn_film_forward writes); required iff use_film.  taps may be NULL.                            */
int mst_tcn_forward(const mst_tcn* tcn, const float* x, const float* film, int B, long long T, float* y,
                    const mst_tcn_taps* taps, void* workspace, size_t workspace_bytes, void* stream);
/* Opt-in split-precision inference of the dilated convolutions on the f16 matrix pipe (csrc/tcn_f16x3.inc).
 * MST_TCN_FP32 (default): the exact-fp32 MFMA kernels.  MST_TCN_F16X3: activations and filters as hi + lo f16 (22
 * significant bits together), three f16 MFMA products per term with fp32 accumulation (only lo * lo is dropped), an exact
 * power-of-two range scale per (convolution, clip) and per (convolution, output channel) derived on the device; same
 * parity bar as fp32, bit-reproducible, a clip's result does not depend on its batch.  mst_tcn_set_precision builds the
 * f16 weight fragments from the handle's weights on `stream` (mst_tcn_update_params rebuilds them while the mode is on)
 * and returns MST_EINVAL for an unknown mode.  mst_tcn_workspace_bytes and mst_tcn_forward follow the handle's mode (the
 * workspace grows by two f16 planes and the absmax array; H padded to 32 times T must stay below 2^31).  The training
 * entry points (mst_tcn_forward_train, mst_tcn_backward, mst_tcn_train_*) IGNORE the mode and compute in fp32.          */
enum { MST_TCN_FP32 = 0, MST_TCN_F16X3 = 1 };
int mst_tcn_set_precision(mst_tcn* tcn, int mode, void* stream);
int mst_tcn_get_precision(const mst_tcn* tcn);
/* Linear(embed_dim, 512) - LeakyReLU - Linear(512, 512) - LeakyReLU - Linear(512, num_blocks*4*hidden); embed_dim % 4 == 0. */
int mst_tcn_film_create(mst_tcn_film** out, int embed_dim, int num_blocks, int hidden, const mst_tcn_film_weights* w);
void mst_tcn_film_destroy(mst_tcn_film* gen);
size_t mst_tcn_film_workspace_bytes(const mst_tcn_film* gen, int B);
/* emb: dev [B][embed_dim] (input and target embedding concatenated); film: dev [B][num_blocks][4][hidden]. */
int mst_tcn_film_forward(const mst_tcn_film* gen, const float* emb, int B, float* film, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage C, streaming: block-wise inference of a CAUSAL mixer (csrc/tcn_stream.inc).  A push takes the next N samples of B
 * streams and returns their N output samples.  The result does not depend on how the signal was cut into blocks: with the
 * zero history a reset leaves, the pushes concatenated are the mst_tcn_forward result of the whole clip BIT FOR BIT (fp32
 * mode).  The state is caller-owned device memory: the folded BatchNorm / FiLM table and, for every dilated convolution, a
 * ring holding the last (K-1)*d samples of its input plus the block in flight (rounded up to a power of two of rows; at
 * K = 15, num_blocks = 14, max_block = 16384 about 2^19 rows of H_padded floats per stream).  No allocation, no host
 * synchronisation, everything on `stream`.  B, max_block and the handle must be those of the reset in every push.
 * Refused (MST_EINVAL, the size queries return 0; mst_last_error names the way out): a non-causal mixer (it needs look-ahead:
 * mst_tcn_forward), a handle in MST_TCN_F16X3 mode, B outside 1..65535, max_block < 1 or so large that a ring reaches
 * 2^31 elements, N outside 1..max_block, t0 < 0, film not matching use_film; MST_ENOMEM for a state or workspace smaller
 * than the size queries say.  After mst_tcn_update_params the state's folded table is stale: reset before the next push.
 * FiLM is fixed per reset.  A non-causal mixer streams with a fixed latency through mst_tcn_lookahead_* below.  Not built:
 * f16x3 streaming, gradients.
 * ------------------------------------------------------------------------------------------ */
size_t mst_tcn_stream_state_bytes(const mst_tcn* tcn, int B, int max_block);
size_t mst_tcn_stream_workspace_bytes(const mst_tcn* tcn, int B, int max_block);
/* Zeroes every ring (the stream starts from zero history, which is the offline forward's padding) and folds the table
 * from the handle's BatchNorm parameters and `film` (dev [B][num_blocks][4][H], required iff use_film).                  */
int mst_tcn_stream_reset(const mst_tcn* tcn, void* state, size_t state_bytes, int B, int max_block, const float* film,
                         void* stream);
/* t0: samples pushed since the reset (the caller counts; 64-bit).  x, y: dev [B][8][N] fp32, y may not alias x.
 * 2 * num_blocks + 2 kernel launches.                                                                                   */
int mst_tcn_stream_push(const mst_tcn* tcn, void* state, size_t state_bytes, int B, int max_block, long long t0,
                        const float* x, int N, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The consecutive samples one wave of the convolution kernel owns in a push of N samples of B streams: 16, 32, or the
 * offline kernel's 64 / 128.  Short blocks get the smaller tiles, so that they are spread over the chip's SIMDs; the result
 * does not depend on the tile.  For the tests and the probe; 0 for a NULL handle or B, N < 1.                            */
int mst_tcn_stream_samples_per_wave(const mst_tcn* tcn, int B, int N);

/* ------------------------------------------------------------------------------------------
 * Stage C, streaming with a fixed latency: block-wise inference of a NON-CAUSAL mixer (csrc/tcn_lookahead.inc).  Every
 * layer runs (K-1)*d/2 samples behind its input, so a push of N samples returns the N output samples that lie
 * latency = (K-1) * (2^num_blocks - 1) samples back: y[i] is the output at time t0 + i - latency, zeros where that time is
 * outside the clip.  The stream has an end: drain pushes (t_end >= 0) feed "after the end" until the last `latency` samples
 * are out.  The outputs of all pushes, delayed by the latency, are the mst_tcn_forward result of the whole clip BIT FOR BIT,
 * whatever the block sizes, for a clip of any length (no H_padded * T limit; the state does not depend on T).  A causal mixer is
 * accepted: latency 0, the result of mst_tcn_stream_push.  State: that of the causal stream (same rings) plus a delay ring
 * of x, [B][8][cap_x] floats with cap_x the power of two >= latency + max_block.  No allocation, no host synchronisation,
 * 2 * num_blocks + 2 launches per push.  Refusals as for the causal stream, except the one of a non-causal mixer.
 * ------------------------------------------------------------------------------------------ */
/* (K-1) * (2^num_blocks - 1) samples; 0 for a causal mixer; -1 for a NULL handle. */
long long mst_tcn_lookahead_latency(const mst_tcn* tcn);
size_t mst_tcn_lookahead_state_bytes(const mst_tcn* tcn, int B, int max_block);
/* Zeroes every ring and folds the BatchNorm / FiLM table, as mst_tcn_stream_reset. */
int mst_tcn_lookahead_reset(const mst_tcn* tcn, void* state, size_t state_bytes, int B, int max_block, const float* film,
                            void* stream);
/* t0: samples pushed since the reset, drain pushes included (the caller counts; 64-bit).  t_end < 0: the stream is open and
 * x: dev [B][8][N] holds its next N samples.  t_end >= 0: the stream's length is t_end, every sample of it has been pushed
 * (t0 >= t_end is required) and this is a drain push: x is not read and may be NULL.  y: dev [B][8][N], may not alias x.   */
int mst_tcn_lookahead_push(const mst_tcn* tcn, void* state, size_t state_bytes, int B, int max_block, long long t0,
                           long long t_end, const float* x, int N, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage C, training: the mixer in train() mode and its backward (src/train_style_transfer.py:255-317,
 * inference/test_tcn_style_transfer.py:84-200 back-propagate through it).  BatchNorm1d uses the batch statistics over
 * (B, T), biased variance; the whole batch goes through one call.  Exact fp32, fixed summation orders, no float atomics:
 * two calls on the same input give the same bits.
 * ------------------------------------------------------------------------------------------ */
/* Refreshes the handle from DEVICE tensors in the layouts of mst_tcn_weights, on `stream`, without a host copy or
 * synchronisation.  Two groups, each given whole or left NULL: the parameters (input_*, conv_*, bn_w, bn_b, output_*;
 * the first such call allocates the training copies) and the running statistics (bn_mean, bn_var; read by
 * mst_tcn_forward only).  The parameters are required once before the training calls and after every change of one.     */
int mst_tcn_update_params(mst_tcn* tcn, const mst_tcn_weights* device_weights, void* stream);
/* 0 (and mst_last_error) when the shape is refused.  The workspace serves the forward and the backward.                 */
size_t mst_tcn_train_save_bytes(const mst_tcn* tcn, int B, long long T);
size_t mst_tcn_train_workspace_bytes(const mst_tcn* tcn, int B, long long T);
/* x, y, film as mst_tcn_forward.  batch_mean, batch_var: dev [num_blocks][2][H], the statistics of norm1 / norm2 of
 * every block (biased variance; the caller updates the running statistics from them).  save: dev, caller-owned, what the
 * backward reads ((3 num_blocks + 1) * H_padded * 4 bytes per sample); NULL when no backward follows (same y).          */
int mst_tcn_forward_train(const mst_tcn* tcn, const float* x, const float* film, int B, long long T, float* y,
                          float* batch_mean, float* batch_var, void* save, size_t save_bytes, void* workspace,
                          size_t workspace_bytes, void* stream);
/* dev fp32, the reference's parameter layouts stacked as in mst_tcn_weights; every element is overwritten. */
typedef struct mst_tcn_grads {
  float *input_w, *input_b;   /* [H][8][1], [H]                 */
  float *conv_w, *conv_b;     /* [nb][2][H][H][K], [nb][2][H]   */
  float *bn_w, *bn_b;         /* [nb][2][H] each                */
  float *output_w, *output_b; /* [8][H][1], [8]                 */
} mst_tcn_grads;
/* dy: dev [B][8][T].  x, film, save: what the forward was given and wrote.  dx: dev [B][8][T] or NULL (skipped).
 * dfilm: dev [B][num_blocks][4][H] or NULL (must be NULL for a mixer without FiLM).                                     */
int mst_tcn_backward(const mst_tcn* tcn, const float* dy, const float* x, const float* film, int B, long long T,
                     const void* save, size_t save_bytes, const mst_tcn_grads* grads, float* dx, float* dfilm,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Tests: masks dev [2 num_blocks][B][H][T] bytes, 1 where the backward takes LeakyReLU slope 1 (the device function the
 * backward itself uses), in the order conv1, conv2 of block 0, 1, ...                                                   */
int mst_tcn_train_masks(const mst_tcn* tcn, const void* save, size_t save_bytes, int B, long long T, unsigned char* masks,
                        void* stream);
/* Tests: the two linear kernels of one convolution (block, layer 0 / 1) alone.  du, in, din: dev [B][H][T] in the
 * reference's layout; din = input gradient of du, dw [H][H][K] = weight gradient of du against the input `in`.          */
int mst_tcn_train_conv_grads(const mst_tcn* tcn, int block, int layer, const float* du, const float* in, int B, long long T,
                             float* din, float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage C, training: the FiLM generator (TCNFiLMGenerator src/tcn_mixer.py:148-216; the module the trainer optimises
 * next to the mixer, src/train_style_transfer.py:255-317), train-mode forward and full backward of
 *     z1 = W0 x + b0;   h1 = Dropout_p1(LeakyReLU_s(z1))
 *     z2 = W3 h1 + b3;  h2 = Dropout_p2(LeakyReLU_s(z2))
 *     film = W6 h2 + b6
 * emb: dev [B][embed_dim]; film, dfilm: dev [B][out_dim], out_dim = num_blocks * 4 * hidden_channels, i.e. the
 * [B][num_blocks][4][H] tensor mst_tcn_forward_train reads and mst_tcn_backward writes.  Weights and gradients are DEVICE
 * tensors in state_dict layout (mst_tcn_film_weights), the module's live parameters by pointer: no handle, nothing swizzled
 * or cached.  fp32 on v_mfma_f32_16x16x4_f32; every forward product is split-K with the slices added in slice order (the
 * gamma rounding finding of mst_tcn_film_forward); no float atomics, fixed summation orders: the same seeds give the same
 * bits, and a row's film does not depend on B.
 * Dropout: element m * mlp_hidden + n of h1 / h2 is kept iff mst_dropout_mask keeps it under seed1 / seed2; survivors are
 * scaled by 1 / (1 - p); p == 0 switches a Dropout off.  Masks are never stored: the backward re-derives each decision from
 * (seed, index) -- behind a LeakyReLU a saved 0 may be a kept unit whose pre-activation was exactly 0 -- and takes slope 1
 * where the saved activation is > 0, `slope` elsewhere (PyTorch's branch for x <= 0); a dropped unit gets 0.
 * Limits (refused by name): 1 <= embed_dim <= 4096 (no % 4 rule here), 1 <= mlp_hidden <= 2048, 1 <= out_dim <= 8192,
 * 1 <= B <= 65535, 0 <= p < 1, 0 <= slope <= 1.  The *_bytes functions return 0 for refused dims; a smaller buffer is
 * MST_ENOMEM.  No allocation, no host synchronisation, everything on `stream`.
 * mst_tcn_film_backward: the six parameter gradients are overwritten (not accumulated); demb [B][embed_dim] is written
 * unless NULL (its GEMM is then skipped).  emb, save and the seeds are what the forward was given and wrote.
 * ------------------------------------------------------------------------------------------ */
typedef struct mst_tcn_film_train_dims { int32_t embed_dim, mlp_hidden, out_dim; } mst_tcn_film_train_dims;
typedef struct mst_tcn_film_grads { float *mlp0_w, *mlp0_b, *mlp3_w, *mlp3_b, *mlp6_w, *mlp6_b; } mst_tcn_film_grads;
size_t mst_tcn_film_train_save_bytes(const mst_tcn_film_train_dims* dims, int B);
size_t mst_tcn_film_train_backward_workspace_bytes(const mst_tcn_film_train_dims* dims, int B);
int mst_tcn_film_forward_train(const mst_tcn_film_train_dims* dims, const mst_tcn_film_weights* w, const float* emb, int B,
                               float slope, float drop_p1, uint64_t seed1, float drop_p2, uint64_t seed2, float* film,
                               void* save, size_t save_bytes, void* stream);
int mst_tcn_film_backward(const mst_tcn_film_train_dims* dims, const mst_tcn_film_weights* w, const float* emb, int B,
                          float slope, float drop_p1, uint64_t seed1, float drop_p2, uint64_t seed2, const float* dfilm,
                          const void* save, const mst_tcn_film_grads* grads, float* demb, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The optimiser tail: gradient clipping and the parameter update of both trainers and of the per-pair fit
 * (clip_grad_norm_ + AdamW src/train_style_transfer.py:284-288, 602-605; AdamW under GradScaler src/train.py:292-296,
 * 323-326; Adam / AdamW / SGD(momentum=0.9) of the fit inference/test_tcn_style_transfer.py:130-189, grid_search_tcn.py:92-97).
 *
 * Multi-tensor form: one call handles an ordered list of fp32 tensors, described by two DEVICE tables the caller builds once
 * and keeps while a call is in flight (mst_optim_list holds their device pointers and is itself read on the host):
 *   tensors   [n_tensors] mst_optim_tensor: parameter, gradient, state and step-count pointers and the element count n >= 1;
 *   chunk_map [n_chunks][2] int32: (tensor index, chunk index inside that tensor), one row per chunk of
 *             mst_optim_chunk_elems() elements, chunk c of a tensor covering elements [c * chunk, min(n, (c + 1) * chunk)).
 *             One workgroup serves one row.  The rows of the map must cover every tensor exactly once (the library cannot
 *             check device memory; a row past its tensor's end is ignored).
 * Pointers need 4-byte alignment only (views at odd element offsets are fine): 16-byte accesses are used between a scalar
 * head and tail where a tensor's arrays allow it.  An element's result depends on its own inputs and the call's scalars only,
 * not on the list, its position or its chunk: every stored value is the double-precision evaluation of the formula on the fp32
 * inputs, rounded once.  No float atomics, no workgroup waits on another; no allocation, no host synchronisation; capturable.
 *
 * mst_optim_grad_norm: *norm = fp32(sqrt(sum g^2)) over the whole list -- squares and sums in double, one partial per chunk
 *   (workspace), the partials added in index order by a second launch -- and *coef = min(1, max_norm * (1 / (norm + 1e-6)))
 *   evaluated in fp32, the arithmetic of torch.nn.utils.clip_grad_norm_ (its scalar / tensor is reciprocal-then-multiply).
 *   A NaN norm gives a NaN coefficient; an infinite norm gives 0, as torch's does.  Reads tensors[i].grad and n only.
 * mst_optim_scale_grads: g *= *coef, one fp32 multiply per element.
 * mst_optim_step: one step of torch.optim's single-tensor formulas, per element
 *   MST_OPTIM_ADAM   g += wd p;  m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g g;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *   MST_OPTIM_ADAMW  p *= 1 - lr wd;  then as Adam without the first term
 *   MST_OPTIM_SGD    g += wd p;  buf = momentum buf + g  (a zero buffer: the first step's copy of g);  p -= lr buf
 *                    (momentum == 0: state1 may be NULL and p -= lr g)
 *   state1 = exp_avg / momentum_buffer, state2 = exp_avg_sq (Adam, AdamW), step = dev fp32 scalar per tensor (Adam, AdamW):
 *   the call first adds 1 to it, t is the new value, and the bias corrections are formed from it on the device in double.
 *   Hyper-parameters are passed by value (a host struct read during the call).  amsgrad, maximize, nesterov and
 *   dampening != 0 are refused by name.
 *   grad_scale (dev fp32 scalar or NULL): the gradient is multiplied by 1 / *grad_scale before use (the stored gradient is
 *   left as it is).  found_inf (dev fp32 scalar or NULL): when non-zero the call changes nothing -- parameters, state and
 *   step counts keep their bits (the contract of PyTorch's fused optimisers under GradScaler).
 *   Workspace (Adam, AdamW; SGD takes NULL): mst_optim_step_workspace_bytes(n_tensors).
 * mst_keep_best: the fit loop's best-so-far bookkeeping without a host read.  With dev scalars *loss and *best:
 *   history[index] = *loss (unless history is NULL); if *loss < *best (strictly: the first minimum wins, a NaN never does):
 *   every copies[k].src is copied to its dst (bytes and pointers multiples of 4, at most 8 copies, src and dst disjoint),
 *   *best = *loss and *best_index = index.  `copies` is a host array read during the call.
 * ------------------------------------------------------------------------------------------ */
typedef struct mst_optim_tensor {
  float* param;
  float* grad;
  float* state1;
  float* state2;
  float* step;
  long long n;
} mst_optim_tensor;
typedef struct mst_optim_list {
  const mst_optim_tensor* tensors; /* dev [n_tensors]   */
  const int32_t* chunk_map;        /* dev [n_chunks][2] */
  int32_t n_tensors, n_chunks;
} mst_optim_list;
#define MST_OPTIM_ADAM 0
#define MST_OPTIM_ADAMW 1
#define MST_OPTIM_SGD 2
typedef struct mst_optim_hyper {
  int32_t algo, amsgrad, maximize, nesterov;
  double lr, beta1, beta2, eps, weight_decay, momentum, dampening;
} mst_optim_hyper;
typedef struct mst_keep_copy {
  const void* src;
  void* dst;
  long long bytes;
} mst_keep_copy;
int mst_optim_chunk_elems(void);
size_t mst_optim_grad_norm_workspace_bytes(int n_chunks);
int mst_optim_grad_norm(const mst_optim_list* list, float max_norm, float* norm, float* coef, void* workspace,
                        size_t workspace_bytes, void* stream);
int mst_optim_scale_grads(const mst_optim_list* list, const float* coef, void* stream);
size_t mst_optim_step_workspace_bytes(int n_tensors);
int mst_optim_step(const mst_optim_list* list, const mst_optim_hyper* hyper, const float* grad_scale, const float* found_inf,
                   void* workspace, size_t workspace_bytes, void* stream);
int mst_keep_best(const float* loss, float* best, int32_t* best_index, float* history, int index, const mst_keep_copy* copies,
                  int n_copies, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MST_H_ */
