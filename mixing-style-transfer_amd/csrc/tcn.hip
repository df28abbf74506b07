// Stage C: TCN mixer (eval) -- the reference's second stage, src/tcn_mixer.py (TCNMixer, TCNFiLMGenerator).
//
// Hidden state layout (private): channel-minor [B][T][HP] fp32, HP = hidden channels padded to a multiple of 16 with
// zero weights (exact).  A time sample's HP channels are contiguous, so every operand fetch of the convolution is a
// 16-byte aligned float4 whatever the dilation, and a tap's strip is addressed by the time index alone.
//
// Dilated convolution = implicit GEMM on __builtin_amdgcn_mfma_f32_16x16x4f32 (exact fp32):
//   D[out channel][time] += W[out channel][(tap, in channel)] * X[(tap, in channel)][time]
// One wave owns TT*16 consecutive time samples and all HP output channels (half of them above 64 channels), so an
// activation is fetched by one wave (two above 64 channels: no LDS staging would be reused) and the weights, pre-swizzled into A-fragment order at handle creation, are
// streamed through L1/L2 as one float4 per lane and 16x16 tile.  The MFMA's K index is free to permute as long as A and
// B agree: lane group g = lane/16 supplies input channels 16*chunk + 4*g + s for the four k-steps s of a chunk from one
// float4.  Samples outside [0, T) are zeros of the layer's own input (clamped address + select), and a tap whose strip
// lies wholly outside the clip for the wave's tile is skipped (it contributes exact zeros).
// Epilogue in the accumulators: S*acc + C (conv bias, BatchNorm(eval) and FiLM folded per clip/block/layer/channel by
// tcn_fold_kernel), LeakyReLU(0.2), residual in the order of the block type.  The accumulator holds four consecutive
// output channels of one time sample, so residual read and result store are float4 as well.
#include "common.h"

namespace mst {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxHidden = 128, kMaxTaps = 15, kMaxBlocks = 16, kFilmHidden = 512;
constexpr float kSlope = 0.2f;

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : kSlope * v; }

enum { EPI_ACT = 0, EPI_ACT_THEN_RES = 1, EPI_RES_THEN_ACT = 2 };

// One tap of a wave's tile: acc += W_tap * X[ts .. ts + TT*16).  EDGE: the strip crosses a clip boundary -- a lane's sample
// index is clamped for the address and its value replaced by zero outside [0, T) (zeros of the layer's own input; no
// out-of-range address is formed).  Interior strips (all but a few per launch) take the path without clamps and selects.
// Sample indices and element offsets are 32-bit: HP * T < 2^31 is checked by the caller and |tap offset| < 2^19.
// Accumulation is two-level: the products of ONE tap go into `part` (a chain of HP terms), and `part` is added to `acc`
// once per tap.  One sequential fp32 chain over all K * HP terms (1920 at H = 128) rounds every step at the magnitude of
// the running total and measured 3x the reference's own distance from float64; the two-level sum has 15 such roundings.
// RING (streaming, tcn_stream.inc): `inb` is a ring of T + 1 rows, T + 1 a power of two, and sample t lives in row t & T.
// Only the row address differs: every row of a ring is readable and history before the stream's start is stored zeros.
template <int NT, int TT, int NO, bool EDGE, bool ODD, bool RING = false>
__device__ __forceinline__ void tcn_conv_tap(f32x4 (&acc)[NO][TT], const float* __restrict__ inb, const float* __restrict__ wt,
                                             int ts, int T, int j, int g, int o0) {
  constexpr int HP = NT * 16;
  const float* xrow[TT];
  bool ok[TT];
#pragma unroll
  for (int m = 0; m < TT; ++m) {
    const int t = ts + m * 16 + j;
    ok[m] = !EDGE || (t >= 0 && t < T);
    const int tc = RING ? (t & T) : !EDGE ? t : (t < 0 ? 0 : (t >= T ? T - 1 : t));
    xrow[m] = inb + (tc * HP + 4 * g);
  }
  f32x4 part[NO][TT];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int m = 0; m < TT; ++m) part[o][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ch = 0; ch < NT; ++ch) {
    f32x4 xv[TT], wv[NO];
#pragma unroll
    for (int m = 0; m < TT; ++m) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xrow[m] + ch * 16);
      xv[m] = ok[m] ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int ot = !ODD || o0 + o < NT ? o0 + o : NT - 1;   // NT odd: the last tile of the second half does not exist
      wv[o] = *reinterpret_cast<const f32x4*>(wt + (ch * NT + ot) * 256);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int o = 0; o < NO; ++o)
        if (!ODD || o0 + o < NT) {
#pragma unroll
          for (int m = 0; m < TT; ++m)
            part[o][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[o][s], xv[m][s], part[o][m], 0, 0, 0);
        }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int m = 0; m < TT; ++m) acc[o][m] += part[o][m];
}

// The folded epilogue of one output element: S * acc + C, LeakyReLU, residual in the order of
// the block type.  One spelling for the offline and the streaming kernel, whose results must agree bit for bit.
__device__ __forceinline__ float tcn_conv_epilogue(float acc, float S, float Cc, float r, int epi) {
  float z = fmaf(S, acc, Cc);
  if (epi == EPI_RES_THEN_ACT) z += r;
  z = leaky(z);
  if (epi == EPI_ACT_THEN_RES) z += r;
  return z;
}

// in/out/res: one buffer of [B][T][HP].  wsw: [K][NT chunk][NT out tile][64 lanes][4] of this convolution.
// sc: [B] x sc_stride floats, S at +0 and C at +HP for this (block, layer).  off0: offset of tap 0 (= -padding).
// NT = HP / 16 tiles of input / output channels, TT time tiles per wave.  SPLIT = 2 (wide mixers): the four waves of a
// workgroup are 2 time groups x 2 halves of the output channels, so that the accumulators of a wave fit twice.
// RAW (training): no fold, no activation -- out = acc + C (+ res when res != NULL); S and epi are not read.
template <int NT, int TT, int SPLIT, bool RAW = false>
__global__ __launch_bounds__(256, 2) void tcn_conv_kernel(const float* __restrict__ in, const float* __restrict__ wsw,
                                                          const float* __restrict__ sc, long long sc_stride, const float* res,
                                                          float* out, int T, int K, int dil, int off0, int epi) {
  constexpr int HP = NT * 16, NO = (NT + SPLIT - 1) / SPLIT;
  constexpr bool ODD = NT % SPLIT != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int o0 = (wave % SPLIT) * NO;
  const long long b = blockIdx.y;
  const long long t0l = ((long long)blockIdx.x * (4 / SPLIT) + wave / SPLIT) * (TT * 16);
  if (t0l >= T) return;
  const int t0 = (int)t0l;
  const float* inb = in + b * T * HP;

  f32x4 acc[NO][TT];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int m = 0; m < TT; ++m) acc[o][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tap = 0; tap < K; ++tap) {
    const int ts = t0 + off0 + tap * dil;
    if (ts >= T || ts + TT * 16 <= 0) continue;   // the whole strip is padding: exact zeros
    const float* wt = wsw + tap * HP * HP + lane * 4;
    if (NT <= 2 && ts >= 0 && ts + TT * 16 <= T)   // measured: the second code path pays at H <= 32 only (-8 %), costs 1-3 % above
      tcn_conv_tap<NT, TT, NO, false, ODD>(acc, inb, wt, ts, T, j, g, o0);
    else
      tcn_conv_tap<NT, TT, NO, true, ODD>(acc, inb, wt, ts, T, j, g, o0);
  }

  const float* scb = sc + b * sc_stride;
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    if (o0 + o >= NT) continue;
    const int c = (o0 + o) * 16 + 4 * g;
    const f32x4 S = *reinterpret_cast<const f32x4*>(scb + c), Cc = *reinterpret_cast<const f32x4*>(scb + HP + c);
#pragma unroll
    for (int m = 0; m < TT; ++m) {
      const int t = t0 + m * 16 + j;
      if (t >= T) continue;
      const size_t at = ((size_t)b * T + t) * HP + c;
      f32x4 v = acc[o][m], r = f32x4{0.f, 0.f, 0.f, 0.f};
      if (RAW ? res != nullptr : epi != EPI_ACT) r = *reinterpret_cast<const f32x4*>(res + at);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = RAW ? (v[q] + Cc[q]) + r[q] : tcn_conv_epilogue(v[q], S[q], Cc[q], r[q], epi);
      *reinterpret_cast<f32x4*>(out + at) = v;
    }
  }
}

// S, C of every (clip, block, layer, channel): z = conv + bias; BN(eval) = (z - mean) * w / sqrt(var + eps) + b;
// FiLM = gamma * BN + beta.  Folded in double, rounded once.  Padded channels get S = C = 0 (they stay exactly zero).
// sc: [B][nb][2][2][HP];  per-layer parameters: [nb][2][H];  film: [B][nb][4][H] or NULL.
__global__ void tcn_fold_kernel(const float* __restrict__ cb, const float* __restrict__ bw, const float* __restrict__ bb,
                                const float* __restrict__ bm, const float* __restrict__ bv, const float* __restrict__ film,
                                float* __restrict__ sc, int B, int nb, int H, int HP, float eps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * nb * 2 * HP) return;
  const int c = (int)(i % HP), l = (int)(i / HP % 2), k = (int)(i / (2 * HP) % nb), b = (int)(i / ((long long)2 * HP * nb));
  double S = 0.0, Cc = 0.0;
  if (c < H) {
    const int p = (k * 2 + l) * H + c;
    const double inv = (double)bw[p] / sqrt((double)bv[p] + (double)eps);
    S = inv;
    Cc = ((double)cb[p] - (double)bm[p]) * inv + (double)bb[p];
    if (film) {
      const float* f = film + (((size_t)b * nb + k) * 4 + 2 * l) * H + c;
      S *= (double)f[0];
      Cc = (double)f[0] * Cc + (double)f[H];
    }
  }
  float* o = sc + (((size_t)b * nb + k) * 2 + l) * 2 * HP;
  o[c] = (float)S;
  o[HP + c] = (float)Cc;
}

// h[b][t][:] = W_in x[b][:][t] + b_in.  wi: [HP][8], bi: [HP] (zero rows for padded channels).
__global__ __launch_bounds__(256) void tcn_input_kernel(const float* __restrict__ x, const float* __restrict__ wi,
                                                        const float* __restrict__ bi, float* __restrict__ h, long long T,
                                                        int HP) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  float xv[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) xv[c] = x[(b * 8 + c) * T + t];
  float* ho = h + (b * T + t) * HP;
  for (int o = 0; o < HP; o += 4) {
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) a = fmaf(wi[(o + q) * 8 + c], xv[c], a);
      v[q] = a + bi[o + q];
    }
    *reinterpret_cast<f32x4*>(ho + o) = v;
  }
}

// y[b][c][t] = (W_out h[b][t][:] + b_out)[c] + x[b][c][t].  wo: [HP][8] (transposed, zero rows for padded channels).
__global__ __launch_bounds__(256) void tcn_output_kernel(const float* __restrict__ h, const float* __restrict__ wo,
                                                         const float* __restrict__ bo, const float* __restrict__ x,
                                                         float* __restrict__ y, long long T, int HP) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const float* hi = h + (b * T + t) * HP;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < HP; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(hi + k);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int c = 0; c < 8; ++c) a[c] = fmaf(wo[(k + q) * 8 + c], v[q], a[c]);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const size_t at = (b * 8 + c) * T + t;
    y[at] = (a[c] + bo[c]) + x[at];
  }
}

// hidden state in the reference's layout for the tests: out[b][c][t] = h[b][t][c], c < H.
__global__ __launch_bounds__(256) void tcn_tap_kernel(const float* __restrict__ h, float* __restrict__ out, long long T,
                                                      int H, int HP) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const float* hi = h + (b * T + t) * HP;
  for (int c = 0; c < H; ++c) out[(b * H + c) * T + t] = hi[c];
}

// out[b][n] = act(sum_k in[b][k] * w[n][k] + bias[n]): one workgroup per 16 x 16 tile of (clip, n), fp32 MFMA, Kd % 4 == 0.
// Split-K: each of the 4 waves takes every fourth 16-wide slice of K into two alternating accumulators, and the 8 partial
// sums are added in a fixed order -- short accumulation chains (the rounding error of one sequential fp32 chain over
// 1536 terms is several times that of a blocked sum), deterministic, and the whole K loop overlaps.
__global__ __launch_bounds__(256) void tcn_linear_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, int B,
                                                         int Kd, int N, int act) {
  __shared__ f32x4 part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int n = blockIdx.x * 16 + j, bi = blockIdx.y * 16 + j;
  const bool nok = n < N, bok = bi < B;
  const float* wr = w + (size_t)(nok ? n : 0) * Kd;
  const float* ar = in + (size_t)(bok ? bi : 0) * Kd;
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  int it = 0;
  for (int k0 = wave * 16; k0 < Kd; k0 += 64, it ^= 1) {
    const int k = k0 + 4 * g;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
    if (k < Kd) {
      if (bok) a = *reinterpret_cast<const f32x4*>(ar + k);
      if (nok) bv = *reinterpret_cast<const f32x4*>(wr + k);
    }
    f32x4 c = it ? acc[1] : acc[0];
#pragma unroll
    for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bv[s], c, 0, 0, 0);
    if (it) acc[1] = c; else acc[0] = c;
  }
  part[wave][lane] = acc[0] + acc[1];
  __syncthreads();
  if (wave != 0 || !nok) return;
  const f32x4 sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  const float bn = bias[n];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = blockIdx.y * 16 + 4 * g + r;
    if (row >= B) continue;
    float v = sum[r] + bn;
    if (act) v = leaky(v);
    out[(size_t)row * N + n] = v;
  }
}

template <int NT, int TT, int SPLIT, bool RAW = false>
void launch_conv(const float* in, const float* wsw, const float* sc, long long sc_stride, const float* res, float* out, int B,
                 int T, int K, int dil, int off0, int epi, hipStream_t st) {
  const long long per_block = (4LL / SPLIT) * TT * 16;
  dim3 grid((unsigned)((T + per_block - 1) / per_block), (unsigned)B);
  hipLaunchKernelGGL((tcn_conv_kernel<NT, TT, SPLIT, RAW>), grid, dim3(256), 0, st, in, wsw, sc, sc_stride, res, out, T, K, dil, off0,
                     epi);
}

typedef void (*conv_fn)(const float*, const float*, const float*, long long, const float*, float*, int, int, int, int, int,
                        int, hipStream_t);
conv_fn conv_for(int nt) {
  switch (nt) {
    case 1: return launch_conv<1, 8, 1>;
    case 2: return launch_conv<2, 8, 1>;
    case 3: return launch_conv<3, 4, 1>;
    case 4: return launch_conv<4, 4, 1>;
    case 5: return launch_conv<5, 4, 2>;
    case 6: return launch_conv<6, 4, 2>;
    case 7: return launch_conv<7, 4, 2>;
    case 8: return launch_conv<8, 4, 2>;
  }
  return nullptr;
}
conv_fn conv_raw_for(int nt) {
  switch (nt) {
    case 1: return launch_conv<1, 8, 1, true>;
    case 2: return launch_conv<2, 8, 1, true>;
    case 3: return launch_conv<3, 4, 1, true>;
    case 4: return launch_conv<4, 4, 1, true>;
    case 5: return launch_conv<5, 4, 2, true>;
    case 6: return launch_conv<6, 4, 2, true>;
    case 7: return launch_conv<7, 4, 2, true>;
    case 8: return launch_conv<8, 4, 2, true>;
  }
  return nullptr;
}

}  // namespace
}  // namespace mst

struct mst_tcn {
  mst_tcn_config cfg;
  int HP;
  float *wsw, *wi, *bi, *wo, *bo, *cb, *bw, *bb, *bm, *bv;
  // training only, allocated by the first mst_tcn_update_params: the transposed, tap-reversed weights of the input
  // gradient in A-fragment order, and [2 nb + 1][2][HP] = (1, conv bias) per convolution, then one entry of zeros
  float *wswT, *rawsc;
  // f16x3 mode only (tcn_f16x3.inc), allocated by the first mst_tcn_set_precision(MST_TCN_F16X3): hi / lo f16 weight
  // fragments and the power-of-two exponent of every (convolution, output channel); mode: MST_TCN_FP32 / MST_TCN_F16X3
  void* wf;
  int* wexp;
  int mode;
};

namespace mst {   // tcn_f16x3.inc
size_t tcn_f16x3_extra_bytes(const mst_tcn* h, int B, long long T);
int tcn_f16x3_shape_ok(const mst_tcn* h, long long T, const char* who);
int tcn_f16x3_build(mst_tcn* h, hipStream_t st);
int tcn_forward_f16x3(const mst_tcn* h, const float* x, const float* film, int B, long long T, float* y, const mst_tcn_taps* taps,
                      void* ws, hipStream_t st);
}  // namespace mst

struct mst_tcn_film {
  int E, nb, H;
  float *w0, *b0, *w3, *b3, *w6, *b6;
};

using namespace mst;

extern "C" {

void mst_tcn_destroy(mst_tcn* h) {
  if (!h) return;
  float* p[] = {h->wsw, h->wi, h->bi, h->wo, h->bo, h->cb, h->bw, h->bb, h->bm, h->bv, h->wswT, h->rawsc};
  for (float* q : p)
    if (q) (void)hipFree(q);
  if (h->wf) (void)hipFree(h->wf);
  if (h->wexp) (void)hipFree(h->wexp);
  delete h;
}

int mst_tcn_create(mst_tcn** out, const mst_tcn_config* cfg, const mst_tcn_weights* w) {
  MST_REQUIRE(out && cfg && w, "mst_tcn_create: NULL argument");
  *out = nullptr;
  MST_REQUIRE(cfg->in_channels == 8, "mst_tcn_create: in_channels must be 8 (4 stems x stereo), got %d", cfg->in_channels);
  MST_REQUIRE(cfg->hidden_channels >= 1 && cfg->hidden_channels <= kMaxHidden, "mst_tcn_create: hidden_channels must be in 1..%d, got %d",
              kMaxHidden, cfg->hidden_channels);
  MST_REQUIRE(cfg->kernel_size >= 1 && cfg->kernel_size <= kMaxTaps, "mst_tcn_create: kernel_size must be in 1..%d, got %d", kMaxTaps,
              cfg->kernel_size);
  MST_REQUIRE(cfg->num_blocks >= 1 && cfg->num_blocks <= kMaxBlocks, "mst_tcn_create: num_blocks must be in 1..%d, got %d", kMaxBlocks,
              cfg->num_blocks);
  MST_REQUIRE(cfg->causal || (cfg->kernel_size & 1), "mst_tcn_create: a non-causal TCN needs an odd kernel_size (symmetric padding of an "
              "even kernel changes the length), got %d", cfg->kernel_size);
  MST_REQUIRE(cfg->bn_eps > 0.f, "mst_tcn_create: bn_eps must be positive");
  const float* req[] = {w->input_w, w->input_b, w->conv_w, w->conv_b, w->bn_w, w->bn_b, w->bn_mean, w->bn_var, w->output_w, w->output_b};
  for (const float* q : req) MST_REQUIRE(q, "mst_tcn_create: NULL weight pointer");

  const int H = cfg->hidden_channels, K = cfg->kernel_size, nb = cfg->num_blocks, HP = (H + 15) / 16 * 16, NT = HP / 16;
  mst_tcn* h = new mst_tcn();
  h->cfg = *cfg;
  h->HP = HP;
  // weights in A-fragment order: [conv = 2*blk + layer][tap][chunk][out tile][lane][s]
  const size_t per_conv = (size_t)K * HP * HP;
  float* sw = (float*)calloc(per_conv * 2 * nb, sizeof(float));
  float* pin = (float*)calloc((size_t)HP * 8 + HP + (size_t)HP * 8, sizeof(float));
  if (!sw || !pin) {
    free(sw), free(pin), delete h;
    return fail(MST_ENOMEM, "mst_tcn_create: host allocation failed");
  }
  for (int cv = 0; cv < 2 * nb; ++cv)
    for (int tap = 0; tap < K; ++tap)
      for (int ch = 0; ch < NT; ++ch)
        for (int o = 0; o < NT; ++o)
          for (int lane = 0; lane < 64; ++lane)
            for (int s = 0; s < 4; ++s) {
              const int co = o * 16 + (lane & 15), ci = ch * 16 + 4 * (lane >> 4) + s;
              if (co < H && ci < H)
                sw[cv * per_conv + ((((size_t)tap * NT + ch) * NT + o) * 64 + lane) * 4 + s] =
                    w->conv_w[(((size_t)cv * H + co) * H + ci) * K + tap];
            }
  float *wi = pin, *bi = pin + HP * 8, *wo = bi + HP;
  for (int c = 0; c < H; ++c) {
    for (int q = 0; q < 8; ++q) wi[c * 8 + q] = w->input_w[c * 8 + q], wo[c * 8 + q] = w->output_w[q * H + c];
    bi[c] = w->input_b[c];
  }
  const size_t nl = (size_t)nb * 2 * H;
  int rc = upload(&h->wsw, sw, per_conv * 2 * nb);
  if (rc == MST_OK) rc = upload(&h->wi, wi, (size_t)HP * 8);
  if (rc == MST_OK) rc = upload(&h->bi, bi, (size_t)HP);
  if (rc == MST_OK) rc = upload(&h->wo, wo, (size_t)HP * 8);
  if (rc == MST_OK) rc = upload(&h->bo, w->output_b, (size_t)8);
  if (rc == MST_OK) rc = upload(&h->cb, w->conv_b, nl);
  if (rc == MST_OK) rc = upload(&h->bw, w->bn_w, nl);
  if (rc == MST_OK) rc = upload(&h->bb, w->bn_b, nl);
  if (rc == MST_OK) rc = upload(&h->bm, w->bn_mean, nl);
  if (rc == MST_OK) rc = upload(&h->bv, w->bn_var, nl);
  free(sw), free(pin);
  if (rc != MST_OK) {
    mst_tcn_destroy(h);
    return rc;
  }
  *out = h;
  return MST_OK;
}

static int tcn_shape_ok(const mst_tcn* h, int B, long long T, const char* who) {
  MST_REQUIRE(h, "%s: NULL handle", who);
  MST_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in 1..65535, got %d", who, B);
  MST_REQUIRE(T >= 1, "%s: T must be positive, got %lld", who, T);
  MST_REQUIRE((long long)h->HP * T < (1LL << 31), "%s: H_padded * T must stay below 2^31 per clip (H_padded = %d, T = %lld): "
              "split the clip in time", who, h->HP, T);
  return MST_OK;
}

static size_t tcn_sc_floats(const mst_tcn* h, int B) { return (size_t)B * h->cfg.num_blocks * 4 * h->HP; }

size_t mst_tcn_workspace_bytes(const mst_tcn* h, int B, long long T) {
  if (tcn_shape_ok(h, B, T, "mst_tcn_workspace_bytes") != MST_OK) return 0;
  if (h->mode == MST_TCN_F16X3 && tcn_f16x3_shape_ok(h, T, "mst_tcn_workspace_bytes") != MST_OK) return 0;
  return 2 * align_up((size_t)B * T * h->HP * sizeof(float), 256) + align_up(tcn_sc_floats(h, B) * sizeof(float), 256) +
         (h->mode == MST_TCN_F16X3 ? tcn_f16x3_extra_bytes(h, B, T) : 0);
}

int mst_tcn_forward(const mst_tcn* h, const float* x, const float* film, int B, long long T, float* y, const mst_tcn_taps* taps,
                    void* ws, size_t ws_bytes, void* stream) {
  int rc = tcn_shape_ok(h, B, T, "mst_tcn_forward");
  if (rc == MST_OK && h->mode == MST_TCN_F16X3) rc = tcn_f16x3_shape_ok(h, T, "mst_tcn_forward");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(x && y && ws, "mst_tcn_forward: NULL pointer");
  MST_REQUIRE(!h->cfg.use_film == !film, "mst_tcn_forward: film parameters are %s for this mixer (use_film = %d)",
              h->cfg.use_film ? "required" : "not accepted", h->cfg.use_film);
  const size_t need = mst_tcn_workspace_bytes(h, B, T);
  if (ws_bytes < need) return fail(MST_ENOMEM, "mst_tcn_forward: workspace %zu B < required %zu B", ws_bytes, need);
  if (taps) {
    MST_REQUIRE(taps->n >= 0 && taps->n <= 4, "mst_tcn_forward: at most 4 taps, got %d", taps->n);
    for (int i = 0; i < taps->n; ++i)
      MST_REQUIRE(taps->block[i] >= 0 && taps->block[i] < h->cfg.num_blocks && taps->h[i], "mst_tcn_forward: tap %d names block %d / NULL", i,
                  taps->block[i]);
  }
  hipStream_t st = (hipStream_t)stream;
  if (h->mode == MST_TCN_F16X3) return tcn_forward_f16x3(h, x, film, B, T, y, taps, ws, st);
  const int H = h->cfg.hidden_channels, HP = h->HP, K = h->cfg.kernel_size, nb = h->cfg.num_blocks;
  const size_t hb = align_up((size_t)B * T * HP * sizeof(float), 256);
  float* hbuf = (float*)ws;
  float* gbuf = (float*)((char*)ws + hb);
  float* sc = (float*)((char*)ws + 2 * hb);

  const long long nsc = (long long)B * nb * 2 * HP;
  hipLaunchKernelGGL(tcn_fold_kernel, dim3((unsigned)((nsc + 255) / 256)), dim3(256), 0, st, h->cb, h->bw, h->bb, h->bm, h->bv, film, sc,
                     B, nb, H, HP, h->cfg.bn_eps);
  dim3 tgrid((unsigned)((T + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(tcn_input_kernel, tgrid, dim3(256), 0, st, x, h->wi, h->bi, hbuf, T, HP);
  conv_fn conv = conv_for(HP / 16);
  const size_t per_conv = (size_t)K * HP * HP;
  const long long sc_stride = (long long)nb * 4 * HP;
  for (int k = 0; k < nb; ++k) {
    const int dil = 1 << k;   // <= 2^15, |off0| <= 14 * 2^15 < 2^19
    const int off0 = h->cfg.causal ? -(K - 1) * dil : -(((K - 1) * dil) / 2);
    conv(hbuf, h->wsw + (size_t)(2 * k) * per_conv, sc + (size_t)(2 * k) * 2 * HP, sc_stride, nullptr, gbuf, B, (int)T, K, dil, off0,
         EPI_ACT, st);
    conv(gbuf, h->wsw + (size_t)(2 * k + 1) * per_conv, sc + (size_t)(2 * k + 1) * 2 * HP, sc_stride, hbuf, hbuf, B, (int)T, K, dil, off0,
         h->cfg.use_film ? EPI_ACT_THEN_RES : EPI_RES_THEN_ACT, st);
    if (taps)
      for (int i = 0; i < taps->n; ++i)
        if (taps->block[i] == k) hipLaunchKernelGGL(tcn_tap_kernel, tgrid, dim3(256), 0, st, hbuf, taps->h[i], T, H, HP);
  }
  hipLaunchKernelGGL(tcn_output_kernel, tgrid, dim3(256), 0, st, hbuf, h->wo, h->bo, x, y, T, HP);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

void mst_tcn_film_destroy(mst_tcn_film* f) {
  if (!f) return;
  float* p[] = {f->w0, f->b0, f->w3, f->b3, f->w6, f->b6};
  for (float* q : p)
    if (q) (void)hipFree(q);
  delete f;
}

int mst_tcn_film_create(mst_tcn_film** out, int embed_dim, int num_blocks, int hidden, const mst_tcn_film_weights* w) {
  MST_REQUIRE(out && w, "mst_tcn_film_create: NULL argument");
  *out = nullptr;
  MST_REQUIRE(embed_dim >= 4 && embed_dim % 4 == 0, "mst_tcn_film_create: embed_dim must be a positive multiple of 4, got %d", embed_dim);
  MST_REQUIRE(num_blocks >= 1 && num_blocks <= kMaxBlocks, "mst_tcn_film_create: num_blocks must be in 1..%d, got %d", kMaxBlocks, num_blocks);
  MST_REQUIRE(hidden >= 1 && hidden <= kMaxHidden, "mst_tcn_film_create: hidden must be in 1..%d, got %d", kMaxHidden, hidden);
  MST_REQUIRE(w->mlp0_w && w->mlp0_b && w->mlp3_w && w->mlp3_b && w->mlp6_w && w->mlp6_b, "mst_tcn_film_create: NULL weight pointer");
  mst_tcn_film* f = new mst_tcn_film();
  f->E = embed_dim, f->nb = num_blocks, f->H = hidden;
  const size_t N = (size_t)num_blocks * 4 * hidden;
  int rc = upload(&f->w0, w->mlp0_w, (size_t)kFilmHidden * embed_dim);
  if (rc == MST_OK) rc = upload(&f->b0, w->mlp0_b, (size_t)kFilmHidden);
  if (rc == MST_OK) rc = upload(&f->w3, w->mlp3_w, (size_t)kFilmHidden * kFilmHidden);
  if (rc == MST_OK) rc = upload(&f->b3, w->mlp3_b, (size_t)kFilmHidden);
  if (rc == MST_OK) rc = upload(&f->w6, w->mlp6_w, N * kFilmHidden);
  if (rc == MST_OK) rc = upload(&f->b6, w->mlp6_b, N);
  if (rc != MST_OK) {
    mst_tcn_film_destroy(f);
    return rc;
  }
  *out = f;
  return MST_OK;
}

size_t mst_tcn_film_workspace_bytes(const mst_tcn_film* f, int B) {
  if (!f || B < 1) return 0;
  return 2 * align_up((size_t)B * kFilmHidden * sizeof(float), 256);
}

int mst_tcn_film_forward(const mst_tcn_film* f, const float* emb, int B, float* film, void* ws, size_t ws_bytes, void* stream) {
  MST_REQUIRE(f && emb && film && ws, "mst_tcn_film_forward: NULL pointer");
  MST_REQUIRE(B >= 1 && B <= 65535 * 16, "mst_tcn_film_forward: B out of range: %d", B);
  const size_t need = mst_tcn_film_workspace_bytes(f, B);
  if (ws_bytes < need) return fail(MST_ENOMEM, "mst_tcn_film_forward: workspace %zu B < required %zu B", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  float* a = (float*)ws;
  float* b = (float*)((char*)ws + need / 2);
  const int N = f->nb * 4 * f->H;
  const unsigned by = (unsigned)((B + 15) / 16);
  hipLaunchKernelGGL(tcn_linear_kernel, dim3(kFilmHidden / 16, by), dim3(256), 0, st, emb, f->w0, f->b0, a, B, f->E, kFilmHidden, 1);
  hipLaunchKernelGGL(tcn_linear_kernel, dim3(kFilmHidden / 16, by), dim3(256), 0, st, a, f->w3, f->b3, b, B, kFilmHidden, kFilmHidden, 1);
  hipLaunchKernelGGL(tcn_linear_kernel, dim3((unsigned)((N + 15) / 16), by), dim3(256), 0, st, b, f->w6, f->b6, film, B, kFilmHidden, N, 0);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"

#include "tcn_f16x3.inc"
#include "tcn_train.inc"
#include "tcn_stream.inc"
#include "tcn_lookahead.inc"
