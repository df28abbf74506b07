// Stage C, streaming: block-wise inference of a CAUSAL mixer (included by tcn.hip).  DESIGN 3.15.
//
// A push takes the next N samples of B streams and returns their N output samples; the result does not depend on how the
// signal was cut into blocks, and with zero history it is the offline mst_tcn_forward result bit for bit: every output
// element is the same chain (per-tap partial sums in channel order, acc += part once per tap, the folded epilogue) on the
// same operands, whichever lane or tile computes it, and history before the stream's start is stored zeros where the
// offline kernel selects zeros or skips an all-padding tap (part = +0 and acc is never -0, so acc += part is the identity).
//
// State (device, caller-owned): the folded S, C table [B][nb][2][2][HP] of tcn_fold_kernel, then one RING per layer input.
// Ring 2k is h_k (input of block k's conv1 and residual of its conv2), ring 2k + 1 is g_k (input of its conv2), ring 2 nb is
// the last block's output, read by the output convolution.  A ring is [B][cap][HP] fp32 with cap the power of two
// >= (K - 1) * 2^k + max_block (max_block for the last): sample t lives in row t & (cap - 1).  The ring is the only home of
// its tensor: the producer's epilogue stores straight into it, the consumer reads history and current rows from it.  A push
// writes rows [t0, t0 + N) and reads rows [t0 - (K - 1) d, t0 + N); cap >= (K - 1) d + N keeps the two apart modulo cap, so
// there is no copy, append or ping-pong.  Ring offsets come from the host's t0: no device counter, no synchronisation.

namespace mst {
namespace {

// tcn_conv_kernel on rings.  in / res: the ring of this convolution's input / of its block's input (same cap, mask imask);
// out: the consumer's ring (mask omask).  tin = t0 & imask, tout = t0 & omask.  Rows >= N of the last tile are computed from
// whatever their ring rows hold (finite or not, they are never stored).
template <int NT, int TT, int SPLIT>
__global__ __launch_bounds__(256, 2) void tcn_conv_stream_kernel(const float* __restrict__ in, const float* __restrict__ wsw,
                                                                 const float* __restrict__ sc, long long sc_stride,
                                                                 const float* __restrict__ res, float* __restrict__ out, int N, int K,
                                                                 int dil, int off0, int epi, int tin, int imask, int tout, int omask) {
  constexpr int HP = NT * 16, NO = (NT + SPLIT - 1) / SPLIT;
  constexpr bool ODD = NT % SPLIT != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int o0 = (wave % SPLIT) * NO;
  const size_t b = blockIdx.y;
  const int tl = (blockIdx.x * (4 / SPLIT) + wave / SPLIT) * (TT * 16);   // first sample of the wave's tile within the block
  if (tl >= N) return;
  const float* inb = in + b * ((size_t)imask + 1) * HP;

  f32x4 acc[NO][TT];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int m = 0; m < TT; ++m) acc[o][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tap = 0; tap < K; ++tap)
    tcn_conv_tap<NT, TT, NO, false, ODD, true>(acc, inb, wsw + tap * HP * HP + lane * 4, tin + tl + off0 + tap * dil, imask, j, g, o0);

  const float* scb = sc + b * sc_stride;
  const float* resb = res + b * ((size_t)imask + 1) * HP;
  float* outb = out + b * ((size_t)omask + 1) * HP;
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    if (o0 + o >= NT) continue;
    const int c = (o0 + o) * 16 + 4 * g;
    const f32x4 S = *reinterpret_cast<const f32x4*>(scb + c), Cc = *reinterpret_cast<const f32x4*>(scb + HP + c);
#pragma unroll
    for (int m = 0; m < TT; ++m) {
      const int t = tl + m * 16 + j;
      if (t >= N) continue;
      f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
      if (epi != EPI_ACT) r = *reinterpret_cast<const f32x4*>(resb + (((tin + t) & imask) * HP + c));
      f32x4 v = acc[o][m];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = tcn_conv_epilogue(v[q], S[q], Cc[q], r[q], epi);
      *reinterpret_cast<f32x4*>(outb + (((tout + t) & omask) * HP + c)) = v;
    }
  }
}

// tcn_input_kernel into ring 0, the same fmaf chain per element.  x: [B][8][N].  (The two 1x1 kernels are restated, not
// shared: moving their bodies into helpers changed the offline kernels' register allocation.)
__global__ __launch_bounds__(256) void tcn_input_stream_kernel(const float* __restrict__ x, const float* __restrict__ wi,
                                                               const float* __restrict__ bi, float* __restrict__ h, int N, int HP,
                                                               int tout, int omask) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t b = blockIdx.y;
  if (t >= N) return;
  float xv[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) xv[c] = x[(b * 8 + c) * N + t];
  float* ho = h + (b * ((size_t)omask + 1) + ((tout + t) & omask)) * HP;
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

// tcn_output_kernel from the last ring.  x, y: [B][8][N].
__global__ __launch_bounds__(256) void tcn_output_stream_kernel(const float* __restrict__ h, const float* __restrict__ wo,
                                                                const float* __restrict__ bo, const float* __restrict__ x,
                                                                float* __restrict__ y, int N, int HP, int tin, int imask) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t b = blockIdx.y;
  if (t >= N) return;
  const float* hi = h + (b * ((size_t)imask + 1) + ((tin + t) & imask)) * HP;
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
    const size_t at = (b * 8 + c) * N + t;
    y[at] = (a[c] + bo[c]) + x[at];
  }
}

template <int NT, int TT, int SPLIT>
void launch_conv_stream(const float* in, const float* wsw, const float* sc, long long sc_stride, const float* res, float* out, int B,
                        int N, int K, int dil, int off0, int epi, int tin, int imask, int tout, int omask, hipStream_t st) {
  const int per_block = (4 / SPLIT) * TT * 16;
  dim3 grid((unsigned)((N + per_block - 1) / per_block), (unsigned)B);
  hipLaunchKernelGGL((tcn_conv_stream_kernel<NT, TT, SPLIT>), grid, dim3(256), 0, st, in, wsw, sc, sc_stride, res, out, N, K, dil, off0,
                     epi, tin, imask, tout, omask);
}

// Time tiles per wave.  A wave's tile is one serial MFMA stream (measured at H = 128 with the offline tile: 0.14 ms per
// convolution whether the block has 128 or 2048 samples), so a block is spread over as many waves as the chip has SIMDs before
// a wave gets more than 16 samples: the largest of (offline tile, 2, 1) with which the launch still has kStreamWaves waves,
// else 1.  The result does not depend on the tile (the chain of an output element is the same in every lane and tile).
constexpr int kStreamWaves = 1024;   // 256 CUs x 4 SIMDs
int stream_time_tile(int nt, int B, int N) {
  const int big = nt <= 2 ? 8 : 4, split = nt <= 4 ? 1 : 2;   // the tiles of conv_for
  for (int tt : {big, 2})
    if ((long long)B * ((N + 16 * tt - 1) / (16 * tt)) * split >= kStreamWaves) return tt;
  return 1;
}

typedef void (*conv_stream_fn)(const float*, const float*, const float*, long long, const float*, float*, int, int, int, int, int,
                               int, int, int, int, int, hipStream_t);
template <int NT, int TT, int SPLIT>
conv_stream_fn conv_stream_pick(int tt) {
  return tt == TT ? launch_conv_stream<NT, TT, SPLIT> : tt == 2 ? launch_conv_stream<NT, 2, SPLIT> : launch_conv_stream<NT, 1, SPLIT>;
}
conv_stream_fn conv_stream_for(int nt, int tt) {
  switch (nt) {
    case 1: return conv_stream_pick<1, 8, 1>(tt);
    case 2: return conv_stream_pick<2, 8, 1>(tt);
    case 3: return conv_stream_pick<3, 4, 1>(tt);
    case 4: return conv_stream_pick<4, 4, 1>(tt);
    case 5: return conv_stream_pick<5, 4, 2>(tt);
    case 6: return conv_stream_pick<6, 4, 2>(tt);
    case 7: return conv_stream_pick<7, 4, 2>(tt);
    case 8: return conv_stream_pick<8, 4, 2>(tt);
  }
  return nullptr;
}

constexpr size_t kStreamWorkspace = 256;   // nothing is kept there today; the argument is reserved

// Rows of ring r (0 .. 2 nb): the power of two >= history + max_block.
long long stream_cap(const mst_tcn* h, int r, int max_block) {
  const long long hist = r < 2 * h->cfg.num_blocks ? (long long)(h->cfg.kernel_size - 1) << (r / 2) : 0;
  long long cap = 1;
  while (cap < hist + max_block) cap <<= 1;
  return cap;
}

int stream_shape_ok(const mst_tcn* h, int B, int max_block, const char* who) {
  MST_REQUIRE(h, "%s: NULL handle", who);
  MST_REQUIRE(h->cfg.causal, "%s: streaming needs a causal mixer; a non-causal one looks ahead ((K - 1) * d) / 2 samples per layer, "
              "which a block-wise call does not have: evaluate whole clips with mst_tcn_forward, or stream with a fixed latency "
              "through mst_tcn_lookahead_push", who);
  MST_REQUIRE(h->mode == MST_TCN_FP32, "%s: the handle is in MST_TCN_F16X3 mode, whose per-clip range scale is a function of the whole "
              "clip: call mst_tcn_set_precision(MST_TCN_FP32) before streaming", who);
  MST_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in 1..65535, got %d", who, B);
  MST_REQUIRE(max_block >= 1, "%s: max_block must be positive, got %d", who, max_block);
  const long long top = (long long)(h->cfg.kernel_size - 1) << (h->cfg.num_blocks - 1);   // < 2^20
  MST_REQUIRE(max_block < (1 << 30) && stream_cap(h, 2 * h->cfg.num_blocks - 2, max_block) * h->HP < (1LL << 31),
              "%s: max_block = %d is too large: the ring of the last block (%lld rows of history + max_block, rounded up to a power of "
              "two) times H_padded = %d must stay below 2^31 elements", who, max_block, top, h->HP);
  return MST_OK;
}

size_t stream_sc_bytes(const mst_tcn* h, int B) { return align_up(tcn_sc_floats(h, B) * sizeof(float), 256); }

size_t stream_state_bytes(const mst_tcn* h, int B, int max_block) {
  size_t rows = 0;
  for (int r = 0; r <= 2 * h->cfg.num_blocks; ++r) rows += (size_t)stream_cap(h, r, max_block);
  return stream_sc_bytes(h, B) + rows * B * h->HP * sizeof(float);
}

}  // namespace
}  // namespace mst

extern "C" {

size_t mst_tcn_stream_state_bytes(const mst_tcn* h, int B, int max_block) {
  if (stream_shape_ok(h, B, max_block, "mst_tcn_stream_state_bytes") != MST_OK) return 0;
  return stream_state_bytes(h, B, max_block);
}

size_t mst_tcn_stream_workspace_bytes(const mst_tcn* h, int B, int max_block) {
  if (stream_shape_ok(h, B, max_block, "mst_tcn_stream_workspace_bytes") != MST_OK) return 0;
  return kStreamWorkspace;
}

int mst_tcn_stream_samples_per_wave(const mst_tcn* h, int B, int N) {
  if (!h || B < 1 || N < 1) return 0;
  return 16 * stream_time_tile(h->HP / 16, B, N);
}

int mst_tcn_stream_reset(const mst_tcn* h, void* state, size_t state_bytes, int B, int max_block, const float* film, void* stream) {
  const int rc = stream_shape_ok(h, B, max_block, "mst_tcn_stream_reset");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(state, "mst_tcn_stream_reset: NULL state");
  MST_REQUIRE(!h->cfg.use_film == !film, "mst_tcn_stream_reset: film parameters are %s for this mixer (use_film = %d)",
              h->cfg.use_film ? "required" : "not accepted", h->cfg.use_film);
  const size_t need = stream_state_bytes(h, B, max_block);
  if (state_bytes < need) return fail(MST_ENOMEM, "mst_tcn_stream_reset: state %zu B < required %zu B", state_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int H = h->cfg.hidden_channels, HP = h->HP, nb = h->cfg.num_blocks;
  const long long nsc = (long long)B * nb * 2 * HP;
  hipLaunchKernelGGL(tcn_fold_kernel, dim3((unsigned)((nsc + 255) / 256)), dim3(256), 0, st, h->cb, h->bw, h->bb, h->bm, h->bv, film,
                     (float*)state, B, nb, H, HP, h->cfg.bn_eps);
  MST_HIP_CHECK(hipGetLastError());
  MST_HIP_CHECK(hipMemsetAsync((char*)state + stream_sc_bytes(h, B), 0, need - stream_sc_bytes(h, B), st));
  return MST_OK;
}

int mst_tcn_stream_push(const mst_tcn* h, void* state, size_t state_bytes, int B, int max_block, long long t0, const float* x, int N,
                        float* y, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = stream_shape_ok(h, B, max_block, "mst_tcn_stream_push");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(state && x && y, "mst_tcn_stream_push: NULL pointer");
  MST_REQUIRE((uintptr_t)state % 16 == 0, "mst_tcn_stream_push: state must be 16-byte aligned");
  MST_REQUIRE(N >= 1 && N <= max_block, "mst_tcn_stream_push: N must be in 1..max_block = %d, got %d", max_block, N);
  MST_REQUIRE(t0 >= 0, "mst_tcn_stream_push: t0 (samples pushed so far) must not be negative, got %lld", t0);
  const size_t need = stream_state_bytes(h, B, max_block);
  if (state_bytes < need) return fail(MST_ENOMEM, "mst_tcn_stream_push: state %zu B < required %zu B", state_bytes, need);
  if (workspace_bytes < kStreamWorkspace)
    return fail(MST_ENOMEM, "mst_tcn_stream_push: workspace %zu B < required %zu B", workspace_bytes, kStreamWorkspace);
  (void)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int HP = h->HP, K = h->cfg.kernel_size, nb = h->cfg.num_blocks;
  const float* sc = (const float*)state;
  float* ring[2 * kMaxBlocks + 1];
  int mask[2 * kMaxBlocks + 1], at[2 * kMaxBlocks + 1];   // cap - 1 and t0 & (cap - 1) of every ring
  float* p = (float*)((char*)state + stream_sc_bytes(h, B));
  for (int r = 0; r <= 2 * nb; ++r) {
    const long long cap = stream_cap(h, r, max_block);
    ring[r] = p, mask[r] = (int)(cap - 1), at[r] = (int)(t0 & (cap - 1));
    p += (size_t)cap * B * HP;
  }
  dim3 tgrid((unsigned)((N + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(tcn_input_stream_kernel, tgrid, dim3(256), 0, st, x, h->wi, h->bi, ring[0], N, HP, at[0], mask[0]);
  conv_stream_fn conv = conv_stream_for(HP / 16, stream_time_tile(HP / 16, B, N));
  const size_t per_conv = (size_t)K * HP * HP;
  const long long sc_stride = (long long)nb * 4 * HP;
  const int epi2 = h->cfg.use_film ? EPI_ACT_THEN_RES : EPI_RES_THEN_ACT;
  for (int k = 0; k < nb; ++k) {
    const int dil = 1 << k, off0 = -(K - 1) * dil;
    float *hk = ring[2 * k], *gk = ring[2 * k + 1];
    conv(hk, h->wsw + (size_t)(2 * k) * per_conv, sc + (size_t)(2 * k) * 2 * HP, sc_stride, hk, gk, B, N, K, dil, off0, EPI_ACT,
         at[2 * k], mask[2 * k], at[2 * k + 1], mask[2 * k + 1], st);
    conv(gk, h->wsw + (size_t)(2 * k + 1) * per_conv, sc + (size_t)(2 * k + 1) * 2 * HP, sc_stride, hk, ring[2 * k + 2], B, N, K, dil,
         off0, epi2, at[2 * k + 1], mask[2 * k + 1], at[2 * k + 2], mask[2 * k + 2], st);
  }
  hipLaunchKernelGGL(tcn_output_stream_kernel, tgrid, dim3(256), 0, st, ring[2 * nb], h->wo, h->bo, x, y, N, HP, at[2 * nb], mask[2 * nb]);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"
