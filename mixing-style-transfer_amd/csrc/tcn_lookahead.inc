// Stage C, streaming with a fixed latency: block-wise inference of a NON-CAUSAL mixer (included by tcn.hip).  DESIGN 3.16.
//
// On a delayed timeline a symmetric convolution is a causal one: give each layer the lag pad = (K - 1) d / 2 and relabel row t
// of a causal convolution over [t - (K - 1) d, t] as row t - pad.  Ring r (the layout of tcn_stream.inc, same capacities) has
// the lag L_r, L_0 = 0 and L_{r+1} = L_r + pad of its producer; in a push its producer writes the times [t0 - L_r, t0 + N - L_r)
// and its consumer reads [t0 - L_r - (K - 1) d, t0 + N - L_r), the causal stream's span.  The last ring's lag is the latency
// (K - 1) (2^nb - 1): y[i] of a push is the output sample at time t0 + i - latency.  A causal mixer has pad = 0 everywhere.
//
// The offline forward pads EVERY layer's input with zeros outside the clip [0, T), so a row whose time is outside [0, T) is
// stored as zeros (a select in the epilogue: such a row may be computed from stale ring rows), at the clip's start (t < 0) and,
// once t_end = T is known, at its end.  The residual of conv2 and the skip x of the output are read at the time of the row they
// are added to: the block's input ring at the lag of the block's output, and x from a delay ring [B][8][cap_x], cap_x the power
// of two >= latency + max_block.  Every stored element is the chain of the offline kernel on the same operands (tcn_stream.inc,
// DESIGN 3.15), now at both ends of the clip, so the output delayed by the latency is mst_tcn_forward's bit for bit.

namespace mst {
namespace {

// tcn_conv_stream_kernel with a lagged residual and the zero-row rule.  tres: the ring row of this push's first residual
// sample (ring `res`, mask imask); rows outside [zlo, zhi) of the push are stored as zeros.  A wave whose whole tile is outside
// stores its zeros without the tap loop.
template <int NT, int TT, int SPLIT>
__global__ __launch_bounds__(256, 2) void tcn_conv_lookahead_kernel(const float* __restrict__ in, const float* __restrict__ wsw,
                                                                    const float* __restrict__ sc, long long sc_stride,
                                                                    const float* __restrict__ res, float* __restrict__ out, int N,
                                                                    int K, int dil, int off0, int epi, int tin, int tres, int imask,
                                                                    int tout, int omask, int zlo, int zhi) {
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

  if (tl + TT * 16 > zlo && tl < zhi)
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
      if (epi != EPI_ACT) r = *reinterpret_cast<const f32x4*>(resb + (((tres + t) & imask) * HP + c));
      f32x4 v = acc[o][m];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = tcn_conv_epilogue(v[q], S[q], Cc[q], r[q], epi);
      if (t < zlo || t >= zhi) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(outb + (((tout + t) & omask) * HP + c)) = v;
    }
  }
}

// tcn_input_stream_kernel that also keeps x in the delay ring xr: [B][8][xmask + 1], sample t in column t & xmask.  x == NULL
// (a drain push: N rows after the clip's end): zero rows of h and zeros in the delay ring.
__global__ __launch_bounds__(256) void tcn_input_lookahead_kernel(const float* __restrict__ x, const float* __restrict__ wi,
                                                                  const float* __restrict__ bi, float* __restrict__ h,
                                                                  float* __restrict__ xr, int N, int HP, int tout, int omask, int xat,
                                                                  int xmask) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t b = blockIdx.y;
  if (t >= N) return;
  float xv[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) xv[c] = x ? x[(b * 8 + c) * N + t] : 0.f;
  float* xo = xr + b * 8 * ((size_t)xmask + 1) + ((xat + t) & xmask);
#pragma unroll
  for (int c = 0; c < 8; ++c) xo[c * ((size_t)xmask + 1)] = xv[c];
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
    if (!x) v = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(ho + o) = v;
  }
}

// tcn_output_stream_kernel with x from the delay ring (xin: the column of this push's first output sample) and zeros
// outside [zlo, zhi).
__global__ __launch_bounds__(256) void tcn_output_lookahead_kernel(const float* __restrict__ h, const float* __restrict__ wo,
                                                                   const float* __restrict__ bo, const float* __restrict__ xr,
                                                                   float* __restrict__ y, int N, int HP, int tin, int imask, int xin,
                                                                   int xmask, int zlo, int zhi) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t b = blockIdx.y;
  if (t >= N) return;
  const bool live = t >= zlo && t < zhi;
  const float* hi = h + (b * ((size_t)imask + 1) + ((tin + t) & imask)) * HP;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live)
    for (int k = 0; k < HP; k += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(hi + k);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] = fmaf(wo[(k + q) * 8 + c], v[q], a[c]);
    }
  const float* xi = xr + b * 8 * ((size_t)xmask + 1) + ((xin + t) & xmask);
#pragma unroll
  for (int c = 0; c < 8; ++c) y[(b * 8 + c) * N + t] = live ? (a[c] + bo[c]) + xi[c * ((size_t)xmask + 1)] : 0.f;
}

template <int NT, int TT, int SPLIT>
void launch_conv_lookahead(const float* in, const float* wsw, const float* sc, long long sc_stride, const float* res, float* out,
                           int B, int N, int K, int dil, int off0, int epi, int tin, int tres, int imask, int tout, int omask, int zlo,
                           int zhi, hipStream_t st) {
  const int per_block = (4 / SPLIT) * TT * 16;
  dim3 grid((unsigned)((N + per_block - 1) / per_block), (unsigned)B);
  hipLaunchKernelGGL((tcn_conv_lookahead_kernel<NT, TT, SPLIT>), grid, dim3(256), 0, st, in, wsw, sc, sc_stride, res, out, N, K, dil,
                     off0, epi, tin, tres, imask, tout, omask, zlo, zhi);
}

typedef void (*conv_lookahead_fn)(const float*, const float*, const float*, long long, const float*, float*, int, int, int, int, int,
                                  int, int, int, int, int, int, int, int, hipStream_t);
template <int NT, int TT, int SPLIT>
conv_lookahead_fn conv_lookahead_pick(int tt) {
  return tt == TT ? launch_conv_lookahead<NT, TT, SPLIT> : tt == 2 ? launch_conv_lookahead<NT, 2, SPLIT> : launch_conv_lookahead<NT, 1, SPLIT>;
}
conv_lookahead_fn conv_lookahead_for(int nt, int tt) {   // the tiles of conv_stream_for
  switch (nt) {
    case 1: return conv_lookahead_pick<1, 8, 1>(tt);
    case 2: return conv_lookahead_pick<2, 8, 1>(tt);
    case 3: return conv_lookahead_pick<3, 4, 1>(tt);
    case 4: return conv_lookahead_pick<4, 4, 1>(tt);
    case 5: return conv_lookahead_pick<5, 4, 2>(tt);
    case 6: return conv_lookahead_pick<6, 4, 2>(tt);
    case 7: return conv_lookahead_pick<7, 4, 2>(tt);
    case 8: return conv_lookahead_pick<8, 4, 2>(tt);
  }
  return nullptr;
}

// Lag of a convolution of block k: 0 for a causal mixer.
long long lookahead_pad(const mst_tcn* h, int k) { return h->cfg.causal ? 0 : ((long long)(h->cfg.kernel_size - 1) << k) / 2; }

long long lookahead_latency(const mst_tcn* h) {
  long long L = 0;
  for (int k = 0; k < h->cfg.num_blocks; ++k) L += 2 * lookahead_pad(h, k);
  return L;
}

// Columns of the x delay ring: the power of two >= latency + max_block.
long long lookahead_cap_x(const mst_tcn* h, int max_block) {
  long long cap = 1;
  while (cap < lookahead_latency(h) + max_block) cap <<= 1;
  return cap;
}

// stream_shape_ok without the refusal of a non-causal mixer.
int lookahead_shape_ok(const mst_tcn* h, int B, int max_block, const char* who) {
  MST_REQUIRE(h, "%s: NULL handle", who);
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

size_t lookahead_state_bytes(const mst_tcn* h, int B, int max_block) {
  return stream_state_bytes(h, B, max_block) + (size_t)lookahead_cap_x(h, max_block) * 8 * B * sizeof(float);
}

int clamp_row(long long v, int N) { return v < 0 ? 0 : v > N ? N : (int)v; }

}  // namespace
}  // namespace mst

extern "C" {

long long mst_tcn_lookahead_latency(const mst_tcn* h) {
  if (!h) {
    (void)fail(MST_EINVAL, "mst_tcn_lookahead_latency: NULL handle");
    return -1;
  }
  return lookahead_latency(h);
}

size_t mst_tcn_lookahead_state_bytes(const mst_tcn* h, int B, int max_block) {
  if (lookahead_shape_ok(h, B, max_block, "mst_tcn_lookahead_state_bytes") != MST_OK) return 0;
  return lookahead_state_bytes(h, B, max_block);
}

int mst_tcn_lookahead_reset(const mst_tcn* h, void* state, size_t state_bytes, int B, int max_block, const float* film, void* stream) {
  const int rc = lookahead_shape_ok(h, B, max_block, "mst_tcn_lookahead_reset");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(state, "mst_tcn_lookahead_reset: NULL state");
  MST_REQUIRE(!h->cfg.use_film == !film, "mst_tcn_lookahead_reset: film parameters are %s for this mixer (use_film = %d)",
              h->cfg.use_film ? "required" : "not accepted", h->cfg.use_film);
  const size_t need = lookahead_state_bytes(h, B, max_block);
  if (state_bytes < need) return fail(MST_ENOMEM, "mst_tcn_lookahead_reset: state %zu B < required %zu B", state_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int H = h->cfg.hidden_channels, HP = h->HP, nb = h->cfg.num_blocks;
  const long long nsc = (long long)B * nb * 2 * HP;
  hipLaunchKernelGGL(tcn_fold_kernel, dim3((unsigned)((nsc + 255) / 256)), dim3(256), 0, st, h->cb, h->bw, h->bb, h->bm, h->bv, film,
                     (float*)state, B, nb, H, HP, h->cfg.bn_eps);
  MST_HIP_CHECK(hipGetLastError());
  MST_HIP_CHECK(hipMemsetAsync((char*)state + stream_sc_bytes(h, B), 0, need - stream_sc_bytes(h, B), st));
  return MST_OK;
}

int mst_tcn_lookahead_push(const mst_tcn* h, void* state, size_t state_bytes, int B, int max_block, long long t0, long long t_end,
                           const float* x, int N, float* y, void* stream) {
  const int rc = lookahead_shape_ok(h, B, max_block, "mst_tcn_lookahead_push");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(state && y, "mst_tcn_lookahead_push: NULL pointer");
  MST_REQUIRE((uintptr_t)state % 16 == 0, "mst_tcn_lookahead_push: state must be 16-byte aligned");
  MST_REQUIRE(N >= 1 && N <= max_block, "mst_tcn_lookahead_push: N must be in 1..max_block = %d, got %d", max_block, N);
  MST_REQUIRE(t0 >= 0, "mst_tcn_lookahead_push: t0 (samples pushed so far) must not be negative, got %lld", t0);
  MST_REQUIRE(t0 <= (1LL << 62), "mst_tcn_lookahead_push: t0 must stay below 2^62, got %lld", t0);
  MST_REQUIRE(t_end >= 0 || x, "mst_tcn_lookahead_push: an open push (t_end < 0) needs x; only a drain push (t_end >= 0) takes NULL");
  MST_REQUIRE(t_end < 0 || t0 >= t_end, "mst_tcn_lookahead_push: t_end = %lld closes the stream at that length, so a push with t_end >= 0 "
              "is a drain push and needs t0 >= t_end, got t0 = %lld", t_end, t0);
  const size_t need = lookahead_state_bytes(h, B, max_block);
  if (state_bytes < need) return fail(MST_ENOMEM, "mst_tcn_lookahead_push: state %zu B < required %zu B", state_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int HP = h->HP, K = h->cfg.kernel_size, nb = h->cfg.num_blocks;
  const float* sc = (const float*)state;
  float* ring[2 * kMaxBlocks + 1];
  // of every ring: cap - 1, the row of time t0 - L_r, and the rows [zlo, zhi) of this push whose time is inside the clip
  int mask[2 * kMaxBlocks + 1], at[2 * kMaxBlocks + 1], zlo[2 * kMaxBlocks + 1], zhi[2 * kMaxBlocks + 1];
  long long lag[2 * kMaxBlocks + 1];
  float* p = (float*)((char*)state + stream_sc_bytes(h, B));
  long long L = 0;
  for (int r = 0; r <= 2 * nb; ++r) {
    const long long cap = stream_cap(h, r, max_block);
    lag[r] = L;
    ring[r] = p, mask[r] = (int)(cap - 1), at[r] = (int)((t0 - L) & (cap - 1));   // two's complement: times before 0 are negative
    zlo[r] = clamp_row(L - t0, N), zhi[r] = t_end < 0 ? N : clamp_row(t_end - t0 + L, N);
    p += (size_t)cap * B * HP;
    if (r < 2 * nb) L += lookahead_pad(h, r / 2);
  }
  float* xring = p;
  const long long capx = lookahead_cap_x(h, max_block);
  const int xmask = (int)(capx - 1);
  const bool drain = t_end >= 0;
  dim3 tgrid((unsigned)((N + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(tcn_input_lookahead_kernel, tgrid, dim3(256), 0, st, drain ? nullptr : x, h->wi, h->bi, ring[0], xring, N, HP, at[0],
                     mask[0], (int)(t0 & (capx - 1)), xmask);
  conv_lookahead_fn conv = conv_lookahead_for(HP / 16, stream_time_tile(HP / 16, B, N));
  const size_t per_conv = (size_t)K * HP * HP;
  const long long sc_stride = (long long)nb * 4 * HP;
  const int epi2 = h->cfg.use_film ? EPI_ACT_THEN_RES : EPI_RES_THEN_ACT;
  for (int k = 0; k < nb; ++k) {
    const int dil = 1 << k, off0 = -(K - 1) * dil;
    const int r0 = 2 * k, r1 = 2 * k + 1, r2 = 2 * k + 2;
    const int tres = (int)((t0 - lag[r2]) & mask[r0]);   // the block's input at the times of the block's output
    conv(ring[r0], h->wsw + (size_t)r0 * per_conv, sc + (size_t)r0 * 2 * HP, sc_stride, ring[r0], ring[r1], B, N, K, dil, off0, EPI_ACT,
         at[r0], at[r0], mask[r0], at[r1], mask[r1], zlo[r1], zhi[r1], st);
    conv(ring[r1], h->wsw + (size_t)r1 * per_conv, sc + (size_t)r1 * 2 * HP, sc_stride, ring[r0], ring[r2], B, N, K, dil, off0, epi2,
         at[r1], tres, mask[r1], at[r2], mask[r2], zlo[r2], zhi[r2], st);
  }
  hipLaunchKernelGGL(tcn_output_lookahead_kernel, tgrid, dim3(256), 0, st, ring[2 * nb], h->wo, h->bo, xring, y, N, HP, at[2 * nb],
                     mask[2 * nb], (int)((t0 - L) & (capx - 1)), xmask, zlo[2 * nb], zhi[2 * nb]);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"
