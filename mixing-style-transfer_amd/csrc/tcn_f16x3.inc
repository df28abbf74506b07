// Stage C, opt-in split-precision inference (mst_tcn_set_precision(tcn, MST_TCN_F16X3)): the dilated convolutions of
// tcn.hip on the f16 matrix pipe.  Included by tcn.hip; the fp32 kernels above are not touched and stay the default.
//
// x = xh + xl, w = wh + wl, f16 each (22 significant bits together).  Three v_mfma_f32_16x16x32_f16 products with fp32
// accumulation per (tap, 32-channel chunk, output tile, time tile), small terms first: wl*xh, wh*xl, wh*xh; only wl*xl
// (2^-22 of the product) is dropped.  Every f16 x f16 product is exact in fp32, so the arithmetic differs from the fp32
// kernel's only by the 2^-23 rounding of the two splits and by the order of the sum.
//
// Operands (the MFMA's K is 32): lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15],
// j = 0..7; C/D is col = l & 15, row = 4 (l >> 4) + reg -- the accumulator layout of tcn_conv_kernel, so the epilogue is
// that kernel's.  Activations: two f16 planes [B][T][HP32], HP32 = H padded to a multiple of 32 with exact zeros; a lane's
// B operand is one 16-byte load (8 input channels of one time sample) whatever the dilation.  Weights: hi and lo fragments
// in A order, [conv][tap][chunk][out tile][hi, lo][64 lanes][8], one 16-byte load each per lane.
//
// Range control, no host check.  Each convolution's input gets one exact power-of-two scale PER CLIP that puts the clip's
// max|v| into [2^14, 2^15): nothing saturates (f16 max 65504), and the low part of an element down to 2^-17 of the clip's
// maximum is still a normal f16 with all its 11 bits; below that the absolute error is 2^-39 of the maximum.  max|v| comes
// from the PRODUCING kernel: the convolution's epilogue reduces it per wave and issues one integer atomicMax on the bit
// pattern of the non-negative float into absmax[conv][clip] (tcn_absmax_kernel does it for the input projection, whose
// kernel stays as it is).  An integer max is exact and order-independent: results stay bit-reproducible, and a clip's
// scale does not depend on its neighbours in the batch.  tcn_split_kernel then reads the fp32 buffer once and writes the
// two scaled planes (split on the producer side: the consumer would redo the conversion for each of its K taps, 15 times).
// Filters get one power-of-two exponent per (convolution, output channel) the same way (tcn_f16x3_weights_kernel, from the
// handle's fp32 wsw).  The epilogue undoes both with one ldexpf, exact.

namespace mst {
namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// k with a * 2^k in [2^14, 2^15).  Zero takes k = 0 (scale 1); the clamp keeps 2^k and the epilogue's 2^-(kx + kw) finite.
__device__ __forceinline__ int f16x3_exponent(float a) {
  if (!(a > 0.f)) return 0;
  if (!(a < INFINITY)) return -100;
  int ex;
  (void)frexpf(a, &ex);   // a in [2^(ex - 1), 2^ex)
  return max(-100, min(100, 15 - ex));
}

// absmax[b] = max |h[b][:][:]| as the bit pattern of the non-negative float.  h: [B][n] fp32, n % 4 == 0.
__global__ __launch_bounds__(256) void tcn_absmax_kernel(const float* __restrict__ h, long long n, unsigned* __restrict__ absmax) {
  const f32x4* p = reinterpret_cast<const f32x4*>(h + (size_t)blockIdx.y * n);
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (n >> 2); i += (long long)gridDim.x * 256) {
    const f32x4 v = p[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) atomicMax(absmax + blockIdx.y, __float_as_uint(m));
}

// xh + xl = in * 2^k(clip), f16 each.  in: [B][T][HP] fp32; xh, xl: [B][T][HP32].  One thread per 8 channels of one sample
// (HP is a multiple of 16, so a group of 8 is all data or all padding).
__global__ __launch_bounds__(256) void tcn_split_kernel(const float* __restrict__ in, const unsigned* __restrict__ absmax,
                                                        _Float16* __restrict__ xh, _Float16* __restrict__ xl, long long T, int HP,
                                                        int HP32) {
  const int per = HP32 >> 3;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= T * per) return;
  const long long t = i / per;
  const int c = (int)(i % per) * 8;
  h16x8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) hi[q] = lo[q] = (_Float16)0.f;
  if (c < HP) {
    const float s = ldexpf(1.0f, f16x3_exponent(__uint_as_float(absmax[b])));
    const float* p = in + ((size_t)b * T + t) * HP + c;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p), v1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float v = (q < 4 ? v0[q] : v1[q - 4]) * s;
      hi[q] = (_Float16)v;
      lo[q] = (_Float16)(v - (float)hi[q]);
    }
  }
  const size_t at = ((size_t)b * T + t) * HP32 + c;
  *reinterpret_cast<h16x8*>(xh + at) = hi;
  *reinterpret_cast<h16x8*>(xl + at) = lo;
}

// THE builder of the f16 weight fragments, on the device, from the handle's fp32 wsw ([conv][tap][16-chunk][out tile][lane][4],
// tcn.hip).  One wave per (convolution, output channel): the row's max|w| gives its exponent kw (an all-zero row takes 0
// and yields zeros), then wh + wl = w * 2^kw go to [conv][tap][32-chunk][out tile][hi, lo][lane][8].  Input channels
// HP..HP32 are zeros.
__global__ __launch_bounds__(64) void tcn_f16x3_weights_kernel(const float* __restrict__ wsw, _Float16* __restrict__ wf,
                                                               int* __restrict__ wexp, int HP, int K) {
  const int NT = HP / 16, NC = (NT + 1) / 2, HP32 = NC * 32;
  const int co = blockIdx.x, cv = blockIdx.y, lane = threadIdx.x;
  const int o = co >> 4, r = co & 15;
  const float* w = wsw + (size_t)cv * K * HP * HP;
  // element (tap, ci) of this row in wsw
  auto at = [&](int tap, int ci) { return ((((size_t)tap * NT + (ci >> 4)) * NT + o) * 64 + ((ci >> 2 & 3) * 16 + r)) * 4 + (ci & 3); };
  float m = 0.f;
  for (int e = lane; e < K * HP; e += 64) m = fmaxf(m, fabsf(w[at(e / HP, e % HP)]));
  m = wave_max(m);
  const int k = f16x3_exponent(m);
  if (lane == 0) wexp[cv * HP + co] = k;
  const float s = ldexpf(1.0f, k);
  _Float16* f = wf + (size_t)cv * K * NC * NT * 1024;
  for (int e = lane; e < K * HP32; e += 64) {
    const int tap = e / HP32, ci = e % HP32;
    const float v = ci < HP ? w[at(tap, ci)] * s : 0.f;
    const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
    const size_t d = (((size_t)tap * NC + (ci >> 5)) * NT + o) * 1024 + ((ci >> 3 & 3) * 16 + r) * 8 + (ci & 7);
    f[d] = hi;
    f[d + 512] = lo;
  }
}

// One tap of a wave's tile, as tcn_conv_tap: the clamped address plus select at clip edges (EDGE), no out-of-range address
// formed, 32-bit offsets (HP32 * T < 2^31 is checked by the caller), and the two-level sum -- the three products of every
// chunk of ONE tap go into `part`, and `part` is added to `acc` once per tap.
template <int NT, int TT, int NO, bool EDGE, bool ODD>
__device__ __forceinline__ void tcn_conv_f16x3_tap(f32x4 (&acc)[NO][TT], const _Float16* __restrict__ xhb,
                                                   const _Float16* __restrict__ xlb, const _Float16* __restrict__ wt, int ts, int T,
                                                   int j, int g, int o0) {
  constexpr int NC = (NT + 1) / 2, HP32 = NC * 32;
  int xoff[TT];
  bool ok[TT];
#pragma unroll
  for (int m = 0; m < TT; ++m) {
    const int t = ts + m * 16 + j;
    ok[m] = !EDGE || (t >= 0 && t < T);
    const int tc = !EDGE ? t : (t < 0 ? 0 : (t >= T ? T - 1 : t));
    xoff[m] = tc * HP32 + 8 * g;
  }
  f32x4 part[NO][TT];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int m = 0; m < TT; ++m) part[o][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) {
    h16x8 xh[TT], xl[TT], wh[NO], wl[NO];
#pragma unroll
    for (int m = 0; m < TT; ++m) {
      const h16x8 vh = *reinterpret_cast<const h16x8*>(xhb + xoff[m] + ch * 32);
      const h16x8 vl = *reinterpret_cast<const h16x8*>(xlb + xoff[m] + ch * 32);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        xh[m][q] = ok[m] ? vh[q] : (_Float16)0.f;
        xl[m][q] = ok[m] ? vl[q] : (_Float16)0.f;
      }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int ot = !ODD || o0 + o < NT ? o0 + o : NT - 1;   // NT odd: the last tile of the second half does not exist
      const _Float16* wp = wt + (ch * NT + ot) * 1024;
      wh[o] = *reinterpret_cast<const h16x8*>(wp);
      wl[o] = *reinterpret_cast<const h16x8*>(wp + 512);
    }
    // small terms first; the NO * TT accumulators between two products of one accumulator keep the matrix pipe busy
#pragma unroll
    for (int term = 0; term < 3; ++term)
#pragma unroll
      for (int o = 0; o < NO; ++o)
        if (!ODD || o0 + o < NT) {
#pragma unroll
          for (int m = 0; m < TT; ++m)
            part[o][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(term == 0 ? wl[o] : wh[o], term == 1 ? xl[m] : xh[m], part[o][m], 0, 0, 0);
        }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int m = 0; m < TT; ++m) acc[o][m] += part[o][m];
}

// xh, xl: [B][T][HP32] planes of this convolution's input; am_in: [B] the absmax patterns they were scaled by.
// wf: this convolution's fragments; wexp: [HP] its filter exponents.  sc, res, out, epi, T, K, dil, off0: as tcn_conv_kernel.
// am_out: [B] absmax patterns of the result (the next convolution's am_in), or NULL.  NT, TT, SPLIT: as tcn_conv_kernel.
template <int NT, int TT, int SPLIT>
__global__ __launch_bounds__(256, 2) void tcn_conv_f16x3_kernel(const _Float16* __restrict__ xh, const _Float16* __restrict__ xl,
                                                                const unsigned* __restrict__ am_in, const _Float16* __restrict__ wf,
                                                                const int* __restrict__ wexp, const float* __restrict__ sc,
                                                                long long sc_stride, const float* res, float* out,
                                                                unsigned* am_out, int T, int K, int dil, int off0, int epi) {
  constexpr int HP = NT * 16, NC = (NT + 1) / 2, HP32 = NC * 32, NO = (NT + SPLIT - 1) / SPLIT;
  constexpr bool ODD = NT % SPLIT != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int o0 = (wave % SPLIT) * NO;
  const long long b = blockIdx.y;
  const long long t0l = ((long long)blockIdx.x * (4 / SPLIT) + wave / SPLIT) * (TT * 16);
  if (t0l >= T) return;
  const int t0 = (int)t0l;
  const _Float16* xhb = xh + b * T * HP32;
  const _Float16* xlb = xl + b * T * HP32;

  f32x4 acc[NO][TT];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int m = 0; m < TT; ++m) acc[o][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tap = 0; tap < K; ++tap) {
    const int ts = t0 + off0 + tap * dil;
    if (ts >= T || ts + TT * 16 <= 0) continue;   // the whole strip is padding: exact zeros
    const _Float16* wt = wf + tap * (NC * NT * 1024) + lane * 8;
    if (NT <= 2 && ts >= 0 && ts + TT * 16 <= T)
      tcn_conv_f16x3_tap<NT, TT, NO, false, ODD>(acc, xhb, xlb, wt, ts, T, j, g, o0);
    else
      tcn_conv_f16x3_tap<NT, TT, NO, true, ODD>(acc, xhb, xlb, wt, ts, T, j, g, o0);
  }

  const int kx = f16x3_exponent(__uint_as_float(am_in[b]));
  const float* scb = sc + b * sc_stride;
  float amax = 0.f;
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    if (o0 + o >= NT) continue;
    const int c = (o0 + o) * 16 + 4 * g;
    const f32x4 S = *reinterpret_cast<const f32x4*>(scb + c), Cc = *reinterpret_cast<const f32x4*>(scb + HP + c);
    int kq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) kq[q] = -(kx + wexp[c + q]);
#pragma unroll
    for (int m = 0; m < TT; ++m) {
      const int t = t0 + m * 16 + j;
      if (t >= T) continue;
      const size_t at = ((size_t)b * T + t) * HP + c;
      f32x4 v = acc[o][m], r = f32x4{0.f, 0.f, 0.f, 0.f};
      if (epi != EPI_ACT) r = *reinterpret_cast<const f32x4*>(res + at);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z = fmaf(S[q], ldexpf(v[q], kq[q]), Cc[q]);
        if (epi == EPI_RES_THEN_ACT) z += r[q];
        z = leaky(z);
        if (epi == EPI_ACT_THEN_RES) z += r[q];
        v[q] = z;
        amax = fmaxf(amax, fabsf(z));
      }
      *reinterpret_cast<f32x4*>(out + at) = v;
    }
  }
  if (am_out) {
    amax = wave_max(amax);
    if (lane == 0) atomicMax(am_out + b, __float_as_uint(amax));
  }
}

template <int NT, int TT, int SPLIT>
void launch_conv_f16x3(const _Float16* xh, const _Float16* xl, const unsigned* am_in, const _Float16* wf, const int* wexp,
                       const float* sc, long long sc_stride, const float* res, float* out, unsigned* am_out, int B, int T, int K,
                       int dil, int off0, int epi, hipStream_t st) {
  const long long per_block = (4LL / SPLIT) * TT * 16;
  dim3 grid((unsigned)((T + per_block - 1) / per_block), (unsigned)B);
  hipLaunchKernelGGL((tcn_conv_f16x3_kernel<NT, TT, SPLIT>), grid, dim3(256), 0, st, xh, xl, am_in, wf, wexp, sc, sc_stride, res, out,
                     am_out, T, K, dil, off0, epi);
}

typedef void (*conv_f16x3_fn)(const _Float16*, const _Float16*, const unsigned*, const _Float16*, const int*, const float*, long long,
                              const float*, float*, unsigned*, int, int, int, int, int, int, hipStream_t);
// output tiles NT = 1..8, input chunks (NT + 1) / 2 = 1..4; TT and SPLIT as the fp32 kernel's (the accumulators are the same)
conv_f16x3_fn conv_f16x3_for(int nt) {
  switch (nt) {
    case 1: return launch_conv_f16x3<1, 8, 1>;
    case 2: return launch_conv_f16x3<2, 8, 1>;
    case 3: return launch_conv_f16x3<3, 4, 1>;
    case 4: return launch_conv_f16x3<4, 4, 1>;
    case 5: return launch_conv_f16x3<5, 4, 2>;
    case 6: return launch_conv_f16x3<6, 4, 2>;
    case 7: return launch_conv_f16x3<7, 4, 2>;
    case 8: return launch_conv_f16x3<8, 4, 2>;
  }
  return nullptr;
}

int tcn_hp32(const mst_tcn* h) { return (h->HP + 31) / 32 * 32; }
size_t tcn_f16x3_plane_bytes(const mst_tcn* h, int B, long long T) { return align_up((size_t)B * T * tcn_hp32(h) * sizeof(_Float16), 256); }
size_t tcn_f16x3_absmax_bytes(const mst_tcn* h, int B) { return align_up((size_t)2 * h->cfg.num_blocks * B * sizeof(unsigned), 256); }

}  // namespace

size_t tcn_f16x3_extra_bytes(const mst_tcn* h, int B, long long T) {
  return 2 * tcn_f16x3_plane_bytes(h, B, T) + tcn_f16x3_absmax_bytes(h, B);
}

int tcn_f16x3_shape_ok(const mst_tcn* h, long long T, const char* who) {
  MST_REQUIRE((long long)tcn_hp32(h) * T < (1LL << 31), "%s: in the f16x3 mode H padded to 32 (%d) * T must stay below 2^31 per clip "
              "(T = %lld): split the clip in time", who, tcn_hp32(h), T);
  return MST_OK;
}

int tcn_f16x3_build(mst_tcn* h, hipStream_t st) {
  const int HP = h->HP, NT = HP / 16, NC = (NT + 1) / 2, K = h->cfg.kernel_size, nconv = 2 * h->cfg.num_blocks;
  if (!h->wf) {
    hipError_t e = hipMalloc((void**)&h->wf, (size_t)nconv * K * NC * NT * 1024 * sizeof(_Float16));
    if (e != hipSuccess) return fail(MST_ENOMEM, "mst_tcn_set_precision: hipMalloc failed: %s", hipGetErrorString(e));
  }
  if (!h->wexp) {
    hipError_t e = hipMalloc((void**)&h->wexp, (size_t)nconv * HP * sizeof(int));
    if (e != hipSuccess) return fail(MST_ENOMEM, "mst_tcn_set_precision: hipMalloc failed: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(tcn_f16x3_weights_kernel, dim3((unsigned)HP, (unsigned)nconv), dim3(64), 0, st, h->wsw, (_Float16*)h->wf, h->wexp, HP, K);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

// mst_tcn_forward in the f16x3 mode, after its checks.  ws: [hbuf][gbuf][sc] as in fp32, then [xh][xl][absmax].
int tcn_forward_f16x3(const mst_tcn* h, const float* x, const float* film, int B, long long T, float* y, const mst_tcn_taps* taps,
                      void* ws, hipStream_t st) {
  const int H = h->cfg.hidden_channels, HP = h->HP, HP32 = tcn_hp32(h), K = h->cfg.kernel_size, nb = h->cfg.num_blocks;
  const int NT = HP / 16, NC = HP32 / 32;
  const size_t hb = align_up((size_t)B * T * HP * sizeof(float), 256), pb = tcn_f16x3_plane_bytes(h, B, T);
  float* hbuf = (float*)ws;
  float* gbuf = (float*)((char*)ws + hb);
  float* sc = (float*)((char*)ws + 2 * hb);
  char* extra = (char*)ws + 2 * hb + align_up(tcn_sc_floats(h, B) * sizeof(float), 256);
  _Float16* xh = (_Float16*)extra;
  _Float16* xl = (_Float16*)(extra + pb);
  unsigned* am = (unsigned*)(extra + 2 * pb);   // [2 nb][B]
  const _Float16* wf = (const _Float16*)h->wf;

  MST_HIP_CHECK(hipMemsetAsync(am, 0, (size_t)2 * nb * B * sizeof(unsigned), st));
  const long long nsc = (long long)B * nb * 2 * HP;
  hipLaunchKernelGGL(tcn_fold_kernel, dim3((unsigned)((nsc + 255) / 256)), dim3(256), 0, st, h->cb, h->bw, h->bb, h->bm, h->bv, film, sc,
                     B, nb, H, HP, h->cfg.bn_eps);
  dim3 tgrid((unsigned)((T + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(tcn_input_kernel, tgrid, dim3(256), 0, st, x, h->wi, h->bi, hbuf, T, HP);
  const long long nclip = T * HP;
  hipLaunchKernelGGL(tcn_absmax_kernel, dim3((unsigned)std::min<long long>(1024, (nclip / 4 + 255) / 256), (unsigned)B), dim3(256), 0, st,
                     hbuf, nclip, am);
  conv_f16x3_fn conv = conv_f16x3_for(NT);
  const size_t per_conv = (size_t)K * NC * NT * 1024;
  const long long sc_stride = (long long)nb * 4 * HP;
  dim3 sgrid((unsigned)((T * (HP32 / 8) + 255) / 256), (unsigned)B);
  for (int k = 0; k < nb; ++k) {
    const int dil = 1 << k;
    const int off0 = h->cfg.causal ? -(K - 1) * dil : -(((K - 1) * dil) / 2);
    unsigned *a0 = am + (size_t)(2 * k) * B, *a1 = a0 + B, *a2 = k + 1 < nb ? a1 + B : nullptr;
    hipLaunchKernelGGL(tcn_split_kernel, sgrid, dim3(256), 0, st, hbuf, a0, xh, xl, T, HP, HP32);
    conv(xh, xl, a0, wf + (size_t)(2 * k) * per_conv, h->wexp + (size_t)(2 * k) * HP, sc + (size_t)(2 * k) * 2 * HP, sc_stride, nullptr, gbuf,
         a1, B, (int)T, K, dil, off0, EPI_ACT, st);
    hipLaunchKernelGGL(tcn_split_kernel, sgrid, dim3(256), 0, st, gbuf, a1, xh, xl, T, HP, HP32);
    conv(xh, xl, a1, wf + (size_t)(2 * k + 1) * per_conv, h->wexp + (size_t)(2 * k + 1) * HP, sc + (size_t)(2 * k + 1) * 2 * HP, sc_stride,
         hbuf, hbuf, a2, B, (int)T, K, dil, off0, h->cfg.use_film ? EPI_ACT_THEN_RES : EPI_RES_THEN_ACT, st);
    if (taps)
      for (int i = 0; i < taps->n; ++i)
        if (taps->block[i] == k) hipLaunchKernelGGL(tcn_tap_kernel, tgrid, dim3(256), 0, st, hbuf, taps->h[i], T, H, HP);
  }
  hipLaunchKernelGGL(tcn_output_kernel, tgrid, dim3(256), 0, st, hbuf, h->wo, h->bo, x, y, T, HP);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // namespace mst

extern "C" {

int mst_tcn_set_precision(mst_tcn* h, int mode, void* stream) {
  MST_REQUIRE(h, "mst_tcn_set_precision: NULL handle");
  MST_REQUIRE(mode == MST_TCN_FP32 || mode == MST_TCN_F16X3, "mst_tcn_set_precision: unknown mode %d (MST_TCN_FP32 = 0, MST_TCN_F16X3 = 1)",
              mode);
  if (mode == MST_TCN_F16X3) {
    const int rc = tcn_f16x3_build(h, (hipStream_t)stream);
    if (rc != MST_OK) return rc;
  }
  h->mode = mode;
  return MST_OK;
}

int mst_tcn_get_precision(const mst_tcn* h) { return h ? h->mode : MST_TCN_FP32; }

}  // extern "C"
