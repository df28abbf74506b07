// f16-operand TRAINING kernels of the conv trunk (mst_encoder_set_train_precision(enc, 1); SURVEY 8 f1, BASELINE
// configs[4]: the reference's `--use_amp` step, src/train.py:251-253 / src/params.py:71).  Included by encoder.hip inside
// its anonymous namespace.
//
// Arithmetic contract of the mode (what tests/ check against the oracle evaluated with the same roundings): the two
// operands of every convolution-shaped product are rounded to float16 --
//     forward          y  = conv(f16(x), f16(w)) + b
//     input gradient   dx = conv^T(f16(dy), f16(w))
//     weight gradient  dW = corr(f16(x), f16(dy))
// -- products exact, sums in fp32 (v_mfma_f32_16x16x32_f16); BatchNorm statistics, FiLM, ReLU, pooling, their backward,
// the master weights and every reduction stay fp32 / order-independent integer accumulators as in the fp32 mode.
// All f16 conversions happen on values that were multiplied by an exact power of two first (weights: per output channel;
// pool1: per band; gradients: one factor per backward pass from max |d pool_in|, the internal equivalent of AMP's loss
// scale) so that neither f16's 65504 ceiling nor its subnormals are reached by well-scaled OR badly-scaled tensors; the
// factors are divided out again in fp32.
//
//   f16_wstats_kernel / f16_fragments_kernel   per-step rebuild of the f16 MFMA weight fragments from the fp32 masters
//   conv2_dgrad_f16_kernel                     Conv2d(64 -> 32) of dy2 with the mirrored weights, 2 x 40 tiles
//   wgrad_f16_kernel<1 / 2>                    weight gradients with K = positions x clips (clip-minor operands)

// ---- per-(band, channel) weight statistics: power-of-two pre-scale (max |w| in [2^13, 2^14)), its inverse, L1 norm
// element (band b, channel c, o < outer, i < inner) sits at w[b * band_stride + c * ch_stride + o * outer_stride + i]
__global__ __launch_bounds__(64) void f16_wstats_kernel(const float* __restrict__ w, int nch, long long band_stride, int ch_stride,
                                                         int outer, int outer_stride, int inner, float* scale, float* inv,
                                                         float* norm) {
  const int b = blockIdx.x / nch, c = blockIdx.x % nch, lane = threadIdx.x;
  const float* base = w + (size_t)b * band_stride + (size_t)c * ch_stride;
  float mx = 0.f;
  double sum = 0.0;
  for (int o = 0; o < outer; ++o)
    for (int i = lane; i < inner; i += 64) {
      const float v = fabsf(base[(size_t)o * outer_stride + i]);
      mx = fmaxf(mx, v);
      sum += (double)v;
    }
  mx = mst::wave_max(mx);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) {
    int k = 10;
    if (mx > 0.f && mx < INFINITY) {
      int ex;
      (void)frexpf(mx, &ex);   // mx in [2^(ex-1), 2^ex)
      k = max(-100, min(100, 14 - ex));
    }
    scale[blockIdx.x] = ldexpf(1.0f, k);
    inv[blockIdx.x] = ldexpf(1.0f, -k);
    if (norm) norm[blockIdx.x] = (float)(sum * 1.001);
  }
}

// f16 MFMA B fragments [band][chunk][13 steps][NT][HL][lane][8] of scale[out channel] * w  (HL = 2: hi and lo = w - hi,
// the layout of the eval-path fragments; HL = 1: hi only).  A k-step is 4 taps x 8 input channels: lane (n, kq) holds
// tap 4 st + kq, out channel 16 nt + n, in channels 8 chunk + 0..7.
// flip = 0: w is [band][nout][nin][49].  flip = 1 (conv2's input gradient): w is conv2's weight [band][nin][nout][49]
// and the taps are mirrored -- out channel = conv2's INPUT channel, in channel = conv2's OUTPUT channel.
__global__ void f16_fragments_kernel(const float* __restrict__ w, const float* __restrict__ scale, _Float16* f, int nsub, int nout,
                                     int nin, int hl, int flip) {
  const int nt = nout / 16, nch = nin / 8;
  const long long total = (long long)nsub * nch * kF16Steps * nt * 64 * 8;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
  long long r = i >> 9;
  const int n = (int)(r % nt);
  r /= nt;
  const int st = (int)(r % kF16Steps);
  r /= kF16Steps;
  const int ck = (int)(r % nch), b = (int)(r / nch);
  const int tap = 4 * st + (lane >> 4), o = n * 16 + (lane & 15), c = ck * 8 + j;
  float v = 0.f;
  if (tap < 49) {
    const float src = flip ? w[(((size_t)b * nin + c) * nout + o) * 49 + (48 - tap)] : w[(((size_t)b * nout + o) * nin + c) * 49 + tap];
    v = src * scale[b * nout + o];
  }
  const _Float16 h = (_Float16)v;
  const size_t base = ((((size_t)b * nch + ck) * kF16Steps + st) * nt + n) * hl * 512;
  f[base + (size_t)lane * 8 + j] = h;
  if (hl == 2) f[base + 512 + (size_t)lane * 8 + j] = (_Float16)(v - (float)h);
}

// ---- the backward pass's internal loss scale: s = 2^k with max |d pool_in| * s in [2^7, 2^8)  (bits = absmax_kernel's result)
__global__ void f16_bscale_kernel(const unsigned* bits, float* scale) {
  const float m = __uint_as_float(bits[0]);
  int k = 0;
  if (m > 0.f && m < INFINITY) {
    int ex;
    (void)frexpf(m, &ex);
    k = max(-100, min(100, 8 - ex));
  }
  scale[0] = ldexpf(1.0f, k);
  scale[1] = ldexpf(1.0f, -k);
}

// Range scale of the STORED raw convolution outputs of f16 training (mode 1): one power of two per band from the bound
// |y| <= ||w_c||_1 * max|x| + |b_c|.  xb: layer 1 -- max |log-mel| over all clips (bits, [B]); layer 2 -- the bound on pool1 that
// the band's forward range scale was derived from, 2^14 / s (fscale = [B][nsub][2], constant over clips).
__global__ __launch_bounds__(64) void f16_yscale_kernel(const float* __restrict__ wnorm, const float* __restrict__ bias, int cout,
                                                         const unsigned* __restrict__ xmax_bits, int B,
                                                         const float* __restrict__ fscale, float* yscale) {
  const int band = blockIdx.x;
  float xb = 0.f;
  if (xmax_bits) {
    for (int c = threadIdx.x; c < B; c += 64) xb = fmaxf(xb, __uint_as_float(xmax_bits[c]));
    xb = mst::wave_max(xb);
  } else {
    xb = 16384.f * fscale[band * 2 + 1];
  }
  float bound = 0.f;
  for (int c = threadIdx.x; c < cout; c += 64) bound = fmaxf(bound, fmaf(wnorm[band * cout + c], xb, fabsf(bias[band * cout + c])));
  bound = mst::wave_max(bound);
  if (threadIdx.x == 0) {
    int k = 0;
    if (bound > 0.f && bound < INFINITY) {
      int ex;
      (void)frexpf(bound, &ex);
      k = max(-60, min(60, 14 - ex));
    } else if (!(bound < INFINITY)) {
      k = -60;
    }
    yscale[band * 2] = ldexpf(1.0f, k);
    yscale[band * 2 + 1] = ldexpf(1.0f, -k);
  }
}

// Range scale of pool1 for the f16 TRAINING forward: ONE power of two per band (over all clips, so that the weight gradient
// can mix clips in its K dimension), from the same rigorous bound as f16_scale_kernel -- the affine acts on acc + bias and
// Dropout rescales by `gain`.  Written to every clip's slot of scale[B][nsub][2] = (s, 1/s).
__global__ __launch_bounds__(64) void f16_scale_band_kernel(const float2* __restrict__ aff1, const float* __restrict__ w1norm,
                                                             const unsigned* __restrict__ xmax_bits, const float* __restrict__ bias,
                                                             float gain, float* scale, int B, int nsub) {
  const int band = blockIdx.x, c = threadIdx.x & 31;
  float bound = 0.f;
  for (int clip = threadIdx.x >> 5; clip < B; clip += 2) {
    const float xmax = __uint_as_float(xmax_bits[clip]);
    const float2 a = aff1[((size_t)clip * nsub + band) * 32 + c];
    bound = fmaxf(bound, fmaf(fabsf(a.x), fmaf(w1norm[band * 32 + c], xmax, fabsf(bias[band * 32 + c])), fabsf(a.y)) * gain);
  }
  bound = mst::wave_max(bound);
  int k = 0;
  if (bound > 0.f && bound < INFINITY) {
    int ex;
    (void)frexpf(bound, &ex);
    k = max(-60, min(60, 14 - ex));
  } else if (!(bound < INFINITY)) {
    k = -60;
  }
  const float s = ldexpf(1.0f, k), si = ldexpf(1.0f, -k);
  for (int clip = threadIdx.x; clip < B; clip += 64) {
    scale[((size_t)clip * nsub + band) * 2] = s;
    scale[((size_t)clip * nsub + band) * 2 + 1] = si;
  }
}

// ------------------------------------------------------------------------------------------
// The three backward kernels below are templated on TERMS, as the forward f16 kernels are:
//   TERMS = 1  plain f16 operands (training mode 1, the reference's --use_amp arithmetic)
//   TERMS = 3  split precision (training mode 2): every operand is hi + lo (two f16, 22 significant bits), a product is
//              lo*hi + hi*lo + hi*hi in three MFMAs with fp32 accumulation -- fp32-equivalent results (per-product error
//              ~2^-22; tested at the fp32 kernels' bar) at a third of the f16 matrix rate, still ~5x the fp32 rate.
// ------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------
// conv2 INPUT gradient on the f16 matrix cores: d pool1 = Conv2d(64 -> 32, 7x7, pad 3) of d(conv2 output) with the
// mirrored weights.  dy2 arrives as f16, channel-minor [band][clip][row][col][64] (apply_bwd_dx_f16_kernel; TERMS = 3: a
// second tensor of the same shape holds the low parts); tiles are conv1's 2 x 40 geometry over the 10 x 344 plane
// (CC<3, 2>), the 64 input channels run in 8 chunks of 8 (13 k-steps of 4 taps x 8 channels each) whose weight fragments
// (26 KB, 53 KB with the low parts) are shared by the 8 waves; every wave has a private 8 x 46-position patch.
// Epilogue: raw values (times the inverse weight pre-scale) through the Dropout keep-mask to
// [clip][band][32][rows][cols], as conv_kernel<3, 2, 2>.
// ------------------------------------------------------------------------------------------
template <int TERMS>   // dynamic LDS in 16-byte vectors, hi (and lo: TERMS 3) each: a weight chunk [step][nt][lane] + a patch per wave
constexpr size_t kConv2DgradF16Lds = (size_t)(TERMS == 3 ? 2 : 1) * (kF16Steps * CC<3, 2>::NT * 64 + kConvWaves * CC<3, 2>::PR * CC<3, 2>::PC) * 16;
template <int TERMS>
__global__ __launch_bounds__(kConvThreads) void conv2_dgrad_f16_kernel(const ConvParams p, const h16x8* __restrict__ dy_hi,
                                                                      const h16x8* __restrict__ dy_lo,
                                                                      const h16x8* __restrict__ wfrag16) {
  using C = CC<3, 2>;
  constexpr int MT = C::MT, NT = C::NT, NCH = 8, PR = C::PR, PC = C::PC, NPOS = PR * PC;
  constexpr int HL = TERMS == 3 ? 2 : 1;
  constexpr int WV = kF16Steps * NT * HL * 64;                          // vectors per weight chunk: [step][nt][hi(/lo)][lane]
  constexpr int NWF = (WV + kConvThreads - 1) / kConvThreads;
  constexpr int NPF = (NPOS + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  h16x8* wres = reinterpret_cast<h16x8*>(smem);       // [WV]
  h16x8* pa = wres + WV + wave * HL * NPOS;           // wave-private patch (hi, then lo)
  h16x8* pl = pa + NPOS;

  const int G = gridDim.x;
  const int wg = mst::xcd_remap(blockIdx.x, G);
  const int total_sets = p.nsub * p.sets_per_band;
  const int my_sets = wg < total_sets ? (total_sets - wg + G - 1) / G : 0;
  const int nq = my_sets * NCH;
  const int tpb = p.tiles_r * p.tiles_c;
  auto decode = [&](int q) __attribute__((always_inline)) {
    const int s = wg + (q / NCH) * G;
    Tile t;
    t.band = min(s / p.sets_per_band, p.nsub - 1);
    const int idx = (s - t.band * p.sets_per_band) * kConvWaves + wave;
    t.valid = (q < nq) && idx < p.B * tpb;
    t.clip = t.valid ? idx / tpb : 0;
    const int ti = t.valid ? idx - t.clip * tpb : 0;
    t.tc = ti / p.tiles_r;
    t.tr = ti - t.tc * p.tiles_r;
    return t;
  };
  const int kq = lane >> 4, ai = lane & 15, ag = ai >> 2, areg = ai & 3;
  int abase[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int e = 4 * t + areg, wv = e / C::WIN, pos = e % C::WIN;
    abase[t] = (pos / 5) * PC + 5 * (C::WPG * ag + wv) + pos % 5;
  }
  int toff[kF16Steps];
#pragma unroll
  for (int st = 0; st < kF16Steps; ++st) {
    const int tap = min(4 * st + kq, 48);
    toff[st] = (tap / 7) * PC + tap % 7;
  }

  h16x8 wreg[NWF], ph[NPF], pq[NPF];
  auto prefetch = [&](int q, const Tile& t) __attribute__((always_inline)) {
    const int chunk = q % NCH;
    const h16x8* wsrc = wfrag16 + ((size_t)t.band * NCH + chunk) * WV;
#pragma unroll
    for (int i = 0; i < NWF; ++i) wreg[i] = wsrc[min(tid + kConvThreads * i, WV - 1)];
    const int row0 = C::TROWS * t.tr - 3, col0 = C::TCOLS * t.tc - 3;
    const size_t plane = ((size_t)t.band * p.B + t.clip) * p.in_rows;
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int e = lane + 64 * i;
      const int r = e / PC, c = e - r * PC;
      const int rin = row0 + r, cin = col0 + c;
      const int rc = min(max(rin, 0), p.in_rows - 1), cl = min(max(cin, 0), p.in_cols - 1);
      const bool ok = t.valid && e < NPOS && rin == rc && cin == cl;
      const size_t v = ((plane + rc) * p.in_cols + cl) * NCH + chunk;
      const h16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      const h16x8 a = dy_hi[v];
      ph[i] = ok ? a : z;
      if (TERMS == 3) {
        const h16x8 b = dy_lo[v];
        pq[i] = ok ? b : z;
      }
    }
  };

  f32x4 acc[MT][NT];
  Tile cur{}, nxt = decode(0);
  if (nq > 0) prefetch(0, nxt);
  for (int q = 0; q < nq; ++q) {
    __syncthreads();  // every wave is done with the previous chunk's weights
#pragma unroll
    for (int i = 0; i < NWF; ++i)
      if (tid + kConvThreads * i < WV) wres[tid + kConvThreads * i] = wreg[i];
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int e = lane + 64 * i;
      if (e < NPOS) {
        pa[e] = ph[i];
        if (TERMS == 3) pl[e] = pq[i];
      }
    }
    __syncthreads();
    cur = nxt;
    nxt = decode(q + 1);
    prefetch(q + 1, nxt);   // lands while this chunk is on the MFMAs; past the end it re-reads valid memory
    const int chunk = q % NCH;
    if (chunk == 0) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int st = 0; st < kF16Steps; ++st) {
      h16x8 ah[MT], al[MT], bh[NT], bl[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        bh[n] = wres[((st * NT + n) * HL + 0) * 64 + lane];
        if (TERMS == 3) bl[n] = wres[((st * NT + n) * HL + 1) * 64 + lane];
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        ah[t] = pa[abase[t] + toff[st]];
        if (TERMS == 3) al[t] = pl[abase[t] + toff[st]];
      }
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          if (TERMS == 3) {
            acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], bh[n], acc[t][n], 0, 0, 0);
            acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bl[n], acc[t][n], 0, 0, 0);
          }
          acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bh[n], acc[t][n], 0, 0, 0);
        }
    }
    if (chunk == NCH - 1 && cur.valid) {
      const int j = lane & 15, g = lane >> 4;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int ch = n * 16 + j;
        const float wi = p.f16_winv[cur.band * C::COUT + ch];
        float* ob = p.out + (((size_t)cur.clip * p.nsub + cur.band) * C::COUT + ch) * (size_t)p.raw_rows * p.raw_cols;
        const unsigned char* mb = p.mask ? p.mask + (((size_t)cur.clip * p.nsub + cur.band) * C::COUT + ch) * (size_t)p.raw_rows * p.raw_cols
                                         : nullptr;
#pragma unroll
        for (int e = 0; e < 4 * MT; ++e) {
          const int wv = e / C::WIN, pos = e % C::WIN;
          const int row = C::TROWS * cur.tr + pos / 5, col = C::TCOLS * cur.tc + 5 * (C::WPG * g + wv) + pos % 5;
          if (row < p.raw_rows && col < p.raw_cols) {
            const size_t o = (size_t)row * p.raw_cols + col;
            float v = acc[e >> 2][n][e & 3] * wi;
            if (mb) v = mb[o] ? v * p.mask_scale : 0.f;
            ob[o] = v;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Pass B of the pool / ReLU / FiLM / BatchNorm backward for the f16 training modes (pass A = apply_bwd_reduce_kernel,
// unchanged): d(conv output) is written ONCE, as float16 (TERMS = 3: hi and lo), directly in the operand layout of
// wgrad_f16_kernel --
//     dyg[band][group of 8 clips][tile row][tile col][half][M-tile][slot e'][hi(/lo)][lane][8 clips]     (16-byte vectors)
// (TERMS = 1: one half holding all NV slots; TERMS = 3: two halves of NV / 2 slots, the unit the weight gradient stages)
// -- so the weight gradient stages its A operand with plain 16-byte copies.  A thread owns one lane-unit (band, clip
// group, tile, M-tile, lane) and walks the group's 8 clips; clips past the batch and positions outside the plane are 0.
// Layer 2 also writes the channel-minor copy [band][clip][row][col][64] (+ its low parts) that conv2_dgrad_f16_kernel
// convolves.
// ------------------------------------------------------------------------------------------
template <int LAYER, int SUB, int TERMS>
__global__ __launch_bounds__(256) void apply_bwd_dx_f16_kernel(const ApplyBwdParams p, long long units, h16x8* __restrict__ dyg,
                                                                int CG) {
  using C = CC<LAYER, SUB>;
  constexpr int NT = C::NT, NV = 4 * C::MT;
  constexpr int HL = TERMS == 3 ? 2 : 1, NH = TERMS == 3 ? 2 : 1, NVH = NV / NH;
  // a thread takes FOUR of the group's eight clips (`half`): half the output registers of an 8-clip thread, twice the threads
  // -- the two halves of a 16-byte vector are written by neighbouring threads of one wave (8 bytes each, L2 merges them)
  const long long u2 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u2 >= 2 * units) return;
  const int half = (int)((u2 >> 6) & 1);
  const long long u = ((u2 >> 7) << 6) | (u2 & 63);
  const int lane = (int)(u & 63), n = (int)((u >> 6) % NT);
  long long tile = (u >> 6) / NT;
  const int tc = (int)(tile % p.tiles_c);
  tile /= p.tiles_c;
  const int tr = (int)(tile % p.tiles_r);
  tile /= p.tiles_r;
  const int cg = (int)(tile % CG), band = (int)(tile / CG);
  const int j = lane & 15, g = lane >> 4, ch = n * 16 + j;
  const float2 ms = p.bnstat[band * C::COUT + ch];
  const float kk = p.bn_w[band * C::COUT + ch] * ms.y;
  const double cnt = bwd_count(p);
  const double m1 = mst::det_get(p.sums[((size_t)band * C::COUT + ch) * 2]) / cnt,
               m2 = mst::det_get(p.sums[((size_t)band * C::COUT + ch) * 2 + 1]) / cnt;
  h16x4 out[NV], outl[TERMS == 3 ? NV : 1];
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    out[e] = h16x4{0, 0, 0, 0};
    if constexpr (TERMS == 3) outl[e] = h16x4{0, 0, 0, 0};
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int clip = 8 * cg + 4 * half + k;
    if (clip < p.B) {
      const float2 ac = p.aff[((size_t)clip * p.nsub + band) * C::COUT + ch];
      const float gf = p.film[((size_t)clip * p.nsub + band) * 192 + p.goff + ch];
      const size_t uu = ((((size_t)clip * p.nsub + band) * p.tiles_r + tr) * p.tiles_c + tc) * NT + n;
      float v[NV], df[NV];
      load_unit<NV>(p.yraw, p.y_scale, band, uu * 64 + lane, v);
      unit_df<LAYER, SUB>(p, v, ac, clip, band, ch, tr, tc, g, df);
      const size_t plane = ((size_t)band * p.B + clip) * (size_t)p.rows * p.cols * C::COUT + ch;
      _Float16* dyh = LAYER == 2 && p.dy_h16 ? p.dy_h16 + plane : nullptr;
      _Float16* dyl = LAYER == 2 && TERMS == 3 && p.dy_h16 ? p.dy_h16 + (size_t)p.nsub * p.B * p.rows * p.cols * C::COUT + plane : nullptr;
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        int row, col;
        unit_geometry<LAYER, SUB>(tr, tc, g, e, row, col);
        if (row < p.rows && col < p.cols) {
          const float zh = (v[e] - ms.x) * ms.y;
          const float d = kk * (float)((double)gf * (double)df[e] - m1 - (double)zh * m2);
          const _Float16 h = to_f16_sat(d);
          out[e][k] = h;
          if (LAYER == 2 && dyh) dyh[((size_t)row * p.cols + col) * C::COUT] = h;
          if constexpr (TERMS == 3) {
            const _Float16 l = (_Float16)(d - (float)h);
            outl[e][k] = l;
            if (LAYER == 2 && dyl) dyl[((size_t)row * p.cols + col) * C::COUT] = l;
          }
        }
      }
    }
  }
  h16x4* dst = reinterpret_cast<h16x4*>(dyg + ((((size_t)band * CG + cg) * p.tiles_r + tr) * p.tiles_c + tc) * (size_t)(NT * NV * HL * 64) + lane) + half;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    const size_t o = ((((size_t)(e / NVH) * NT + n) * NVH + e % NVH) * HL) * 64;   // in 16-byte vectors
    dst[o * 2] = out[e];
    if constexpr (TERMS == 3) dst[(o + 64) * 2] = outl[e];
  }
}

// ------------------------------------------------------------------------------------------
// Weight gradients on the f16 matrix cores:  dW[band][co][ci][tap] = sum over clips and positions of dy[co][pos] * x[ci][pos + tap].
// K = positions x CLIPS.  A k-step of v_mfma_f32_16x16x32_f16 covers the positions P(g, e) of the four lane groups for one
// accumulator slot e (the fp32 kernels' k-step) times EIGHT clips: lane (i, g) holds, for output channel i, the eight
// clips' dy at P(g, e) (A operand), lane (n, g) the eight clips' x[ci_n] at P(g, e) + tap_n (B operand).  With the clip
// index minor in LDS -- patch [ci][row][col][8 clips], dy tile [M-tile][e][lane][8 clips] -- both operands are ONE aligned
// 16-byte LDS read whatever the tap shift (a position-minor K would need unaligned 2-byte gathers for B).
// A workgroup walks a contiguous range of (band, group of 8 clips, tile) items; its 8 waves own different N-tiles of the
// 392 (ci, tap) columns (24 full tiles round-robin + the half-empty 25th dealt by k-steps, as in the fp32 kernels) and keep
// MT x 4 accumulator tiles until the band changes.  dy arrives as f16 in exactly this layout from apply_bwd_dx_f16_kernel
// (already times the backward scale); x comes from the fp32 activations and is rounded to f16 (TERMS = 3: split into hi +
// lo) when it is staged.  LAYER 2: the 32 input channels are 4 chunks of 8, one per member of a group of 4 workgroups that
// walk the same items side by side (dy is found in L2 by three of them); x = pool1 is multiplied by the band's forward
// range scale.  TERMS = 3 doubles both operands, which no longer fit the 160 KB of LDS together: the dy tile is staged in
// two halves of NV / 2 k-steps.  The global loads of the next stage (second half, or the next item) are issued before the
// MFMAs of the current one and staged after them.
// ------------------------------------------------------------------------------------------
struct WgradF16Params {
  const void* x;             // LAY 0: fp32 (reference layout / pool1); LAY 2: float16 high parts, channel-minor
  const h16x8* dy;            // apply_bwd_dx_f16_kernel's layout
  mst::DetAcc* dw;            // LAYER 1: [nsub][32][392]; LAYER 2: [nsub][64][1568]
  const float* xscale;        // LAYER 2: forward range scale table [B][nsub][2] (constant over clips in training), or NULL
  int B, nsub, tiles_r, tiles_c;
  int in_rows, in_cols, in_cstride, in_bandoff;
  long long in_clipstride;
  // LAY 2 (LAYER 1 only): x = the high parts of stage A's float16 log-mel, channel-minor [B][frames][cm_mels][8] (mst.h
  // MST_LOGMEL_CM16), x_lo the low parts (TERMS 3); in_clipstride then counts float16 elements
  const void* x_lo;
  int cm_mels, cm_overlap;
};

// LAY 0: x is fp32 in the reference layout -- 8 scalar loads (one per clip) per patch position and channel, rounded to float16
//        (hi / lo) while it is staged.
// LAY 2: x arrives as float16 planes, channel-minor: a thread owns ONE patch position, loads the 8 channels of each of the 8
//        clips as one 16-byte vector (8 rows of a frame = 128 contiguous bytes per 8 lanes), transposes the 8 x 8 block in
//        registers to clip-minor and writes the 8 channels' vectors: a sixth of the load instructions, no conversions; the same
//        bits as LAY 0 produces (stage A's hi / lo ARE f16(x), f16(x - hi)).
// LAY 3: (LAYER 2) x = the range-scaled float16 pool1 the training forward wrote for conv2, [B][nsub][rows][cols][32] (+ low
//        parts in x_lo): the same one-position-per-thread loader on this workgroup's 8-channel chunk; the fp32 pool1 is not
//        needed at all (the forward pass then does not write it).
template <int LAYER, int TERMS>   // dynamic LDS in 16-byte vectors: the patch [hi(/lo)][8 ci][PR][PC] + the dy vectors [MTN][NV][64]
constexpr size_t kWgradF16Lds = (size_t)((TERMS == 3 ? 2 : 1) * 8 * (LAYER == 1 ? 8 * 46 : 14 * 14) + (LAYER == 1 ? 2 * 20 : 4 * 16) * 64) * 16;
template <int LAYER, int TERMS, int LAY = 0>
__global__ __launch_bounds__(kConvThreads) void wgrad_f16_kernel(const WgradF16Params p) {
  static_assert(LAY == 0 || (LAY == 2 && LAYER == 1) || (LAY == 3 && LAYER == 2),
                "channel-minor loaders: LAY 2 reads stage A's log-mel planes (conv1), LAY 3 the forward pass's pool1 planes (conv2)");
  constexpr int MTN = LAYER == 1 ? 2 : 4;               // M-tiles of 16 output channels
  constexpr int NV = LAYER == 1 ? 20 : 16;              // accumulator slots = k-steps per item
  constexpr int HL = TERMS == 3 ? 2 : 1, NH = TERMS == 3 ? 2 : 1, NVH = NV / NH;
  constexpr int PR = LAYER == 1 ? 8 : 14, PC = LAYER == 1 ? 46 : 14, NPOS = PR * PC;
  constexpr int NX = 8 * NPOS;                           // patch positions (8 input channels); HL vectors each: [hi(/lo)][NX]
  constexpr int XIT = (NX + kConvThreads - 1) / kConvThreads;
  constexpr int NA = MTN * NVH * HL * 64;                // dy vectors of one half
  constexpr int DIT = (NA + kConvThreads - 1) / kConvThreads;
  constexpr int NTN = 25, KF = 3, KN = KF + 1, NW = 8, NCHK = LAYER == 1 ? 1 : 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  h16x8* xp = reinterpret_cast<h16x8*>(smem);           // [hi(/lo)][8 ci][PR][PC]
  h16x8* ap = xp + HL * NX;                              // [MTN][NVH][hi(/lo)][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int G = gridDim.x, wg = mst::xcd_remap(blockIdx.x, G);
  const int CG = (p.B + 7) / 8;
  const int tpb = CG * p.tiles_r * p.tiles_c;            // items per band
  const int total = p.nsub * tpb;
  const int my_chunk = wg & (NCHK - 1), rg = wg / NCHK, RG = G / NCHK;
  const int s_begin = (int)((long long)rg * total / RG), s_end = (int)((long long)(rg + 1) * total / RG);
  if (rg >= RG || s_begin >= s_end) return;

  // per N-tile lane constants: patch offset of column (ci, tap) plus this lane group's position offset
  const int goff = LAYER == 1 ? 10 * g : (4 * (g >> 1)) * PC + 4 * (g & 1);
  int nbase[KF];
#pragma unroll
  for (int k = 0; k < KF; ++k) {
    const int nidx = (wave + NW * k) * 16 + j, ci = nidx / 49, tap = nidx % 49;
    nbase[k] = ci * NPOS + (tap / 7) * PC + tap % 7 + goff;
  }
  // LAYER 2, LOW tiles (last tile row with at most 2 output rows): the two lower lane groups, whose slots are padding there, take
  // the tile's second row -- A = slot 4 + e of the lane 32 below, B = the patch one row down -- 4 k-steps instead of 8
  // (see conv2_wgrad_kernel)
  const int glow = LAYER == 2 ? (g >> 1) * PC + 4 * (g & 1) - goff : 0;
  const int sh_nidx = (NTN - 1) * 16 + j;
  const bool sh_ok = sh_nidx < 392;
  const int sh_base = (sh_ok ? (sh_nidx / 49) * NPOS + ((sh_nidx % 49) / 7) * PC + (sh_nidx % 49) % 7 : 0) + goff;
  auto eoff = [](int e) __attribute__((always_inline)) {   // patch offset of accumulator slot e inside the lane group's window
    if constexpr (LAYER == 1) {
      const int wv = e / 10, pos = e % 10;
      return (pos / 5) * PC + 5 * wv + pos % 5;
    } else {
      return (e >> 2) * PC + (e & 3);
    }
  };

  struct Item {
    int band, cg, tr, tc;
  };
  auto decode = [&](int s) __attribute__((always_inline)) {
    Item t;
    t.band = s / tpb;
    int r = s - t.band * tpb;
    t.cg = r / (p.tiles_r * p.tiles_c);
    r -= t.cg * p.tiles_r * p.tiles_c;
    t.tr = r / p.tiles_c, t.tc = r - t.tr * p.tiles_c;
    return t;
  };

  float xv[LAY == 0 ? XIT : 1][8];
  h16x8 xh[LAY >= 2 ? 8 : 1], xl[LAY >= 2 && TERMS == 3 ? 8 : 1];   // LAY 2 / 3: [clip] x 8 channels of this thread's position
  h16x8 dv[DIT];
  unsigned xmask = 0;      // bit it: this thread's patch position of iteration `it` lies inside the image
  static_assert(LAY == 0 || NPOS <= kConvThreads, "one patch position per thread");
  auto issue_x = [&](const Item& t) __attribute__((always_inline)) {
    const int clip0 = 8 * t.cg;
    const int row0 = (LAYER == 1 ? 2 : 8) * t.tr - 3, col0 = (LAYER == 1 ? 40 : 8) * t.tc - 3;
    if constexpr (LAY >= 2) {   // LAY 2: position u = 8 c + r (the 8 rows of a frame are 128 contiguous bytes); LAY 3: u = PC r + c
      const int u = min(tid, NPOS - 1), r = LAY == 2 ? (u & 7) : u / PC, c = LAY == 2 ? (u >> 3) : u % PC;
      const int rin = row0 + r, cin = col0 + c;
      const int rc = min(max(rin, 0), p.in_rows - 1), cl = min(max(cin, 0), p.in_cols - 1);
      xmask = (rin == rc && cin == cl) ? 1u : 0u;
      const size_t off = LAY == 2 ? ((size_t)cl * p.cm_mels + (size_t)(t.band * p.cm_overlap + rc)) * 8   // float16 elements inside a clip
                                  : (((size_t)t.band * p.in_rows + rc) * p.in_cols + cl) * 32 + 8 * my_chunk;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const size_t o = (size_t)min(clip0 + k, p.B - 1) * p.in_clipstride + off;
        xh[k] = *reinterpret_cast<const h16x8*>(reinterpret_cast<const _Float16*>(p.x) + o);
        if constexpr (TERMS == 3) xl[k] = *reinterpret_cast<const h16x8*>(static_cast<const _Float16*>(p.x_lo) + o);
      }
    } else {
      const float* xb = static_cast<const float*>(p.x) + (size_t)t.band * p.in_bandoff + (size_t)(8 * my_chunk) * p.in_cstride;
      xmask = 0;
#pragma unroll
      for (int it = 0; it < XIT; ++it) {
        const int u = min(tid + kConvThreads * it, NX - 1);
        const int ci = u / NPOS, pos = u - ci * NPOS, r = pos / PC, c = pos - r * PC;
        const int rin = row0 + r, cin = col0 + c;
        const int rc = min(max(rin, 0), p.in_rows - 1), cl = min(max(cin, 0), p.in_cols - 1);
        if (rin == rc && cin == cl) xmask |= 1u << it;
        const float* src = xb + (size_t)ci * p.in_cstride + (size_t)rc * p.in_cols + cl;
#pragma unroll
        for (int k = 0; k < 8; ++k) xv[it][k] = src[(size_t)min(clip0 + k, p.B - 1) * p.in_clipstride];
      }
    }
  };
  auto issue_a = [&](const Item& t, int half) __attribute__((always_inline)) {
    const h16x8* dsrc = p.dy + (((((size_t)t.band * CG + t.cg) * p.tiles_r + t.tr) * p.tiles_c + t.tc) * NH + half) * (size_t)NA;
#pragma unroll
    for (int it = 0; it < DIT; ++it) dv[it] = dsrc[min(tid + kConvThreads * it, NA - 1)];
  };
  auto stage_x = [&](const Item& t) __attribute__((always_inline)) {
    if constexpr (LAY >= 2) {
      if (tid < NPOS) {
        const int pos = LAY == 2 ? (tid & 7) * PC + (tid >> 3) : tid;
        const bool ok = xmask & 1u;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {   // 8 x 8 transposition in registers: [clip][channel] -> [channel][clip]
          h16x8 h, l;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            h[k] = ok ? xh[k][ci] : (_Float16)0.f;
            if constexpr (TERMS == 3) l[k] = ok ? xl[k][ci] : (_Float16)0.f;
          }
          xp[ci * NPOS + pos] = h;
          if constexpr (TERMS == 3) xp[NX + ci * NPOS + pos] = l;
        }
      }
    } else {
      float xs = 1.0f;
      if (LAYER == 2 && p.xscale) xs = p.xscale[(size_t)t.band * 2];
#pragma unroll
      for (int it = 0; it < XIT; ++it) {
        const int u = tid + kConvThreads * it;
        h16x8 h, l;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float v = ((xmask >> it) & 1u) ? fminf(fmaxf(xv[it][k] * xs, -65504.f), 65504.f) : 0.f;
          h[k] = (_Float16)v;
          if (TERMS == 3) l[k] = (_Float16)(v - (float)h[k]);
        }
        if (u < NX) {
          xp[u] = h;
          if (TERMS == 3) xp[NX + u] = l;
        }
      }
    }
  };
  auto stage_a = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < DIT; ++it) {
      const int u = tid + kConvThreads * it;
      if (u < NA) ap[u] = dv[it];
    }
  };

  f32x4 acc[MTN][KN];
#pragma unroll
  for (int c = 0; c < MTN; ++c)
#pragma unroll
    for (int k = 0; k < KN; ++k) acc[c][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto flush = [&](int band) __attribute__((always_inline)) {
    float us = 1.0f;
    if (LAYER == 2 && p.xscale) us = p.xscale[(size_t)band * 2 + 1];
#pragma unroll
    for (int k = 0; k < KN; ++k) {
      const int nt = k < KF ? wave + NW * k : NTN - 1;
      const int nidx = nt * 16 + j;
      if (nidx < 392) {
#pragma unroll
        for (int c = 0; c < MTN; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = 16 * c + 4 * g + r;
            mst::DetAcc* d = LAYER == 1 ? p.dw + ((size_t)band * 32 + co) * 392 + nidx
                                        : p.dw + ((size_t)band * 64 + co) * 1568 + my_chunk * 392 + nidx;
            mst::det_add(d, (double)(acc[c][k][r] * us));
            acc[c][k][r] = 0.f;
          }
      }
    }
  };
  // the k-steps of one staged half: slots e = e0 .. e0 + NVH - 1
  auto compute = [&](int e0, bool low) __attribute__((always_inline)) {
#pragma unroll
    for (int eh = 0; eh < NVH; ++eh) {
      const int e = e0 + eh;
      if (LAYER == 2 && e >= 4 && low) break;   // wave-uniform: only rows 8 tr, 8 tr + 1 exist -- 16 positions, 4 k-steps (see glow)
      const bool lw = LAYER == 2 && low;
      const int sl = lw ? 4 * (lane >> 5) + eh : eh, la = lw ? (lane & 31) : lane;   // (low tiles live in the first staged half: e0 = 0)
      h16x8 ah[MTN], al[MTN];
#pragma unroll
      for (int c = 0; c < MTN; ++c) {
        ah[c] = ap[((c * NVH + sl) * HL + 0) * 64 + la];
        if (TERMS == 3) al[c] = ap[((c * NVH + sl) * HL + 1) * 64 + la];
      }
      const int eo = lw ? glow + e : eoff(e);
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        const h16x8 bh = xp[nbase[k] + eo];
        h16x8 bl;
        if (TERMS == 3) bl = xp[NX + nbase[k] + eo];
#pragma unroll
        for (int c = 0; c < MTN; ++c) {
          if (TERMS == 3) {
            acc[c][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[c], bh, acc[c][k], 0, 0, 0);
            acc[c][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[c], bl, acc[c][k], 0, 0, 0);
          }
          acc[c][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[c], bh, acc[c][k], 0, 0, 0);
        }
      }
      // the shared 25th N-tile: k-step e belongs to wave e % 8
      if ((e & (NW - 1)) == wave) {
        const h16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        const h16x8 bv = xp[sh_base + eo];
        const h16x8 bh = sh_ok ? bv : z;
        h16x8 bl = z;
        if (TERMS == 3) {
          const h16x8 bw = xp[NX + sh_base + eo];
          bl = sh_ok ? bw : z;
        }
#pragma unroll
        for (int c = 0; c < MTN; ++c) {
          if (TERMS == 3) {
            acc[c][KF] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[c], bh, acc[c][KF], 0, 0, 0);
            acc[c][KF] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[c], bl, acc[c][KF], 0, 0, 0);
          }
          acc[c][KF] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[c], bh, acc[c][KF], 0, 0, 0);
        }
      }
    }
  };

  Item cur = decode(s_begin), nxt = cur;
  int cur_band = cur.band;
  issue_x(cur);
  issue_a(cur, 0);
  stage_x(cur);
  stage_a();
  __syncthreads();
  for (int s = s_begin; s < s_end; ++s) {
    if (s + 1 < s_end) nxt = decode(s + 1);
    if (cur.band != cur_band) {
      flush(cur_band);
      cur_band = cur.band;
    }
    const bool low = LAYER == 2 && 8 * __builtin_amdgcn_readfirstlane(cur.tr) + 2 >= p.in_rows;
#pragma unroll
    for (int half = 0; half < NH; ++half) {
      const bool last = half + 1 == NH;
      // loads of the next stage, then this stage's MFMAs, then the next stage goes into LDS
      if (!last) {
        issue_a(cur, half + 1);
      } else {
        issue_x(nxt);   // past the end: re-reads the last item (never staged)
        issue_a(nxt, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      compute(half * NVH, low);
      __syncthreads();            // every wave is done reading this stage's operands
      if (!last) {
        stage_a();
      } else if (s + 1 < s_end) {
        stage_x(nxt);
        stage_a();
      }
      __syncthreads();
    }
    cur = nxt;
  }
  flush(cur_band);
}
