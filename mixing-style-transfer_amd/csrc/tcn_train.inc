// Stage C, training: train-mode forward (BatchNorm on batch statistics) and the full backward of the TCN mixer.
// Included at the end of tcn.hip: it reuses the implicit-GEMM convolution (RAW instantiation), the 1x1 kernels, the
// private [B][T][HP] layout and the handle.
//
// Forward, per block and layer: u = conv + bias (RAW convolution) -> per-channel sum / sum of squares over (B, T)
// (double partials per time chunk, added in a fixed order) -> S, C per (clip, channel) from the batch statistics, the
// BatchNorm affine and FiLM (double, rounded once) -> f = fmaf(S, u, C), LeakyReLU and the residual in the block's order.
// Saved for the backward: h_0 .. h_nb, u of every convolution, S / C and mean / rstd: (3 nb + 1) * HP * 4 bytes per sample.
//
// Backward, per block in reverse and per layer (2 then 1), with df = dout * slope(f), n = (u - mean) * rstd:
//   pass 1   s1 = sum_t df, s2 = sum_t df n per (clip, channel)              tcn_bwd_reduce_kernel
//   fold     dbeta = s1, dgamma = bn_w s2 + bn_b s1, d bn_b = sum_b gamma s1, d bn_w = sum_b gamma s2,
//            m1, m2 = those two sums / (B T)                                  tcn_bwd_coef_kernel
//   pass 2   du = rstd bn_w (gamma df - m1 - n m2), d bias = sum du           tcn_bwd_du_kernel
//   weight gradient on the fp32 MFMA, time split over waves, partials added in double in a fixed order
//   input gradient = the RAW convolution on du with the transposed, tap-reversed weights, added to the running dh
// Every reduction has a fixed order and no float atomics: two runs give the same bits.

namespace mst {
namespace {

constexpr int kRowsChunk = 1024;   // time samples per workgroup of the row reductions
constexpr int kRowsWave = 512;     // time samples per wave of the weight gradient: one fp32 chain of 128 MFMAs
constexpr int kProjQ = 10;         // sums of tcn_proj_grad_kernel

// The LeakyReLU argument and its branch: the ONE definition the forward, both backward passes and the mask dump share.
__device__ __forceinline__ float tcn_act_arg(float S, float u, float C, float r, bool res_first) {
  const float f = fmaf(S, u, C);
  return res_first ? f + r : f;
}
__device__ __forceinline__ bool tcn_slope_one(float f) { return f > 0.f; }

// Thread (c, slot) of a 256-thread workgroup holds NQ partial sums of channel c; out[q][c] = sum over the slots in
// slot order.  All 256 threads call it (threads beyond nslots * HP pass active = false).
template <int NQ>
__device__ __forceinline__ void tcn_block_reduce(const double (&acc)[NQ], int c, int slot, int nslots, int HP, bool active,
                                                 double* __restrict__ out) {
  __shared__ double red[NQ * 256];
  if (active)
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[(q * nslots + slot) * HP + c] = acc[q];
  __syncthreads();
  for (int i = threadIdx.x; i < NQ * HP; i += 256) {
    const int q = i / HP, cc = i - q * HP;
    double s = 0.0;
    for (int sl = 0; sl < nslots; ++sl) s += red[(q * nslots + sl) * HP + cc];
    out[i] = s;
  }
}

// part[b][chunk][2][HP] = sum, sum of squares of u over the chunk's time samples.  grid (chunks, B).
__global__ __launch_bounds__(256) void tcn_stats_kernel(const float* __restrict__ u, double* __restrict__ part, int T, int HP) {
  const int nslots = 256 / HP, c = threadIdx.x % HP, slot = threadIdx.x / HP;
  const bool active = slot < nslots;
  const int t0 = blockIdx.x * kRowsChunk, t1 = min(T, t0 + kRowsChunk);
  const float* ub = u + (size_t)blockIdx.y * T * HP;
  double acc[2] = {0.0, 0.0};
  if (active)
    for (int t = t0 + slot; t < t1; t += nslots) {
      const double v = (double)ub[(size_t)t * HP + c];
      acc[0] += v;
      acc[1] = fma(v, v, acc[1]);
    }
  tcn_block_reduce<2>(acc, c, slot, nslots, HP, active, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * HP);
}

// One thread per channel: batch mean and biased variance from the P partials (fixed order), then S, C of every clip.
// mean_o / var_o: [H] of this layer; st: [2][HP] = mean, rstd; sc: [B][2][HP]; bw, bb: [H]; film: this block's
// [B][nb][4][H] tensor offset to (block, layer) or NULL.
__global__ void tcn_stats_fold_kernel(const double* __restrict__ part, int P, double count, const float* __restrict__ bw,
                                      const float* __restrict__ bb, const float* __restrict__ film, long long film_stride, int B,
                                      int H, int HP, float eps, float* __restrict__ mean_o, float* __restrict__ var_o,
                                      float* __restrict__ st, float* __restrict__ sc) {
  const int c = threadIdx.x;
  if (c >= HP) return;
  if (c >= H) {   // padded channel: stays exactly zero
    st[c] = 0.f, st[HP + c] = 0.f;
    for (int b = 0; b < B; ++b) sc[(size_t)b * 2 * HP + c] = 0.f, sc[(size_t)b * 2 * HP + HP + c] = 0.f;
    return;
  }
  double s = 0.0, q = 0.0;
  for (int p = 0; p < P; ++p) s += part[(size_t)p * 2 * HP + c], q += part[(size_t)p * 2 * HP + HP + c];
  const double m = s / count;
  double v = q / count - m * m;
  if (v < 0.0) v = 0.0;
  const float mf = (float)m, vf = (float)v;
  mean_o[c] = mf, var_o[c] = vf;
  const float rstd = (float)(1.0 / sqrt((double)vf + (double)eps));
  st[c] = mf, st[HP + c] = rstd;
  const double S0 = (double)bw[c] * (double)rstd, C0 = (double)bb[c] - (double)mf * S0;
  for (int b = 0; b < B; ++b) {
    double S = S0, Cc = C0;
    if (film) {
      const float* f = film + (size_t)b * film_stride + c;
      S = (double)f[0] * S0;
      Cc = (double)f[0] * C0 + (double)f[H];
    }
    sc[(size_t)b * 2 * HP + c] = (float)S;
    sc[(size_t)b * 2 * HP + HP + c] = (float)Cc;
  }
}

// out = act(S u + C) with the residual in the order of `epi` (the inference epilogue's arithmetic).  One float4 per thread;
// out may be u or res (an element is read and written by the same thread).
__global__ __launch_bounds__(256) void tcn_apply_kernel(const float* u, const float* __restrict__ sc, const float* res,
                                                        float* out, long long T, int HP, int epi) {
  const long long per_clip = T * (HP / 4);
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per_clip) return;
  const long long b = blockIdx.y;
  const int c = (int)(i % (HP / 4)) * 4;
  const size_t at = (size_t)b * T * HP + (size_t)i * 4;
  const float* scb = sc + b * 2 * HP;
  const f32x4 S = *reinterpret_cast<const f32x4*>(scb + c), Cc = *reinterpret_cast<const f32x4*>(scb + HP + c);
  f32x4 v = *reinterpret_cast<const f32x4*>(u + at), r = f32x4{0.f, 0.f, 0.f, 0.f};
  if (epi != EPI_ACT) r = *reinterpret_cast<const f32x4*>(res + at);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float z = leaky(tcn_act_arg(S[q], v[q], Cc[q], r[q], epi == EPI_RES_THEN_ACT));
    if (epi == EPI_ACT_THEN_RES) z += r[q];
    v[q] = z;
  }
  *reinterpret_cast<f32x4*>(out + at) = v;
}

// Pass 1.  part[b][chunk][2][HP] = sum df, sum df n over the chunk.  res != NULL: the activation follows the residual sum.
__global__ __launch_bounds__(256) void tcn_bwd_reduce_kernel(const float* __restrict__ dout, const float* __restrict__ u,
                                                             const float* __restrict__ sc, const float* __restrict__ st,
                                                             const float* __restrict__ res, double* __restrict__ part, int T, int HP) {
  const int nslots = 256 / HP, c = threadIdx.x % HP, slot = threadIdx.x / HP;
  const bool active = slot < nslots;
  const int t0 = blockIdx.x * kRowsChunk, t1 = min(T, t0 + kRowsChunk);
  const size_t base = (size_t)blockIdx.y * T * HP;
  double acc[2] = {0.0, 0.0};
  if (active) {
    const float S = sc[(size_t)blockIdx.y * 2 * HP + c], Cc = sc[(size_t)blockIdx.y * 2 * HP + HP + c];
    const float mean = st[c], rstd = st[HP + c];
    for (int t = t0 + slot; t < t1; t += nslots) {
      const size_t at = base + (size_t)t * HP + c;
      const float uu = u[at], d = dout[at];
      const float f = tcn_act_arg(S, uu, Cc, res ? res[at] : 0.f, res != nullptr);
      const float df = tcn_slope_one(f) ? d : kSlope * d;
      acc[0] += (double)df;
      acc[1] = fma((double)df, (double)((uu - mean) * rstd), acc[1]);
    }
  }
  tcn_block_reduce<2>(acc, c, slot, nslots, HP, active, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * HP);
}

// One thread per channel, after pass 1.  coef[b][HP] = rstd bn_w gamma_b; c12[2][HP] = rstd bn_w m1, rstd bn_w m2.
// dbw / dbb: [H] of this layer.  film / dfilm: offset to (block, layer) or NULL.
__global__ void tcn_bwd_coef_kernel(const double* __restrict__ part, int B, int nchunk, double count, const float* __restrict__ bw,
                                    const float* __restrict__ bb, const float* __restrict__ st, const float* __restrict__ film,
                                    float* __restrict__ dfilm, long long film_stride, int H, int HP, float* __restrict__ coef,
                                    float* __restrict__ c12, float* __restrict__ dbw, float* __restrict__ dbb) {
  const int c = threadIdx.x;
  if (c >= HP) return;
  if (c >= H) {
    for (int b = 0; b < B; ++b) coef[(size_t)b * HP + c] = 0.f;
    c12[c] = 0.f, c12[HP + c] = 0.f;
    return;
  }
  const double w = (double)bw[c], bias = (double)bb[c], rw = (double)st[HP + c] * w;
  double G1 = 0.0, G2 = 0.0;
  for (int b = 0; b < B; ++b) {
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nchunk; ++k) {
      const double* p = part + ((size_t)b * nchunk + k) * 2 * HP;
      s1 += p[c], s2 += p[HP + c];
    }
    double gamma = 1.0;
    if (film) gamma = (double)film[(size_t)b * film_stride + c];
    if (dfilm) {
      dfilm[(size_t)b * film_stride + c] = (float)(w * s2 + bias * s1);
      dfilm[(size_t)b * film_stride + H + c] = (float)s1;
    }
    G1 += gamma * s1, G2 += gamma * s2;
    coef[(size_t)b * HP + c] = (float)(rw * gamma);
  }
  dbb[c] = (float)G1, dbw[c] = (float)G2;
  c12[c] = (float)(rw * (G1 / count)), c12[HP + c] = (float)(rw * (G2 / count));
}

// Pass 2.  du = coef df - c1 - c2 n; part[b][chunk][HP] = sum of du over the chunk.  write_df: dout := df in place (the
// plain block's gradient behind its activation, which is also the gradient of the skip path).
__global__ __launch_bounds__(256) void tcn_bwd_du_kernel(float* dout, const float* __restrict__ u, const float* __restrict__ sc,
                                                         const float* __restrict__ st, const float* __restrict__ res,
                                                         const float* __restrict__ coef, const float* __restrict__ c12,
                                                         float* __restrict__ du, double* __restrict__ part, int T, int HP,
                                                         int write_df) {
  const int nslots = 256 / HP, c = threadIdx.x % HP, slot = threadIdx.x / HP;
  const bool active = slot < nslots;
  const int t0 = blockIdx.x * kRowsChunk, t1 = min(T, t0 + kRowsChunk);
  const size_t base = (size_t)blockIdx.y * T * HP;
  double acc[1] = {0.0};
  if (active) {
    const float S = sc[(size_t)blockIdx.y * 2 * HP + c], Cc = sc[(size_t)blockIdx.y * 2 * HP + HP + c];
    const float mean = st[c], rstd = st[HP + c], ca = coef[(size_t)blockIdx.y * HP + c], c1 = c12[c], c2 = c12[HP + c];
    for (int t = t0 + slot; t < t1; t += nslots) {
      const size_t at = base + (size_t)t * HP + c;
      const float uu = u[at], d = dout[at];
      const float f = tcn_act_arg(S, uu, Cc, res ? res[at] : 0.f, res != nullptr);
      const float df = tcn_slope_one(f) ? d : kSlope * d;
      const float v = fmaf(-c2, (uu - mean) * rstd, fmaf(ca, df, -c1));
      du[at] = v;
      if (write_df) dout[at] = df;
      acc[0] += (double)v;
    }
  }
  tcn_block_reduce<1>(acc, c, slot, nslots, HP, active, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * HP);
}

// out[c] = sum over the P partials of part[p][HP] (fixed order), c < H.
__global__ void tcn_colsum_kernel(const double* __restrict__ part, int P, int H, int HP, float* __restrict__ out) {
  const int c = threadIdx.x;
  if (c >= H) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += part[(size_t)p * HP + c];
  out[c] = (float)s;
}

// Weight gradient of one convolution: D[out channel][in channel] += du[t][out] * in[t + off0 + tap * dil][in], time as the
// MFMA's K index (lane group g supplies sample t + g of a step of four).  One wave owns kRowsWave samples of one clip and
// one 16 x 16 tile of (out, in) channels for all taps; grid (wave chunks / 4, NT * NT, B).  Samples of `in` outside [0, T)
// are zeros (clamped address + select), and a tap whose strip lies wholly outside the clip is skipped: exact zeros.
// part: [b][wave chunk][tap][tile][64 lanes][4].
__global__ __launch_bounds__(256) void tcn_wgrad_kernel(const float* __restrict__ du, const float* __restrict__ in,
                                                        float* __restrict__ part, int T, int HP, int K, int dil, int off0,
                                                        int nwchunk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int wc = blockIdx.x * 4 + wave;
  if (wc >= nwchunk) return;
  const int NT = HP / 16, ot = blockIdx.y / NT, it = blockIdx.y % NT;
  const int t0 = wc * kRowsWave, t1 = min(T, t0 + kRowsWave);
  const float* dub = du + (size_t)blockIdx.z * T * HP + ot * 16 + j;
  const float* inb = in + (size_t)blockIdx.z * T * HP + it * 16 + j;
  unsigned live = 0;
  for (int tap = 0; tap < K; ++tap) {
    const int s0 = t0 + off0 + tap * dil;
    if (s0 < T && s0 + (t1 - t0) > 0) live |= 1u << tap;
  }
  f32x4 acc[kMaxTaps];
#pragma unroll
  for (int tap = 0; tap < kMaxTaps; ++tap) acc[tap] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = t0; t < t1; t += 4) {
    const int ta = t + g;
    const bool oka = ta < t1;
    const float a = oka ? dub[(oka ? ta : t1 - 1) * HP] : 0.f;
#pragma unroll
    for (int tap = 0; tap < kMaxTaps; ++tap) {
      if (!(live >> tap & 1)) continue;
      const int tb = ta + off0 + tap * dil;
      const bool okb = oka && tb >= 0 && tb < T;
      const float v = inb[(tb < 0 ? 0 : (tb >= T ? T - 1 : tb)) * HP];
      acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, okb ? v : 0.f, acc[tap], 0, 0, 0);
    }
  }
  float* po = part + (((size_t)blockIdx.z * nwchunk + wc) * K * (NT * NT) + blockIdx.y) * 256 + lane * 4;
#pragma unroll
  for (int tap = 0; tap < kMaxTaps; ++tap)
    if (tap < K) *reinterpret_cast<f32x4*>(po + (size_t)tap * (NT * NT) * 256) = acc[tap];
}

// dw[out][in][tap] (the reference's layout) = sum over the P partials in order, in double.
__global__ __launch_bounds__(256) void tcn_wgrad_final_kernel(const float* __restrict__ part, int P, int H, int HP, int K,
                                                              float* __restrict__ dw) {
  const int NT = HP / 16, per = K * NT * NT * 256;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per) return;
  const int r = i & 3, lane = i >> 2 & 63, tile = (i >> 8) % (NT * NT), tap = (i >> 8) / (NT * NT);
  const int o = (tile / NT) * 16 + 4 * (lane >> 4) + r, ci = (tile % NT) * 16 + (lane & 15);
  if (o >= H || ci >= H) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += (double)part[(size_t)p * per + i];
  dw[((size_t)o * H + ci) * K + tap] = (float)s;
}

// The sums behind the gradients of a 1x1 projection.  a8: [B][8][T] (dy or x), hid: [B][T][HP] (h_nb or dh_0).
// part[b][chunk][10][HP]: q < 8: sum_t a8[q][t] hid[t][c]; q = 8: sum_t hid[t][c]; q = 9: sum_t a8[c][t] in the threads c < 8.
__global__ __launch_bounds__(256) void tcn_proj_grad_kernel(const float* __restrict__ a8, const float* __restrict__ hid,
                                                            double* __restrict__ part, int T, int HP) {
  const int nslots = 256 / HP, c = threadIdx.x % HP, slot = threadIdx.x / HP;
  const bool active = slot < nslots;
  const int t0 = blockIdx.x * kRowsChunk, t1 = min(T, t0 + kRowsChunk);
  const float* hb = hid + (size_t)blockIdx.y * T * HP;
  const float* ab = a8 + (size_t)blockIdx.y * 8 * T;
  double acc[kProjQ];
#pragma unroll
  for (int q = 0; q < kProjQ; ++q) acc[q] = 0.0;
  if (active)
    for (int t = t0 + slot; t < t1; t += nslots) {
      const double hv = (double)hb[(size_t)t * HP + c];
      acc[8] += hv;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double av = (double)ab[(size_t)q * T + t];
        acc[q] = fma(av, hv, acc[q]);
        if (q == c) acc[9] += av;
      }
    }
  tcn_block_reduce<kProjQ>(acc, c, slot, nslots, HP, active, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kProjQ * HP);
}

// Thread (q, c) sums the P partials.  hid_major = 0: w[q][c] ([8][H], output_conv), bias[c < 8] = sum of a8[c].
// hid_major = 1: w[c][q] ([H][8], input_conv), bias[c] = sum of hid.
__global__ __launch_bounds__(256) void tcn_proj_final_kernel(const double* __restrict__ part, int P, int H, int HP, int hid_major,
                                                             float* __restrict__ w, float* __restrict__ bias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kProjQ * HP) return;
  const int q = i / HP, c = i - q * HP;
  const bool is_w = q < 8 && c < H, is_b = hid_major ? (q == 8 && c < H) : (q == 9 && c < 8);
  if (!is_w && !is_b) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += part[(size_t)p * kProjQ * HP + i];
  if (is_w) w[hid_major ? c * 8 + q : q * H + c] = (float)s;
  else bias[c] = (float)s;
}

// masks[b][c][t] of one convolution = 1 where the backward takes slope 1.  (Tests only.)
__global__ __launch_bounds__(256) void tcn_masks_kernel(const float* __restrict__ u, const float* __restrict__ sc,
                                                        const float* __restrict__ res, unsigned char* __restrict__ out, long long T,
                                                        int H, int HP) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const size_t row = (size_t)(b * T + t) * HP;
  for (int c = 0; c < H; ++c) {
    const float f = tcn_act_arg(sc[b * 2 * HP + c], u[row + c], sc[b * 2 * HP + HP + c], res ? res[row + c] : 0.f, res != nullptr);
    out[(b * H + c) * T + t] = tcn_slope_one(f) ? 1 : 0;
  }
}

// private layout from the reference's: h[b][t][c] = in[b][c][t], zeros in the padded channels.  (Tests only.)
__global__ __launch_bounds__(256) void tcn_pack_kernel(const float* __restrict__ in, float* __restrict__ h, long long T, int H, int HP) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  float* ho = h + (b * T + t) * HP;
  for (int c = 0; c < HP; ++c) ho[c] = c < H ? in[(b * H + c) * T + t] : 0.f;
}

// Device-side refresh of the convolution weights: wsw as mst_tcn_create lays it out, wswT the same order for the input
// gradient (out and in channels exchanged, taps reversed).  One thread per element of wsw.
__global__ __launch_bounds__(256) void tcn_swizzle_kernel(const float* __restrict__ w, float* __restrict__ wsw, float* __restrict__ wswT,
                                                          long long total, int H, int HP, int K) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int NT = HP / 16;
  const int s = (int)(i & 3), lane = (int)(i >> 2 & 63);
  long long r = i >> 8;
  const int o = (int)(r % NT);
  r /= NT;
  const int ch = (int)(r % NT);
  r /= NT;
  const int tap = (int)(r % K), cv = (int)(r / K);
  const int co = o * 16 + (lane & 15), ci = ch * 16 + 4 * (lane >> 4) + s;
  const bool ok = co < H && ci < H;
  wsw[i] = ok ? w[(((size_t)cv * H + co) * H + ci) * K + tap] : 0.f;
  wswT[i] = ok ? w[(((size_t)cv * H + ci) * H + co) * K + (K - 1 - tap)] : 0.f;
}

// The small vectors of the handle from device tensors in the reference's layouts.  One thread per padded channel.
__global__ void tcn_small_params_kernel(const float* __restrict__ iw, const float* __restrict__ ib, const float* __restrict__ ow,
                                        const float* __restrict__ ob, const float* __restrict__ cb, int H, int HP, int nconv,
                                        float* __restrict__ wi, float* __restrict__ bi, float* __restrict__ wo, float* __restrict__ bo,
                                        float* __restrict__ rawsc) {
  const int c = threadIdx.x;
  if (c >= HP) return;
  for (int q = 0; q < 8; ++q) {
    wi[c * 8 + q] = c < H ? iw[c * 8 + q] : 0.f;
    wo[c * 8 + q] = c < H ? ow[q * H + c] : 0.f;
  }
  bi[c] = c < H ? ib[c] : 0.f;
  if (c < 8) bo[c] = ob[c];
  for (int cv = 0; cv <= nconv; ++cv) {
    rawsc[(cv * 2) * HP + c] = cv < nconv ? 1.f : 0.f;
    rawsc[(cv * 2 + 1) * HP + c] = cv < nconv && c < H ? cb[cv * H + c] : 0.f;
  }
}

struct TrainPlan {
  size_t big;                       // bytes of one [B][T][HP] buffer
  int nchunk, nwchunk;              // time chunks of the row reductions / wave chunks of the weight gradient
  size_t sc_bytes, st_bytes;        // [2 nb][B][2][HP], [2 nb][2][HP]
  size_t red_bytes, wpart_bytes, coef_bytes;
  size_t save_total, ws_total;
};

TrainPlan train_plan(const mst_tcn* h, int B, long long T) {
  TrainPlan p;
  const size_t HP = h->HP, nb = h->cfg.num_blocks, K = h->cfg.kernel_size;
  p.big = align_up((size_t)B * T * HP * sizeof(float), 256);
  p.nchunk = (int)((T + kRowsChunk - 1) / kRowsChunk);
  p.nwchunk = (int)((T + kRowsWave - 1) / kRowsWave);
  p.sc_bytes = align_up(2 * nb * B * 2 * HP * sizeof(float), 256);
  p.st_bytes = align_up(2 * nb * 2 * HP * sizeof(float), 256);
  p.red_bytes = align_up((size_t)B * p.nchunk * kProjQ * HP * sizeof(double), 256);
  p.wpart_bytes = align_up((size_t)B * p.nwchunk * K * HP * HP * sizeof(float), 256);
  p.coef_bytes = align_up(((size_t)B + 2) * HP * sizeof(float), 256);
  p.save_total = (3 * nb + 1) * p.big + p.sc_bytes + p.st_bytes;
  p.ws_total = 3 * p.big + p.sc_bytes + p.st_bytes + p.red_bytes + p.wpart_bytes + p.coef_bytes;
  return p;
}

// pointers into a save buffer (or, with save == NULL, the part of the workspace that stands in for it)
struct TrainSave {
  float *hs, *us, *sc, *st;   // hs: [nb + 1] big buffers, us: [2 nb] big buffers
};
TrainSave train_save_at(void* save, const TrainPlan& p, int nb) {
  TrainSave s;
  char* q = (char*)save;
  s.hs = (float*)q, q += (size_t)(nb + 1) * p.big;
  s.us = (float*)q, q += (size_t)2 * nb * p.big;
  s.sc = (float*)q, q += p.sc_bytes;
  s.st = (float*)q;
  return s;
}

int tcn_train_ready(const mst_tcn* h, const char* who) {
  MST_REQUIRE(h->wswT && h->rawsc, "%s: the handle has no training weights; call mst_tcn_update_params first", who);
  return MST_OK;
}

void launch_wgrad(const mst_tcn* h, const TrainPlan& p, const float* du, const float* in, float* wpart, int B, int T, int dil,
                  int off0, float* dw, hipStream_t st) {
  const int HP = h->HP, NT = HP / 16, K = h->cfg.kernel_size, H = h->cfg.hidden_channels;
  hipLaunchKernelGGL(tcn_wgrad_kernel, dim3((unsigned)((p.nwchunk + 3) / 4), (unsigned)(NT * NT), (unsigned)B), dim3(256), 0, st, du, in,
                     wpart, T, HP, K, dil, off0, p.nwchunk);
  const int per = K * NT * NT * 256;
  hipLaunchKernelGGL(tcn_wgrad_final_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, wpart, B * p.nwchunk, H, HP, K, dw);
}

}  // namespace
}  // namespace mst

extern "C" {

int mst_tcn_update_params(mst_tcn* h, const mst_tcn_weights* w, void* stream) {
  MST_REQUIRE(h && w, "mst_tcn_update_params: NULL argument");
  const float* par[] = {w->input_w, w->input_b, w->conv_w, w->conv_b, w->bn_w, w->bn_b, w->output_w, w->output_b};
  int npar = 0;
  for (const float* q : par) npar += q != nullptr;
  MST_REQUIRE(npar == 0 || npar == 8, "mst_tcn_update_params: the parameter pointers are given all or none (%d of 8)", npar);
  MST_REQUIRE(!w->bn_mean == !w->bn_var, "mst_tcn_update_params: bn_mean and bn_var are given both or neither");
  MST_REQUIRE(npar || w->bn_mean, "mst_tcn_update_params: nothing to update");
  hipStream_t st = (hipStream_t)stream;
  const int H = h->cfg.hidden_channels, HP = h->HP, K = h->cfg.kernel_size, nb = h->cfg.num_blocks;
  const size_t nw = (size_t)2 * nb * K * HP * HP, nl = (size_t)nb * 2 * H;
  if (npar) {
    if (!h->wswT) {
      hipError_t e = hipMalloc((void**)&h->wswT, nw * sizeof(float));
      if (e != hipSuccess) return fail(MST_ENOMEM, "mst_tcn_update_params: hipMalloc failed: %s", hipGetErrorString(e));
    }
    if (!h->rawsc) {
      hipError_t e = hipMalloc((void**)&h->rawsc, (size_t)(2 * nb + 1) * 2 * HP * sizeof(float));
      if (e != hipSuccess) return fail(MST_ENOMEM, "mst_tcn_update_params: hipMalloc failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(tcn_swizzle_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, w->conv_w, h->wsw, h->wswT, (long long)nw,
                       H, HP, K);
    if (h->mode == MST_TCN_F16X3) {   // the f16 fragments follow wsw: never stale
      const int rc = tcn_f16x3_build(h, st);
      if (rc != MST_OK) return rc;
    }
    hipLaunchKernelGGL(tcn_small_params_kernel, dim3(1), dim3(kMaxHidden), 0, st, w->input_w, w->input_b, w->output_w, w->output_b,
                       w->conv_b, H, HP, 2 * nb, h->wi, h->bi, h->wo, h->bo, h->rawsc);
    const struct { float* d; const float* s; } cp[] = {{h->cb, w->conv_b}, {h->bw, w->bn_w}, {h->bb, w->bn_b}};
    for (const auto& c : cp) MST_HIP_CHECK(hipMemcpyAsync(c.d, c.s, nl * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (w->bn_mean) {   // read by the inference path only
    MST_HIP_CHECK(hipMemcpyAsync(h->bm, w->bn_mean, nl * sizeof(float), hipMemcpyDeviceToDevice, st));
    MST_HIP_CHECK(hipMemcpyAsync(h->bv, w->bn_var, nl * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

size_t mst_tcn_train_save_bytes(const mst_tcn* h, int B, long long T) {
  if (tcn_shape_ok(h, B, T, "mst_tcn_train_save_bytes") != MST_OK) return 0;
  return train_plan(h, B, T).save_total;
}

size_t mst_tcn_train_workspace_bytes(const mst_tcn* h, int B, long long T) {
  if (tcn_shape_ok(h, B, T, "mst_tcn_train_workspace_bytes") != MST_OK) return 0;
  return train_plan(h, B, T).ws_total;
}

int mst_tcn_forward_train(const mst_tcn* h, const float* x, const float* film, int B, long long T, float* y, float* batch_mean,
                          float* batch_var, void* save, size_t save_bytes, void* ws, size_t ws_bytes, void* stream) {
  int rc = tcn_shape_ok(h, B, T, "mst_tcn_forward_train");
  if (rc != MST_OK) return rc;
  if ((rc = tcn_train_ready(h, "mst_tcn_forward_train")) != MST_OK) return rc;
  MST_REQUIRE(x && y && ws && batch_mean && batch_var, "mst_tcn_forward_train: NULL pointer");
  MST_REQUIRE(!h->cfg.use_film == !film, "mst_tcn_forward_train: film parameters are %s for this mixer (use_film = %d)",
              h->cfg.use_film ? "required" : "not accepted", h->cfg.use_film);
  MST_REQUIRE((long long)B * T >= 2, "mst_tcn_forward_train: batch statistics need more than one value per channel (B * T = %lld)",
              (long long)B * T);
  const TrainPlan p = train_plan(h, B, T);
  if (ws_bytes < p.ws_total) return fail(MST_ENOMEM, "mst_tcn_forward_train: workspace %zu B < required %zu B", ws_bytes, p.ws_total);
  if (save && save_bytes < p.save_total)
    return fail(MST_ENOMEM, "mst_tcn_forward_train: save buffer %zu B < required %zu B", save_bytes, p.save_total);
  hipStream_t st = (hipStream_t)stream;
  const int H = h->cfg.hidden_channels, HP = h->HP, K = h->cfg.kernel_size, nb = h->cfg.num_blocks;
  char* wsc = (char*)ws;
  float* big[3] = {(float*)wsc, (float*)(wsc + p.big), (float*)(wsc + 2 * p.big)};
  float* sc_all = (float*)(wsc + 3 * p.big);
  float* st_all = (float*)(wsc + 3 * p.big + p.sc_bytes);
  double* red = (double*)(wsc + 3 * p.big + p.sc_bytes + p.st_bytes);
  TrainSave sv{};
  if (save) {
    sv = train_save_at(save, p, nb);
    sc_all = sv.sc, st_all = sv.st;
  }
  const size_t bigf = p.big / sizeof(float);
  const dim3 tgrid((unsigned)((T + 255) / 256), (unsigned)B), rgrid((unsigned)p.nchunk, (unsigned)B);
  const dim3 agrid((unsigned)((T * (HP / 4) + 255) / 256), (unsigned)B);
  conv_fn conv = conv_raw_for(HP / 16);
  const size_t per_conv = (size_t)K * HP * HP;
  const long long film_stride = (long long)nb * 4 * H;

  float* hin = save ? sv.hs : big[0];
  hipLaunchKernelGGL(tcn_input_kernel, tgrid, dim3(256), 0, st, x, h->wi, h->bi, hin, T, HP);
  for (int k = 0; k < nb; ++k) {
    const int dil = 1 << k;
    const int off0 = h->cfg.causal ? -(K - 1) * dil : -(((K - 1) * dil) / 2);
    float* hout = save ? sv.hs + (size_t)(k + 1) * bigf : big[0];
    float* g = save ? big[0] : big[1];   // the activated first layer; not saved (the backward recomputes it from u1)
    float* in = hin;
    for (int l = 0; l < 2; ++l) {
      const int cv = 2 * k + l;
      float* u = save ? sv.us + (size_t)cv * bigf : big[1 + l];
      float* sc = sc_all + (size_t)cv * B * 2 * HP;
      conv(in, h->wsw + cv * per_conv, h->rawsc + (size_t)cv * 2 * HP, 0, nullptr, u, B, (int)T, K, dil, off0, 0, st);
      hipLaunchKernelGGL(tcn_stats_kernel, rgrid, dim3(256), 0, st, u, red, (int)T, HP);
      hipLaunchKernelGGL(tcn_stats_fold_kernel, dim3(1), dim3(kMaxHidden), 0, st, red, B * p.nchunk, (double)B * (double)T,
                         h->bw + (size_t)cv * H, h->bb + (size_t)cv * H, film ? film + ((size_t)k * 4 + 2 * l) * H : nullptr, film_stride,
                         B, H, HP, h->cfg.bn_eps, batch_mean + (size_t)cv * H, batch_var + (size_t)cv * H,
                         st_all + (size_t)cv * 2 * HP, sc);
      if (l == 0) {
        hipLaunchKernelGGL(tcn_apply_kernel, agrid, dim3(256), 0, st, u, sc, nullptr, g, T, HP, EPI_ACT);
        in = g;
      } else {
        hipLaunchKernelGGL(tcn_apply_kernel, agrid, dim3(256), 0, st, u, sc, hin, hout, T, HP,
                           h->cfg.use_film ? EPI_ACT_THEN_RES : EPI_RES_THEN_ACT);
      }
    }
    hin = hout;
  }
  hipLaunchKernelGGL(tcn_output_kernel, tgrid, dim3(256), 0, st, hin, h->wo, h->bo, x, y, T, HP);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_tcn_backward(const mst_tcn* h, const float* dy, const float* x, const float* film, int B, long long T, const void* save,
                     size_t save_bytes, const mst_tcn_grads* gr, float* dx, float* dfilm, void* ws, size_t ws_bytes, void* stream) {
  int rc = tcn_shape_ok(h, B, T, "mst_tcn_backward");
  if (rc != MST_OK) return rc;
  if ((rc = tcn_train_ready(h, "mst_tcn_backward")) != MST_OK) return rc;
  MST_REQUIRE(dy && x && save && gr && ws, "mst_tcn_backward: NULL pointer");
  MST_REQUIRE(gr->input_w && gr->input_b && gr->conv_w && gr->conv_b && gr->bn_w && gr->bn_b && gr->output_w && gr->output_b,
              "mst_tcn_backward: NULL gradient pointer");
  MST_REQUIRE(!h->cfg.use_film == !film, "mst_tcn_backward: film parameters are %s for this mixer (use_film = %d)",
              h->cfg.use_film ? "required" : "not accepted", h->cfg.use_film);
  MST_REQUIRE(!dfilm || film, "mst_tcn_backward: dfilm given for a mixer without FiLM");
  const TrainPlan p = train_plan(h, B, T);
  if (ws_bytes < p.ws_total) return fail(MST_ENOMEM, "mst_tcn_backward: workspace %zu B < required %zu B", ws_bytes, p.ws_total);
  if (save_bytes < p.save_total) return fail(MST_ENOMEM, "mst_tcn_backward: save buffer %zu B < required %zu B", save_bytes, p.save_total);
  hipStream_t st = (hipStream_t)stream;
  const int H = h->cfg.hidden_channels, HP = h->HP, K = h->cfg.kernel_size, nb = h->cfg.num_blocks;
  const bool use_film = h->cfg.use_film != 0;
  char* wsc = (char*)ws;
  float* dh = (float*)wsc;                 // gradient of the running hidden state
  float* du = (float*)(wsc + p.big);
  float* gb = (float*)(wsc + 2 * p.big);   // g (recomputed), then its gradient
  size_t off = 3 * p.big + p.sc_bytes + p.st_bytes;
  double* red = (double*)(wsc + off);
  off += p.red_bytes;
  float* wpart = (float*)(wsc + off);
  off += p.wpart_bytes;
  float* coef = (float*)(wsc + off);
  float* c12 = coef + (size_t)B * HP;
  const TrainSave sv = train_save_at(const_cast<void*>(save), p, nb);
  const size_t bigf = p.big / sizeof(float);
  const dim3 tgrid((unsigned)((T + 255) / 256), (unsigned)B), rgrid((unsigned)p.nchunk, (unsigned)B);
  const dim3 agrid((unsigned)((T * (HP / 4) + 255) / 256), (unsigned)B);
  const dim3 pgrid((unsigned)((kProjQ * HP + 255) / 256));
  conv_fn conv = conv_raw_for(HP / 16);
  const size_t per_conv = (size_t)K * HP * HP;
  const long long film_stride = (long long)nb * 4 * H;
  const float* zeros = h->rawsc + (size_t)(2 * nb) * 2 * HP;   // [2][HP] of zeros
  const int P = B * p.nchunk;
  const double count = (double)B * (double)T;

  // output_conv: dh = W_out^T dy; its weight and bias gradients from dy and h_nb
  hipLaunchKernelGGL(tcn_input_kernel, tgrid, dim3(256), 0, st, dy, h->wo, zeros, dh, T, HP);
  hipLaunchKernelGGL(tcn_proj_grad_kernel, rgrid, dim3(256), 0, st, dy, sv.hs + (size_t)nb * bigf, red, (int)T, HP);
  hipLaunchKernelGGL(tcn_proj_final_kernel, pgrid, dim3(256), 0, st, red, P, H, HP, 0, gr->output_w, gr->output_b);

  for (int k = nb - 1; k >= 0; --k) {
    const int dil = 1 << k;
    const int off0 = h->cfg.causal ? -(K - 1) * dil : -(((K - 1) * dil) / 2);
    const int goff0 = -off0 - (K - 1) * dil;   // tap 0 of the input gradient
    const float* hk = sv.hs + (size_t)k * bigf;
    for (int l = 1; l >= 0; --l) {
      const int cv = 2 * k + l;
      const float* u = sv.us + (size_t)cv * bigf;
      const float* sc = sv.sc + (size_t)cv * B * 2 * HP;
      const float* stt = sv.st + (size_t)cv * 2 * HP;
      float* dout = l ? dh : gb;
      const float* res = (l && !use_film) ? hk : nullptr;
      const float* fl = film ? film + ((size_t)k * 4 + 2 * l) * H : nullptr;
      float* dfl = dfilm ? dfilm + ((size_t)k * 4 + 2 * l) * H : nullptr;
      hipLaunchKernelGGL(tcn_bwd_reduce_kernel, rgrid, dim3(256), 0, st, dout, u, sc, stt, res, red, (int)T, HP);
      hipLaunchKernelGGL(tcn_bwd_coef_kernel, dim3(1), dim3(kMaxHidden), 0, st, red, B, p.nchunk, count, h->bw + (size_t)cv * H,
                         h->bb + (size_t)cv * H, stt, fl, dfl, film_stride, H, HP, coef, c12, gr->bn_w + (size_t)cv * H,
                         gr->bn_b + (size_t)cv * H);
      hipLaunchKernelGGL(tcn_bwd_du_kernel, rgrid, dim3(256), 0, st, dout, u, sc, stt, res, coef, c12, du, red, (int)T, HP,
                         (l && !use_film) ? 1 : 0);
      hipLaunchKernelGGL(tcn_colsum_kernel, dim3(1), dim3(kMaxHidden), 0, st, red, P, H, HP, gr->conv_b + (size_t)cv * H);
      if (l) {
        // conv2 read g = act(S1 u1 + C1): recompute it, take the weight gradient, then overwrite it with its gradient
        hipLaunchKernelGGL(tcn_apply_kernel, agrid, dim3(256), 0, st, sv.us + (size_t)(cv - 1) * bigf, sv.sc + (size_t)(cv - 1) * B * 2 * HP,
                           nullptr, gb, T, HP, EPI_ACT);
        launch_wgrad(h, p, du, gb, wpart, B, (int)T, dil, off0, gr->conv_w + (size_t)cv * H * H * K, st);
        conv(du, h->wswT + cv * per_conv, zeros, 0, nullptr, gb, B, (int)T, K, dil, goff0, 0, st);
      } else {
        launch_wgrad(h, p, du, hk, wpart, B, (int)T, dil, off0, gr->conv_w + (size_t)cv * H * H * K, st);
        conv(du, h->wswT + cv * per_conv, zeros, 0, dh, dh, B, (int)T, K, dil, goff0, 0, st);
      }
    }
  }
  // input_conv: weight and bias gradients from x and dh_0; dx = dy + W_in^T dh_0
  hipLaunchKernelGGL(tcn_proj_grad_kernel, rgrid, dim3(256), 0, st, x, dh, red, (int)T, HP);
  hipLaunchKernelGGL(tcn_proj_final_kernel, pgrid, dim3(256), 0, st, red, P, H, HP, 1, gr->input_w, gr->input_b);
  if (dx) hipLaunchKernelGGL(tcn_output_kernel, tgrid, dim3(256), 0, st, dh, h->wi, zeros, dy, dx, T, HP);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_tcn_train_masks(const mst_tcn* h, const void* save, size_t save_bytes, int B, long long T, unsigned char* masks, void* stream) {
  int rc = tcn_shape_ok(h, B, T, "mst_tcn_train_masks");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(save && masks, "mst_tcn_train_masks: NULL pointer");
  const TrainPlan p = train_plan(h, B, T);
  if (save_bytes < p.save_total) return fail(MST_ENOMEM, "mst_tcn_train_masks: save buffer %zu B < required %zu B", save_bytes, p.save_total);
  const int H = h->cfg.hidden_channels, HP = h->HP, nb = h->cfg.num_blocks;
  const TrainSave sv = train_save_at(const_cast<void*>(save), p, nb);
  const size_t bigf = p.big / sizeof(float);
  const dim3 tgrid((unsigned)((T + 255) / 256), (unsigned)B);
  for (int cv = 0; cv < 2 * nb; ++cv)
    hipLaunchKernelGGL(tcn_masks_kernel, tgrid, dim3(256), 0, (hipStream_t)stream, sv.us + (size_t)cv * bigf, sv.sc + (size_t)cv * B * 2 * HP,
                       (cv & 1) && !h->cfg.use_film ? sv.hs + (size_t)(cv / 2) * bigf : nullptr, masks + (size_t)cv * B * H * T, T, H, HP);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_tcn_train_conv_grads(const mst_tcn* h, int block, int layer, const float* du, const float* in, int B, long long T, float* din,
                             float* dw, void* ws, size_t ws_bytes, void* stream) {
  int rc = tcn_shape_ok(h, B, T, "mst_tcn_train_conv_grads");
  if (rc != MST_OK) return rc;
  if ((rc = tcn_train_ready(h, "mst_tcn_train_conv_grads")) != MST_OK) return rc;
  MST_REQUIRE(du && in && din && dw && ws, "mst_tcn_train_conv_grads: NULL pointer");
  MST_REQUIRE(block >= 0 && block < h->cfg.num_blocks && (layer == 0 || layer == 1), "mst_tcn_train_conv_grads: no convolution (%d, %d)",
              block, layer);
  const TrainPlan p = train_plan(h, B, T);
  if (ws_bytes < p.ws_total) return fail(MST_ENOMEM, "mst_tcn_train_conv_grads: workspace %zu B < required %zu B", ws_bytes, p.ws_total);
  hipStream_t st = (hipStream_t)stream;
  const int H = h->cfg.hidden_channels, HP = h->HP, K = h->cfg.kernel_size, nb = h->cfg.num_blocks, cv = 2 * block + layer;
  char* wsc = (char*)ws;
  float *a = (float*)wsc, *b = (float*)(wsc + p.big), *c = (float*)(wsc + 2 * p.big);
  float* wpart = (float*)(wsc + 3 * p.big + p.sc_bytes + p.st_bytes + p.red_bytes);
  const dim3 tgrid((unsigned)((T + 255) / 256), (unsigned)B);
  const int dil = 1 << block;
  const int off0 = h->cfg.causal ? -(K - 1) * dil : -(((K - 1) * dil) / 2);
  hipLaunchKernelGGL(tcn_pack_kernel, tgrid, dim3(256), 0, st, du, a, T, H, HP);
  hipLaunchKernelGGL(tcn_pack_kernel, tgrid, dim3(256), 0, st, in, b, T, H, HP);
  launch_wgrad(h, p, a, b, wpart, B, (int)T, dil, off0, dw, st);
  conv_raw_for(HP / 16)(a, h->wswT + (size_t)cv * K * HP * HP, h->rawsc + (size_t)(2 * nb) * 2 * HP, 0, nullptr, c, B, (int)T, K, dil,
                        -off0 - (K - 1) * dil, 0, st);
  hipLaunchKernelGGL(tcn_tap_kernel, tgrid, dim3(256), 0, st, c, din, T, H, HP);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"
