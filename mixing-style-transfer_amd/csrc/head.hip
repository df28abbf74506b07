// Training forward / backward of the two small networks around the convolution trunk:
//   * the attention-pooling head, reference src/model.py:187-211 behind the Dropout of :118 --
//       xd = Dropout(pool_in);  h = tanh(W0 xd_t + b0);  s_t = w2 . h_t + b2;  a = softmax_t(s);  pooled = sum_t a_t xd_t;
//       emb = Dropout(ReLU(Wp pooled + bp))
//   * the FiLM MLP, reference src/model.py:385-464 --
//       h1 = Dropout(ReLU(W1 f + b1));  h2 = ReLU(W3 h1 + b3);  film = Wh h2 + bh
//   * (at the end of the file) the song-identity discriminator and the cosine-distance loss of the adversarial branch, and the
//     FiLM generator of the TCN mixer (reference src/tcn_mixer.py:148-216) in training
// with the gradients autograd derives from them.  fp32 (the head's scores, softmax, softmax backward and sums over frames, and the
// slice sums of the FiLM MLP's d h2, in double: the cancelling paths; products on v_mfma_f32_16x16x4_f32 where a GEMM is large
// enough to matter, fp32 FMA chains elsewhere); every reduction has a fixed order (no atomics): bit-deterministic.
// Dropout masks are never stored: a keep decision is a pure function of (seed, element index) (Philox-2x32-10, common.h) and
// every kernel that touches a dropped tensor re-derives it.
// The weights are the module's live device tensors in state_dict layout -- nothing is swizzled or cached.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "common.h"
#include "mst.h"

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Drop {
  unsigned long long seed;
  unsigned thresh;   // 0: no dropout
  float scale;       // 1 / (1 - p)
};
__device__ __forceinline__ float drop_apply(const Drop& d, size_t o, float v) {
  if (d.thresh == 0) return v;
  return mst::dropout_keep(d.seed, o, d.thresh) ? v * d.scale : 0.f;
}
Drop make_drop(float p, unsigned long long seed) {
  Drop d{seed, 0u, 1.f};
  if (p > 0.f) {
    const double t = (double)p * 4294967296.0;
    d.thresh = (unsigned)(t > 4294967295.0 ? 4294967295.0 : t);
    d.scale = 1.f / (1.f - p);
  }
  return d;
}

// ------------------------------------------------------------------------------------------
// fp32-MFMA GEMM  C[m][n] = sum_k A(m, k) B(k, n)  with operand FUNCTORS (they return 0 outside the matrix) and an epilogue
// functor.  Workgroup = 4 waves = a 64 x 64 tile; wave w owns rows 16 w .. 16 w + 15 and the four 16-column tiles.
// K runs in chunks of 16 through LDS ([k][64 + 16 words]: the 4 k rows of a fragment read fall into 4 disjoint bank groups).
// AM / BN: the operand's memory is contiguous along m / n (else along k) -- picks the thread -> element mapping of the staging
// loads so that a wave reads runs of consecutive addresses.
// ------------------------------------------------------------------------------------------
constexpr int kGP = 80;   // LDS row pitch (words)
constexpr int kKC = 32;   // K chunk
// blockIdx.z = slice * Z + z: batch entry z (functor argument) and K slice [slice * kslice, (slice + 1) * kslice) -- split-K for the
// GEMMs whose M x N gives too few workgroups to fill the chip; the epilogue then receives the slice's partial sum and a second
// kernel adds the slices in a fixed order (deterministic).
template <bool AM, bool BN, class FA, class FB, class FE>
__global__ __launch_bounds__(256) void gemm_kernel(int M, int N, int K, int Z, int kslice, FA fa, FB fb, FE fe) {
  __shared__ float As[kKC * kGP], Bs[kKC * kGP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64, z = blockIdx.z % Z, slice = blockIdx.z / Z;
  const int kbeg = slice * kslice, kend = min(K, kbeg + kslice);
  const int i = lane & 15, kq = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ra[8], rb[8];
  auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int am = AM ? (tid & 63) : (tid >> 5) + 8 * r, ak = AM ? (tid >> 6) + 4 * r : (tid & 31);
      const int bn = BN ? (tid & 63) : (tid >> 5) + 8 * r, bk = BN ? (tid >> 6) + 4 * r : (tid & 31);
      ra[r] = (m0 + am < M && k0 + ak < kend) ? fa(z, m0 + am, k0 + ak) : 0.f;
      rb[r] = (n0 + bn < N && k0 + bk < kend) ? fb(z, k0 + bk, n0 + bn) : 0.f;
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int am = AM ? (tid & 63) : (tid >> 5) + 8 * r, ak = AM ? (tid >> 6) + 4 * r : (tid & 31);
      const int bn = BN ? (tid & 63) : (tid >> 5) + 8 * r, bk = BN ? (tid >> 6) + 4 * r : (tid & 31);
      As[ak * kGP + am] = ra[r];
      Bs[bk * kGP + bn] = rb[r];
    }
  };
  fetch(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += kKC) {
    __syncthreads();   // the previous chunk's fragment reads are done
    stage();
    __syncthreads();
    if (k0 + kKC < kend) fetch(k0 + kKC);   // in flight behind this chunk's MFMAs
#pragma unroll
    for (int s = 0; s < kKC / 4; ++s) {
      const float a = As[(4 * s + kq) * kGP + 16 * wave + i];
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[(4 * s + kq) * kGP + 16 * n + i], acc[n], 0, 0, 0);
    }
  }
  // D: lane (i, kq) holds rows 16 wave + 4 kq + r, column 16 n + i
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 16 * wave + 4 * kq + r, nn = n0 + 16 * n + i;
      if (m < M && nn < N) fe(z, slice, m, nn, acc[n][r]);
    }
}
// sum of the S slices' partial results [S][count] in slice order, handed to the epilogue functor element by element
// (WIDE: the slices are added in double and rounded once -- for the products cut into many short slices)
template <bool WIDE, class FE>
__global__ __launch_bounds__(256) void splitk_finish_kernel(const float* __restrict__ part, int S, long long count, FE fe) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  if (WIDE) {
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += (double)part[(size_t)k * count + i];
    fe(i, (float)s);
  } else {
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += part[(size_t)k * count + i];
    fe(i, s);
  }
}
struct PartEpi {   // partial sums of slice s -> part[s][m][n]
  float* part; int M, N;
  __device__ void operator()(int, int slice, int m, int n, float v) const { part[((size_t)slice * M + m) * N + n] = v; }
};
struct FinHid { float* h; const float* b0; int A; __device__ void operator()(long long i, float v) const { h[i] = tanhf(v + b0[i % A]); } };
struct FinStore { float* out; __device__ void operator()(long long i, float v) const { out[i] = v; } };
struct FinMask {   // d input = sum * (ref > 0 ? gscale : 0): the ReLU (and Dropout) in front of the layer
  float* out; const float* ref; float gscale;
  __device__ void operator()(long long i, float v) const { out[i] = ref[i] > 0.f ? v * gscale : 0.f; }
};
struct FinProj {   // r = ReLU(sum + bias[e]) (kept for the backward), emb = Dropout(r)
  float* emb; float* r; const float* bias; int E; Drop d;
  __device__ void operator()(long long i, float v) const {
    float x = v + bias[i % E];
    x = x < 0.f ? 0.f : x;   // ReLU that keeps NaN (fmaxf would turn a diverged value into 0)
    r[i] = x;
    emb[i] = drop_apply(d, (size_t)i, x);
  }
};
struct LinEpi {   // out[m][n] = Dropout(act(v + bias[n]))
  float* out; const float* bias; int N, relu; Drop d;
  __device__ void operator()(int, int, int m, int n, float v) const {
    float x = v + bias[n];
    if (relu) x = x < 0.f ? 0.f : x;   // (keeps NaN)
    const size_t o = (size_t)m * N + n;
    out[o] = drop_apply(d, o, x);
  }
};
struct RowMajA { const float* a; int ld; __device__ float operator()(int, int m, int k) const { return a[(size_t)m * ld + k]; } };   // A(m, k) = X[m][k]
struct RowMajB { const float* w; int ld; __device__ float operator()(int, int k, int n) const { return w[(size_t)k * ld + n]; } };   // B(k, n) = W[k][n]
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// out[n] = sum_b A[b][n]   (bias gradient): block = 64 columns x 4 row quarters, fixed-order combination
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ A, float* __restrict__ out, int B, int N) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, n = blockIdx.x * 64 + lane;
  const int per = (B + 3) / 4, b0 = q * per, b1 = min(B, b0 + per);
  float s0 = 0.f, s1 = 0.f;
  if (n < N) {
    int b = b0;
    for (; b + 1 < b1; b += 2) s0 += A[(size_t)b * N + n], s1 += A[(size_t)(b + 1) * N + n];
    if (b < b1) s0 += A[(size_t)b * N + n];
  }
  part[q][lane] = s0 + s1;
  __syncthreads();
  if (q == 0 && n < N) out[n] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// ------------------------------------------------------------------------------------------
// attention pooling
// ------------------------------------------------------------------------------------------
// The scores, the softmax over frames and its backward are formed in double (a few thousand values per clip): the gradients of
// attention.0 / attention.2 are sums over frames of ds_t = a_t (da_t - sum a da) times a bounded factor, sum_t ds_t = 0, so a
// relative error of 2^-24 in the weights a_t or in the difference survives the cancellation at full size.  With fp32 here the
// attention.0.bias gradient is as far from float64 as any fp32 evaluation (1e-4 of its maximum element-wise); with double it is
// 3 to 10 times closer.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// xd = Dropout(x), materialised once per forward pass (the GEMM operand loaders would otherwise spend more time on the keep
// decisions than the matrix cores on the products)
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const float* __restrict__ x, float* __restrict__ xd, long long n, Drop d) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i + k < n) xd[i + k] = drop_apply(d, (size_t)(i + k), x[i + k]);
}
// block = (clip, channel slice): scores s_t = b2 + w2 . h_t, softmax over frames -> a[b][t] (slice 0 writes it),
// pooled[b][c] = sum_t a_t xd[b][c][t] for the slice's channels
__global__ __launch_bounds__(256) void head_pool_kernel(const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, float* __restrict__ a_out, float* __restrict__ pooled,
                                                        int C, int T, int A) {   // x = xd (already dropped)
  extern __shared__ double sd[];   // [T] scores -> exp (double), then [T] weights (float)
  float* sm = reinterpret_cast<float*>(sd + T);
  __shared__ double red[8];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int t = wave; t < T; t += 4) {   // a wave per frame: lanes over the hidden units
    const float* hr = h + ((size_t)b * T + t) * A;
    double s = 0.0;
    for (int j = lane; j < A; j += 64) s = fma((double)w2[j], (double)hr[j], s);
    s = wave_sum_d(s);
    if (lane == 0) sd[t] = s + (double)b2[0];
  }
  __syncthreads();
  double mx = -INFINITY;
  for (int t = tid; t < T; t += 256) mx = fmax(mx, sd[t]);
  mx = wave_max_d(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  double sum = 0.0;
  for (int t = tid; t < T; t += 256) {
    const double e = exp(sd[t] - mx);
    sd[t] = e;   // (only this thread touches frame t)
    sum += e;
  }
  sum = wave_sum_d(sum);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();
  const double invd = 1.0 / ((red[4] + red[5]) + (red[6] + red[7]));
  for (int t = tid; t < T; t += 256) {
    const float a = (float)(sd[t] * invd);
    sm[t] = a;
    if (blockIdx.y == 0) a_out[(size_t)b * T + t] = a;
  }
  __syncthreads();
  const int c_per_blk = (C + gridDim.y - 1) / gridDim.y;
  const int c0 = blockIdx.y * c_per_blk, c1 = min(C, c0 + c_per_blk);
  const float* xb = x + (size_t)b * C * T;
  const int sub = lane >> 4, l16 = lane & 15;
  for (int c = c0 + wave * 4 + sub; c < c1 + 3; c += 16) {   // 16 lanes per channel
    float v = 0.f;
    if (c < c1)
      for (int t = l16; t < T; t += 16) v = fmaf(xb[(size_t)c * T + t], sm[t], v);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (l16 == 0 && c < c1) pooled[(size_t)b * C + c] = v;
  }
}
// dz[b][e] = demb[b][e] * keep3 * scale3 * (r[b][e] > 0)
__global__ __launch_bounds__(256) void head_dz_kernel(const float* __restrict__ demb, const float* __restrict__ r, float* __restrict__ dz,
                                                      long long n, Drop d) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o < n) dz[o] = r[o] > 0.f ? drop_apply(d, (size_t)o, demb[o]) : 0.f;
}
// da_t = sum_c dpooled[b][c] xd[b][c][t], in kDaSlices channel slices per clip (block = (clip, slice): lanes over frames, waves
// over the slice's channels) -> dapart[b][slice][t]
constexpr int kDaSlices = 8;
__global__ __launch_bounds__(256) void head_da_kernel(const float* __restrict__ x, const float* __restrict__ dpooled, float* __restrict__ dapart,
                                                      int C, int T) {   // x = xd
  extern __shared__ float sm[];   // [4][T] per-wave partial da
  const int b = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cper = (C + kDaSlices - 1) / kDaSlices, c0 = sl * cper, c1 = min(C, c0 + cper);
  const float* xb = x + (size_t)b * C * T;
  const float* dp = dpooled + (size_t)b * C;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    float s = 0.f;
    if (t < T)
      for (int c = c0 + wave; c < c1; c += 4) s = fmaf(dp[c], xb[(size_t)c * T + t], s);
    if (t < T) sm[wave * T + t] = s;
  }
  __syncthreads();
  for (int t = tid; t < T; t += 256) dapart[((size_t)b * kDaSlices + sl) * T + t] = (sm[t] + sm[T + t]) + (sm[2 * T + t] + sm[3 * T + t]);
}
// block per clip: da_t = sum of the slices (fixed order);  ds_t = a_t (da_t - sum_t' a_t' da_t')
__global__ __launch_bounds__(256) void head_ds_kernel(const float* __restrict__ dapart, const float* __restrict__ a, float* __restrict__ ds, int T) {
  extern __shared__ double sd[];   // [T]
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double dot = 0.0;
  for (int t = tid; t < T; t += 256) {
    double da = 0.0;
    for (int k = 0; k < kDaSlices; ++k) da += (double)dapart[((size_t)b * kDaSlices + k) * T + t];
    sd[t] = da;   // (only this thread touches column t)
    dot = fma((double)a[(size_t)b * T + t], da, dot);
  }
  dot = wave_sum_d(dot);
  if (lane == 0) red[wave] = dot;
  __syncthreads();
  dot = (red[0] + red[1]) + (red[2] + red[3]);
  for (int t = tid; t < T; t += 256) ds[(size_t)b * T + t] = (float)((double)a[(size_t)b * T + t] * (sd[t] - dot));
}
// block = 64 rows m = (clip, frame): du[m][j] = ds[m] w2[j] (1 - h[m][j]^2);  per-block partial column sums of du (-> db0) and of
// ds h (-> dw2), and the block's sum of ds (-> db2); thread = hidden unit j
__global__ __launch_bounds__(256) void head_du_kernel(const float* __restrict__ h, const float* __restrict__ ds, const float* __restrict__ w2,
                                                      float* __restrict__ du, double* __restrict__ part, int Mrows, int A) {
  const int j = threadIdx.x, m0 = blockIdx.x * 64;
  double s_du = 0.0, s_dw = 0.0, s_ds = 0.0;   // cancelling sums over the frames: in double, rounded once in the finish kernel
  if (j < A) {
    const float w = w2[j];
    for (int r = 0; r < 64; ++r) {
      const int m = m0 + r;
      if (m >= Mrows) break;
      const float hv = h[(size_t)m * A + j], g = ds[m];
      const float v = g * w * (1.f - hv * hv);
      du[(size_t)m * A + j] = v;
      s_du += (double)v;
      s_dw = fma((double)g, (double)hv, s_dw);
      s_ds += (double)g;
    }
  }
  double* pb = part + (size_t)blockIdx.x * (2 * A + 1);
  if (j < A) pb[j] = s_du, pb[A + j] = s_dw;
  if (j == 0) pb[2 * A] = s_ds;
}
// second stage: fixed-order sums of the per-block partials
__global__ __launch_bounds__(256) void head_du_finish_kernel(const double* __restrict__ part, int nblk, int A, float* __restrict__ db0,
                                                             float* __restrict__ dw2, float* __restrict__ db2) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > 2 * A) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[(size_t)k * (2 * A + 1) + j];
  if (j < A) db0[j] = (float)s;
  else if (j < 2 * A) dw2[j - A] = (float)s;
  else db2[0] = (float)s;
}

// keep[i] = 1 iff element i survives a Dropout(p) keyed by `seed` (what every kernel above re-derives on the fly)
__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char* keep, long long n, Drop d) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keep[i] = (d.thresh == 0 || mst::dropout_keep(d.seed, (size_t)i, d.thresh)) ? 1 : 0;
}

// GEMM functors ---------------------------------------------------------------------------
struct XdOp {   // (m = clip * T + frame, c) -> xd[clip][c][frame]
  const float* x;
  int C, T;
  __device__ float at(int m, int c) const {
    const int b = m / T, t = m - b * T;
    return x[((size_t)b * C + c) * T + t];
  }
};
struct ColMajA { const float* a; int ld; __device__ float operator()(int, int m, int k) const { return a[(size_t)k * ld + m]; } };   // A(m, k) = X[k][m]
struct EpiStore { float* out; int ld; __device__ void operator()(int, int, int m, int n, float v) const { out[(size_t)m * ld + n] = v; } };
struct FwdA { XdOp xd; __device__ float operator()(int, int m, int k) const { return xd.at(m, k); } };
struct RowMajT { const float* w; int ld; __device__ float operator()(int, int k, int n) const { return w[(size_t)n * ld + k]; } };   // B(k, n) = W[n][k]
struct DuT { const float* du; int A; __device__ float operator()(int, int j, int m) const { return du[(size_t)m * A + j]; } };       // A(j, m) = du[m][j]
struct XdB { XdOp xd; __device__ float operator()(int, int m, int c) const { return xd.at(m, c); } };                           // B(m, c)
struct W0T { const float* w; int C; __device__ float operator()(int, int c, int j) const { return w[(size_t)j * C + c]; } };       // A(c, j) = W0[j][c]
struct DuB {   // B(j, t) of clip z = du[(z, t)][j]
  const float* du; int T, A;
  __device__ float operator()(int z, int j, int t) const { return du[((size_t)z * T + t) * A + j]; }
};
struct DxEpi {   // dx[z][c][t] = keep2 scale2 (v + a[z][t] dpooled[z][c])
  float* dx; const float* a; const float* dpooled; int C, T; Drop d;
  __device__ void operator()(int z, int, int c, int t, float v) const {
    const size_t o = ((size_t)z * C + c) * T + t;
    dx[o] = drop_apply(d, o, v + a[(size_t)z * T + t] * dpooled[(size_t)z * C + c]);
  }
};

// C = A B with the K range split over S workgroup slices: partial sums to `part` ([S][M][N]), then a fixed-order sum + epilogue
template <bool AM, bool BN, bool WIDE = false, class FA, class FB, class FIN>
void gemm_split(int M, int N, int K, int S, FA fa, FB fb, float* part, FIN fin, hipStream_t st) {
  const int kslice = round_up((K + S - 1) / S, kKC);
  const int S2 = (K + kslice - 1) / kslice;
  PartEpi pe{part, M, N};
  hipLaunchKernelGGL((gemm_kernel<AM, BN, FA, FB, PartEpi>), dim3((N + 63) / 64, (M + 63) / 64, S2), dim3(256), 0, st, M, N, K, 1, kslice, fa, fb, pe);
  const long long cnt = (long long)M * N;
  hipLaunchKernelGGL((splitk_finish_kernel<WIDE, FIN>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, part, S2, cnt, fin);
}
constexpr int kSplitProj = 4, kSplitDW0 = 8, kSplitFilm = 8, kSplitHid = 4;
// d h2 = d film Wh of the FiLM MLP sums over the out_dim = n_sub * 192 outputs (2112 in the model).  Its rounding is the largest
// error of that backward (at B = 33 it put mlp.3.weight at 2.07 x the fp32 reference's own distance from float64, h1 contributing
// half as much): cut into slices of at most 96 terms, added in double.
constexpr int kSplitFilmOut = 32;

struct HeadSave {   // offsets (floats) into the caller's save buffer
  size_t h, a, pooled, r, part, xd, hpart, total;
};
HeadSave head_save(int B, int C, int T, int A, int E, bool drop_in) {
  HeadSave s{};
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 63) & ~(size_t)63; return at; };
  s.h = take((size_t)B * T * A), s.a = take((size_t)B * T), s.pooled = take((size_t)B * C), s.r = take((size_t)B * E);
  s.part = take((size_t)kSplitProj * B * E);   // (forward scratch: split-K partial sums of the projection)
  s.xd = take(drop_in ? (size_t)B * C * T : 0);   // Dropout(pool_in), when there is a Dropout
  s.hpart = take((size_t)kSplitHid * B * T * A);   // (forward scratch: split-K partial sums of the hidden layer)
  s.total = o;
  return s;
}
struct HeadWork {   // backward scratch
  size_t dz, dpooled, ds, du, part, gpart, dapart, total;
  int nblk;
};
HeadWork head_work(int B, int C, int T, int A, int E) {
  HeadWork s{};
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 63) & ~(size_t)63; return at; };
  s.nblk = (B * T + 63) / 64;
  s.dz = take((size_t)B * E), s.dpooled = take((size_t)B * C), s.ds = take((size_t)B * T), s.du = take((size_t)B * T * A);
  s.part = take((size_t)2 * s.nblk * (2 * A + 1));   // doubles
  s.gpart = take(std::max((size_t)kSplitDW0 * A * C, (size_t)kSplitProj * B * C));   // split-K partial sums
  s.dapart = take((size_t)B * kDaSlices * T);
  s.total = o;
  return s;
}

// ------------------------------------------------------------------------------------------
// Linear -> act -> Dropout -> Linear -> act -> Dropout -> Linear: the FiLM MLP, the discriminator and the TCN FiLM generator.
// One description of a call, one forward chain, one backward chain; an entry point states its finish functors and split counts.
// ------------------------------------------------------------------------------------------
struct Mlp {   // one call: B rows through I -> H -> H -> O, weights [out][in] (state_dict layout); fn = the entry point, for messages
  const char* fn;
  int B, I, H, O;
  const float *w[3], *b[3];
};
struct MlpGrads { float *w[3], *b[3]; };
struct MlpLimits { const char *in, *hid; int I, H, O, B; };   // names of the first two dims in the public struct, largest sizes
// (the public dims / weights / grads structs of the three networks are three ints / six pointers w, b, w, b, w, b each)
template <class D, class W>
Mlp mlp_net(const char* fn, const D* d, const W* w, int B) {
  const auto [I, H, O] = *d;
  const auto [w0, b0, w1, b1, w2, b2] = *w;
  return Mlp{fn, B, I, H, O, {w0, w1, w2}, {b0, b1, b2}};
}
template <class G>
MlpGrads mlp_grads(const G* g) {
  const auto [w0, b0, w1, b1, w2, b2] = *g;
  return MlpGrads{{w0, w1, w2}, {b0, b1, b2}};
}
bool mlp_dims_ok(const MlpLimits& l, int I, int H, int O) { return I >= 1 && I <= l.I && H >= 1 && H <= l.H && O >= 1 && O <= l.O; }
template <class D>
bool mlp_in_limits(const MlpLimits& l, const D* d, int B) {   // (the *_bytes functions answer 0 for a call the entry points refuse)
  if (!d) return false;
  const auto [I, H, O] = *d;
  return B >= 1 && B <= l.B && mlp_dims_ok(l, I, H, O);
}
// what every entry point refuses, under its own name (g: the gradient pointers of a backward, else NULL)
int mlp_check(const Mlp& n, const MlpLimits& l, const MlpGrads* g, float p1, float p2) {
  MST_REQUIRE(n.w[0] && n.b[0] && n.w[1] && n.b[1] && n.w[2] && n.b[2], "%s: NULL weight", n.fn);
  MST_REQUIRE(!g || (g->w[0] && g->b[0] && g->w[1] && g->b[1] && g->w[2] && g->b[2]), "%s: NULL gradient pointer", n.fn);
  MST_REQUIRE(mlp_dims_ok(l, n.I, n.H, n.O), "%s: dims out of range (%s=%d in 1..%d, %s=%d in 1..%d, out_dim=%d in 1..%d)", n.fn, l.in, n.I, l.I,
              l.hid, n.H, l.H, n.O, l.O);
  MST_REQUIRE(n.B >= 1 && n.B <= l.B, "%s: B=%d rows, must be in 1..%d", n.fn, n.B, l.B);
  MST_REQUIRE(p1 >= 0.f && p1 < 1.f && p2 >= 0.f && p2 < 1.f, "%s: dropout p must be in [0, 1)", n.fn);
  return MST_OK;
}
// a save buffer or a workspace (offsets in floats): nt tensors of B x H, then S slices of B x W split-K partial sums
struct MlpBuf {
  size_t bh, part, total;
  size_t at(int i) const { return i * bh; }
};
MlpBuf mlp_buf(int B, int H, int nt, int S, int W) {
  MlpBuf s{(size_t)B * H, (size_t)nt * B * H, 0};
  s.total = s.part + (size_t)S * B * W;
  return s;
}
int mlp_room(const char* fn, const char* what, size_t have, const MlpBuf& need) {
  if (have < need.total * sizeof(float)) return mst::fail(MST_ENOMEM, "%s: %s %zu B < %zu B", fn, what, have, need.total * sizeof(float));
  return MST_OK;
}
// out = fin(X W^T) for X [B][K], W [N][K]: split-K over S slices with the bias / activation / Dropout in the finish kernel, or
// (a LinEpi) one GEMM over all of K with them in its epilogue
template <class FIN>
void linear(const float* X, int K, const float* W, int N, int B, int S, float* part, FIN fin, hipStream_t st) {
  gemm_split<false, false>(B, N, K, S, RowMajA{X, K}, RowMajT{W, K}, part, fin, st);
}
void linear(const float* X, int K, const float* W, int N, int B, int, float*, LinEpi epi, hipStream_t st) {
  hipLaunchKernelGGL((gemm_kernel<false, false, RowMajA, RowMajT, LinEpi>), dim3((N + 63) / 64, (B + 63) / 64, 1), dim3(256), 0, st, B, N, K, 1,
                     round_up(K, kKC), RowMajA{X, K}, RowMajT{W, K}, epi);
}
// db = colsum(dy), dw = dy^T in   for dy [B][N], in [B][K]
void linear_wgrad(const float* dy, int N, const float* in, int K, float* dw, float* db, int B, hipStream_t st) {
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(256), 0, st, dy, db, B, N);
  hipLaunchKernelGGL((gemm_kernel<true, true, ColMajA, RowMajB, EpiStore>), dim3((K + 63) / 64, (N + 63) / 64, 1), dim3(256), 0, st, N, K, B, 1,
                     round_up(B, kKC), ColMajA{dy, N}, RowMajB{in, K}, EpiStore{dw, K});
}
// f1 / f2 write the activations h1 / h2 ([B][H]) that the next layer reads, f3 the output
template <class F1, class F2, class F3>
void mlp_forward(const Mlp& n, const float* x, const float* h1, const float* h2, int S, float* part, F1 f1, F2 f2, F3 f3, hipStream_t st) {
  linear(x, n.I, n.w[0], n.H, n.B, S, part, f1, st);
  linear(h1, n.H, n.w[1], n.H, n.B, S, part, f2, st);
  linear(h2, n.H, n.w[2], n.O, n.B, S, part, f3, st);
}
// dy [B][O] back through the three layers: m2 / m1 take d h2 / d h1 through the activation and Dropout in front of the layer and
// write them to dh2 / dh1; weight gradients if g, input gradient if dx.  S2 / S1 / S0: split counts of the three products
// (WIDE2: the slices of d h2 are added in double)
template <bool WIDE2, class M2, class M1>
void mlp_backward(const Mlp& n, const float* x, const float* h1, const float* h2, const float* dy, const MlpGrads* g, float* dx, const float* dh2,
                  const float* dh1, float* part, int S2, M2 m2, int S1, M1 m1, int S0, hipStream_t st) {
  if (g) linear_wgrad(dy, n.O, h2, n.H, g->w[2], g->b[2], n.B, st);
  gemm_split<false, true, WIDE2>(n.B, n.H, n.O, S2, RowMajA{dy, n.O}, RowMajB{n.w[2], n.H}, part, m2, st);
  if (g) linear_wgrad(dh2, n.H, h1, n.H, g->w[1], g->b[1], n.B, st);
  gemm_split<false, true>(n.B, n.H, n.H, S1, RowMajA{dh2, n.H}, RowMajB{n.w[1], n.H}, part, m1, st);
  if (g) linear_wgrad(dh1, n.H, x, n.I, g->w[0], g->b[0], n.B, st);
  if (dx) gemm_split<false, true>(n.B, n.I, n.H, S0, RowMajA{dh1, n.H}, RowMajB{n.w[0], n.I}, part, FinStore{dx}, st);
}
// FiLM MLP: dims <= 2048 (mst.h), any B
const MlpLimits kFilmLimits{"feature_dim", "hidden", 2048, 2048, INT_MAX, INT_MAX};
}  // namespace

// head_pool_kernel / head_ds_kernel / head_da_kernel keep 12 T / 8 T / 16 T bytes in dynamic LDS: bounded here, in BOTH
// entry points, so that an over-long clip is refused before any kernel of the pass has run (2048 pooled frames = 4 minutes of audio)
constexpr int kHeadMaxFrames = 2048;
static bool head_dims_ok(int C, int T, int A, int E) {
  return C >= 1 && C <= 3072 && T >= 1 && T <= kHeadMaxFrames && A >= 1 && A <= 256 && E >= 1;
}

extern "C" {

int mst_dropout_mask(float p, uint64_t seed, long long n, unsigned char* keep, void* stream) {
  MST_REQUIRE(keep && n >= 0 && p >= 0.f && p < 1.f, "mst_dropout_mask: bad argument");
  if (n == 0) return MST_OK;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), keep, n,
                     make_drop(p, seed));
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

size_t mst_head_save_bytes(const mst_head_dims* d, int B, float drop_in_p) {
  if (!d || B <= 0) return 0;
  return head_save(B, d->channels, d->frames, d->attn_hidden, d->embed_dim, drop_in_p > 0.f).total * sizeof(float);
}
size_t mst_head_backward_workspace_bytes(const mst_head_dims* d, int B) {
  if (!d || B <= 0) return 0;
  return head_work(B, d->channels, d->frames, d->attn_hidden, d->embed_dim).total * sizeof(float);
}

int mst_head_forward_train(const mst_head_dims* dm, const mst_head_weights* w, const float* pool_in, int B, float drop_in_p,
                           uint64_t drop_in_seed, float drop_out_p, uint64_t drop_out_seed, float* emb, void* save,
                           size_t save_bytes, void* stream) {
  MST_REQUIRE(dm && w && pool_in && emb && save && B > 0, "mst_head_forward_train: NULL / bad argument");
  MST_REQUIRE(w->att0_w && w->att0_b && w->att2_w && w->att2_b && w->proj_w && w->proj_b, "mst_head_forward_train: NULL weight");
  const int C = dm->channels, T = dm->frames, A = dm->attn_hidden, E = dm->embed_dim;
  MST_REQUIRE(head_dims_ok(C, T, A, E), "mst_head_forward_train: dims out of range (C=%d T=%d A=%d E=%d; limits C <= 3072, T <= %d, A <= 256)", C, T, A, E, kHeadMaxFrames);
  MST_REQUIRE(drop_in_p >= 0.f && drop_in_p < 1.f && drop_out_p >= 0.f && drop_out_p < 1.f, "mst_head_forward_train: dropout p must be in [0, 1)");
  const HeadSave S = head_save(B, C, T, A, E, drop_in_p > 0.f);
  if (save_bytes < S.total * sizeof(float)) return mst::fail(MST_ENOMEM, "mst_head_forward_train: save buffer %zu B < %zu B", save_bytes, S.total * sizeof(float));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* sv = static_cast<float*>(save);
  const Drop d2 = make_drop(drop_in_p, drop_in_seed), d3 = make_drop(drop_out_p, drop_out_seed);
  const int M = B * T;
  const float* xd = pool_in;
  if (d2.thresh) {
    const long long n = (long long)B * C * T;
    hipLaunchKernelGGL(dropout_fwd_kernel, dim3((unsigned)((n / 4 + 255) / 256 + 1)), dim3(256), 0, st, pool_in, sv + S.xd, n, d2);
    xd = sv + S.xd;
  }
  {   // h = tanh(xd W0^T + b0)
    FwdA fa{XdOp{xd, C, T}};
    RowMajT fb{w->att0_w, C};
    // (split-K: 4 x the workgroups -- enough of them per CU to cover each other's load latency; the partial sums are 25 MB)
    gemm_split<true, false>(M, A, C, kSplitHid, fa, fb, sv + S.hpart, FinHid{sv + S.h, w->att0_b, A}, st);
  }
  hipLaunchKernelGGL(head_pool_kernel, dim3(B, (C + 127) / 128), dim3(256), (size_t)T * (sizeof(double) + sizeof(float)), st, xd, sv + S.h, w->att2_w,
                     w->att2_b, sv + S.a, sv + S.pooled, C, T, A);
  // emb = Dropout(ReLU(pooled Wp^T + bp))
  gemm_split<false, false>(B, E, C, kSplitProj, RowMajA{sv + S.pooled, C}, RowMajT{w->proj_w, C}, sv + S.part, FinProj{emb, sv + S.r, w->proj_b, E, d3}, st);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_head_backward(const mst_head_dims* dm, const mst_head_weights* w, const float* pool_in, int B, float drop_in_p,
                      uint64_t drop_in_seed, float drop_out_p, uint64_t drop_out_seed, const float* demb, const void* save,
                      const mst_head_grads* g, float* dpool_in, void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(dm && w && pool_in && demb && save && g && dpool_in && workspace && B > 0, "mst_head_backward: NULL / bad argument");
  MST_REQUIRE(g->att0_w && g->att0_b && g->att2_w && g->att2_b && g->proj_w && g->proj_b, "mst_head_backward: NULL gradient pointer");
  const int C = dm->channels, T = dm->frames, A = dm->attn_hidden, E = dm->embed_dim;
  MST_REQUIRE(head_dims_ok(C, T, A, E), "mst_head_backward: dims out of range (C=%d T=%d A=%d E=%d; limits C <= 3072, T <= %d, A <= 256)", C, T, A, E, kHeadMaxFrames);
  MST_REQUIRE(drop_in_p >= 0.f && drop_in_p < 1.f && drop_out_p >= 0.f && drop_out_p < 1.f, "mst_head_backward: dropout p must be in [0, 1)");
  const HeadSave S = head_save(B, C, T, A, E, drop_in_p > 0.f);
  const HeadWork Wk = head_work(B, C, T, A, E);
  if (workspace_bytes < Wk.total * sizeof(float)) return mst::fail(MST_ENOMEM, "mst_head_backward: workspace %zu B < %zu B", workspace_bytes, Wk.total * sizeof(float));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float* sv = static_cast<const float*>(save);
  float* ws = static_cast<float*>(workspace);
  const Drop d2 = make_drop(drop_in_p, drop_in_seed), d3 = make_drop(drop_out_p, drop_out_seed);
  const int M = B * T;
  const float* xd = d2.thresh ? sv + S.xd : pool_in;
  // projection
  hipLaunchKernelGGL(head_dz_kernel, dim3((unsigned)(((long long)B * E + 255) / 256)), dim3(256), 0, st, demb, sv + S.r, ws + Wk.dz, (long long)B * E, d3);
  linear_wgrad(ws + Wk.dz, E, sv + S.pooled, C, g->proj_w, g->proj_b, B, st);   // dWp = dz^T pooled
  gemm_split<false, true>(B, C, E, kSplitProj, RowMajA{ws + Wk.dz, E}, RowMajB{w->proj_w, C}, ws + Wk.gpart, FinStore{ws + Wk.dpooled}, st);   // dpooled = dz Wp
  // softmax / scores
  hipLaunchKernelGGL(head_da_kernel, dim3(B, kDaSlices), dim3(256), (size_t)4 * T * sizeof(float), st, xd, ws + Wk.dpooled, ws + Wk.dapart, C, T);
  hipLaunchKernelGGL(head_ds_kernel, dim3(B), dim3(256), (size_t)T * sizeof(double), st, ws + Wk.dapart, sv + S.a, ws + Wk.ds, T);
  hipLaunchKernelGGL(head_du_kernel, dim3(Wk.nblk), dim3(256), 0, st, sv + S.h, ws + Wk.ds, w->att2_w, ws + Wk.du, reinterpret_cast<double*>(ws + Wk.part), M, A);
  hipLaunchKernelGGL(head_du_finish_kernel, dim3((2 * A + 1 + 255) / 256), dim3(256), 0, st, reinterpret_cast<const double*>(ws + Wk.part), Wk.nblk, A, g->att0_b, g->att2_w, g->att2_b);
  {   // dW0[j][c] = sum_m du[m][j] xd[m][c]
    DuT fa{ws + Wk.du, A};
    XdB fb{XdOp{xd, C, T}};
    gemm_split<true, false>(A, C, M, kSplitDW0, fa, fb, ws + Wk.gpart, FinStore{g->att0_w}, st);
  }
  {   // d pool_in[z][c][t] = keep (a[z][t] dpooled[z][c] + sum_j W0[j][c] du[(z, t)][j])
    W0T fa{w->att0_w, C};
    DuB fb{ws + Wk.du, T, A};
    DxEpi fe{dpool_in, sv + S.a, ws + Wk.dpooled, C, T, d2};
    hipLaunchKernelGGL((gemm_kernel<true, false, W0T, DuB, DxEpi>), dim3((T + 63) / 64, (C + 63) / 64, B), dim3(256), 0, st, C, T, A, B,
                       round_up(A, kKC), fa, fb, fe);
  }
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

size_t mst_film_save_bytes(const mst_film_dims* d, int B) {
  if (!d || B <= 0) return 0;
  return mlp_buf(B, d->hidden, 2, 0, 0).total * sizeof(float);   // h1 (dropped), h2
}
size_t mst_film_backward_workspace_bytes(const mst_film_dims* d, int B) {
  if (!d || B <= 0) return 0;
  return mlp_buf(B, d->hidden, 2, kSplitFilmOut, d->hidden).total * sizeof(float);   // dh2, dh1, split-K partial sums
}

int mst_film_forward_train(const mst_film_dims* dm, const mst_film_weights* w, const float* feats, int B, float drop_p, uint64_t drop_seed,
                           float* film, void* save, size_t save_bytes, void* stream) {
  MST_REQUIRE(dm && w && feats && film && save, "mst_film_forward_train: NULL argument");
  const Mlp n = mlp_net("mst_film_forward_train", dm, w, B);
  if (const int rc = mlp_check(n, kFilmLimits, nullptr, drop_p, 0.f)) return rc;
  const MlpBuf S = mlp_buf(B, n.H, 2, 0, 0);
  if (const int rc = mlp_room(n.fn, "save buffer", save_bytes, S)) return rc;
  float* h1d = static_cast<float*>(save) + S.at(0);
  float* h2 = static_cast<float*>(save) + S.at(1);
  const Drop d0 = make_drop(0.f, 0);   // (Dropout behind the first layer only)
  mlp_forward(n, feats, h1d, h2, 0, nullptr, LinEpi{h1d, n.b[0], n.H, 1, make_drop(drop_p, drop_seed)}, LinEpi{h2, n.b[1], n.H, 1, d0},
              LinEpi{film, n.b[2], n.O, 0, d0}, reinterpret_cast<hipStream_t>(stream));
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_film_backward(const mst_film_dims* dm, const mst_film_weights* w, const float* feats, int B, float drop_p, const float* dfilm,
                      const void* save, const mst_film_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(dm && w && feats && dfilm && save && g && workspace, "mst_film_backward: NULL argument");
  const Mlp n = mlp_net("mst_film_backward", dm, w, B);
  const MlpGrads G = mlp_grads(g);
  if (const int rc = mlp_check(n, kFilmLimits, &G, drop_p, 0.f)) return rc;
  const MlpBuf S = mlp_buf(B, n.H, 2, 0, 0), Wk = mlp_buf(B, n.H, 2, kSplitFilmOut, n.H);
  if (const int rc = mlp_room(n.fn, "workspace", workspace_bytes, Wk)) return rc;
  const float *sv = static_cast<const float*>(save), *h1d = sv + S.at(0), *h2 = sv + S.at(1);
  float *ws = static_cast<float*>(workspace), *dh2 = ws + Wk.at(0), *dh1 = ws + Wk.at(1);
  // d h2 through the ReLU; d h1 through Dropout and ReLU: the survivors are exactly the positive entries of the dropped activation
  mlp_backward<true>(n, feats, h1d, h2, dfilm, &G, nullptr, dh2, dh1, ws + Wk.part, kSplitFilmOut, FinMask{dh2, h2, 1.f}, 2,
                     FinMask{dh1, h1d, make_drop(drop_p, 0).scale}, 2, reinterpret_cast<hipStream_t>(stream));
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

// Gradient to the INPUT of the FiLM MLP in eval mode (no Dropout): dfilm [B][O] -> dfeats [B][Fd] through head -> ReLU ->
// mlp3 -> ReLU -> mlp0.  The two hidden activations are recomputed from `feats` (B x H each); every product is split-K with a
// fixed-order sum, as in mst_film_backward.  Workspace: h1, h2, dh2, dh1 and the partial sums.
size_t mst_film_input_grad_workspace_bytes(const mst_film_dims* d, int B) {
  if (!d || B <= 0) return 0;
  return mlp_buf(B, d->hidden, 4, kSplitFilmOut, std::max(d->hidden, d->feature_dim)).total * sizeof(float);
}

int mst_film_input_grad(const mst_film_dims* dm, const mst_film_weights* w, const float* feats, int B, const float* dfilm, float* dfeats,
                        void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(dm && w && feats && dfilm && dfeats && workspace, "mst_film_input_grad: NULL argument");
  const Mlp n = mlp_net("mst_film_input_grad", dm, w, B);
  if (const int rc = mlp_check(n, kFilmLimits, nullptr, 0.f, 0.f)) return rc;
  const MlpBuf Wk = mlp_buf(B, n.H, 4, kSplitFilmOut, std::max(n.H, n.I));
  if (const int rc = mlp_room(n.fn, "workspace", workspace_bytes, Wk)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float *ws = static_cast<float*>(workspace), *h1 = ws + Wk.at(0), *h2 = ws + Wk.at(1), *dh2 = ws + Wk.at(2), *dh1 = ws + Wk.at(3);
  const Drop d0 = make_drop(0.f, 0);
  linear(feats, n.I, n.w[0], n.H, B, 0, nullptr, LinEpi{h1, n.b[0], n.H, 1, d0}, st);
  linear(h1, n.H, n.w[1], n.H, B, 0, nullptr, LinEpi{h2, n.b[1], n.H, 1, d0}, st);
  mlp_backward<true>(n, feats, h1, h2, dfilm, nullptr, dfeats, dh2, dh1, ws + Wk.part, kSplitFilmOut, FinMask{dh2, h2, 1.f}, 2, FinMask{dh1, h1, 1.f},
                     2, st);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Song-identity discriminator of the adversarial branch (reference src/model.py:545-587) --
//     h1 = Dropout(ReLU(W0 x + b0));  h2 = Dropout(ReLU(W3 h1 + b3));  pred = W6 h2 + b6
// -- and the cosine-distance loss it is trained with (src/train.py:199-202).  The same GEMM kernel as above, every product
// split-K (the M x N tile grids of these shapes are 8 to 48 workgroups) with the bias / ReLU / Dropout epilogue in the finish
// kernel; the input of this network is the embedding, so the backward also returns dx.
// ------------------------------------------------------------------------------------------
namespace {
constexpr int kDiscMaxDim = 2048, kDiscMaxRows = 1 << 20;
const MlpLimits kDiscLimits{"in_dim", "hidden", kDiscMaxDim, kDiscMaxDim, kDiscMaxDim, kDiscMaxRows};
// save buffer: the two dropped activations, then the forward's split-K partial sums; backward scratch: dh2, dh1, partial sums
// (the discriminator's and the generator's: every product of both is cut into kSplitFilm slices)
MlpBuf split_save(int B, int H, int O) { return mlp_buf(B, H, 2, kSplitFilm, std::max(H, O)); }
MlpBuf split_work(int B, int I, int H) { return mlp_buf(B, H, 2, kSplitFilm, std::max(H, I)); }
struct FinLin {   // out[m][n] = Dropout(act(sum + bias[n])), element index m * N + n
  float* out; const float* bias; int N, relu; Drop d;
  __device__ void operator()(long long i, float v) const {
    float x = v + bias[i % N];
    if (relu) x = x < 0.f ? 0.f : x;   // (keeps NaN)
    out[i] = drop_apply(d, (size_t)i, x);
  }
};

// The forward without a save buffer (no backward will follow, nowhere to keep the activations): block = one row, the three
// layers back to back with x, h1 and h2 in LDS; a wave per output unit, lanes over the input units (consecutive addresses of
// the weight row), fixed-order wave sum.  The same Dropout decisions as the GEMM path; sums in another order.
// disc_row_layer: out[n] = Dropout(act(W[n] . in + bias[n])) of row m.
__device__ __forceinline__ void disc_row_layer(const float* in, int K, const float* __restrict__ W, const float* __restrict__ bias, int N,
                                               float* out, int relu, const Drop& d, int m) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int n = wave; n < N; n += 4) {
    const float* wr = W + (size_t)n * K;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s = fmaf(wr[k], in[k], s);
    s = mst::wave_sum(s);
    if (lane == 0) {
      float v = s + bias[n];
      if (relu) v = v < 0.f ? 0.f : v;
      out[n] = drop_apply(d, (size_t)m * N + n, v);
    }
  }
}
__global__ __launch_bounds__(256) void disc_row_kernel(const float* __restrict__ x, const float* __restrict__ w0, const float* __restrict__ b0,
                                                       const float* __restrict__ w3, const float* __restrict__ b3, const float* __restrict__ w6,
                                                       const float* __restrict__ b6, float* __restrict__ pred, int I, int H, int O, Drop d1, Drop d2) {
  __shared__ float xs[kDiscMaxDim], h1[kDiscMaxDim], h2[kDiscMaxDim];
  const int m = blockIdx.x;
  for (int k = threadIdx.x; k < I; k += 256) xs[k] = x[(size_t)m * I + k];
  __syncthreads();
  disc_row_layer(xs, I, w0, b0, H, h1, 1, d1, m);
  __syncthreads();
  disc_row_layer(h1, H, w3, b3, H, h2, 1, d2, m);
  __syncthreads();
  disc_row_layer(h2, H, w6, b6, O, pred + (size_t)m * O, 0, Drop{0ull, 0u, 1.f}, m);
}

// cosine distance: a wave per row, save[row] = (p . p, t . t, p . t)
constexpr float kCosEps = 1e-12f;   // F.normalize's clamp
__global__ __launch_bounds__(256) void cosdist_rows_kernel(const float* __restrict__ pred, const float* __restrict__ target, int K, int D,
                                                           float* __restrict__ save) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= K) return;
  const float* p = pred + (size_t)row * D;
  const float* t = target + (size_t)row * D;
  float pp = 0.f, tt = 0.f, pt = 0.f;
  for (int k = lane; k < D; k += 64) {
    const float a = p[k], b = t[k];
    pp = fmaf(a, a, pp), tt = fmaf(b, b, tt), pt = fmaf(a, b, pt);
  }
  pp = mst::wave_sum(pp), tt = mst::wave_sum(tt), pt = mst::wave_sum(pt);
  if (lane == 0) save[(size_t)3 * row] = pp, save[(size_t)3 * row + 1] = tt, save[(size_t)3 * row + 2] = pt;
}
// one workgroup: thread i sums its run of consecutive rows in index order, thread 0 the 256 run sums in thread order.  The K row
// terms and their sum are formed in double and rounded once (K divisions and square roots in all: the loss then carries the
// rounding of the fp32 dot products and one final rounding, not K more on top)
__device__ __forceinline__ double cosdist_row_loss(const float* s) {
  return 1.0 - (double)s[2] / (fmax(sqrt((double)s[0]), (double)kCosEps) * fmax(sqrt((double)s[1]), (double)kCosEps));
}
__global__ __launch_bounds__(256) void cosdist_mean_kernel(const float* __restrict__ save, int K, float* __restrict__ loss) {
  __shared__ double part[256];
  const int tid = threadIdx.x, per = (K + 255) / 256, r0 = tid * per, r1 = min(K, r0 + per);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += cosdist_row_loss(save + (size_t)3 * r);
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int i = 0; i < 256; ++i) tot += part[i];
    loss[0] = (float)(tot / (double)K);
  }
}
// dpred_i = -(dloss / K) (t^_i - cos_i p^_i) / |p_i|   (|p_i| > eps; else -(dloss / K) t^_i / eps): a wave per row
__global__ __launch_bounds__(256) void cosdist_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, int K, int D,
                                                          const float* __restrict__ save, const float* __restrict__ dloss,
                                                          float* __restrict__ dpred) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= K) return;
  const float* s = save + (size_t)3 * row;
  const float np = sqrtf(s[0]), nt = fmaxf(sqrtf(s[1]), kCosEps), g = -dloss[0] / (float)K;
  const float* p = pred + (size_t)row * D;
  const float* t = target + (size_t)row * D;
  float* o = dpred + (size_t)row * D;
  if (np > kCosEps) {
    const float inp = 1.f / np, cs = s[2] / (np * nt);
    for (int k = lane; k < D; k += 64) o[k] = g * (t[k] / nt - cs * (p[k] * inp)) * inp;
  } else {
    for (int k = lane; k < D; k += 64) o[k] = g * (t[k] / nt) / kCosEps;
  }
}
}  // namespace

extern "C" {

size_t mst_disc_save_bytes(const mst_disc_dims* d, int B) {
  if (!mlp_in_limits(kDiscLimits, d, B)) return 0;
  return split_save(B, d->hidden, d->out_dim).total * sizeof(float);
}
size_t mst_disc_backward_workspace_bytes(const mst_disc_dims* d, int B) {
  if (!mlp_in_limits(kDiscLimits, d, B)) return 0;
  return split_work(B, d->in_dim, d->hidden).total * sizeof(float);
}

int mst_disc_forward(const mst_disc_dims* dm, const mst_disc_weights* w, const float* x, int B, float drop_p, uint64_t seed1,
                     uint64_t seed2, float* pred, void* save, size_t save_bytes, void* stream) {
  MST_REQUIRE(dm && w && x && pred, "mst_disc_forward: NULL argument");
  const Mlp n = mlp_net("mst_disc_forward", dm, w, B);
  if (const int rc = mlp_check(n, kDiscLimits, nullptr, drop_p, drop_p)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Drop d1 = make_drop(drop_p, seed1), d2 = make_drop(drop_p, seed2), d0 = make_drop(0.f, 0);
  if (!save) {
    hipLaunchKernelGGL(disc_row_kernel, dim3(B), dim3(256), 0, st, x, n.w[0], n.b[0], n.w[1], n.b[1], n.w[2], n.b[2], pred, n.I, n.H, n.O, d1, d2);
    MST_HIP_CHECK(hipGetLastError());
    return MST_OK;
  }
  const MlpBuf S = split_save(B, n.H, n.O);
  if (const int rc = mlp_room(n.fn, "save buffer", save_bytes, S)) return rc;
  float *sv = static_cast<float*>(save), *h1 = sv + S.at(0), *h2 = sv + S.at(1);
  mlp_forward(n, x, h1, h2, kSplitFilm, sv + S.part, FinLin{h1, n.b[0], n.H, 1, d1}, FinLin{h2, n.b[1], n.H, 1, d2}, FinLin{pred, n.b[2], n.O, 0, d0}, st);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_disc_backward(const mst_disc_dims* dm, const mst_disc_weights* w, const float* x, int B, float drop_p, uint64_t seed1,
                      uint64_t seed2, const float* dpred, const void* save, const mst_disc_grads* g, float* dx, void* workspace,
                      size_t workspace_bytes, void* stream) {
  (void)seed1, (void)seed2;   // the survivors of a Dropout behind a ReLU are exactly the positive entries of the saved activation
  MST_REQUIRE(dm && w && x && dpred && save && g && workspace, "mst_disc_backward: NULL argument");
  const Mlp n = mlp_net("mst_disc_backward", dm, w, B);
  const MlpGrads G = mlp_grads(g);
  if (const int rc = mlp_check(n, kDiscLimits, &G, drop_p, drop_p)) return rc;
  const MlpBuf S = split_save(B, n.H, n.O), Wk = split_work(B, n.I, n.H);
  if (const int rc = mlp_room(n.fn, "workspace", workspace_bytes, Wk)) return rc;
  const float *sv = static_cast<const float*>(save), *h1 = sv + S.at(0), *h2 = sv + S.at(1);
  float *ws = static_cast<float*>(workspace), *dh2 = ws + Wk.at(0), *dh1 = ws + Wk.at(1);
  const float gscale = make_drop(drop_p, 0).scale;
  mlp_backward<false>(n, x, h1, h2, dpred, &G, dx, dh2, dh1, ws + Wk.part, kSplitFilm, FinMask{dh2, h2, gscale}, kSplitFilm, FinMask{dh1, h1, gscale},
                      kSplitFilm, reinterpret_cast<hipStream_t>(stream));
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_cosdist_forward(const float* pred, const float* target, int K, int D, float* loss, float* save, void* stream) {
  MST_REQUIRE(pred && target && loss && save, "mst_cosdist_forward: NULL argument");
  MST_REQUIRE(K >= 1 && D >= 1 && D <= kDiscMaxDim, "mst_cosdist_forward: K=%d rows, D=%d (K >= 1, 1 <= D <= %d)", K, D, kDiscMaxDim);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cosdist_rows_kernel, dim3((K + 3) / 4), dim3(256), 0, st, pred, target, K, D, save);
  hipLaunchKernelGGL(cosdist_mean_kernel, dim3(1), dim3(256), 0, st, save, K, loss);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_cosdist_backward(const float* pred, const float* target, int K, int D, const float* save, const float* dloss, float* dpred,
                         void* stream) {
  MST_REQUIRE(pred && target && save && dloss && dpred, "mst_cosdist_backward: NULL argument");
  MST_REQUIRE(K >= 1 && D >= 1 && D <= kDiscMaxDim, "mst_cosdist_backward: K=%d rows, D=%d (K >= 1, 1 <= D <= %d)", K, D, kDiscMaxDim);
  hipLaunchKernelGGL(cosdist_bwd_kernel, dim3((K + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pred, target, K, D, save,
                     dloss, dpred);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// TCNFiLMGenerator in training (reference src/tcn_mixer.py:148-216, optimised by src/train_style_transfer.py:255-317) --
//     h1 = Dropout_p1(LeakyReLU_s(W0 x + b0));  h2 = Dropout_p2(LeakyReLU_s(W3 h1 + b3));  film = W6 h2 + b6
// The discriminator's structure on the same GEMM kernel, every product split-K (gamma multiplies every activation of the mixer:
// no single chain over embed_dim or mlp_hidden), with two differences.  The output has up to 8192 columns.  And
// behind a LeakyReLU a saved zero does not say "dropped": it is a dropped unit (gradient 0) or a kept unit whose pre-activation
// was exactly 0 (gradient slope * scale * dh), so the backward re-derives every keep decision from (seed, element index) and
// reads the saved activation only for its sign (h > 0 -> 1, else the slope: PyTorch's branch for x <= 0).
// ------------------------------------------------------------------------------------------
namespace {
const MlpLimits kGenLimits{"embed_dim", "mlp_hidden", 4096, 2048, 8192, 65535};
struct FinLeaky {   // out[m][n] = Dropout(LeakyReLU(sum + bias[n])), element index m * N + n
  float* out; const float* bias; int N; float slope; Drop d;
  __device__ void operator()(long long i, float v) const {
    float x = v + bias[i % N];
    x = x > 0.f ? x : x * slope;   // (keeps NaN)
    out[i] = drop_apply(d, (size_t)i, x);
  }
};
struct FinLeakyMask {   // d pre-activation = keep(seed, i) ? sum * scale * (h > 0 ? 1 : slope) : 0
  float* out; const float* h; float slope; Drop d;
  __device__ void operator()(long long i, float v) const {
    if (d.thresh != 0 && !mst::dropout_keep(d.seed, (size_t)i, d.thresh)) { out[i] = 0.f; return; }
    const float g = v * d.scale;
    out[i] = h[i] > 0.f ? g : g * slope;
  }
};
// what both entry points refuse: mlp_check and the slope
int gen_check(const Mlp& n, const MlpGrads* g, float p1, float p2, float slope) {
  if (const int rc = mlp_check(n, kGenLimits, g, p1, p2)) return rc;
  MST_REQUIRE(slope >= 0.f && slope <= 1.f, "%s: LeakyReLU slope must be in [0, 1]", n.fn);
  return MST_OK;
}
}  // namespace

extern "C" {

size_t mst_tcn_film_train_save_bytes(const mst_tcn_film_train_dims* d, int B) {
  if (!mlp_in_limits(kGenLimits, d, B)) return 0;
  return split_save(B, d->mlp_hidden, d->out_dim).total * sizeof(float);
}
size_t mst_tcn_film_train_backward_workspace_bytes(const mst_tcn_film_train_dims* d, int B) {
  if (!mlp_in_limits(kGenLimits, d, B)) return 0;
  return split_work(B, d->embed_dim, d->mlp_hidden).total * sizeof(float);
}

int mst_tcn_film_forward_train(const mst_tcn_film_train_dims* dm, const mst_tcn_film_weights* w, const float* emb, int B, float slope,
                               float drop_p1, uint64_t seed1, float drop_p2, uint64_t seed2, float* film, void* save, size_t save_bytes,
                               void* stream) {
  MST_REQUIRE(dm && w && emb && film && save, "mst_tcn_film_forward_train: NULL argument");
  const Mlp n = mlp_net("mst_tcn_film_forward_train", dm, w, B);
  if (const int rc = gen_check(n, nullptr, drop_p1, drop_p2, slope)) return rc;
  const MlpBuf S = split_save(B, n.H, n.O);
  if (const int rc = mlp_room(n.fn, "save buffer", save_bytes, S)) return rc;
  float *sv = static_cast<float*>(save), *h1 = sv + S.at(0), *h2 = sv + S.at(1);
  mlp_forward(n, emb, h1, h2, kSplitFilm, sv + S.part, FinLeaky{h1, n.b[0], n.H, slope, make_drop(drop_p1, seed1)},
              FinLeaky{h2, n.b[1], n.H, slope, make_drop(drop_p2, seed2)}, FinLin{film, n.b[2], n.O, 0, make_drop(0.f, 0)},
              reinterpret_cast<hipStream_t>(stream));
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_tcn_film_backward(const mst_tcn_film_train_dims* dm, const mst_tcn_film_weights* w, const float* emb, int B, float slope,
                          float drop_p1, uint64_t seed1, float drop_p2, uint64_t seed2, const float* dfilm, const void* save,
                          const mst_tcn_film_grads* g, float* demb, void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(dm && w && emb && dfilm && save && g && workspace, "mst_tcn_film_backward: NULL argument");
  const Mlp n = mlp_net("mst_tcn_film_backward", dm, w, B);
  const MlpGrads G = mlp_grads(g);
  if (const int rc = gen_check(n, &G, drop_p1, drop_p2, slope)) return rc;
  const MlpBuf S = split_save(B, n.H, n.O), Wk = split_work(B, n.I, n.H);
  if (const int rc = mlp_room(n.fn, "workspace", workspace_bytes, Wk)) return rc;
  const float *sv = static_cast<const float*>(save), *h1 = sv + S.at(0), *h2 = sv + S.at(1);
  float *ws = static_cast<float*>(workspace), *dh2 = ws + Wk.at(0), *dh1 = ws + Wk.at(1);
  mlp_backward<false>(n, emb, h1, h2, dfilm, &G, demb, dh2, dh1, ws + Wk.part, kSplitFilm, FinLeakyMask{dh2, h2, slope, make_drop(drop_p2, seed2)},
                      kSplitFilm, FinLeakyMask{dh1, h1, slope, make_drop(drop_p1, seed1)}, kSplitFilm, reinterpret_cast<hipStream_t>(stream));
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"
