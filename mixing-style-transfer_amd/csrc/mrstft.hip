// Multi-resolution STFT loss (the cycle-consistency loss of the style-transfer trainer), forward and the gradient to the
// first argument.  Replaces MultiResolutionSTFTLoss.forward src/loss.py:332-448 and what autograd derives from it:
//   per resolution  X = stft(x), Y = stft(y)  (center=True, reflect padding n/2, periodic Hann, one-sided, 1 + T/hop frames),
//   xm = |X|, ym = |Y|,  sc = ||ym - xm||_F / (||ym||_F + 1e-8),  lg = mean |log(xm + 1e-5) - log(ym + 1e-5)|,
//   loss = mean over resolutions of (sc_weight sc + log_weight lg).
// One wave transforms a PAIR of consecutive frames of one signal as re/im of one complex FFT (fft_wave.h) and splits the
// two spectra apart.  x and y go through the SAME instruction sequence in separate transforms, so x == y gives xm == ym bit
// for bit (loss and gradient exactly 0, as the reference) -- packing x and y into one transform would not.
// n_fft = 2048 is one decimation-in-time step over two 1024-point wave FFTs (even / odd samples), as stage A does.
// The three sums of a resolution are added up in double per lane, per wave, per workgroup and then across workgroups through
// the order-independent integer accumulators (DetAcc): the loss is bit-reproducible.
// Backward recomputes the frames (storing the complex spectra of 64 x 441 000 samples at three resolutions would be
// 2-4x the audio per resolution, written and read again): per bin the real cotangent on xm is
//   c = -sc_weight (ym - xm) / (||ym - xm|| (||ym|| + 1e-8)) + log_weight sign(log(xm + 1e-5) - log(ym + 1e-5)) / (Nbins (xm + 1e-5)),
// G = c X / |X| (0 where X == 0), and the adjoint STFT of G: the Hermitian completions of the two frames' G ride as re / im of
// ONE inverse transform, the result is windowed and overlap-added.  A workgroup owns a contiguous span of hop-sized chunks of
// the PADDED signal and computes every frame that touches it (n/hop - 1 frames of halo per 64 chunks); the frames are added
// into an LDS ring in a fixed order (no floating-point atomics), finished chunks are flushed.  The two n/2-sample borders of
// the padding go to a small buffer and are folded back into the clip by a second kernel (adjoint of the reflection).
//
// Second half of the file: the waveform gradient of the log-mel front end (stage A, melfeat.hip), mst_logmel_backward.
//   L = log(mel + 1e-10), mel[m,f] = sum_k fb[k,m] |X[k,f]|^2, cotangent g on L:
//   w = g / (mel + 1e-10) with mel RECOMPUTED from the recomputed |X|^2 (exp(-L) of the saved output missed the parity rule:
//   stage A's log is the hardware log2, 1e-6 absolute), dP[k,f] = sum_m fb[k,m] w[m,f], G = 2 dP X,
// and the SAME adjoint STFT: logmel_bwd_kernel is mrstft_bwd_kernel with one signal per frame pair and this per-bin
// cotangent.  The cotangent tile of a workgroup's frames (n_mels x (chunks + R - 1)) is staged into LDS once; the filterbank
// enters as a per-bin band table (first mel index, count, up to kBandMax weights: HTK triangles touch at most 2 mels per
// bin) and, for the mel sums, per mel the two runs of bins that hold it as their first / second mel.
#include "common.h"
#include <algorithm>

#include "fft_wave.h"

namespace {
using namespace mstfft;

constexpr int kWaves = 4, kThreads = kWaves * 64, kRound = 2 * kWaves;   // frames per round of a workgroup
constexpr int kChunksPerBlock = 64;
constexpr int kFwdMaxBlocks = 2048;   // DetAcc takes up to 2^14 contributions
constexpr int kMaxRes = 16;
constexpr int kBorder = 1024;         // floats per border and row (n_fft / 2 at most)
constexpr int kMelMax = 256, kMelRounds = kMelMax / 64;   // log-mel backward: one lane per mel, kMelRounds mels per lane

template <int N>
struct Geo {
  static constexpr int NC = N == 2048 ? 1024 : N;   // complex length of the wave FFT
  static constexpr int NF = N / NC, NCR = NC / 64, REGS = N / 64, SCR = N + N / 8, TW = FftPlan<NC>::TW;
  static constexpr int TWD = N == 2048 ? 1024 : 0, NB = N / 128 + 1;
  static constexpr size_t kLds = (size_t)(TW + TWD) * 8 + (size_t)N * 4 + (size_t)kWaves * SCR * 8;
  // The backward kernels keep more behind kLds, in floats from Lds::acc: the overlap-add ring of kRound + R - 1 hop-sized
  // chunks, and behind the ring (log-mel backward only) the waves' wv[2][kMelMax] and the cotangent tile gt[n_mels][wstride].
  static constexpr int ring(int R, int hop) { return (kRound + R - 1) * hop; }
  static constexpr int kWv = 0, kGt = kWv + 2 * kWaves * kMelMax;
  static constexpr size_t bwd_lds(int R, int hop) { return kLds + (size_t)ring(R, hop) * 4; }
  static constexpr size_t logmel_bwd_lds(int R, int hop, int n_mels, int wstride) { return bwd_lds(R, hop) + ((size_t)kGt + (size_t)n_mels * wstride) * 4; }
};

// element a lane holds in register r before the first pass / after the last pass
template <int N>
__device__ __forceinline__ int in_idx(int r, int lane) {
  if constexpr (N == 2048) return 2 * (lane + 64 * in_q<1024>(r & 15)) + (r >> 4);
  else return lane + 64 * in_q<N>(r);
}
template <int N>
__device__ __forceinline__ int out_idx(int r, int lane) {
  constexpr int NC = Geo<N>::NC, RL = FftPlan<NC>::RL, NBFL = NC / RL / 64;
  const int rr = r % (NC / 64);
  return lane + 64 * ((rr / RL) + (rr % RL) * NBFL) + (N == 2048 ? 1024 * (r / (NC / 64)) : 0);
}

__device__ __forceinline__ void wsync() {   // the wave's LDS traffic before / after this point stays there
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int N>
struct Lds {
  float2* tw;    // FftPlan<NC> twiddles
  float2* twd;   // N == 2048: W_2048^k, k < 1024
  float* win;    // [N]
  float2* scr;   // this wave's scratch [SCR]
  float* acc;    // backward: ring of chunks
  __device__ Lds(unsigned char* smem, int wave) {
    using G = Geo<N>;
    tw = reinterpret_cast<float2*>(smem);
    twd = tw + G::TW;
    float2* s0 = twd + G::TWD;
    scr = s0 + wave * G::SCR;
    win = reinterpret_cast<float*>(s0 + kWaves * G::SCR);
    acc = win + N;
  }
  __device__ void fill(const float* window, int tid) {
    fill_twiddles<Geo<N>::NC>(tw, tid, kThreads);
    if constexpr (N == 2048)
      for (int k = tid; k < 1024; k += kThreads) {
        double sn, cs;
        sincospi(-2.0 * (double)k / 2048.0, &sn, &cs);
        twd[k] = make_float2((float)cs, (float)sn);
      }
    for (int i = tid; i < N; i += kThreads) win[i] = window[i];
  }
};

template <int N>
__device__ __forceinline__ void wave_fft(float2 (&v)[Geo<N>::NF][Geo<N>::NCR], const Lds<N>& l, int lane) {
  using G = Geo<N>;
  wsync();
  FftPlan<G::NC>::template run<G::NF>(v, l.scr, l.tw, lane);
  if constexpr (N == 2048) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float2 t = cmul(v[1][i], l.twd[out_idx<N>(i, lane)]), e = v[0][i];
      v[0][i] = cadd(e, t);
      v[1][i] = csub(e, t);
    }
  }
  wsync();
}

__device__ __forceinline__ int reflect(int t, int T) { return t < 0 ? -t : (t >= T ? 2 * (T - 1) - t : t); }

// windowed frames starting at sample `start` (re) and `start + hop` (im, zero without a second frame) of one row
template <int N>
__device__ __forceinline__ void load_pair(const float* __restrict__ s, int T, int start, int hop, bool hasB, const Lds<N>& l,
                                          float2 (&v)[Geo<N>::NF][Geo<N>::NCR], int lane) {
  using G = Geo<N>;
  const bool inner = hasB && start >= 0 && start + hop + N <= T;   // wave-uniform
#pragma unroll
  for (int r = 0; r < G::REGS; ++r) {
    const int n = in_idx<N>(r, lane);
    const float w = l.win[n];
    const int ta = inner ? start + n : reflect(start + n, T);
    const int tb = !hasB ? ta : (inner ? start + hop + n : reflect(start + hop + n, T));   // (no read past the row without a frame)
    const float a = s[ta], b = hasB ? s[tb] : 0.f;
    v[r / G::NCR][r % G::NCR] = make_float2(a * w, b * w);
  }
}

// Z = FFT(a + i b) in registers -> the one-sided spectra of a and b; bin k = lane + 64 j in slot j, Nyquist in the last slot of lane 0
template <int N>
__device__ __forceinline__ void split_pair(const float2 (&v)[Geo<N>::NF][Geo<N>::NCR], const Lds<N>& l, int lane,
                                           float2 (&SA)[Geo<N>::NB], float2 (&SB)[Geo<N>::NB]) {
  using G = Geo<N>;
#pragma unroll
  for (int r = 0; r < G::REGS; ++r) l.scr[pad8(out_idx<N>(r, lane))] = v[r / G::NCR][r % G::NCR];
  wsync();
#pragma unroll
  for (int j = 0; j < G::NB - 1; ++j) {
    const int k = lane + 64 * j;
    const float2 a = l.scr[pad8(k)], b = l.scr[pad8((N - k) & (N - 1))];
    SA[j] = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    SB[j] = make_float2(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
  }
  const float2 q = l.scr[pad8(N / 2)];
  SA[G::NB - 1] = make_float2(lane == 0 ? q.x : 0.f, 0.f);
  SB[G::NB - 1] = make_float2(lane == 0 ? q.y : 0.f, 0.f);
  wsync();
}

__device__ __forceinline__ float cabs2(float2 z) { return sqrtf(fmaf(z.x, z.x, z.y * z.y)); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct FwdParams {
  const float* x;
  const float* y;
  const float* window;
  mst::DetAcc* acc;   // [3]: sum (ym - xm)^2, sum ym^2, sum |log(xm + 1e-5) - log(ym + 1e-5)|
  int rows, T, hop, F, pairs_per_row;
};

template <int N>
__global__ __launch_bounds__(kThreads) void mrstft_fwd_kernel(const FwdParams p) {
  using G = Geo<N>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double red[kWaves][3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Lds<N> l(smem, wave);
  l.fill(p.window, tid);
  __syncthreads();
  double d2 = 0.0, y2 = 0.0, la = 0.0;
  const int items = p.rows * p.pairs_per_row;
  for (int it = blockIdx.x * kWaves + wave; it < items; it += gridDim.x * kWaves) {
    const int row = it / p.pairs_per_row, f = 2 * (it % p.pairs_per_row);
    const bool hasB = f + 1 < p.F;
    const int start = f * p.hop - N / 2;
    float2 v[G::NF][G::NCR], SA[G::NB], SB[G::NB];
    float xa[G::NB], xb[G::NB];
    load_pair<N>(p.x + (size_t)row * p.T, p.T, start, p.hop, hasB, l, v, lane);
    wave_fft<N>(v, l, lane);
    split_pair<N>(v, l, lane, SA, SB);
#pragma unroll
    for (int j = 0; j < G::NB; ++j) xa[j] = cabs2(SA[j]), xb[j] = cabs2(SB[j]);
    load_pair<N>(p.y + (size_t)row * p.T, p.T, start, p.hop, hasB, l, v, lane);
    wave_fft<N>(v, l, lane);
    split_pair<N>(v, l, lane, SA, SB);
#pragma unroll
    for (int j = 0; j < G::NB; ++j) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (e && !hasB) continue;   // no second frame: its "spectrum" is the rounding residue of the split, not zero
        const float xm = e ? xb[j] : xa[j], ym = cabs2(e ? SB[j] : SA[j]);
        const float d = ym - xm, lg = fabsf(logf(xm + 1e-5f) - logf(ym + 1e-5f));
        d2 += (double)d * (double)d;
        y2 += (double)ym * (double)ym;
        la += (double)lg;
      }
    }
  }
  d2 = wave_sum_d(d2), y2 = wave_sum_d(y2), la = wave_sum_d(la);
  if (lane == 0) red[wave][0] = d2, red[wave][1] = y2, red[wave][2] = la;
  __syncthreads();
  if (tid < 3) {
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) s += red[w][tid];
    mst::det_add(p.acc + tid, s);
  }
}

// out: [0] loss, [1 + 2 r + {0, 1}] (sc, lg) of resolution r, [1 + 2 n + 2 r + {0, 1}] (||ym - xm||, ||ym||) for the backward pass
struct BinCounts {
  double v[kMaxRes];
};
__global__ void mrstft_finish_kernel(const mst::DetAcc* acc, int n_res, const BinCounts nbins, float sc_w, float log_w, float* out) {
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int r = 0; r < n_res; ++r) {
    const double dn = sqrt(mst::det_get(acc[3 * r])), yn = sqrt(mst::det_get(acc[3 * r + 1]));
    const double sc = dn / (yn + 1e-8), lg = mst::det_get(acc[3 * r + 2]) / nbins.v[r];
    out[1 + 2 * r] = (float)sc;
    out[2 + 2 * r] = (float)lg;
    out[1 + 2 * n_res + 2 * r] = (float)dn;
    out[2 + 2 * n_res + 2 * r] = (float)yn;
    total += (double)sc_w * sc + (double)log_w * lg;
  }
  out[0] = (float)(total / n_res);
}

struct BwdParams {
  const float* x;
  const float* y;
  const float* window;
  const float* norms;   // dev [2]: ||ym - xm||, ||ym|| of this resolution (from the forward pass)
  float* grad;          // [rows][T]
  float* border;        // [rows][2][kBorder]: cotangent of the left padding (sample -1 - j) and of the right (sample T + j)
  int rows, T, hop, lh, R, F, nchunks, blocks_per_row, accumulate;
  float sc_w, log_w_over_n;
};

template <int N>
__global__ __launch_bounds__(kThreads) void mrstft_bwd_kernel(const BwdParams p) {
  using G = Geo<N>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Lds<N> l(smem, wave);
  l.fill(p.window, tid);
  const int hop = p.hop, lh = p.lh, R = p.R, nslot = kRound + R - 1;
  for (int i = tid; i < G::ring(R, hop); i += kThreads) l.acc[i] = 0.f;
  const int row = blockIdx.x / p.blocks_per_row, blk = blockIdx.x % p.blocks_per_row;
  const int c0 = blk * kChunksPerBlock, c1 = min(c0 + kChunksPerBlock, p.nchunks);
  const int fa = max(0, c0 - R + 1), fb = min(p.F - 1, c1 - 1);
  const float dn = p.norms[0], yn = p.norms[1];
  const float ksc = dn > 0.f ? p.sc_w / (dn * (yn + 1e-8f)) : 0.f, klog = p.log_w_over_n;
  const float* xr = p.x + (size_t)row * p.T;
  const float* yr = p.y + (size_t)row * p.T;
  float* gr = p.grad + (size_t)row * p.T;
  float* bl = p.border + (size_t)row * 2 * kBorder;
  __syncthreads();
  for (int fr0 = fa; fr0 < c1; fr0 += kRound) {
    const int gA = fr0 + 2 * wave;
    const bool hasA = gA <= fb, hasB = gA + 1 <= fb;
    float2 v[G::NF][G::NCR];
    if (hasA) {   // wave-uniform
      const int start = gA * hop - N / 2;
      float2 XA[G::NB], XB[G::NB], SA[G::NB], SB[G::NB];
      load_pair<N>(xr, p.T, start, hop, hasB, l, v, lane);
      wave_fft<N>(v, l, lane);
      split_pair<N>(v, l, lane, XA, XB);
      load_pair<N>(yr, p.T, start, hop, hasB, l, v, lane);
      wave_fft<N>(v, l, lane);
      split_pair<N>(v, l, lane, SA, SB);
      // cotangent of the two spectra, packed: conj(H), H = herm(G_A) + i herm(G_B)
#pragma unroll
      for (int j = 0; j < G::NB; ++j) {
        float2 g[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float2 X = e ? XB[j] : XA[j];
          const float xm = cabs2(X), ym = cabs2(e ? SB[j] : SA[j]);
          const float d = ym - xm, lg = logf(xm + 1e-5f) - logf(ym + 1e-5f);
          const float sg = lg > 0.f ? 1.f : (lg < 0.f ? -1.f : 0.f);
          const float c = -ksc * d + klog * sg / (xm + 1e-5f);
          g[e] = (xm > 0.f && !(e && !hasB)) ? make_float2(c * (X.x / xm), c * (X.y / xm)) : make_float2(0.f, 0.f);   // (no frame: no cotangent)
        }
        const float ar = g[0].x, ai = g[0].y, br = g[1].x, bi = g[1].y;
        if (j == G::NB - 1) {
          if (lane == 0) l.scr[pad8(N / 2)] = make_float2(ar, -br);
        } else {
          const int k = lane + 64 * j;
          if (k == 0) {
            l.scr[pad8(0)] = make_float2(ar, -br);
          } else {
            l.scr[pad8(k)] = make_float2(0.5f * (ar - bi), -0.5f * (ai + br));
            l.scr[pad8(N - k)] = make_float2(0.5f * (ar + bi), 0.5f * (ai - br));
          }
        }
      }
      wsync();
#pragma unroll
      for (int r = 0; r < G::REGS; ++r) v[r / G::NCR][r % G::NCR] = l.scr[pad8(in_idx<N>(r, lane))];
      wave_fft<N>(v, l, lane);   // = g_A[n] - i g_B[n]
    }
    // overlap-add in a fixed order: in phase ph the frames fr0 + ph (mod R) -- R frames apart, they do not overlap
    for (int ph = 0; ph < R; ++ph) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int g = gA + e;
        if ((e ? hasB : hasA) && ((g - fr0) & (R - 1)) == ph) {   // wave-uniform
#pragma unroll
          for (int r = 0; r < G::REGS; ++r) {
            const int nb = out_idx<N>(r, 0);   // lane + 64 q stays inside one chunk: hop is a multiple of 64
            const int slot = (g + (nb >> lh)) % nslot;
            const float2 z = v[r / G::NCR][r % G::NCR];
            l.acc[slot * hop + (nb & (hop - 1)) + lane] += l.win[nb + lane] * (e ? -z.y : z.x);
          }
        }
      }
      __syncthreads();
    }
    // chunks [fr0, fr0 + kRound) are complete: no later frame reaches them
    const int nfl = min(fr0 + kRound, c1) - fr0;
    for (int i = tid; i < nfl * hop; i += kThreads) {
      const int c = fr0 + (i >> lh), off = i & (hop - 1);
      float* a = l.acc + (c % nslot) * hop + off;
      const float val = *a;
      *a = 0.f;
      const int pp = c * hop + off;
      if (c >= c0 && pp < p.T + N) {
        const int t = pp - N / 2;
        if (t < 0) bl[-t - 1] = val;
        else if (t >= p.T) bl[kBorder + t - p.T] = val;
        else gr[t] = p.accumulate ? gr[t] + val : val;
      }
    }
    __syncthreads();
  }
}

// adjoint of the reflect padding: sample -1 - j folds onto 1 + j, sample T + j onto T - 2 - j
__global__ __launch_bounds__(256) void mrstft_fold_kernel(float* grad, const float* border, int T, int half) {
  float* g = grad + (size_t)blockIdx.x * T;
  const float* b = border + (size_t)blockIdx.x * 2 * kBorder;
  for (int j = threadIdx.x; j < half; j += 256) g[1 + j] += b[j];
  __syncthreads();
  for (int j = threadIdx.x; j < half; j += 256) g[T - 2 - j] += b[kBorder + j];
}

__global__ __launch_bounds__(256) void mrstft_scale_kernel(float* grad, size_t n, const float* scale, float inv_res) {
  const float s = scale ? *scale : 1.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) grad[i] = s * (grad[i] * inv_res);
}

int log2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

template <int N>
hipError_t launch_fwd(const FwdParams& p, int grid, hipStream_t st) {
  return mst::launch_lds<mrstft_fwd_kernel<N>>(dim3(grid), dim3(kThreads), Geo<N>::kLds, st, p);
}
template <int N>
hipError_t launch_bwd(const BwdParams& p, int grid, hipStream_t st) {
  return mst::launch_lds<mrstft_bwd_kernel<N>>(dim3(grid), dim3(kThreads), Geo<N>::bwd_lds(p.R, p.hop), st, p);
}

size_t acc_bytes(int n_res) { return mst::align_up((size_t)3 * n_res * sizeof(mst::DetAcc), 256); }

int check_args(const char* who, int rows, int T, int n_res, const int* fft, const int* hop) {
  MST_REQUIRE(fft && hop, "%s: NULL argument", who);
  MST_REQUIRE(n_res >= 1 && n_res <= kMaxRes, "%s: n_res=%d outside 1..%d", who, n_res, kMaxRes);
  MST_REQUIRE(rows > 0 && rows <= (1 << 20) && T > 0 && T < (1 << 30), "%s: bad sizes rows=%d T=%d", who, rows, T);
  for (int r = 0; r < n_res; ++r) {
    MST_REQUIRE(fft[r] == 512 || fft[r] == 1024 || fft[r] == 2048, "%s: n_fft=%d is not 512, 1024 or 2048", who, fft[r]);
    MST_REQUIRE(hop[r] == fft[r] / 8 || hop[r] == fft[r] / 4 || hop[r] == fft[r] / 2, "%s: hop=%d is not n_fft/8, /4 or /2 (n_fft=%d)",
                who, hop[r], fft[r]);
    MST_REQUIRE(T > fft[r] / 2, "%s: T=%d needs more than n_fft/2 = %d samples (reflect padding)", who, T, fft[r] / 2);
  }
  return MST_OK;
}

}  // namespace

extern "C" {

size_t mst_mrstft_workspace_bytes(int n_res, const int* fft, const int* hop, int rows, int T) {
  if (n_res <= 0 || rows <= 0 || T <= 0 || !fft || !hop) return 0;
  return acc_bytes(n_res) + mst::align_up((size_t)rows * 2 * kBorder * sizeof(float), 256);
}

int mst_mrstft_forward(const float* x, const float* y, int rows, int T, int n_res, const int* fft, const int* hop,
                       const float* const* windows, float sc_weight, float log_weight, float* out, void* workspace,
                       size_t workspace_bytes, void* stream) {
  MST_REQUIRE(x && y && windows && out, "mst_mrstft_forward: NULL argument");
  if (int rc = check_args("mst_mrstft_forward", rows, T, n_res, fft, hop)) return rc;
  const size_t need = mst_mrstft_workspace_bytes(n_res, fft, hop, rows, T);
  if (!workspace || workspace_bytes < need)
    return mst::fail(MST_ENOMEM, "mst_mrstft_forward: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  mst::DetAcc* acc = reinterpret_cast<mst::DetAcc*>(workspace);
  MST_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)3 * n_res * sizeof(mst::DetAcc), st));
  BinCounts nb;
  for (int r = 0; r < kMaxRes; ++r) nb.v[r] = 1.0;
  for (int r = 0; r < n_res; ++r) {
    MST_REQUIRE(windows[r], "mst_mrstft_forward: NULL window table %d", r);
    FwdParams p;
    p.x = x, p.y = y, p.window = windows[r], p.acc = acc + 3 * r;
    p.rows = rows, p.T = T, p.hop = hop[r], p.F = 1 + T / hop[r], p.pairs_per_row = (p.F + 1) / 2;
    nb.v[r] = (double)rows * p.F * (fft[r] / 2 + 1);
    const long long items = (long long)rows * p.pairs_per_row;
    MST_REQUIRE(items < (1LL << 31), "mst_mrstft_forward: %lld frame pairs", items);
    const int grid = (int)std::min<long long>((items + kWaves - 1) / kWaves, kFwdMaxBlocks);
    MST_HIP_CHECK(fft[r] == 512 ? launch_fwd<512>(p, grid, st) : fft[r] == 1024 ? launch_fwd<1024>(p, grid, st) : launch_fwd<2048>(p, grid, st));
  }
  hipLaunchKernelGGL(mrstft_finish_kernel, dim3(1), dim3(64), 0, st, acc, n_res, nb, sc_weight, log_weight, out);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_mrstft_backward(const float* x, const float* y, int rows, int T, int n_res, const int* fft, const int* hop,
                        const float* const* windows, float sc_weight, float log_weight, const float* fwd_out,
                        const float* grad_scale, float* grad_x, void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(x && y && windows && fwd_out && grad_x, "mst_mrstft_backward: NULL argument");
  if (int rc = check_args("mst_mrstft_backward", rows, T, n_res, fft, hop)) return rc;
  const size_t need = mst_mrstft_workspace_bytes(n_res, fft, hop, rows, T);
  if (!workspace || workspace_bytes < need)
    return mst::fail(MST_ENOMEM, "mst_mrstft_backward: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* border = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + acc_bytes(n_res));
  for (int r = 0; r < n_res; ++r) {
    MST_REQUIRE(windows[r], "mst_mrstft_backward: NULL window table %d", r);
    BwdParams p;
    p.x = x, p.y = y, p.window = windows[r], p.norms = fwd_out + 1 + 2 * n_res + 2 * r, p.grad = grad_x, p.border = border;
    p.rows = rows, p.T = T, p.hop = hop[r], p.lh = log2_exact(hop[r]), p.R = fft[r] / hop[r], p.F = 1 + T / hop[r];
    p.nchunks = (int)(((long long)T + fft[r] + hop[r] - 1) / hop[r]);
    p.blocks_per_row = (p.nchunks + kChunksPerBlock - 1) / kChunksPerBlock;
    p.accumulate = r > 0;
    p.sc_w = sc_weight;
    p.log_w_over_n = (float)((double)log_weight / ((double)rows * p.F * (fft[r] / 2 + 1)));
    const long long grid = (long long)rows * p.blocks_per_row;
    MST_REQUIRE(grid < (1LL << 31), "mst_mrstft_backward: %lld workgroups", grid);
    MST_HIP_CHECK(fft[r] == 512 ? launch_bwd<512>(p, (int)grid, st) : fft[r] == 1024 ? launch_bwd<1024>(p, (int)grid, st) : launch_bwd<2048>(p, (int)grid, st));
    hipLaunchKernelGGL(mrstft_fold_kernel, dim3(rows), dim3(256), 0, st, grad_x, border, T, fft[r] / 2);
  }
  const size_t n = (size_t)rows * T;
  hipLaunchKernelGGL(mrstft_scale_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, grad_x, n, grad_scale,
                     1.0f / (float)n_res);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// Log-mel front end: gradient to the waveform
namespace {

constexpr int kBandMax = MST_LOGMEL_BAND_MAX;   // mel weights per bin the kernel carries
constexpr size_t kMaxLds = 160 * 1024;

struct LogmelBwdParams {
  const float* x;        // [rows][T]
  const float* g;        // [rows][n_mels][F] cotangent on the log-mel (kPower: on the mel POWER, used as w as it stands)
  const float* window;
  const int2* band;      // [N / 2 + 1] (first mel index, count <= kBandMax)
  const float2* bandw;   // [N / 2 + 1] weights of (first, first + 1), zero where absent
  const int4* melr;      // [n_mels] bins that hold mel m as their first mel (start, count) and as their second (start, count)
  float* grad;           // [rows][T]
  float* border;         // [rows][2][kBorder]
  int rows, T, hop, lh, R, F, nchunks, cpb, blocks_per_row, accumulate, n_mels, wstride;
};

// Mel power of the two frames of a pair, as the log-mel backward recomputes it: every bin lays out its power times its two mel
// weights, one lane per mel adds up the bins of its triangle (rising half: bins whose second mel it is; falling half: bins whose
// first) in bin order.  Uses the wave's scratch; the caller fences before the scratch is written again.
template <int N>
__device__ __forceinline__ void mel_power_pair(const float2 (&XA)[Geo<N>::NB], const float2 (&XB)[Geo<N>::NB], const float2* __restrict__ bandw,
                                               const int4 (&mr)[kMelRounds], int n_mels, const Lds<N>& l, int lane,
                                               float (&sa)[kMelRounds], float (&sb)[kMelRounds]) {
  using G = Geo<N>;
  float4* Q = reinterpret_cast<float4*>(l.scr);   // per bin (w0 P_A, w0 P_B, w1 P_A, w1 P_B): the power spectrum times its two mel weights
#pragma unroll
  for (int j = 0; j < G::NB; ++j) {
    const int k = j == G::NB - 1 ? N / 2 : lane + 64 * j;
    const float2 bw = bandw[k];
    const float pa = fmaf(XA[j].x, XA[j].x, XA[j].y * XA[j].y), pb = fmaf(XB[j].x, XB[j].x, XB[j].y * XB[j].y);
    if (j < G::NB - 1 || lane == 0) Q[k] = make_float4(bw.x * pa, bw.x * pb, bw.y * pa, bw.y * pb);
  }
  wsync();
#pragma unroll
  for (int q = 0; q < kMelRounds; ++q) {
    sa[q] = sb[q] = 0.f;
    if (lane + 64 * q < n_mels) {
      for (int i = 0; i < mr[q].w; ++i) {
        const float4 t = Q[mr[q].z + i];
        sa[q] += t.z, sb[q] += t.w;
      }
      for (int i = 0; i < mr[q].y; ++i) {
        const float4 t = Q[mr[q].x + i];
        sa[q] += t.x, sb[q] += t.y;
      }
    }
  }
}

// kPower: the cotangent arrives on the mel POWER (w = g, nothing recomputed but the spectra) -- mst_melfeat_backward
template <int N, bool kPower>
__global__ __launch_bounds__(kThreads) void logmel_bwd_kernel(const LogmelBwdParams p) {
  using G = Geo<N>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Lds<N> l(smem, wave);
  l.fill(p.window, tid);
  const int hop = p.hop, lh = p.lh, R = p.R, nslot = kRound + R - 1;
  for (int i = tid; i < G::ring(R, hop); i += kThreads) l.acc[i] = 0.f;
  float* behind = l.acc + G::ring(R, hop);
  float2* wv = reinterpret_cast<float2*>(behind + G::kWv) + wave * kMelMax;   // this wave's w = g / (mel + 1e-10), frames (A, B)
  float* gt = behind + G::kGt;   // cotangent tile of this workgroup's frames, [n_mels][wstride]
  const int row = blockIdx.x / p.blocks_per_row, blk = blockIdx.x % p.blocks_per_row;
  const int c0 = blk * p.cpb, c1 = min(c0 + p.cpb, p.nchunks);
  const int fa = max(0, c0 - R + 1), fb = min(p.F - 1, c1 - 1);
  const int nfr = fb - fa + 1, ws = p.wstride;   // nfr <= cpb + R - 1 <= wstride (<= 0: a tail block no frame reaches)
  const float* xr = p.x + (size_t)row * p.T;
  float* gr = p.grad + (size_t)row * p.T;
  float* bl = p.border + (size_t)row * 2 * kBorder;
  if (nfr > 0) {   // contiguous runs along f of the (rows, n_mels, F) layout
    const size_t base = (size_t)row * p.n_mels * p.F + fa;
    for (int i = tid; i < p.n_mels * nfr; i += kThreads) {
      const int m = i / nfr, f = i - m * nfr;
      const size_t at = base + (size_t)m * p.F + f;
      gt[m * ws + f] = p.g[at];
    }
  }
  int4 mr[kMelRounds];   // the bin ranges of this lane's mels
#pragma unroll
  for (int q = 0; q < kMelRounds; ++q) mr[q] = lane + 64 * q < p.n_mels ? p.melr[lane + 64 * q] : make_int4(0, 0, 0, 0);
  __syncthreads();
  for (int fr0 = fa; fr0 < c1; fr0 += kRound) {
    const int gA = fr0 + 2 * wave;
    const bool hasA = gA <= fb, hasB = gA + 1 <= fb;
    float2 v[G::NF][G::NCR];
    // a frame whose cotangent is zero in every bin adds NOTHING (its true gradient is exactly 0, while its half of the packed
    // inverse transform holds the other frame's rounding residue)
    bool nzA = false, nzB = false;
    if (hasA) {   // wave-uniform
      const int start = gA * hop - N / 2;
      float2 XA[G::NB], XB[G::NB];
      load_pair<N>(xr, p.T, start, hop, hasB, l, v, lane);
      wave_fft<N>(v, l, lane);
      split_pair<N>(v, l, lane, XA, XB);
      // w of the two frames: g / (mel + 1e-10) with the mel power recomputed, or g itself (cotangent on the power)
      const float* ga = gt + (gA - fa);
      const float* gb = ga + (hasB ? 1 : 0);   // (no second frame: no read past the tile)
      if constexpr (kPower) {
#pragma unroll
        for (int q = 0; q < kMelRounds; ++q) {
          const int m = lane + 64 * q;
          if (m < p.n_mels) wv[m] = make_float2(ga[m * ws], gb[m * ws]);
        }
      } else {
        float sa[kMelRounds], sb[kMelRounds];
        mel_power_pair<N>(XA, XB, p.bandw, mr, p.n_mels, l, lane, sa, sb);
#pragma unroll
        for (int q = 0; q < kMelRounds; ++q) {
          const int m = lane + 64 * q;
          if (m < p.n_mels) wv[m] = make_float2(ga[m * ws] / (sa[q] + 1e-10f), gb[m * ws] / (sb[q] + 1e-10f));
        }
      }
      wsync();
      // cotangent of the two spectra G = 2 dP X, packed: conj(H), H = herm(G_A) + i herm(G_B)
#pragma unroll
      for (int j = 0; j < G::NB; ++j) {
        const int k = j == G::NB - 1 ? N / 2 : lane + 64 * j;
        const int2 bd = p.band[k];
        const float2 bw = p.bandw[k];
        float da = 0.f, db = 0.f;
        if (bd.y > 0) {
          const float2 w = wv[bd.x];
          da = bw.x * w.x, db = bw.x * w.y;
        }
        if (bd.y > 1) {
          const float2 w = wv[bd.x + 1];
          da = fmaf(bw.y, w.x, da), db = fmaf(bw.y, w.y, db);
        }
        da *= 2.f;
        db = hasB ? 2.f * db : 0.f;   // (no frame: no cotangent)
        const float ar = da * XA[j].x, ai = da * XA[j].y, br = db * XB[j].x, bi = db * XB[j].y;
        nzA |= ar != 0.f || ai != 0.f;
        nzB |= br != 0.f || bi != 0.f;
        if (j == G::NB - 1) {
          if (lane == 0) l.scr[pad8(N / 2)] = make_float2(ar, -br);
        } else {
          if (k == 0) {
            l.scr[pad8(0)] = make_float2(ar, -br);
          } else {
            l.scr[pad8(k)] = make_float2(0.5f * (ar - bi), -0.5f * (ai + br));
            l.scr[pad8(N - k)] = make_float2(0.5f * (ar + bi), 0.5f * (ai - br));
          }
        }
      }
      wsync();
#pragma unroll
      for (int r = 0; r < G::REGS; ++r) v[r / G::NCR][r % G::NCR] = l.scr[pad8(in_idx<N>(r, lane))];
      wave_fft<N>(v, l, lane);   // = g_A[n] - i g_B[n]
      nzA = __any(nzA), nzB = __any(nzB);
    }
    // overlap-add in a fixed order: in phase ph the frames fr0 + ph (mod R) -- R frames apart, they do not overlap
    for (int ph = 0; ph < R; ++ph) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int g = gA + e;
        if ((e ? hasB && nzB : hasA && nzA) && ((g - fr0) & (R - 1)) == ph) {   // wave-uniform
#pragma unroll
          for (int r = 0; r < G::REGS; ++r) {
            const int nb = out_idx<N>(r, 0);   // lane + 64 q stays inside one chunk: hop is a multiple of 64
            const int slot = (g + (nb >> lh)) % nslot;
            const float2 z = v[r / G::NCR][r % G::NCR];
            l.acc[slot * hop + (nb & (hop - 1)) + lane] += l.win[nb + lane] * (e ? -z.y : z.x);
          }
        }
      }
      __syncthreads();
    }
    // chunks [fr0, fr0 + kRound) are complete: no later frame reaches them
    const int nfl = min(fr0 + kRound, c1) - fr0;
    for (int i = tid; i < nfl * hop; i += kThreads) {
      const int c = fr0 + (i >> lh), off = i & (hop - 1);
      float* a = l.acc + (c % nslot) * hop + off;
      const float val = *a;
      *a = 0.f;
      const int pp = c * hop + off;
      if (c >= c0 && pp < p.T + N) {
        const int t = pp - N / 2;
        if (t < 0) bl[-t - 1] = val;
        else if (t >= p.T) bl[kBorder + t - p.T] = val;
        else gr[t] = p.accumulate ? gr[t] + val : val;
      }
    }
    __syncthreads();
  }
}

// row pitch of the cotangent tile: the cpb + R - 1 frames a workgroup reads, made odd
int wstride_of(int cpb, int R) { return (cpb + R - 1) | 1; }

template <int N, bool kPower = false>
int launch_logmel_bwd(LogmelBwdParams& p, hipStream_t st) {
  // a workgroup owns 64 hop-sized chunks; fewer where the cotangent tile of 64 + R - 1 frames would not fit the CU's LDS next to
  // the transform's tables (n_fft = 2048 with more than ~118 mels)
  p.cpb = kChunksPerBlock;
  auto lds_of = [&](int cpb) { return Geo<N>::logmel_bwd_lds(p.R, p.hop, p.n_mels, wstride_of(cpb, p.R)); };
  while (p.cpb > 8 && lds_of(p.cpb) > kMaxLds) p.cpb /= 2;
  const size_t lds = lds_of(p.cpb);
  MST_REQUIRE(lds <= kMaxLds, "mst_logmel_backward: LDS %zu B exceeds 160 KiB (n_fft=%d hop=%d n_mels=%d)", lds, N, p.hop, p.n_mels);
  p.wstride = wstride_of(p.cpb, p.R);
  p.blocks_per_row = (p.nchunks + p.cpb - 1) / p.cpb;
  const long long grid = (long long)p.rows * p.blocks_per_row;
  MST_REQUIRE(grid < (1LL << 31), "mst_logmel_backward: %lld workgroups", grid);
  MST_HIP_CHECK(mst::launch_lds<logmel_bwd_kernel<N, kPower>>(dim3((unsigned)grid), dim3(kThreads), lds, st, p));
  return MST_OK;
}

}  // namespace

extern "C" {

size_t mst_logmel_backward_workspace_bytes(int rows) {
  return rows > 0 ? mst::align_up((size_t)rows * 2 * kBorder * sizeof(float), 256) : 0;
}

int mst_logmel_backward(const float* x, const float* grad_logmel, int rows, int T, int n_fft, int hop, int n_mels,
                        const float* window, const int32_t* band, const float* band_weight, int band_width,
                        const int32_t* mel_ranges, float* grad_x, int accumulate, void* workspace, size_t workspace_bytes,
                        void* stream) {
  MST_REQUIRE(x && grad_logmel && window && band && band_weight && mel_ranges && grad_x, "mst_logmel_backward: NULL argument");
  MST_REQUIRE(n_fft == 1024 || n_fft == 2048, "mst_logmel_backward: n_fft=%d is not 1024 or 2048", n_fft);
  MST_REQUIRE(hop == n_fft / 8 || hop == n_fft / 4 || hop == n_fft / 2, "mst_logmel_backward: hop=%d is not n_fft/8, /4 or /2 (n_fft=%d)",
              hop, n_fft);
  MST_REQUIRE(n_mels >= 1 && n_mels <= kMelMax, "mst_logmel_backward: n_mels=%d outside 1..%d", n_mels, kMelMax);
  MST_REQUIRE(rows > 0 && rows <= (1 << 20) && T > 0 && T < (1 << 30), "mst_logmel_backward: bad sizes rows=%d T=%d", rows, T);
  MST_REQUIRE(T > n_fft / 2, "mst_logmel_backward: T=%d needs more than n_fft/2 = %d samples (reflect padding)", T, n_fft / 2);
  MST_REQUIRE(band_width >= 1 && band_width <= kBandMax,
              "mst_logmel_backward: the filterbank's widest band has %d non-zero mel weights on one bin, the kernel carries %d "
              "(HTK triangles have 2); the table is refused, not truncated", band_width, kBandMax);
  const size_t need = mst_logmel_backward_workspace_bytes(rows);
  if (!workspace || workspace_bytes < need)
    return mst::fail(MST_ENOMEM, "mst_logmel_backward: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LogmelBwdParams p;
  p.x = x, p.g = grad_logmel, p.window = window;
  p.band = reinterpret_cast<const int2*>(band), p.bandw = reinterpret_cast<const float2*>(band_weight);
  p.melr = reinterpret_cast<const int4*>(mel_ranges);
  p.grad = grad_x, p.border = reinterpret_cast<float*>(workspace);
  p.rows = rows, p.T = T, p.hop = hop, p.lh = log2_exact(hop), p.R = n_fft / hop, p.F = 1 + T / hop;
  p.nchunks = (int)(((long long)T + n_fft + hop - 1) / hop);
  p.accumulate = accumulate != 0, p.n_mels = n_mels;
  p.cpb = p.blocks_per_row = p.wstride = 0;
  if (int rc = n_fft == 1024 ? launch_logmel_bwd<1024>(p, st) : launch_logmel_bwd<2048>(p, st)) return rc;
  hipLaunchKernelGGL(mrstft_fold_kernel, dim3(rows), dim3(256), 0, st, grad_x, p.border, T, n_fft / 2);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// Mixing features: gradient to the waveform (mst_melfeat_backward).  Of the 64 features of the default layout 24 carry a
// gradient in the reference (the rest are rebuilt from Python numbers there): per stem rms L/R, crest L/R and rel_loudness --
// functions of a few per-channel scalars (sum x^2, the first arg-max of |x|, sum mix^2) -- and the four masking features,
// means of sigmoid(max_{k != i} S_k - S_i) over the mel power S (channel mean) of the four stems.
//   1. scalars: per channel (8 stem channels + 2 mixture channels of a clip) 32 segments, one workgroup each, fixed-order
//      double sums; the segments are combined in ascending order where the coefficients are formed;
//   2. coefficients: grad = a_row x + m_ch mix + spike at t* -- a_row, m_ch, spike in double per clip;
//   3. one elementwise pass writes (or accumulates) that;
//   4. the mel power of all 8 rows is recomputed into the workspace (mel_power_pair: the log-mel backward's arithmetic),
//   5. one thread per (clip, mel, frame) turns it into the cotangent on the mel power of the 8 rows, plus the log-mel
//      cotangent g_L / (mel + 1e-10) when one arrives in the same backward,
//   6. and the log-mel backward's adjoint stage (logmel_bwd_kernel<N, true>) adds its waveform gradient: ONE adjoint pass.
// A feature whose forward value sits on the clamp (|f| >= 100) or is not finite passes no gradient; a channel with sum x^2 = 0
// gets exact zeros from its own rms / crest / loudness terms (the reference: NaN from sqrt'(0) 0).
namespace {

constexpr int kFeatDim = 64;         // default (basic) layout
constexpr int kScalarThreads = 256, kScalarSegs = 32;   // a channel's samples: 32 segments, one workgroup each
// offsets of the per-stem blocks in the feature vector (keys sorted: bass, drums, masking, other, vocals), rows are v, b, d, o
__device__ __constant__ int kStemOff[4] = {49, 0, 15, 34};
constexpr int kMaskOff = 30;         // masking: vocals, bass, drums, other

struct ChanScalars {   // of one channel (or mixture channel)
  double ss;           // sum x^2
  float xpeak;         // x[t*]
  int tstar;           // first index of max |x|
};
struct RowCoef {
  double a, spike;     // grad[t] = a x[t] + mixc[ch] mix[t] + (t == tstar) spike
  int tstar, pad_;
};

__device__ __forceinline__ float live_cot(const float* g, const float* f, int i) {   // cotangent of feature i, 0 where clamped / NaN
  return fabsf(f[i]) < 100.f ? g[i] : 0.f;
}
__device__ __forceinline__ float mix_at(const float* xc, int ch, int T, int t) {   // sum(stems.values()): ((v + b) + d) + o
  return ((xc[(size_t)ch * T + t] + xc[(size_t)(2 + ch) * T + t]) + xc[(size_t)(4 + ch) * T + t]) + xc[(size_t)(6 + ch) * T + t];
}

// grid (kScalarSegs, B * 10): segment of channel r < 8 of the clip, or of mixture channel r - 8 -> out[channel][segment]
__global__ __launch_bounds__(kScalarThreads) void melfeat_scalars_kernel(const float* __restrict__ x, int T, ChanScalars* __restrict__ out) {
  __shared__ double ssum[kScalarThreads];
  __shared__ float sabs[kScalarThreads];
  __shared__ float sval[kScalarThreads];
  __shared__ int sidx[kScalarThreads];
  const int b = blockIdx.y / 10, r = blockIdx.y % 10, tid = threadIdx.x;
  const int len = (T + kScalarSegs - 1) / kScalarSegs, t0 = blockIdx.x * len, t1 = min(T, t0 + len);
  const float* xc = x + (size_t)b * 8 * T;
  double ss = 0.0;
  float best = -1.f, bval = 0.f;
  int bidx = t0;
  for (int t = t0 + tid; t < t1; t += kScalarThreads) {
    const float v = r < 8 ? xc[(size_t)r * T + t] : mix_at(xc, r - 8, T, t);
    ss += (double)v * (double)v;
    if (fabsf(v) > best) best = fabsf(v), bval = v, bidx = t;   // (strictly greater: the first index of this thread's samples)
  }
  ssum[tid] = ss, sabs[tid] = best, sval[tid] = bval, sidx[tid] = bidx;
  __syncthreads();
  for (int o = kScalarThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      ssum[tid] += ssum[tid + o];
      const bool take = sabs[tid + o] > sabs[tid] || (sabs[tid + o] == sabs[tid] && sidx[tid + o] < sidx[tid]);
      if (take) sabs[tid] = sabs[tid + o], sval[tid] = sval[tid + o], sidx[tid] = sidx[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    ChanScalars s;
    s.ss = ssum[0], s.xpeak = sval[0], s.tstar = sidx[0];
    out[(size_t)blockIdx.y * kScalarSegs + blockIdx.x] = s;
  }
}
// a channel's segments in ascending order: the sum in a fixed order, the FIRST arg-max (strictly greater moves it)
__device__ __forceinline__ ChanScalars chan_scalars(const ChanScalars* __restrict__ seg) {
  ChanScalars s = seg[0];
  for (int k = 1; k < kScalarSegs; ++k) {
    s.ss += seg[k].ss;
    if (fabsf(seg[k].xpeak) > fabsf(s.xpeak)) s.xpeak = seg[k].xpeak, s.tstar = seg[k].tstar;
  }
  return s;
}

// grid B, 64 threads: lanes 0..7 the rows' coefficients, lanes 8, 9 the mixture channels'
__global__ __launch_bounds__(64) void melfeat_coef_kernel(const ChanScalars* __restrict__ sc, const float* __restrict__ g,
                                                          const float* __restrict__ feats, int T, RowCoef* __restrict__ coef,
                                                          double* __restrict__ mixc) {
  const int b = blockIdx.x, r = threadIdx.x;
  __shared__ ChanScalars s[10];
  if (r < 10) s[r] = chan_scalars(sc + ((size_t)b * 10 + r) * kScalarSegs);
  __syncthreads();
  const float* gb = g + (size_t)b * kFeatDim;
  const float* fb = feats + (size_t)b * kFeatDim;
  const double kLog = 10.0 / 2.302585092994045684, dT = (double)T;
  if (r < 8) {
    const int i = r >> 1, c = r & 1, o = kStemOff[i];
    const double ss = s[r].ss, rms = sqrt(ss / dT);
    const double g_rms = live_cot(gb, fb, o + c), g_crest = live_cot(gb, fb, o + 2 + c), g_rel = live_cot(gb, fb, o + 6);
    RowCoef k;
    k.a = k.spike = 0.0, k.tstar = s[r].tstar, k.pad_ = 0;
    if (ss > 0.0) {
      const double peak = fabs((double)s[r].xpeak);
      const double mean2 = (s[2 * i].ss + s[2 * i + 1].ss) / (2.0 * dT);
      k.a = g_rms / (dT * rms) - g_crest * 2.0 * kLog / (dT * rms * (rms + 1e-8)) + g_rel * kLog / (dT * (mean2 + 1e-10));
      k.spike = g_crest * 2.0 * kLog * (s[r].xpeak > 0.f ? 1.0 : -1.0) / peak;
      if (!isfinite(k.a)) k.a = 0.0;
      if (!isfinite(k.spike)) k.spike = 0.0;
    }
    coef[(size_t)b * 8 + r] = k;
  } else if (r < 10) {
    double gs = 0.0;
    for (int i = 0; i < 4; ++i) gs += (double)live_cot(gb, fb, kStemOff[i] + 6);
    const double mean2 = (s[8].ss + s[9].ss) / (2.0 * dT);
    const double m = -gs * kLog / (dT * (mean2 + 1e-10));
    mixc[(size_t)b * 2 + (r - 8)] = isfinite(m) ? m : 0.0;
  }
}

// grid (blocks along T, B * 8)
__global__ __launch_bounds__(256) void melfeat_time_kernel(const float* __restrict__ x, int T, const RowCoef* __restrict__ coef,
                                                           const double* __restrict__ mixc, float* __restrict__ grad, int accumulate) {
  const int row = blockIdx.y, b = row >> 3, r = row & 7;
  const RowCoef k = coef[row];
  const double m = mixc[(size_t)b * 2 + (r & 1)];
  const float* xc = x + (size_t)b * 8 * T;
  float* gr = grad + (size_t)row * T;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < T; t += gridDim.x * 256) {
    double v = k.a * (double)xc[(size_t)r * T + t];
    if (m != 0.0) v += m * (double)mix_at(xc, r & 1, T, t);
    if (t == k.tstar) v += k.spike;
    const float o = (float)v;
    gr[t] = accumulate ? gr[t] + o : o;
  }
}

struct MelpowParams {
  const float* x;
  const float* window;
  const float2* bandw;
  const int4* melr;
  float* P;   // [rows][n_mels][F]
  int rows, T, hop, F, pairs_per_row, n_mels;
};

template <int N>
__global__ __launch_bounds__(kThreads) void melpow_kernel(const MelpowParams p) {
  using G = Geo<N>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Lds<N> l(smem, wave);
  l.fill(p.window, tid);
  int4 mr[kMelRounds];
#pragma unroll
  for (int q = 0; q < kMelRounds; ++q) mr[q] = lane + 64 * q < p.n_mels ? p.melr[lane + 64 * q] : make_int4(0, 0, 0, 0);
  __syncthreads();
  const int items = p.rows * p.pairs_per_row;
  for (int it = blockIdx.x * kWaves + wave; it < items; it += gridDim.x * kWaves) {
    const int row = it / p.pairs_per_row, f = 2 * (it % p.pairs_per_row);
    const bool hasB = f + 1 < p.F;
    float2 v[G::NF][G::NCR], XA[G::NB], XB[G::NB];
    load_pair<N>(p.x + (size_t)row * p.T, p.T, f * p.hop - N / 2, p.hop, hasB, l, v, lane);
    wave_fft<N>(v, l, lane);
    split_pair<N>(v, l, lane, XA, XB);
    float sa[kMelRounds], sb[kMelRounds];
    mel_power_pair<N>(XA, XB, p.bandw, mr, p.n_mels, l, lane, sa, sb);
#pragma unroll
    for (int q = 0; q < kMelRounds; ++q) {
      const int m = lane + 64 * q;
      if (m < p.n_mels) {
        float* o = p.P + ((size_t)row * p.n_mels + m) * p.F + f;
        o[0] = sa[q];
        if (hasB) o[1] = sb[q];
      }
    }
    wsync();
  }
}

// one thread per (clip, mel, frame): P (mel power of the clip's 8 rows) -> W (cotangent on it; + g_L / (P + 1e-10))
__global__ __launch_bounds__(256) void melfeat_cot_kernel(const float* __restrict__ P, const float* __restrict__ gl, const float* __restrict__ g,
                                                          const float* __restrict__ feats, size_t MF, float scale, float* __restrict__ W) {
  const int b = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= MF) return;
  const size_t base = (size_t)b * 8 * MF + i;
  float pv[8], S[4], c[4], cot[4];
  int arg[4];
#pragma unroll
  for (int r = 0; r < 8; ++r) pv[r] = P[base + (size_t)r * MF];
#pragma unroll
  for (int s = 0; s < 4; ++s) S[s] = (pv[2 * s] + pv[2 * s + 1]) * 0.5f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float mx = -1.f;   // S >= 0; the first maximum in stem order without j, as torch.stack(...).max(0) picks
    int am = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k != j && S[k] > mx) mx = S[k], am = k;
    const float sg = 1.f / (1.f + expf(S[j] - mx));
    c[j] = live_cot(g + (size_t)b * kFeatDim, feats + (size_t)b * kFeatDim, kMaskOff + j) * (sg * (1.f - sg));
    arg[j] = am;
    cot[j] = 0.f;
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float t = -c[s];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j != s && arg[j] == s) t += c[j];
    cot[s] = scale * t;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float w = cot[r >> 1];
    if (!(fabsf(w) <= 3.0e38f)) w = 0.f;   // (not finite: inputs that are not)
    if (gl) w += gl[base + (size_t)r * MF] / (pv[r] + 1e-10f);
    W[base + (size_t)r * MF] = w;
  }
}

struct MelfeatBwdLayout {
  size_t border, scalars, coef, mixc, P, W, total;
};
MelfeatBwdLayout melfeat_bwd_layout(int B, int n_mels, int F) {
  MelfeatBwdLayout L;
  size_t o = 0;
  const size_t pf = mst::align_up((size_t)B * 8 * n_mels * F * sizeof(float), 256);
  L.P = o, o += pf;   // first: callers (tests) may read the recomputed mel power back
  L.W = o, o += pf;
  L.border = o, o += mst::align_up((size_t)B * 8 * 2 * kBorder * sizeof(float), 256);
  L.scalars = o, o += mst::align_up((size_t)B * 10 * kScalarSegs * sizeof(ChanScalars), 256);
  L.coef = o, o += mst::align_up((size_t)B * 8 * sizeof(RowCoef), 256);
  L.mixc = o, o += mst::align_up((size_t)B * 2 * sizeof(double), 256);
  L.total = o;
  return L;
}

template <int N>
hipError_t launch_melpow(const MelpowParams& p, int grid, hipStream_t st) {
  return mst::launch_lds<melpow_kernel<N>>(dim3(grid), dim3(kThreads), Geo<N>::kLds, st, p);
}

const char* melfeat_bwd_args(int B, int T, int n_fft, int hop, int n_mels, int feature_dim) {
  static thread_local char why[160];
  if (feature_dim != kFeatDim) {
    snprintf(why, sizeof why, "feature_dim=%d: only the basic 64-feature layout is differentiated (detailed-spectral mode is not)", feature_dim);
    return why;
  }
  if (n_fft != 1024 && n_fft != 2048) return snprintf(why, sizeof why, "n_fft=%d is not 1024 or 2048", n_fft), why;
  if (hop != n_fft / 8 && hop != n_fft / 4 && hop != n_fft / 2)
    return snprintf(why, sizeof why, "hop=%d is not n_fft/8, /4 or /2 (n_fft=%d)", hop, n_fft), why;
  if (n_mels < 1 || n_mels > kMelMax) return snprintf(why, sizeof why, "n_mels=%d outside 1..%d", n_mels, kMelMax), why;
  if (B <= 0 || B > (1 << 12) || T <= 0 || T >= (1 << 30)) return snprintf(why, sizeof why, "bad sizes B=%d T=%d", B, T), why;
  if (T <= n_fft / 2) return snprintf(why, sizeof why, "T=%d needs more than n_fft/2 = %d samples (reflect padding)", T, n_fft / 2), why;
  if ((long long)B * 8 * n_mels * (1 + T / hop) >= (1LL << 31))
    return snprintf(why, sizeof why, "%lld mel-power values exceed 2^31", (long long)B * 8 * n_mels * (1 + T / hop)), why;
  return nullptr;
}

}  // namespace

extern "C" {

size_t mst_melfeat_backward_workspace_bytes(int B, int T, int n_fft, int hop, int n_mels) {
  if (melfeat_bwd_args(B, T, n_fft, hop, n_mels, kFeatDim)) return 0;
  return melfeat_bwd_layout(B, n_mels, 1 + T / hop).total;
}

int mst_melfeat_backward(const float* x, const float* grad_feats, const float* feats, const float* grad_logmel, int B, int T,
                         int n_fft, int hop, int n_mels, int feature_dim, const float* window, const int32_t* band,
                         const float* band_weight, int band_width, const int32_t* mel_ranges, float* grad_x, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(x && grad_feats && feats && window && band && band_weight && mel_ranges && grad_x, "mst_melfeat_backward: NULL argument");
  if (const char* why = melfeat_bwd_args(B, T, n_fft, hop, n_mels, feature_dim)) return mst::fail(MST_EINVAL, "mst_melfeat_backward: %s", why);
  MST_REQUIRE(band_width >= 1 && band_width <= kBandMax,
              "mst_melfeat_backward: the filterbank's widest band has %d non-zero mel weights on one bin, the kernel carries %d "
              "(HTK triangles have 2); the table is refused, not truncated", band_width, kBandMax);
  const int rows = B * 8, F = 1 + T / hop;
  const MelfeatBwdLayout L = melfeat_bwd_layout(B, n_mels, F);
  if (!workspace || workspace_bytes < L.total)
    return mst::fail(MST_ENOMEM, "mst_melfeat_backward: workspace %zu B < required %zu B", workspace_bytes, L.total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  ChanScalars* sc = reinterpret_cast<ChanScalars*>(ws + L.scalars);
  RowCoef* coef = reinterpret_cast<RowCoef*>(ws + L.coef);
  double* mixc = reinterpret_cast<double*>(ws + L.mixc);
  float* P = reinterpret_cast<float*>(ws + L.P);
  float* W = reinterpret_cast<float*>(ws + L.W);
  // time-domain terms
  hipLaunchKernelGGL(melfeat_scalars_kernel, dim3(kScalarSegs, B * 10), dim3(kScalarThreads), 0, st, x, T, sc);
  hipLaunchKernelGGL(melfeat_coef_kernel, dim3(B), dim3(64), 0, st, sc, grad_feats, feats, T, coef, mixc);
  hipLaunchKernelGGL(melfeat_time_kernel, dim3(std::min((T + 255) / 256, 512), rows), dim3(256), 0, st, x, T, coef, mixc, grad_x,
                     accumulate != 0);
  MST_HIP_CHECK(hipGetLastError());
  // masking (+ the log-mel cotangent): mel power of every row, cotangent on it, one adjoint pass
  MelpowParams mp;
  mp.x = x, mp.window = window, mp.bandw = reinterpret_cast<const float2*>(band_weight), mp.melr = reinterpret_cast<const int4*>(mel_ranges);
  mp.P = P, mp.rows = rows, mp.T = T, mp.hop = hop, mp.F = F, mp.pairs_per_row = (F + 1) / 2, mp.n_mels = n_mels;
  const long long items = (long long)rows * mp.pairs_per_row;
  MST_REQUIRE(items < (1LL << 31), "mst_melfeat_backward: %lld frame pairs", items);
  const int pgrid = (int)std::min<long long>((items + kWaves - 1) / kWaves, kFwdMaxBlocks);
  MST_HIP_CHECK(n_fft == 1024 ? launch_melpow<1024>(mp, pgrid, st) : launch_melpow<2048>(mp, pgrid, st));
  const size_t MF = (size_t)n_mels * F;
  hipLaunchKernelGGL(melfeat_cot_kernel, dim3((unsigned)((MF + 255) / 256), B), dim3(256), 0, st, P, grad_logmel, grad_feats, feats, MF,
                     (float)(1.0 / (2.0 * (double)MF)), W);
  MST_HIP_CHECK(hipGetLastError());
  LogmelBwdParams p;
  p.x = x, p.g = W, p.window = window;
  p.band = reinterpret_cast<const int2*>(band), p.bandw = reinterpret_cast<const float2*>(band_weight);
  p.melr = reinterpret_cast<const int4*>(mel_ranges);
  p.grad = grad_x, p.border = reinterpret_cast<float*>(ws + L.border);
  p.rows = rows, p.T = T, p.hop = hop, p.lh = log2_exact(hop), p.R = n_fft / hop, p.F = F;
  p.nchunks = (int)(((long long)T + n_fft + hop - 1) / hop);
  p.accumulate = 1, p.n_mels = n_mels;
  p.cpb = p.blocks_per_row = p.wstride = 0;
  if (int rc = n_fft == 1024 ? launch_logmel_bwd<1024, true>(p, st) : launch_logmel_bwd<2048, true>(p, st)) return rc;
  hipLaunchKernelGGL(mrstft_fold_kernel, dim3(rows), dim3(256), 0, st, grad_x, p.border, T, n_fft / 2);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"
