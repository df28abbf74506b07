// Stage A: waveform -> windowed FFT -> |X|^2 -> sparse HTK mel -> log-mel + mixing-feature
// partial sums, and the finalise kernel that turns the partials into the 64-d feature vector.
//
// Replaces (reference barry-mir/mixing-style-transfer): torchaudio MelSpectrogram as called at
// src/mixing_utils.py:159,280 and src/model.py:58-65; MixingFeatureExtractor src/mixing_utils.py:71-357.
//
// Kernel shape (gfx950, wave64):
//   * one workgroup = one (clip, run of ceil(F/32) frames), all 8 channels; blockIdx is XCD-remapped so the runs of
//     one clip sit on one XCD (overlapping frame reads and partial output lines meet in one L2);
//   * melfeat_spw_kernel (standard configuration): 12 waves, 3 per stem; a wave transforms the L and R channel of
//     one frame as ONE n_fft-point complex Stockham FFT held in registers (radix-8/4 butterflies), exchanged
//     through a wave-private LDS scratch between passes; twiddles / window / sparse mel weights live in LDS tables;
//     melfeat_kernel (any hop, odd T, 256 mels, n_fft 512 / 2048): 8 waves, two frames per wave;
//   * each sample is read from HBM once (frames overlap 4x, re-reads hit L1/L2), each log-mel value is written
//     once, staged through an LDS tile so that stores are frame-contiguous;
//   * all feature statistics (per-band dB sums, flatness sums, inter-stem masking, waveform moments) are
//     accumulated in registers in the same pass and reduced per workgroup.
// The sample type is a template parameter (float, or int16 PCM converted in the load).
#include "common.h"
#include "fft_wave.h"
#include "fft_pk.h"
#include "stage_a_tables.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>


namespace {

constexpr int kWaves = 8;              // waves per workgroup
constexpr int kFPW = 2;                // frames per wave per batch = FFTs a wave runs side by side (ILP)
constexpr int kTF = kWaves * kFPW;     // frames per workgroup batch (one LDS tile flush)
constexpr int kTileStride = kTF + 1;   // +1: conflict-free transposed tile writes
constexpr int kThreads = kWaves * 64;
constexpr int nf_of(int n_fft) { return n_fft >= 2048 ? 1 : kFPW; }  // 2 side-by-side FFTs unless registers forbid
constexpr int kNumScalars = 80;        // scalar slots per partial record (see enum below)

// scalar slots of a partial record, after the 4*M per-band sums
enum : int {
  S_LOGSUM = 0,   // [4] sum log(mel+1e-10) over (2 ch, M, frames)
  S_LINSUM = 4,   // [4] sum mel
  S_MASK = 8,     // [4] sum sigmoid(max_other - own)
  S_SQ = 12,      // [8] sum x^2
  S_PEAK = 20,    // [8] max |x|
  S_DSUM = 28,    // [8] sum (x - pivot)
  S_DSQ = 36,     // [8] sum (x - pivot)^2
  S_PIVOT = 44,   // [8] pivot (first owned sample)
  S_CROSS = 52,   // [4] sum (L - pL)(R - pR)
  S_MID = 56,     // [4] sum (L + R)^2
  S_SIDE = 60,    // [4] sum (L - R)^2
  S_MIX = 64,     // [1] sum over both channels of (v + b + d + o)^2
  S_NSAMP = 65,   // [1] owned samples
  S_NFRAME = 66,  // [1] frames in this run
};

using stage_a::LaneBand;

// Every kernel below has ONE description of its dynamic LDS: a layout struct beside it with the byte offset of each area and
// the total bytes(), which the launch passes.  Offsets are compile-time constants (the kernels' table reads fold them into
// their addresses); areas behind one whose length is known at run time only are named a_* and count from THAT area's end.
constexpr size_t kMaxLds = 160 * 1024;   // LDS of a workgroup
constexpr int pad4(int n) { return (n + 3) & ~3; }

struct KParams {
  const void* stem[4];       // per-stem base pointers (float or int16 PCM), each [B][2][T], clip stride `clip_stride` samples
  long long clip_stride;     // 8*T for a packed [B][8][T] tensor, 2*T for four separate [B][2][T] tensors
  float* logmel;
  float* partials;
  const float* window;
  const float2* tw;
  const float2* tw2;         // twiddles of the n_fft-point complex FFT (frame-pair packing, n_fft <= 1024)
  const float2* post;
  const float* melw;
  const LaneBand* lanebands;  // [NB][64]
  int B, T, F, M, hop;
  int tw_count, tw2_count, nnz;  // nnz = floats in the padded weight table melw[slot][i][lane]
  int glen[4], goff[4];      // per band slot r: uniform gather length (max support over lanes) and table offset
  int frames_per_run, runs_per_clip, pstride;
  int vec_ok;  // 8-byte aligned float2 frame loads allowed
  int vec4_ok; // 16-byte aligned float4 stats loads allowed
  int tile_bufs;  // 2: double-buffered output tile (one barrier per stem); 1: single (LDS-limited configs)
};

using namespace mstfft;

__device__ __forceinline__ int reflect_idx(int i, int T) { return i < 0 ? -i : (i >= T ? 2 * (T - 1) - i : i); }

__device__ __forceinline__ float2 shfl2(float2 a, int src) {
  return make_float2(__shfl(a.x, src, 64), __shfl(a.y, src, 64));
}

// Sample type of the waveform in HBM: fp32, or int16 PCM (the ingest format: half the PCIe / HBM bytes; converted
// with the exact scale 2^-15, so the result equals the fp32 path run on float(pcm) / 32768 bit for bit).
template <typename ST> struct Smp;
template <> struct Smp<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ float lds(const float* p) { return *p; }
  static __device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }
  static __device__ __forceinline__ void ld4(const float* p, float (&x)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
  }
};
template <> struct Smp<short> {
  static constexpr float kScale = 1.0f / 32768.0f;
  static __device__ __forceinline__ float ld(const short* p) { return (float)*p * kScale; }
  static __device__ __forceinline__ float lds(const short* p) {
    return (float)(*p) * kScale;
  }
  static __device__ __forceinline__ float2 ld2(const short* p) {
    const short2 q = *reinterpret_cast<const short2*>(p);
    return make_float2((float)q.x * kScale, (float)q.y * kScale);
  }
  static __device__ __forceinline__ void ld4(const short* p, float (&x)[4]) {
    const short4 q = *reinterpret_cast<const short4*>(p);
    x[0] = (float)q.x * kScale, x[1] = (float)q.y * kScale, x[2] = (float)q.z * kScale, x[3] = (float)q.w * kScale;
  }
};

// mel power of NF frames of one channel, computed side by side (two independent FFT dependency chains per wave;
// window, twiddles and mel weights are loaded once for both): returns this lane's NB band values per frame.
// With hop == NFFT/4 the samples a frame "owns" for the waveform moments, [f*hop, (f+1)*hop), are elements
// Q/2 .. Q/2 + Q/4 - 1 of every lane (float2 index lane + 64*q); RAW builds return them un-windowed in `raw`.
template <int NFFT, int NB, int NF, bool RAW = false, typename ST = float>
__device__ __forceinline__ void frames_mel(const KParams& p, const ST* const (&xchs)[NF], const int (&frame)[NF],
                                           int lane, const float2* s_win, const float2* s_tw, const float2* s_post,
                                           const float* s_melw, float2* scr, const int (&lb_start)[NB],
                                           float (&mel)[NF][NB], float2 (*raw)[NFFT / 512] = nullptr) {
  constexpr int NC = NFFT / 2;
  constexpr int Q = NC / 64;
  constexpr int NOWN = Q / 4;
  constexpr int SCR = NC + NC / 8;
  using Plan = FftPlan<NC>;
  constexpr int R0 = Plan::R0, RL = Plan::RL;
  constexpr int NBF0 = NC / R0 / 64, STR0 = NC / R0, NBFL = NC / RL / 64;
  float2 v[NF][Q];
  int s0[NF];
  bool interior = p.vec_ok != 0;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    s0[f] = frame[f] * p.hop - NFFT / 2;
    interior = interior && (s0[f] >= 0) && (s0[f] + NFFT <= p.T);
  }
  if (interior) {
#pragma unroll
    for (int u = 0; u < NBF0; ++u)
#pragma unroll
      for (int t = 0; t < R0; ++t) {
        const int n = lane + 64 * u + t * STR0;
        const float2 w = s_win[n];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float2 x = Smp<ST>::ld2(xchs[f] + s0[f] + 2 * n);
          v[f][u * R0 + t] = make_float2(x.x * w.x, x.y * w.y);
          if constexpr (RAW) {
            const int q = u + t * NBF0;  // compile-time after unrolling
            if (q >= Q / 2 && q < Q / 2 + NOWN) raw[f][q - Q / 2] = x;
          }
        }
      }
  } else {
#pragma unroll
    for (int u = 0; u < NBF0; ++u)
#pragma unroll
      for (int t = 0; t < R0; ++t) {
        const int n = lane + 64 * u + t * STR0;
        const float2 w = s_win[n];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const int i0 = s0[f] + 2 * n;
          const float2 x = make_float2(Smp<ST>::ld(xchs[f] + reflect_idx(i0, p.T)), Smp<ST>::ld(xchs[f] + reflect_idx(i0 + 1, p.T)));
          v[f][u * R0 + t] = make_float2(x.x * w.x, x.y * w.y);
          if constexpr (RAW) {
            const int q = u + t * NBF0;
            if (q >= Q / 2 && q < Q / 2 + NOWN) raw[f][q - Q / 2] = x;
          }
        }
      }
  }
  Plan::template run<NF>(v, scr, s_tw, lane);

  // real-FFT split: X[k] = E + W^k O with E,O from Z[k] and conj(Z[NC-k]); P = |X|^2
  const int mirror = (64 - lane) & 63;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    auto reg = [](int qq) { return (qq % NBFL) * RL + qq / NBFL; };
    const float2 w = s_post[q * 64 + lane];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const float2 a = v[f][reg(q)];
      const float2 bo = shfl2(v[f][reg(Q - 1 - q)], mirror);
      const float2 bs = v[f][reg((Q - q) % Q)];
      const float2 b = lane == 0 ? bs : bo;
      const float ex = 0.5f * (a.x + b.x), ey = 0.5f * (a.y - b.y);
      const float ox = 0.5f * (a.y + b.y), oy = -0.5f * (a.x - b.x);
      const float xr = ex + (w.x * ox - w.y * oy);
      const float xi = ey + (w.x * oy + w.y * ox);
      reinterpret_cast<float*>(scr + f * SCR)[lane + 64 * q] = xr * xr + xi * xi;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const float ny = v[f][0].x - v[f][0].y;
      reinterpret_cast<float*>(scr + f * SCR)[NC] = ny * ny;
    }
  }
  // sparse mel, branch-free: slot r of every lane walks glen[r] bins from its band's first bin; the weight table
  // is zero beyond a band's true support, the bin index is clamped so that only finite values are touched
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    float acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = 0.f;
    const float* w = s_melw + p.goff[r] + lane;
    const int n = p.glen[r];
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
      const float wi = w[i * 64];
      const int k = min(lb_start[r] + i, NC);
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = fmaf(wi, reinterpret_cast<const float*>(scr + f * SCR)[k], acc[f]);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) mel[f][r] = acc[f];
  }
}

// max over the wave of an unsigned value, returned in an SGPR: 4 DPP steps inside each row of 16 lanes
// (quad_perm xor 1, xor 2, row_half_mirror, row_mirror), then 4 readlanes.  No LDS traffic.
__device__ __forceinline__ unsigned wave_umax_uniform(unsigned m) {
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true));
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true));
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, true));
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xF, 0xF, true));
  const unsigned r0 = __builtin_amdgcn_readlane((int)m, 0), r1 = __builtin_amdgcn_readlane((int)m, 16);
  const unsigned r2 = __builtin_amdgcn_readlane((int)m, 32), r3 = __builtin_amdgcn_readlane((int)m, 48);
  return max(max(r0, r1), max(r2, r3));
}

// Two real frames as the real and imaginary part of ONE NFFT-point complex FFT:
//   z = a + i s b,  A[k] = (Z[k] + conj Z[N-k]) / 2,  s B[k] = (Z[k] - conj Z[N-k]) / (2i).
// The kernels pair the L and the R channel of the same stem and frame.  Unlike the even/odd-sample packing
// (half-length FFT + twiddled split, still used for n_fft = 2048) the split cancels nothing large: the cross-talk
// into A[k] is eps * |s B[k]| -- the SAME bin of the partner -- and s, an exact power of two, equalises the two
// frames' energies first, so each channel's error stays relative to its own level (the noise that remains is the
// complex FFT's own rounding, which any fp32 FFT of that frame carries).  An all-zero frame returns exact zeros.
// RAW: also return the un-windowed samples the frames own ([f*hop, (f+1)*hop): elements Q/2 .. Q/2+Q/4-1) as (a, b).
template <int NFFT, int NB, bool RAW, typename ST>
__device__ __forceinline__ void frames_mel_cplx(const KParams& p, const ST* __restrict__ xa,
                                                const ST* __restrict__ xb, int fA, int fB, int lane,
                                                const float* s_winf, const float2* s_tw2, const float* s_melw,
                                                float2* scr, const int (&lb_start)[NB], float (&mel)[2][NB],
                                                float2 (*raw)) {
  constexpr int NC = NFFT, Q = NC / 64, NOWN = Q / 4;
  using Plan = FftPlan<NC>;
  constexpr int R0 = Plan::R0, RL = Plan::RL;
  constexpr int NBF0 = NC / R0 / 64, STR0 = NC / R0, NBFL = NC / RL / 64;
  constexpr int PB_OFF = NFFT / 2 + 4;   // float offset of the second power spectrum inside the scratch
  float2 v[1][Q];
  const int sA = fA * p.hop - NFFT / 2, sB = fB * p.hop - NFFT / 2;
  const bool interior = sA >= 0 && sB >= 0 && sA + NFFT <= p.T && sB + NFFT <= p.T;
  float ma = 0.f, mb = 0.f;   // max |a w|, max |b w| of this lane
#pragma unroll
  for (int u = 0; u < NBF0; ++u)
#pragma unroll
    for (int t = 0; t < R0; ++t) {
      const int n = lane + 64 * u + t * STR0;
      const float w = s_winf[n];
      float a, b;
      if (interior) a = Smp<ST>::ld(xa + sA + n), b = Smp<ST>::ld(xb + sB + n);
      else a = Smp<ST>::ld(xa + reflect_idx(sA + n, p.T)), b = Smp<ST>::ld(xb + reflect_idx(sB + n, p.T));
      const float aw = a * w, bw = b * w;
      ma = fmaxf(ma, fabsf(aw)), mb = fmaxf(mb, fabsf(bw));
      v[0][u * R0 + t] = make_float2(aw, bw);
      if constexpr (RAW) {
        const int q = u + t * NBF0;  // compile-time after unrolling
        if (q >= Q / 2 && q < Q / 2 + NOWN) raw[q - Q / 2] = make_float2(a, b);
      }
    }
  // wave-uniform peak magnitudes (as raw bits; non-negative floats order like unsigned ints) -> scale exponent
  const unsigned ua = wave_umax_uniform(__float_as_uint(ma)), ub = wave_umax_uniform(__float_as_uint(mb));
  int sh = 0;
  if (ua != 0u && ub != 0u) sh = max(-40, min(40, (int)(ua >> 23) - (int)(ub >> 23)));
  if (sh != 0) {   // scalar branch
    const float sc = __uint_as_float((unsigned)(127 + sh) << 23);
#pragma unroll
    for (int q = 0; q < Q; ++q) v[0][q].y *= sc;
  }
  const float ia = ua != 0u ? 1.0f : 0.f;
  const float ib = ub != 0u ? __uint_as_float((unsigned)(127 - 2 * sh) << 23) : 0.f;
  Plan::template run<1>(v, scr, s_tw2, lane);
  float* PA = reinterpret_cast<float*>(scr);
  float* PB = PA + PB_OFF;
  const int mirror = (64 - lane) & 63;
  auto reg = [](int qq) { return (qq % NBFL) * RL + qq / NBFL; };
#pragma unroll
  for (int q = 0; q < Q / 2; ++q) {
    const float2 a = v[0][reg(q)];
    const float2 bo = shfl2(v[0][reg(Q - 1 - q)], mirror);
    const float2 bs = v[0][reg((Q - q) % Q)];
    const float2 b = lane == 0 ? bs : bo;
    const float ar = 0.5f * (a.x + b.x), ai = 0.5f * (a.y - b.y);   // A[k]
    const float br = 0.5f * (a.y + b.y), bi = -0.5f * (a.x - b.x);  // s B[k]
    PA[lane + 64 * q] = (ar * ar + ai * ai) * ia;
    PB[lane + 64 * q] = (br * br + bi * bi) * ib;
  }
  if (lane == 0) {
    const float2 z = v[0][reg(Q / 2)];   // bin NFFT/2: Z = A + i s B with both real
    PA[NFFT / 2] = z.x * z.x * ia;
    PB[NFFT / 2] = z.y * z.y * ib;
  }
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    float a0 = 0.f, a1 = 0.f;
    const float* w = s_melw + p.goff[r] + lane;
    const int n = p.glen[r];
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
      const float wi = w[i * 64];
      const int k = min(lb_start[r] + i, NFFT / 2);
      a0 = fmaf(wi, PA[k], a0);
      a1 = fmaf(wi, PB[k], a1);
    }
    mel[0][r] = a0;
    mel[1][r] = a1;
  }
}

// LDS of melfeat_kernel<NFFT, ..>; a_*: from the end of tw[twn].  The output tile [tile_bufs][2*M][kTileStride] follows melw.
template <int NFFT>
struct GenericLds {
  static constexpr int NC = NFFT / 2, SCR = nf_of(NFFT) * (NC + NC / 8);   // SCR: padded float2 per wave
  static constexpr bool PAIR = NFFT <= 1024;                  // frame-pair packed full-length FFT (see frames_mel_cplx)
  // float2 win[NC] (window pairs = [NFFT] floats), tw[twn], twn = PAIR ? tw2_count : tw_count
  static constexpr int win = 0, tw = win + NC * 8;
  // float2 post[NC] (even/odd packing only), scr[kWaves][SCR] (the workgroup reductions alias it); float melw[pad4(nnz)]
  static constexpr int a_post = 0, a_scr = a_post + (PAIR ? 0 : NC * 8), a_melw = a_scr + kWaves * SCR * 8;
  static constexpr size_t bytes(int tw_count, int tw2_count, int nnz, int M, int tile_bufs) {
    return (size_t)tw + (size_t)(PAIR ? tw2_count : tw_count) * 8 + a_melw + (size_t)pad4(nnz) * 4 + (size_t)tile_bufs * 2 * M * kTileStride * 4;
  }
  // floats of the spectral reduction: per wave 4 stems x 4 band slots x 64 lanes + 12 scalars
  static_assert(kWaves * 4 * 4 * 64 + kWaves * 12 <= 2 * kWaves * SCR, "the reduction buffer must fit the FFT scratch");
};

template <int NFFT, int NB, typename ST>
__global__ __launch_bounds__(kThreads) void melfeat_kernel(const KParams p) {
  using L = GenericLds<NFFT>;
  constexpr int NC = L::NC, SCR = L::SCR;
  constexpr bool PAIR = L::PAIR;
  constexpr float kLn2 = 0.69314718055994530942f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int twn = PAIR ? p.tw2_count : p.tw_count;
  float2* s_win = reinterpret_cast<float2*>(smem + L::win);
  float2* s_tw = reinterpret_cast<float2*>(smem + L::tw);
  unsigned char* after_tw = reinterpret_cast<unsigned char*>(s_tw + twn);
  float2* s_post = reinterpret_cast<float2*>(after_tw + L::a_post);
  float2* s_scr = reinterpret_cast<float2*>(after_tw + L::a_scr);
  float* s_melw = reinterpret_cast<float*>(after_tw + L::a_melw);
  float* s_tile0 = s_melw + pad4(p.nnz);   // double-buffered unless p.tile_bufs == 1

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int work = mst::xcd_remap(blockIdx.x, gridDim.x);
  const int clip = work / p.runs_per_clip, run = work % p.runs_per_clip;
  const int f_begin = run * p.frames_per_run;
  const int f_end = min(p.F, f_begin + p.frames_per_run);
  const int M = p.M;

  // ---- tables -> LDS
  {
    const float2* gw = reinterpret_cast<const float2*>(p.window);
    for (int i = tid; i < NC; i += kThreads) s_win[i] = gw[i];
    const float2* gt = PAIR ? p.tw2 : p.tw;
    for (int i = tid; i < twn; i += kThreads) s_tw[i] = gt[i];
    if (!PAIR)
      for (int i = tid; i < NC; i += kThreads) s_post[i] = p.post[i];
    for (int i = tid; i < p.nnz; i += kThreads) s_melw[i] = p.melw[i];
  }
  int lb_band[NB], lb_start[NB];
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    const LaneBand q = p.lanebands[r * 64 + lane];
    lb_band[r] = q.band, lb_start[r] = q.start;
  }

  auto chan = [&](int c) {
    return static_cast<const ST*>(p.stem[c >> 1]) + (size_t)clip * p.clip_stride + (size_t)(c & 1) * p.T;
  };
  float* part = p.partials + ((size_t)clip * p.runs_per_clip + run) * p.pstride;
  float* red = reinterpret_cast<float*>(s_scr);  // workgroup reduction buffer (aliases FFT scratch)

  // ---- waveform moments over the samples this run owns: [f_begin*hop, f_end*hop) (last run: to T)
  {
    const int o_begin = f_begin * p.hop;
    const int o_end = (f_end == p.F) ? p.T : min(p.T, f_end * p.hop);
    const int n_own = max(0, o_end - o_begin);
    float piv[8], sq[8], pk[8], ds[8], dq[8], cr[4], mid[4], side[4], mix = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      piv[c] = n_own > 0 ? Smp<ST>::ld(chan(c) + o_begin) : 0.f;
      sq[c] = pk[c] = ds[c] = dq[c] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) cr[s] = mid[s] = side[s] = 0.f;
    // all loads of up to kIT iterations are issued before any arithmetic: the pass is latency-bound otherwise
    constexpr int kIT = 2;
    for (int base = tid * 4; base < n_own; base += kThreads * 4 * kIT) {
      float x[kIT][8][4];
#pragma unroll
      for (int it = 0; it < kIT; ++it) {
        const int i = base + it * kThreads * 4;
        const bool full = (i + 3 < n_own);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const ST* src = chan(c) + o_begin + min(i, max(n_own - 1, 0));
          if (full && p.vec4_ok) {
            Smp<ST>::ld4(src, x[it][c]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[it][c][e] = (i + e < n_own) ? Smp<ST>::ld(src + e) : piv[c];
          }
        }
      }
#pragma unroll
      for (int it = 0; it < kIT; ++it) {
        const int i = base + it * kThreads * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (i + e < n_own) {
            float mL = 0.f, mR = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const float L = x[it][2 * s][e], R = x[it][2 * s + 1][e];
              const float dL = L - piv[2 * s], dR = R - piv[2 * s + 1];
              sq[2 * s] = fmaf(L, L, sq[2 * s]);
              sq[2 * s + 1] = fmaf(R, R, sq[2 * s + 1]);
              pk[2 * s] = fmaxf(pk[2 * s], fabsf(L));
              pk[2 * s + 1] = fmaxf(pk[2 * s + 1], fabsf(R));
              ds[2 * s] += dL;
              ds[2 * s + 1] += dR;
              dq[2 * s] = fmaf(dL, dL, dq[2 * s]);
              dq[2 * s + 1] = fmaf(dR, dR, dq[2 * s + 1]);
              cr[s] = fmaf(dL, dR, cr[s]);
              const float sm = L + R, sd = L - R;
              mid[s] = fmaf(sm, sm, mid[s]);
              side[s] = fmaf(sd, sd, side[s]);
              mL += L;  // python sum(): ((v + b) + d) + o
              mR += R;
            }
            mix = fmaf(mL, mL, mix);
            mix = fmaf(mR, mR, mix);
          }
        }
      }
    }
    // workgroup reduce: 53 sums + 8 maxima
    float vals[53];
#pragma unroll
    for (int c = 0; c < 8; ++c) vals[c] = sq[c], vals[8 + c] = ds[c], vals[16 + c] = dq[c];
#pragma unroll
    for (int s = 0; s < 4; ++s) vals[24 + s] = cr[s], vals[28 + s] = mid[s], vals[32 + s] = side[s];
    vals[36] = mix;
#pragma unroll
    for (int k = 0; k < 37; ++k) {
      const float r = mst::wave_sum(vals[k]);
      if (lane == 0) red[wave * 48 + k] = r;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float r = mst::wave_max(pk[c]);
      if (lane == 0) red[wave * 48 + 37 + c] = r;
    }
    __syncthreads();
    if (tid < 45) {
      float r = red[tid];
      for (int w = 1; w < kWaves; ++w) r = tid < 37 ? r + red[w * 48 + tid] : fmaxf(r, red[w * 48 + tid]);
      int slot;
      if (tid < 8) slot = S_SQ + tid;
      else if (tid < 16) slot = S_DSUM + (tid - 8);
      else if (tid < 24) slot = S_DSQ + (tid - 16);
      else if (tid < 28) slot = S_CROSS + (tid - 24);
      else if (tid < 32) slot = S_MID + (tid - 28);
      else if (tid < 36) slot = S_SIDE + (tid - 32);
      else if (tid == 36) slot = S_MIX;
      else slot = S_PEAK + (tid - 37);
      part[4 * M + slot] = r;
    }
    if (tid < 8) part[4 * M + S_PIVOT + tid] = piv[tid];
    if (tid == 0) {
      part[4 * M + S_NSAMP] = (float)n_own;
      part[4 * M + S_NFRAME] = (float)max(0, f_end - f_begin);
    }
    __syncthreads();  // red aliases the FFT scratch; tables are loaded too
  }

  // ---- spectral pass
  float acc_db[4][NB], acc_log[4], acc_lin[4], acc_mask[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    acc_log[s] = acc_lin[s] = acc_mask[s] = 0.f;
#pragma unroll
    for (int r = 0; r < NB; ++r) acc_db[s][r] = 0.f;
  }
  float2* scr = s_scr + wave * SCR;

  for (int fb = f_begin; fb < f_end; fb += kTF) {
    float S[4][kFPW][NB];  // channel-mean mel power per stem, frame slot, band
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int f = 0; f < kFPW; ++f)
#pragma unroll
        for (int r = 0; r < NB; ++r) S[s][f][r] = 0.f;

#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
      float* s_tile = s_tile0 + (p.tile_bufs == 2 ? (s & 1) : 0) * (2 * M * kTileStride);
      int frame[kFPW];
      bool fok[kFPW];
#pragma unroll
      for (int ff = 0; ff < kFPW; ++ff) {
        const int fr = fb + wave * kFPW + ff;
        fok[ff] = fr < f_end;
        frame[ff] = fok[ff] ? fr : f_end - 1;  // past the run: recompute a valid frame, discard the result
      }
      if (fok[0]) {  // wave-uniform
        float sm[kFPW][NB];
        float melall[2][kFPW][NB];   // [channel][frame slot][band slot]
        if constexpr (PAIR) {
#pragma unroll 1
          for (int ff = 0; ff < kFPW; ++ff) {
            float m2[2][NB];
            frames_mel_cplx<NFFT, NB, false, ST>(p, chan(2 * s), chan(2 * s + 1), frame[ff], frame[ff], lane,
                                             reinterpret_cast<const float*>(s_win), s_tw, s_melw, scr, lb_start, m2,
                                             nullptr);
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
              for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int f2 = 0; f2 < kFPW; ++f2) melall[c][f2][r] = (f2 == ff) ? m2[c][r] : melall[c][f2][r];
          }
        } else {
#pragma unroll 1
          for (int cf = 0; cf < 2 * kFPW; ++cf) {
            const int c = cf / kFPW, ff = cf % kFPW;
            const int one[1] = {frame[ff]};
            float m1[1][NB];
            const ST* const x1[1] = {chan(2 * s + c)};
            frames_mel<NFFT, NB, 1, false, ST>(p, x1, one, lane, s_win, s_tw, s_post, s_melw, scr, lb_start, m1);
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
              for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int f2 = 0; f2 < kFPW; ++f2)
                  melall[c2][f2][r] = (c2 == c && f2 == ff) ? m1[0][r] : melall[c2][f2][r];
          }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float (&mel)[kFPW][NB] = melall[c];
#pragma unroll
          for (int ff = 0; ff < kFPW; ++ff) {
            float lsum = 0.f, msum = 0.f;
#pragma unroll
            for (int r = 0; r < NB; ++r) {
              const bool ok = lb_band[r] >= 0 && fok[ff];
              const float lm = __log2f(mel[ff][r] + 1e-10f) * kLn2;
              if (ok) {
                s_tile[(c * M + lb_band[r]) * kTileStride + wave * kFPW + ff] = lm;
                lsum += lm;
                msum += mel[ff][r];
              }
              const float lmz = ok ? lm : 0.f;
#pragma unroll
              for (int ss = 0; ss < 4; ++ss) acc_db[ss][r] += (s == ss) ? lmz : 0.f;
              sm[ff][r] = (c == 0) ? mel[ff][r] : (sm[ff][r] + mel[ff][r]) * 0.5f;  // mel.mean(dim=0) of (2, M, F)
            }
#pragma unroll
            for (int ss = 0; ss < 4; ++ss) {
              acc_log[ss] += (s == ss) ? lsum : 0.f;
              acc_lin[ss] += (s == ss) ? msum : 0.f;
            }
          }
        }
#pragma unroll
        for (int ss = 0; ss < 4; ++ss)
#pragma unroll
          for (int ff = 0; ff < kFPW; ++ff)
#pragma unroll
            for (int r = 0; r < NB; ++r) S[ss][ff][r] = (s == ss) ? sm[ff][r] : S[ss][ff][r];
      }
      // one barrier per stem: the tile of stem s is complete; its flush below overlaps the FFTs of stem s+1 (other
      // buffer), and buffer (s & 1) is written again only after the barrier of stem s+1, i.e. after this flush
      __syncthreads();
      if (p.logmel) {  // flush the stem's two channels: rows (c, band), kTF consecutive frames each
        const int f = tid % kTF, frame = fb + f;
        if (frame < f_end) {
          for (int row = tid / kTF; row < 2 * M; row += kThreads / kTF) {
            const int c = row / M, band = row - c * M;
            p.logmel[(((size_t)clip * 8 + 2 * s + c) * M + band) * p.F + frame] = s_tile[row * kTileStride + f];
          }
        }
      }
      if (p.tile_bufs == 1) __syncthreads();  // single tile: the next stem overwrites it
    }
    // inter-stem masking for this wave's frames (mixing_utils.py:288-307)
#pragma unroll
    for (int ff = 0; ff < kFPW; ++ff) {
      if (fb + wave * kFPW + ff >= f_end) continue;
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        if (lb_band[r] < 0) continue;
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) {
          float other = -INFINITY;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j != ss) other = fmaxf(other, S[j][ff][r]);
          const float d = S[ss][ff][r] - other;
          acc_mask[ss] += __frcp_rn(1.0f + __expf(d));  // sigmoid((0 - d) / 1)
        }
      }
    }
  }

  // ---- workgroup reduction of the spectral accumulators
  // per-band sums: same lane owns the same bands in every wave
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int r = 0; r < NB; ++r) red[((wave * 4 + s) * NB + r) * 64 + lane] = acc_db[s][r];
  float* red2 = red + kWaves * 4 * NB * 64;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float a = mst::wave_sum(acc_log[s]), b = mst::wave_sum(acc_lin[s]), c = mst::wave_sum(acc_mask[s]);
    if (lane == 0) {
      red2[wave * 12 + S_LOGSUM + s] = a;
      red2[wave * 12 + S_LINSUM + s] = b;
      red2[wave * 12 + S_MASK + s] = c;
    }
  }
  __syncthreads();
  for (int i = tid; i < 4 * NB * 64; i += kThreads) {
    const int l = i & 63, r = (i >> 6) % NB, s = i / (64 * NB);
    float v = 0.f;
    for (int w = 0; w < kWaves; ++w) v += red[((w * 4 + s) * NB + r) * 64 + l];
    const int band = p.lanebands[r * 64 + l].band;
    if (band >= 0) part[s * M + band] = v;
  }
  if (tid < 12) {
    float v = 0.f;
    for (int w = 0; w < kWaves; ++w) v += red2[w * 12 + tid];
    part[4 * M + tid] = v;
  }
}

// ------------------------------------------------------------------------------------------
// Stage A, "stem per wave pair" layout for the standard configuration (hop == n_fft/4, n_mels <= 128, aligned
// input).  Waves 2s and 2s+1 own stem s: a wave transforms the L and the R channel of ONE frame as one complex FFT
// (frames_mel_cplx; even / odd frames of a 16-frame batch), so
//   * per-channel and L/R cross moments come from the un-windowed samples the frame owns (no moment pass; consecutive
//     frames of a wave overlap by half, the partner wave covers the rest: L1/L2 hits),
//   * all 8 channels x 16 frames of log-mel land in one frame-major LDS tile and are flushed once per batch
//     (2 barriers per batch instead of 8), the inter-stem masking is evaluated from that tile,
//   * the mixture energy comes from a short float4 pass over the batch's samples (just loaded: cache-resident).
// Writes the same partial records as melfeat_kernel (same finalise kernel).
// ------------------------------------------------------------------------------------------
// WPS = waves per stem: the workgroup has 4*WPS waves and works on batches of 2*WPS... frames: with WPS = 3 (12 waves,
// 3 per SIMD, 168 VGPRs) the batch is 6 frames (2 per wave), which is what the 160 KB of LDS leave for the tile once
// twelve 9.2 KB FFT scratches are resident; WPS = 2 is the 8-wave / 16-frame layout.
template <int WPS>
struct SpwGeom {
  static constexpr int WAVES = 4 * WPS, THREADS = WAVES * 64;
  static constexpr int FPW = WPS == 2 ? 8 : 2;     // frames per wave per batch
  static constexpr int TF = WPS * FPW;             // frames per batch
};

// LDS of melfeat_spw_kernel<NFFT, ., WPS>; a_*: from the end of tw2[tw2_count].  The log-mel tile [TF][8*M + 1] follows melw.
template <int NFFT, int WPS>
struct SpwLds {
  using G = SpwGeom<WPS>;
  static constexpr int SCR = NFFT + NFFT / 8;                     // float2 per wave
  // float winf[NFFT]; float2 tw2[tw2_count] | float2 scr[WAVES][SCR] (the final reduction aliases it); float melw[pad4(nnz)]
  static constexpr int winf = 0, tw2 = winf + NFFT * 4, a_scr = 0, a_melw = a_scr + G::WAVES * SCR * 8;
  static constexpr size_t bytes(int tw2_count, int nnz, int M) {
    return (size_t)tw2 + (size_t)tw2_count * 8 + a_melw + (size_t)pad4(nnz) * 4 + (size_t)G::TF * (8 * M + 1) * 4;
  }
  static_assert(G::WAVES * 2 * 64 + G::WAVES * 24 <= 2 * G::WAVES * SCR, "the reduction buffer must fit the FFT scratch");
};

template <int NFFT, typename ST, int WPS>
__global__ __launch_bounds__(SpwGeom<WPS>::THREADS) void melfeat_spw_kernel(const KParams p) {
  constexpr int kWaves = SpwGeom<WPS>::WAVES, kThreads = SpwGeom<WPS>::THREADS, kTF = SpwGeom<WPS>::TF;
  constexpr int NB = 2, NOWN = NFFT / 256;
  using L = SpwLds<NFFT, WPS>;
  constexpr int SCR = L::SCR;
  constexpr float kLn2 = 0.69314718055994530942f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_winf = reinterpret_cast<float*>(smem + L::winf);
  float2* s_tw2 = reinterpret_cast<float2*>(smem + L::tw2);
  unsigned char* after_tw2 = reinterpret_cast<unsigned char*>(s_tw2 + p.tw2_count);
  float2* s_scr = reinterpret_cast<float2*>(after_tw2 + L::a_scr);
  float* s_melw = reinterpret_cast<float*>(after_tw2 + L::a_melw);
  float* s_tile = s_melw + pad4(p.nnz);   // frame-major
  const int M = p.M, TS = 8 * M + 1;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int work = mst::xcd_remap(blockIdx.x, gridDim.x);
  const int clip = work / p.runs_per_clip, run = work % p.runs_per_clip;
  const int f_begin = run * p.frames_per_run;
  const int f_end = min(p.F, f_begin + p.frames_per_run);
  {
    for (int i = tid; i < NFFT; i += kThreads) s_winf[i] = p.window[i];
    for (int i = tid; i < p.tw2_count; i += kThreads) s_tw2[i] = p.tw2[i];
    for (int i = tid; i < p.nnz; i += kThreads) s_melw[i] = p.melw[i];
  }
  int lb_band[NB], lb_start[NB];
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    const LaneBand q = p.lanebands[r * 64 + lane];
    lb_band[r] = q.band, lb_start[r] = q.start;
  }
  auto chan = [&](int c) {
    return static_cast<const ST*>(p.stem[c >> 1]) + (size_t)clip * p.clip_stride + (size_t)(c & 1) * p.T;
  };
  float* part = p.partials + ((size_t)clip * p.runs_per_clip + run) * p.pstride;
  const int stem = wave / WPS, half = wave % WPS;   // `half`: which of the stem's WPS waves
  const ST* const xs[2] = {chan(2 * stem), chan(2 * stem + 1)};
  const int o_begin = f_begin * p.hop;
  const int o_end = (f_end == p.F) ? p.T : min(p.T, f_end * p.hop);
  const int o_piv = min(o_begin, p.T - 1);
  const float pvL = Smp<ST>::ld(xs[0] + o_piv), pvR = Smp<ST>::ld(xs[1] + o_piv);
  float2* scr = s_scr + wave * SCR;

  float acc_db[NB] = {0.f, 0.f}, acc_log = 0.f, acc_lin = 0.f;
  float sqL = 0.f, sqR = 0.f, pkL = 0.f, pkR = 0.f, dsL = 0.f, dsR = 0.f, dqL = 0.f, dqR = 0.f;
  float cr = 0.f, mid = 0.f, side = 0.f;
  float mask[4] = {0.f, 0.f, 0.f, 0.f}, mixsq = 0.f;   // accumulated per thread in the tile phase
  __syncthreads();

  for (int fb = f_begin; fb < f_end; fb += kTF) {
    // ---- phase A: every wave: 8 frames of its stem, L and R as one complex FFT
#pragma unroll 1
    for (int i = 0; i < kTF / WPS; ++i) {
      const int fr = fb + WPS * i + half;
      if (fr >= f_end) break;  // wave-uniform
      float mel[2][NB];
      float2 raw[NOWN];        // (L, R) of the samples the frame owns
      frames_mel_cplx<NFFT, NB, true, ST>(p, xs[0], xs[1], fr, fr, lane, s_winf, s_tw2, s_melw, scr, lb_start, mel, raw);
      float* trow = s_tile + (fr - fb) * TS + 2 * stem * M;
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        if (lb_band[r] < 0) continue;
        const float l0 = __log2f(mel[0][r] + 1e-10f) * kLn2, l1 = __log2f(mel[1][r] + 1e-10f) * kLn2;
        trow[lb_band[r]] = l0;
        trow[M + lb_band[r]] = l1;
        acc_db[r] += l0 + l1;
        acc_log += l0 + l1;
        acc_lin += mel[0][r] + mel[1][r];
      }
      // waveform moments from the samples this frame owns
#pragma unroll
      for (int j = 0; j < NOWN; ++j) {
        const int n = fr * p.hop + lane + 64 * j;
        const bool m = n < p.T;
        const float L = m ? raw[j].x : 0.f;
        const float R = m ? raw[j].y : 0.f;
        const float dL = m ? L - pvL : 0.f, dR = m ? R - pvR : 0.f;
        sqL = fmaf(L, L, sqL), sqR = fmaf(R, R, sqR);
        pkL = fmaxf(pkL, fabsf(L)), pkR = fmaxf(pkR, fabsf(R));
        dsL += dL, dsR += dR;
        dqL = fmaf(dL, dL, dqL), dqR = fmaf(dR, dR, dqR);
        cr = fmaf(dL, dR, cr);
        mid = fmaf(L + R, L + R, mid);
        side = fmaf(L - R, L - R, side);
      }
    }
    __syncthreads();
    // ---- phase B (all threads): flush the batch's log-mel, masking, mixture energy
    const int nf = min(kTF, f_end - fb);
    if (p.logmel) {
      const int f = tid % kTF;
      if (f < nf)
        for (int row = tid / kTF; row < 8 * M; row += kThreads / kTF)   // row = ch * M + band
          p.logmel[((size_t)clip * 8 * M + row) * p.F + fb + f] = s_tile[f * TS + row];
    }
    for (int e = tid; e < nf * M; e += kThreads) {  // (frame, band) pairs; 8 channel reads, conflict-free across bands
      const int f = e / M, m = e - f * M;
      const float* t = s_tile + f * TS + m;
      float S[4];
#pragma unroll
      for (int s = 0; s < 4; ++s)   // channel-mean mel power back from the log domain (abs. error ~1e-7 * power)
        S[s] = 0.5f * ((__expf(t[(2 * s) * M]) - 1e-10f) + (__expf(t[(2 * s + 1) * M]) - 1e-10f));
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float other = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j != s) other = fmaxf(other, S[j]);
        mask[s] += __frcp_rn(1.0f + __expf(S[s] - other));
      }
    }
    {
      const int b0 = fb * p.hop, b1 = (fb + nf == p.F) ? p.T : min(p.T, (fb + nf) * p.hop);
      for (int i = b0 + tid * 4; i < b1; i += kThreads * 4) {
        float x[8][4];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const ST* src = chan(c) + i;
          if (i + 3 < b1) {
            Smp<ST>::ld4(src, x[c]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[c][e] = (i + e < b1) ? Smp<ST>::ld(src + e) : 0.f;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float mL = ((x[0][e] + x[2][e]) + x[4][e]) + x[6][e];   // python sum(): ((v + b) + d) + o
          const float mR = ((x[1][e] + x[3][e]) + x[5][e]) + x[7][e];
          mixsq = fmaf(mL, mL, mixsq);
          mixsq = fmaf(mR, mR, mixsq);
        }
      }
    }
    __syncthreads();
  }

  // ---- reductions -> partial record (same slots as melfeat_kernel)
  float* red = reinterpret_cast<float*>(s_scr);   // [kWaves][NB][64] band sums, then per-wave scalars
#pragma unroll
  for (int r = 0; r < NB; ++r) red[(wave * NB + r) * 64 + lane] = acc_db[r];
  float* red2 = red + kWaves * NB * 64;           // [kWaves][24]
  {
    const float v[13] = {acc_log, acc_lin, sqL, sqR, dsL, dsR, dqL, dqR, cr, mid, side, mixsq, 0.f};
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const float r = mst::wave_sum(v[k]);
      if (lane == 0) red2[wave * 24 + k] = r;
    }
    const float a = mst::wave_max(pkL), b = mst::wave_max(pkR);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float r = mst::wave_sum(mask[s]);
      if (lane == 0) red2[wave * 24 + 14 + s] = r;
    }
    if (lane == 0) red2[wave * 24 + 12] = a, red2[wave * 24 + 13] = b;
  }
  __syncthreads();
  for (int i = tid; i < 4 * NB * 64; i += kThreads) {
    const int l = i & 63, r = (i >> 6) % NB, s = i / (64 * NB);
    const int band = p.lanebands[r * 64 + l].band;
    if (band >= 0) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < WPS; ++w) v += red[((WPS * s + w) * NB + r) * 64 + l];
      part[s * M + band] = v;
    }
  }
  if (tid < 4) {  // per-stem scalars: waves WPS*s .. WPS*s + WPS-1
    const int s = tid;
    float v[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) v[k] = 0.f;
    for (int w = 0; w < WPS; ++w) {
      const float* a = red2 + (WPS * s + w) * 24;
#pragma unroll
      for (int k = 0; k < 12; ++k) v[k] += a[k];
      v[12] = fmaxf(v[12], a[12]), v[13] = fmaxf(v[13], a[13]);
    }
    float* q = part + 4 * M;
    q[S_LOGSUM + s] = v[0];
    q[S_LINSUM + s] = v[1];
    q[S_SQ + 2 * s] = v[2], q[S_SQ + 2 * s + 1] = v[3];
    q[S_DSUM + 2 * s] = v[4], q[S_DSUM + 2 * s + 1] = v[5];
    q[S_DSQ + 2 * s] = v[6], q[S_DSQ + 2 * s + 1] = v[7];
    q[S_CROSS + s] = v[8];
    q[S_MID + s] = v[9];
    q[S_SIDE + s] = v[10];
    q[S_PEAK + 2 * s] = v[12], q[S_PEAK + 2 * s + 1] = v[13];
    float mk = 0.f;
    for (int w = 0; w < kWaves; ++w) mk += red2[w * 24 + 14 + s];
    q[S_MASK + s] = mk;
    q[S_PIVOT + 2 * s] = Smp<ST>::ld(chan(2 * s) + o_piv), q[S_PIVOT + 2 * s + 1] = Smp<ST>::ld(chan(2 * s + 1) + o_piv);
  }
  if (tid == 8) {
    float mx = 0.f;
    for (int w = 0; w < kWaves; ++w) mx += red2[w * 24 + 11];
    part[4 * M + S_MIX] = mx;
    part[4 * M + S_NSAMP] = (float)max(0, o_end - o_begin);
    part[4 * M + S_NFRAME] = (float)max(0, f_end - f_begin);
  }
}

// ------------------------------------------------------------------------------------------
// Finalise: reduce the per-run partial records of one clip in double precision and emit the
// feature vector in the reference's sorted-key layout (mixing_utils.py:320-357).
// ------------------------------------------------------------------------------------------
struct FParams {
  const float* partials;
  float* feats;
  int M, F, T, runs_per_clip, pstride, detailed_bins, feat_dim;
};

// fp64 sum over the 64 lanes of a wave: a fixed butterfly, every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave: lane l takes y[l], y[l + 64], ...; the lanes' partial sums meet in wave_sum_f64's tree
__device__ double pearson_vs_index(const double* y, int n, int lane) {
  double my = 0;
  for (int i = lane; i < n; i += 64) my += y[i];
  my = wave_sum_f64(my) / n;
  const double mx = 0.5 * (n - 1);
  double sxy = 0, sxx = 0, syy = 0;
  for (int i = lane; i < n; i += 64) {
    const double dx = i - mx, dy = y[i] - my;
    sxy += dx * dy, sxx += dx * dx, syy += dy * dy;
  }
  sxy = wave_sum_f64(sxy), sxx = wave_sum_f64(sxx), syy = wave_sum_f64(syy);
  const double std_unbiased = sqrt(syy / (n - 1));
  if (std_unbiased < 1e-6) return 0.0;  // mixing_utils.py:184
  double c = sxy / sqrt(sxx * syy);
  return fmin(1.0, fmax(-1.0, c));      // torch.corrcoef clips to [-1, 1]
}

// LDS of melfeat_finalize_kernel, all doubles: band[4*M] mean dB per band, then (a_*: from its end) the reduced scalars
// sc[kNumScalars], chmean[8], chm2[8], cross[4 padded to 8] and the resampled band curves curve[4][detailed_bins]
struct FinalizeLds {
  static constexpr int a_sc = 0, a_chmean = a_sc + kNumScalars * 8, a_chm2 = a_chmean + 64, a_cross = a_chm2 + 64, a_curve = a_cross + 64;
  static constexpr size_t bytes(int M, int detailed_bins) { return (size_t)4 * M * 8 + a_curve + (size_t)4 * (detailed_bins > 0 ? detailed_bins : 0) * 8; }
};

__global__ __launch_bounds__(256) void melfeat_finalize_kernel(const FParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using L = FinalizeLds;
  double* band = reinterpret_cast<double*>(smem);
  unsigned char* after_band = reinterpret_cast<unsigned char*>(band + 4 * p.M);
  double* sc = reinterpret_cast<double*>(after_band + L::a_sc);
  double* chmean = reinterpret_cast<double*>(after_band + L::a_chmean);
  double* chm2 = reinterpret_cast<double*>(after_band + L::a_chm2);
  double* cross = reinterpret_cast<double*>(after_band + L::a_cross);
  const int tid = threadIdx.x, clip = blockIdx.x, M = p.M;
  const float* base = p.partials + (size_t)clip * p.runs_per_clip * p.pstride;
  const double inv_n_db = 1.0 / (2.0 * p.F);
  const double k_db = 10.0 / log(10.0);
  for (int i = tid; i < 4 * M; i += 256) {
    double s = 0;
#pragma unroll 8
    for (int r = 0; r < p.runs_per_clip; ++r) s += base[(size_t)r * p.pstride + i];
    band[i] = s * inv_n_db * k_db;  // mean over (2 ch, F) of 10*log10(mel + 1e-10)
  }
  if (tid < kNumScalars) {
    const bool is_max = tid >= S_PEAK && tid < S_PEAK + 8;
    double s = 0;
#pragma unroll 8
    for (int r = 0; r < p.runs_per_clip; ++r) {
      const double v = base[(size_t)r * p.pstride + 4 * M + tid];
      s = is_max ? fmax(s, v) : s + v;
    }
    sc[tid] = s;
  }
  // pooled mean / M2 / cross moment from pivoted per-run sums (Chan et al. pairwise update)
  if (tid < 8) {
    double n = 0, mean = 0, m2 = 0;
    for (int r = 0; r < p.runs_per_clip; ++r) {
      const float* q = base + (size_t)r * p.pstride + 4 * M;
      const double nr = q[S_NSAMP];
      if (nr <= 0) continue;
      const double sr = q[S_DSUM + tid], qr = q[S_DSQ + tid];
      const double mr = q[S_PIVOT + tid] + sr / nr, m2r = fmax(0.0, qr - sr * sr / nr);
      const double d = mr - mean, nt = n + nr;
      m2 += m2r + d * d * n * nr / nt;
      mean += d * nr / nt;
      n = nt;
    }
    chmean[tid] = mean, chm2[tid] = m2;
  } else if (tid >= 64 && tid < 68) {
    const int s = tid - 64;
    double n = 0, mL = 0, mR = 0, c = 0;
    for (int r = 0; r < p.runs_per_clip; ++r) {
      const float* q = base + (size_t)r * p.pstride + 4 * M;
      const double nr = q[S_NSAMP];
      if (nr <= 0) continue;
      const double sL = q[S_DSUM + 2 * s], sR = q[S_DSUM + 2 * s + 1];
      const double mLr = q[S_PIVOT + 2 * s] + sL / nr, mRr = q[S_PIVOT + 2 * s + 1] + sR / nr;
      const double cr = q[S_CROSS + s] - sL * sR / nr;
      const double dL = mLr - mL, dR = mRr - mR, nt = n + nr;
      c += cr + dL * dR * n * nr / nt;
      mL += dL * nr / nt, mR += dR * nr / nt;
      n = nt;
    }
    cross[s] = c;
  }
  __syncthreads();

  const int sd = p.detailed_bins > 0 ? p.detailed_bins + 2 : 5;
  const int ps = 10 + sd;  // dynamics 6 + rel_loudness 1 + spectral + stereo 3
  float* out = p.feats + (size_t)clip * p.feat_dim;
  const int lane = tid & 63;
  auto put_lane = [&](int idx, double v) {
    float f = (float)v;
    f = fminf(fmaxf(f, -100.0f), 100.0f);  // clamp; fminf/fmaxf drop NaN like the NaN->0 step below
    if (v != v) f = 0.0f;                  // NaN -> 0 (mixing_utils.py:343-348)
    out[idx] = f;
  };
  auto put = [&](int idx, double v) {   // a value every lane of the wave holds: lane 0 stores it
    if (lane == 0) put_lane(idx, v);
  };
  const double n = (double)p.T;
  auto loud = [&](double ms) { return -0.691 + 10.0 * log10(ms + 1e-10); };
  {   // one wave per stem (the block has 4 waves): the sums over the bands are spread over its lanes
    const int s = tid >> 6;  // stem index in input order v,b,d,o ; sorted-key block order b,d,(mask),o,v
    const int blk = (s == 1) ? 0 : (s == 2) ? ps : (s == 3) ? 2 * ps + 4 : 3 * ps + 4;
    const double msL = sc[S_SQ + 2 * s] / n, msR = sc[S_SQ + 2 * s + 1] / n;
    const double rmsL = sqrt(msL), rmsR = sqrt(msR);
    const double l_stem = loud((sc[S_SQ + 2 * s] + sc[S_SQ + 2 * s + 1]) / (2 * n));
    const double l_mix = loud(sc[S_MIX] / (2 * n));
    // dynamics: rms L,R; crest L,R; loudness x2   (mixing_utils.py:107-139)
    put(blk + 0, rmsL);
    put(blk + 1, rmsR);
    put(blk + 2, 20.0 * log10(sc[S_PEAK + 2 * s] / (rmsL + 1e-8)));
    put(blk + 3, 20.0 * log10(sc[S_PEAK + 2 * s + 1] / (rmsR + 1e-8)));
    put(blk + 4, l_stem);
    put(blk + 5, l_stem);
    put(blk + 6, l_stem - l_mix);  // rel_loudness (:94-97)
    // spectral (:141-236)
    const double* e = band + s * M;
    const double cnt = 2.0 * M * p.F;
    const double flat = exp(sc[S_LOGSUM + s] / cnt) / (sc[S_LINSUM + s] / cnt + 1e-10);
    int o = blk + 7;
    if (p.detailed_bins == 0) {
      const int q = M / 4;
      double lo = 0, mi = 0, hi = 0;
      for (int i = lane; i < q; i += 64) lo += e[i];
      for (int i = q + lane; i < 3 * q; i += 64) mi += e[i];
      for (int i = 3 * q + lane; i < M; i += 64) hi += e[i];
      lo = wave_sum_f64(lo), mi = wave_sum_f64(mi), hi = wave_sum_f64(hi);
      put(o + 0, lo / q);
      put(o + 1, mi / (2 * q));
      put(o + 2, hi / (M - 3 * q));
      put(o + 3, pearson_vs_index(e, M, lane));
      put(o + 4, flat);
    } else {
      const int nb = p.detailed_bins;
      double* curve = reinterpret_cast<double*>(after_band + L::a_curve) + s * nb;
      for (int i = lane; i < nb; i += 64) {
        if (nb >= M) { curve[i] = e[i]; continue; }
        const float scale = nb > 1 ? (float)(M - 1) / (float)(nb - 1) : 0.f;  // align_corners=True
        const float src = scale * i;
        int i0 = (int)src;
        if (i0 > M - 1) i0 = M - 1;
        const int i1 = i0 + (i0 < M - 1 ? 1 : 0);
        const double lam = src - (float)i0;
        curve[i] = (1.0 - lam) * e[i0] + lam * e[i1];
      }
      __syncthreads();   // (uniform: every thread of the block takes this branch)
      for (int i = lane; i < nb; i += 64) put_lane(o + i, curve[i]);
      put(o + nb, pearson_vs_index(curve, nb, lane));
      put(o + nb + 1, flat);
    }
    o = blk + 7 + sd;
    // stereo (:238-268)
    put(o + 0, 20.0 * log10(rmsL / (rmsR + 1e-8)));
    put(o + 1, cross[s] / (sqrt(chm2[2 * s] * chm2[2 * s + 1]) + 1e-8));
    put(o + 2, (sc[S_SIDE + s] / (4 * n)) / (sc[S_MID + s] / (4 * n) + 1e-8));
    // masking (:270-309): block after drums
    put(2 * ps + s, sc[S_MASK + s] / ((double)M * p.F));
  }
}

// THE launch of a stage-A kernel: `lds` is the bytes() of the kernel's layout struct
template <auto Kernel, typename Params>
int launch_stage_a(const Params& kp, int grid, int threads, size_t lds, hipStream_t st) {
  MST_REQUIRE(lds <= kMaxLds, "mst_melfeat_forward: LDS %zu B exceeds 160 KiB", lds);
  const hipError_t e = mst::launch_lds<Kernel>(dim3(grid), dim3(threads), lds, st, kp);
  if (e != hipSuccess) return mst::fail(MST_EHIP, "stage-A kernel launch failed: %s", hipGetErrorString(e));
  return MST_OK;
}

template <int NFFT, int NB, typename ST>
int launch_melfeat(const KParams& kp, int grid, hipStream_t st) {
  return launch_stage_a<melfeat_kernel<NFFT, NB, ST>>(kp, grid, kThreads, GenericLds<NFFT>::bytes(kp.tw_count, kp.tw2_count, kp.nnz, kp.M, kp.tile_bufs), st);
}
template <int NFFT, typename ST, int WPS>
int launch_melfeat_spw(const KParams& kp, int grid, hipStream_t st) {
  return launch_stage_a<melfeat_spw_kernel<NFFT, ST, WPS>>(kp, grid, SpwGeom<WPS>::THREADS, SpwLds<NFFT, WPS>::bytes(kp.tw2_count, kp.nnz, kp.M), st);
}

#include "melfeat_v2.inc"
#include "melfeat_v2_2048.inc"

}  // namespace

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static_assert(sizeof(stage_a::F2) == sizeof(float2), "stage_a_tables.h's pairs are uploaded as float2");

struct mst_plan {
  int sr, n_fft, hop, n_mels, detailed_bins, feat_dim;
  int batches_per_run;   // StageAEnv::batches_per_run at creation
  mst::DevBuf<float> window;
  struct {   // melfeat_kernel, melfeat_spw_kernel: wave-FFT twiddles and the lane-band form of the mel table
    int nb, nnz, tw_count, tw2_count, glen[4], goff[4];
    mst::DevBuf<float2> tw, tw2, post;   // tw2: the n_fft-point complex FFT (frame-pair packing, n_fft <= 1024)
    mst::DevBuf<float> melw;
    mst::DevBuf<LaneBand> lanebands;
  } gen;
  struct {   // melfeat_v2_kernel (1024 / 256) or melfeat_v2_2048_kernel (2048 / 512), if `ok`: packed-FFT twiddles shared by both (tw4: 2048) and the piece table
    bool ok = false;
    int wps = 3;   // waves per stem
    int nslot = 0, maxcnt = 0, segw_count = 0, glen[kV2Slots] = {0}, goff[kV2Slots] = {0};
    mst::DevBuf<float2> tw2, tw3, tw4, segw;
    mst::DevBuf<int> start, id, bandtab;   // bandtab: int2 [256] (1024) or int [128] (2048)
  } sw;
};

namespace {

// The environment switches of stage A.  mst_plan_create takes batches_per_run and v2_wps2; every forward (and
// mst_plan_layout_supported) reads the others anew, so they can change between calls.
struct StageAEnv {
  int batches_per_run, spw_wps;   // MST_MELFEAT_BATCHES=n: n*16-frame runs of the older kernels (probes; 0: by clip length); MST_SPW_WPS (3)
  bool v2_wps2, generic, v2_nostd;   // MST_V2_WPS=2: 8-wave melfeat_v2_kernel; MST_MELFEAT_GENERIC: melfeat_kernel only; MST_V2_NOSTD
  bool old_kernels;      // MST_STAGE_A=spw | generic, or `generic`: no sliding-window kernel
};
StageAEnv read_stage_a_env() {
  auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  const char* a = getenv("MST_STAGE_A");
  StageAEnv s;
  s.batches_per_run = getenv("MST_MELFEAT_BATCHES") ? std::max(1, num("MST_MELFEAT_BATCHES", 0)) : 0;
  s.spw_wps = num("MST_SPW_WPS", 3);
  s.v2_wps2 = num("MST_V2_WPS", 0) == 2, s.generic = getenv("MST_MELFEAT_GENERIC"), s.v2_nostd = getenv("MST_V2_NOSTD");
  s.old_kernels = s.generic || (a && (!strcmp(a, "spw") || !strcmp(a, "generic")));
  return s;
}

// Frames per workgroup ("run").  Every workgroup costs about (frames + 2) frame-times and the device executes them in
// rounds of one workgroup per CU; with 32 runs per clip any batch that is a multiple of 8 clips fills whole rounds of
// the 256 CUs: 72 clips of 1723 frames -> 54-frame runs, 2304 workgroups = 9.0 rounds (486 frame-times per CU; fixed
// 32-frame runs took 16 rounds = 512).  The run length depends on the clip length only -- never on the batch size --
// so a clip's partial sums, and with them its features, are bit-identical whatever its batch neighbours are.
int frames_per_run_of(const mst_plan* p, int F) {
  if (p->batches_per_run > 0) return p->batches_per_run * kTF;
  int fpr = (F + 31) / 32;
  fpr += fpr & 1;
  return std::max(2 * kTF, fpr);
}
int runs_per_clip(const mst_plan* p, int F) {
  const int fpr = frames_per_run_of(p, F);
  return (F + fpr - 1) / fpr;
}
int pstride_of(const mst_plan* p) { return 4 * p->n_mels + kNumScalars; }

// sliding-window kernels: frames per wave and runs per clip (a run is wps * fpw frames: a function of the clip length only)
int sw_fpw(const mst_plan* p, int F) { return std::max(1, ((F + 31) / 32 + p->sw.wps - 1) / p->sw.wps); }
int sw_runs(const mst_plan* p, int F) {
  const int fpr = p->sw.wps * sw_fpw(p, F);
  return (F + fpr - 1) / fpr;
}

// the piece table has the shape melfeat_v2_kernel<..., STD> hard-codes (the 128-mel HTK filterbank at 44.1 kHz / n_fft 1024)
bool v2_table_is_standard(const mst_plan* p) {
  const auto& t = p->sw;
  return p->n_mels == 128 && t.nslot == 3 && t.maxcnt == 1 && t.glen[0] == 14 && t.glen[1] == 3 && !t.glen[2] && !t.goff[0] && t.goff[1] == 14 && t.goff[2] == 17;
}

}  // namespace

extern "C" {

int mst_plan_create(mst_plan** out, int sample_rate, int n_fft, int hop, int n_mels, const float* window,
                    const float* fb, int detailed_bins) {
  MST_REQUIRE(out && window && fb, "mst_plan_create: NULL argument");
  *out = nullptr;
  MST_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048,
              "mst_plan_create: n_fft=%d unsupported (512, 1024, 2048)", n_fft);
  MST_REQUIRE(hop >= 1 && n_mels >= 4 && n_mels <= 256, "mst_plan_create: bad hop=%d / n_mels=%d", hop, n_mels);
  MST_REQUIRE(detailed_bins >= 0 && detailed_bins <= 256 && (detailed_bins == 0 || detailed_bins < n_mels ||
              detailed_bins == n_mels), "mst_plan_create: bad detailed_bins=%d", detailed_bins);
  std::unique_ptr<mst_plan> p(new mst_plan());   // (a failed upload below frees what the plan already owns)
  p->sr = sample_rate, p->n_fft = n_fft, p->hop = hop, p->n_mels = n_mels, p->detailed_bins = detailed_bins;
  const int sd = detailed_bins > 0 ? detailed_bins + 2 : 5;
  p->feat_dim = 4 * (10 + sd) + 4;
  const StageAEnv env = read_stage_a_env();
  p->batches_per_run = env.batches_per_run;
  const int n_bins = n_fft / 2 + 1;
  auto& g = p->gen;
  auto& sw = p->sw;
  // sliding-window kernel, where the plan has one: the piece table and the packed-FFT twiddles
  const bool v2 = n_fft == 1024 && hop == 256, v4 = n_fft == 2048 && hop == 512 && n_mels <= 128;
  sw.wps = (env.v2_wps2 || n_mels > 128 || v4) ? 2 : 3;   // 4 bands per lane, and 2048 points, need the 256-register builds
  stage_a::PieceTable t;
  if (v2 || v4) t = stage_a::build_pieces(fb, n_bins, n_mels, v2 ? stage_a::v2_piece_opts(n_mels) : stage_a::v4_piece_opts());
  sw.ok = t.ok, sw.nslot = t.nslot, sw.maxcnt = t.maxcnt, sw.segw_count = (int)t.segw.size();
  for (int r = 0; r < kV2Slots; ++r) sw.glen[r] = t.glen[r], sw.goff[r] = t.goff[r];
  const std::vector<int> bands = !t.ok ? std::vector<int>() : v2 ? stage_a::pack_bands16(t, n_mels, stage_a::kV2Dump) : stage_a::pack_bands8(t, n_mels);
  std::vector<float2> t2(mstpk::kTw2Rows * 64), t3(mstpk::kTw3Rows * 64);
  mstpk::fill_twiddles_host(t2.data(), t3.data());
  const std::vector<stage_a::F2> t4 = v4 ? stage_a::tw4_twiddles() : std::vector<stage_a::F2>();

  // older kernels: the lane-band table and the wave-FFT twiddles
  g.nb = n_mels <= 128 ? 2 : 4;
  const stage_a::LaneBandTable lb = stage_a::build_lane_bands(fb, n_bins, n_mels, g.nb);
  g.nnz = lb.nnz;
  for (int r = 0; r < 4; ++r) g.glen[r] = lb.glen[r], g.goff[r] = lb.goff[r];
  const std::vector<stage_a::F2> tw = stage_a::fft_twiddles(n_fft / 2), post = stage_a::post_twiddles(n_fft);
  std::vector<stage_a::F2> tw2;
  if (n_fft <= 1024) tw2 = stage_a::fft_twiddles(n_fft);
  g.tw_count = (int)tw.size(), g.tw2_count = (int)tw2.size();
  if (tw2.empty()) tw2.push_back(stage_a::F2{1.f, 0.f});
  auto f2 = [](const std::vector<stage_a::F2>& v) { return reinterpret_cast<const float2*>(v.data()); };
  int rc;
  if ((t.ok && ((rc = sw.tw2.upload(t2.data(), t2.size())) || (rc = sw.tw3.upload(t3.data(), t3.size())) ||
                (v4 && (rc = sw.tw4.upload(f2(t4), t4.size()))) || (rc = sw.segw.upload(f2(t.segw), t.segw.size())) ||
                (rc = sw.start.upload(t.start.data(), t.start.size())) || (rc = sw.id.upload(t.id.data(), t.id.size())) ||
                (rc = sw.bandtab.upload(bands.data(), bands.size())))) ||
      (rc = p->window.upload(window, (size_t)n_fft)) || (rc = g.tw.upload(f2(tw), tw.size())) || (rc = g.tw2.upload(f2(tw2), tw2.size())) ||
      (rc = g.post.upload(f2(post), post.size())) || (rc = g.melw.upload(lb.melw.data(), lb.melw.size())) ||
      (rc = g.lanebands.upload(lb.lanebands.data(), lb.lanebands.size())))
    return rc;
  *out = p.release();
  return MST_OK;
}

void mst_plan_destroy(mst_plan* p) { delete p; }

int mst_plan_frames(const mst_plan* p, int T) { return p ? 1 + T / p->hop : MST_EINVAL; }
int mst_plan_feature_dim(const mst_plan* p) { return p ? p->feat_dim : MST_EINVAL; }

size_t mst_melfeat_workspace_bytes(const mst_plan* p, int B, int T) {
  if (!p || B <= 0 || T <= 0) return 0;
  const int F = 1 + T / p->hop;
  const int runs = std::max(runs_per_clip(p, F), p->sw.ok ? sw_runs(p, F) : 0);
  return mst::align_up((size_t)B * runs * pstride_of(p) * sizeof(float), 256);
}

}  // extern "C"

namespace {

struct LogmelOut {   // where and how the log-mel leaves stage A (mst.h: MST_LOGMEL_*)
  int layout = MST_LOGMEL_REF;
  void* lo = nullptr;          // MST_LOGMEL_CM16: low parts
  unsigned* absmax = nullptr;  // optional [B]
};

// MST_STAGE_A=spw | generic selects the older kernels
bool plan_uses_v2(const mst_plan* p) { return p->sw.ok && !read_stage_a_env().old_kernels; }

// fn(float{}) or fn(short{}): the sample type of the waveform;  fn(integral_constant<n_fft>): the generic kernel's FFT length
template <typename Fn>
int with_sample_type(bool pcm16, Fn fn) { return pcm16 ? fn(short{}) : fn(float{}); }
template <typename Fn>
auto with_n_fft(int n_fft, Fn fn) {
  if (n_fft == 512) return fn(std::integral_constant<int, 512>{});
  if (n_fft == 1024) return fn(std::integral_constant<int, 1024>{});
  return fn(std::integral_constant<int, 2048>{});
}

// The launch functions get their parameter struct with the common fields filled in.  K2Params or K4Params: the rest they share
template <typename Params, typename Launch>
int launch_sliding_window(const mst_plan* p, Params& k, const LogmelOut& lmo, bool pcm16, Launch launch) {
  const auto& sw = p->sw;
  k.out_mode = lmo.layout, k.logmel_lo = lmo.lo, k.absmax = lmo.absmax;
  k.tw2 = sw.tw2.get(), k.tw3 = sw.tw3.get(), k.segw = sw.segw.get();
  k.nslot = sw.nslot, k.segw_count = sw.segw_count, k.maxcnt = sw.maxcnt, k.fpw = sw_fpw(p, k.F);
  for (size_t r = 0; r < std::size(k.glen); ++r) k.glen[r] = sw.glen[r], k.goff[r] = sw.goff[r];
  return with_sample_type(pcm16, launch);
}

int launch_v2_2048(const mst_plan* p, K4Params k, const LogmelOut& lmo, bool pcm16, hipStream_t st) {
  k.tw4 = p->sw.tw4.get(), k.pstart = p->sw.start.get(), k.pid = p->sw.id.get(), k.bandtab = p->sw.bandtab.get();
  return launch_sliding_window(p, k, lmo, pcm16, [&](auto s) { return launch_melfeat_v2_2048<decltype(s)>(k, k.B * k.runs_per_clip, st); });
}

int launch_v2(const mst_plan* p, K2Params k, const LogmelOut& lmo, bool pcm16, bool no_std, hipStream_t st) {
  k.segstart = p->sw.start.get(), k.segid = p->sw.id.get(), k.bandtab = reinterpret_cast<const int2*>(p->sw.bandtab.get());
  const bool stdt = v2_table_is_standard(p) && !no_std;
  return launch_sliding_window(p, k, lmo, pcm16, [&](auto s) {
    using ST = decltype(s);
    const int grid = k.B * k.runs_per_clip;
    if (p->n_mels > 128) return launch_melfeat_v2<ST, 2, 4>(k, grid, st);   // 4 bands per lane, 4-frame blocks
    return p->sw.wps == 3 ? launch_melfeat_v2<ST, 3>(k, grid, st, stdt) : launch_melfeat_v2<ST, 2>(k, grid, st);
  });
}

size_t generic_lds_bytes(const mst_plan* p, int tile_bufs) {
  return with_n_fft(p->n_fft, [&](auto N) { return GenericLds<N()>::bytes(p->gen.tw_count, p->gen.tw2_count, p->gen.nnz, p->n_mels, tile_bufs); });
}

// stem-per-wave-pair kernel for the standard configuration; the generic kernel covers everything else
int launch_generic_or_spw(const mst_plan* p, KParams kp, bool pcm16, const StageAEnv& env, hipStream_t st) {
  const auto& g = p->gen;
  kp.tw = g.tw.get(), kp.tw2 = g.tw2.get(), kp.post = g.post.get(), kp.melw = g.melw.get(), kp.lanebands = g.lanebands.get();
  kp.hop = p->hop, kp.tw_count = g.tw_count, kp.tw2_count = g.tw2_count, kp.nnz = g.nnz;
  for (int r = 0; r < 4; ++r) kp.glen[r] = g.glen[r], kp.goff[r] = g.goff[r];
  kp.frames_per_run = frames_per_run_of(p, kp.F);
  bool base16 = true;
  for (int i = 0; i < 4; ++i) base16 = base16 && (reinterpret_cast<uintptr_t>(kp.stem[i]) & 15) == 0;
  kp.vec_ok = base16 && (kp.T % 2 == 0) && (p->hop % 2 == 0) && (kp.clip_stride % 2 == 0);
  kp.vec4_ok = base16 && (kp.T % 4 == 0) && (p->hop % 4 == 0) && (kp.clip_stride % 4 == 0);
  kp.tile_bufs = generic_lds_bytes(p, 2) <= kMaxLds ? 2 : 1;   // the output tile is double-buffered where the LDS allows
  const int grid = kp.B * kp.runs_per_clip, n_fft = p->n_fft, M = p->n_mels;
  const bool spw_ok = kp.vec_ok && kp.vec4_ok && p->hop * 4 == n_fft && M <= 128 && g.nb == 2 && (n_fft == 512 || n_fft == 1024) && !env.generic;
  const bool spw3 = spw_ok && env.spw_wps == 3 && n_fft == 1024 && SpwLds<1024, 3>::bytes(g.tw2_count, g.nnz, M) <= kMaxLds;
  const bool spw2 = spw_ok && !spw3 &&
                    (n_fft == 1024 ? SpwLds<1024, 2>::bytes(g.tw2_count, g.nnz, M) : SpwLds<512, 2>::bytes(g.tw2_count, g.nnz, M)) <= kMaxLds;
  return with_sample_type(pcm16, [&](auto s) {
    using ST = decltype(s);
    if (spw3) return launch_melfeat_spw<1024, ST, 3>(kp, grid, st);
    if (spw2) return n_fft == 1024 ? launch_melfeat_spw<1024, ST, 2>(kp, grid, st) : launch_melfeat_spw<512, ST, 2>(kp, grid, st);
    return with_n_fft(n_fft, [&](auto N) { return g.nb == 2 ? launch_melfeat<N(), 2, ST>(kp, grid, st) : launch_melfeat<N(), 4, ST>(kp, grid, st); });
  });
}

int melfeat_forward_impl(const mst_plan* p, const void* const stems4[4], bool pcm16, long long clip_stride, int B, int T,
                         float* logmel, float* feats, void* workspace, size_t workspace_bytes, void* stream, const LogmelOut& lmo = LogmelOut()) {
  MST_REQUIRE(p && stems4[0] && stems4[1] && stems4[2] && stems4[3], "mst_melfeat_forward: NULL plan/stems");
  MST_REQUIRE(clip_stride >= 2LL * T, "mst_melfeat_forward_stems: clip_stride %lld < 2*T", clip_stride);
  MST_REQUIRE(B > 0 && T > p->n_fft / 2, "mst_melfeat_forward: need B>0 and T > n_fft/2 (reflect pad); B=%d T=%d", B, T);
  MST_REQUIRE((long long)B * 8 * T < (1LL << 40), "mst_melfeat_forward: input too large");
  const size_t need = mst_melfeat_workspace_bytes(p, B, T);
  if (!workspace || workspace_bytes < need)
    return mst::fail(MST_ENOMEM, "mst_melfeat_forward: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = 1 + T / p->hop;
  // (a plan whose tables do not fit melfeat_kernel even with a single output tile is refused whichever kernel would run)
  const size_t lds = generic_lds_bytes(p, generic_lds_bytes(p, 2) <= kMaxLds ? 2 : 1);
  MST_REQUIRE(lds <= kMaxLds, "mst_melfeat_forward: LDS %zu B exceeds 160 KiB", lds);
  const StageAEnv env = read_stage_a_env();
  const bool use_sw = p->sw.ok && !env.old_kernels;
  MST_REQUIRE(lmo.layout == MST_LOGMEL_REF || use_sw, "mst_melfeat_forward: channel-minor log-mel needs the sliding-window kernels");
  if (lmo.absmax) {
    MST_REQUIRE(lmo.layout != MST_LOGMEL_REF, "mst_melfeat_forward: absmax comes with the channel-minor layouts only");
    MST_HIP_CHECK(hipMemsetAsync(lmo.absmax, 0, (size_t)B * sizeof(unsigned), st));
  }
  const int runs = use_sw ? sw_runs(p, F) : runs_per_clip(p, F);   // the finalise kernel walks the same partial records
  auto common = [&](auto k) {   // the fields KParams, K2Params and K4Params share
    for (int i = 0; i < 4; ++i) k.stem[i] = stems4[i];
    k.clip_stride = clip_stride, k.logmel = logmel, k.partials = reinterpret_cast<float*>(workspace), k.window = p->window.get();
    k.B = B, k.T = T, k.F = F, k.M = p->n_mels, k.runs_per_clip = runs, k.pstride = pstride_of(p);
    return k;
  };
  const int rc = !use_sw            ? launch_generic_or_spw(p, common(KParams{}), pcm16, env, st)
                 : p->n_fft == 2048 ? launch_v2_2048(p, common(K4Params{}), lmo, pcm16, st)
                                    : launch_v2(p, common(K2Params{}), lmo, pcm16, env.v2_nostd, st);
  if (rc) return rc;
  if (feats) {
    const FParams fp{reinterpret_cast<const float*>(workspace), feats, p->n_mels, F, T, runs, pstride_of(p), p->detailed_bins, p->feat_dim};
    hipLaunchKernelGGL(melfeat_finalize_kernel, dim3(B), dim3(256), FinalizeLds::bytes(p->n_mels, p->detailed_bins), st, fp);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mst::fail(MST_EHIP, "melfeat_finalize_kernel launch failed: %s", hipGetErrorString(e));
  }
  return MST_OK;
}

}  // namespace

extern "C" {

int mst_melfeat_forward(const mst_plan* p, const float* stems, int B, int T, float* logmel, float* feats,
                        void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(p && stems, "mst_melfeat_forward: NULL plan/stems");
  const void* four[4] = {stems, stems + 2 * (size_t)T, stems + 4 * (size_t)T, stems + 6 * (size_t)T};
  return melfeat_forward_impl(p, four, false, (long long)8 * T, B, T, logmel, feats, workspace, workspace_bytes, stream);
}

int mst_melfeat_forward_stems(const mst_plan* p, const float* const stems4[4], long long clip_stride, int B, int T,
                              float* logmel, float* feats, void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(p && stems4, "mst_melfeat_forward: NULL plan/stems");
  const void* four[4] = {stems4[0], stems4[1], stems4[2], stems4[3]};
  return melfeat_forward_impl(p, four, false, clip_stride, B, T, logmel, feats, workspace, workspace_bytes, stream);
}

int mst_melfeat_forward_pcm16(const mst_plan* p, const int16_t* stems, int B, int T, float* logmel, float* feats,
                              void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(p && stems, "mst_melfeat_forward_pcm16: NULL plan/stems");
  const void* four[4] = {stems, stems + 2 * (size_t)T, stems + 4 * (size_t)T, stems + 6 * (size_t)T};
  return melfeat_forward_impl(p, four, true, (long long)8 * T, B, T, logmel, feats, workspace, workspace_bytes, stream);
}

int mst_melfeat_forward_stems_pcm16(const mst_plan* p, const int16_t* const stems4[4], long long clip_stride, int B,
                                    int T, float* logmel, float* feats, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  MST_REQUIRE(p && stems4, "mst_melfeat_forward_pcm16: NULL plan/stems");
  const void* four[4] = {stems4[0], stems4[1], stems4[2], stems4[3]};
  return melfeat_forward_impl(p, four, true, clip_stride, B, T, logmel, feats, workspace, workspace_bytes, stream);
}

int mst_plan_layout_supported(const mst_plan* p, int layout) {
  if (!p) return 0;
  if (layout == MST_LOGMEL_REF) return 1;
  return (layout == MST_LOGMEL_CM32 || layout == MST_LOGMEL_CM16) && plan_uses_v2(p) ? 1 : 0;
}

int mst_melfeat_forward_io(const mst_plan* p, const mst_melfeat_io* io, int B, int T, void* workspace, size_t workspace_bytes,
                           void* stream) {
  MST_REQUIRE(p && io, "mst_melfeat_forward_io: NULL plan/io");
  MST_REQUIRE(io->layout >= MST_LOGMEL_REF && io->layout <= MST_LOGMEL_CM16, "mst_melfeat_forward_io: unknown layout %d", io->layout);
  MST_REQUIRE(mst_plan_layout_supported(p, io->layout),
              "mst_melfeat_forward_io: layout %d is not available for this plan (n_fft %d, hop %d: query mst_plan_layout_supported)",
              io->layout, p->n_fft, p->hop);
  MST_REQUIRE(io->layout == MST_LOGMEL_REF || !io->logmel || (reinterpret_cast<uintptr_t>(io->logmel) & 15) == 0,
              "mst_melfeat_forward_io: channel-minor log-mel must be 16-byte aligned");
  MST_REQUIRE(io->layout != MST_LOGMEL_CM16 || !io->logmel_lo || (reinterpret_cast<uintptr_t>(io->logmel_lo) & 15) == 0,
              "mst_melfeat_forward_io: channel-minor log-mel must be 16-byte aligned");
  const LogmelOut lo{io->layout, io->logmel_lo, io->absmax};
  const void* four[4] = {io->stems4[0], io->stems4[1], io->stems4[2], io->stems4[3]};
  return melfeat_forward_impl(p, four, io->pcm16 != 0, io->clip_stride, B, T, static_cast<float*>(io->logmel), io->feats, workspace,
                              workspace_bytes, stream, lo);
}

}  // extern "C"
