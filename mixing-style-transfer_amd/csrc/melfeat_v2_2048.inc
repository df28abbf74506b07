// Stage A, sliding-window kernel for n_fft = 2048 / hop 512 (the reference's working launcher configuration,
// scripts/train_baseline.sh: 2048 / 512 / 80 mels) -- included by melfeat.hip after melfeat_v2.inc, whose structure it
// follows (read that file's header first).  What differs:
//   * the wave's window holds sample PAIRS: column t of a lane is the pair (x[2m], x[2m+1]), m = lane + 64 t, of both
//     channels (16 x float4 = 64 registers).  A hop of 512 samples is 256 pairs = 4 columns, so the shift-by-4 /
//     load-4-new-columns walk is the one of the 1024-point kernel, in pair units;
//   * the 2048-point complex FFT of (L + i s R) is ONE decimation-in-time step over two 1024-point FFTs -- E of the even
//     and O of the odd samples, both through fft1024 (fft_pk.h) on the same scratch -- and
//     Z[k] = E[k] + W_2048^k O[k],  Z[k + 1024] = E[k] - W_2048^k O[k].  fft1024 leaves index k and index 1024 - k in the
//     same lane, so Z[k] and its mirror Z[2048 - k] = E[1024 - k] - W^(1024 - k) O[1024 - k] are again lane-local: the
//     L / R split needs no cross-lane traffic.  (Round 1 used the even/odd REAL-FFT packing for 2048 points, whose split
//     leaks eps |bass peak| into the top octave: 3-10x pocketfft's noise on real music.  This is an ordinary complex
//     DIT step -- no such cancellation.)
//   * segments of the 80-mel filterbank are up to 82 bins long: they are cut into PIECES of at most 16 bins, dealt to
//     lanes by length as before, and a band sums the (at most 6) pieces of its rising and of its falling segment.
// Two waves per SIMD (8 waves, ~230 registers), 4-frame blocks.

struct K4Params {
  const void* stem[4];
  long long clip_stride;
  float* logmel;           // out_mode 0: [B][8][M][F]; 1: [B][F][M][8] fp32; 2: [B][F][M][8] float16 high parts (melfeat_v2.inc)
  void* logmel_lo;         // out_mode 2: low parts
  unsigned* absmax;        // optional [B]: max |log-mel| of the clip as float bits (atomicMax; the caller zeroes it)
  int out_mode;
  float* partials;
  const float* window;     // [2048]
  const float2* tw2;       // fft_pk pass-2 twiddles [7][64]
  const float2* tw3;       // fft_pk pass-3 twiddles [14][64]
  const float2* tw4;       // [16][64]: W_2048^k, k = lane + 128 t (rows 0..7) and jb(lane) + 128 t (rows 8..15)
  const float2* segw;      // [(goff[slot] + i) * 64 + lane] = (falling, rising) weight of bin pstart + i
  const int* pstart;       // [slot][64] first bin of the lane's piece
  const int* pid;          // [slot][64] piece index = its slot in the exchange arrays (unused lanes: the dump slot 135)
  const int* bandtab;      // [2][64] band lane + 64 r: first_rising | count << 8 | first_falling << 16 | count << 24
  int B, T, F, M;
  int nslot, glen[4], goff[4], segw_count, maxcnt;
  int fpw, runs_per_clip, pstride;
};

namespace v4 {
constexpr int kScr4 = 1328;      // float2 per wave: FFT scratch (1152) / P2[1025 + 16 zeros] + two piece-sum arrays
constexpr int kEx4Hi = 1056;     // rising-edge sums per piece [136]
constexpr int kEx4Lo = 1192;     // falling-edge sums per piece [136]
constexpr int kWPS = 2, kBLK = 4;
constexpr int kEx4N = stage_a::kV4Dump + 1;   // entries per piece-sum array; the last one is the dump slot of unused lanes
static_assert(kEx4N == 136 && kEx4Hi + kEx4N <= kEx4Lo && kEx4Lo + kEx4N <= kScr4, "exchange areas must fit the FFT scratch");
}  // namespace v4

// LDS of melfeat_v2_2048_kernel; a_*: from the end of segw[segw_count]
struct V4Lds {
  static constexpr int WAVES = 4 * v4::kWPS;
  // v2f tw2[7 * 64], tw3[14 * 64], tw4[16 * 64], segw[segw_count] (even)
  static constexpr int tw2 = 0, tw3 = tw2 + mstpk::kTw2Rows * 64 * 8, tw4 = tw3 + mstpk::kTw3Rows * 64 * 8, segw = tw4 + 16 * 64 * 8;
  // v2f win[1024] pairs (w[2m], w[2m+1]); float exch[WPS][BLK frames][4 stems][128]; v2f scr[WAVES][kScr4]; unsigned amax, padded to 16 bytes
  static constexpr int a_win = 0, a_exch = a_win + 1024 * 8, a_scr = a_exch + v4::kWPS * v4::kBLK * 4 * 128 * 4, a_amax = a_scr + WAVES * v4::kScr4 * 8;
  static constexpr size_t bytes(int segw_count) { return (size_t)segw + (size_t)segw_count * 8 + a_amax + 16; }
  static_assert(WAVES * 2 * 64 + WAVES * 16 <= 2 * WAVES * v4::kScr4, "the reduction buffer must fit the FFT scratch");
};

template <typename ST, bool CM = false>   // CM: channel-minor output build (melfeat_v2.inc)
__global__ __launch_bounds__(512) void melfeat_v2_2048_kernel(const K4Params p) {
  using namespace mstpk;
  using namespace v2;
  using namespace v4;
  using L = V4Lds;
  constexpr int WPS = kWPS, BLK = kBLK, kWaves = L::WAVES, kThreads = kWaves * 64;
  constexpr float kLn2 = 0.69314718055994530942f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  v2f* s_tw2 = reinterpret_cast<v2f*>(smem + L::tw2);
  v2f* s_tw3 = reinterpret_cast<v2f*>(smem + L::tw3);
  v2f* s_tw4 = reinterpret_cast<v2f*>(smem + L::tw4);
  v2f* s_segw = reinterpret_cast<v2f*>(smem + L::segw);
  unsigned char* after_segw = reinterpret_cast<unsigned char*>(s_segw + p.segw_count);
  v2f* s_win = reinterpret_cast<v2f*>(after_segw + L::a_win);
  float* s_exch = reinterpret_cast<float*>(after_segw + L::a_exch);
  v2f* s_scr = reinterpret_cast<v2f*>(after_segw + L::a_scr);
  unsigned* s_amax = reinterpret_cast<unsigned*>(after_segw + L::a_amax);
  const int M = p.M, T = p.T;
  constexpr bool cm = CM;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int work = mst::xcd_remap(blockIdx.x, gridDim.x);
  const int clip = work / p.runs_per_clip, run = work % p.runs_per_clip;
  const int fpr = WPS * p.fpw;
  const int f_begin = run * fpr;
  const int f_end = min(p.F, f_begin + fpr);
  {
    const v2f* g2 = reinterpret_cast<const v2f*>(p.tw2);
    const v2f* g3 = reinterpret_cast<const v2f*>(p.tw3);
    const v2f* g4 = reinterpret_cast<const v2f*>(p.tw4);
    const v2f* gs = reinterpret_cast<const v2f*>(p.segw);
    const v2f* gw = reinterpret_cast<const v2f*>(p.window);
    for (int i = tid; i < kTw2Rows * 64; i += kThreads) s_tw2[i] = g2[i];
    for (int i = tid; i < kTw3Rows * 64; i += kThreads) s_tw3[i] = g3[i];
    for (int i = tid; i < 16 * 64; i += kThreads) s_tw4[i] = g4[i];
    for (int i = tid; i < p.segw_count; i += kThreads) s_segw[i] = gs[i];
    for (int i = tid; i < 1024; i += kThreads) s_win[i] = gw[i];
    if (tid == 0) *s_amax = 0u;
  }
  const int stem = wave / WPS, h = wave % WPS;
  auto chan = [&](int c) {
    return static_cast<const ST*>(p.stem[c >> 1]) + (size_t)clip * p.clip_stride + (size_t)(c & 1) * T;
  };
  const ST* const xL = chan(2 * stem);
  const ST* const xR = chan(2 * stem + 1);
  const int o_begin = f_begin * 512;
  const int o_end = (f_end == p.F) ? T : min(T, f_end * 512);
  const int o_piv = min(o_begin, T - 1);
  const float pvL = Smp<ST>::ld(xL + o_piv), pvR = Smp<ST>::ld(xR + o_piv);
  v2f* scr = s_scr + wave * kScr4;
  float* exch = s_exch + h * (BLK * 4 * 128);

  int pstart[4], pid[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pstart[r] = r < p.nslot ? p.pstart[r * 64 + lane] : 0;
    pid[r] = r < p.nslot ? p.pid[r * 64 + lane] : 135;
  }
  const int btab[2] = {p.bandtab[lane], p.bandtab[64 + lane]};
  const int jb = jb_of(lane);
  const bool l0 = lane == 0;

  float acc_db[2] = {0.f, 0.f}, acc_log = 0.f, acc_lin = 0.f, acc_mask = 0.f, mixsq = 0.f;
  float sqL = 0.f, sqR = 0.f, pkL = 0.f, pkR = 0.f, dsL = 0.f, dsR = 0.f, dqL = 0.f, dqR = 0.f;
  float cr = 0.f, mid = 0.f, side = 0.f;

  const int f0 = f_begin + h * p.fpw;
  const int nfw = max(0, min(p.fpw, f_end - f0));
  // the sample pair (x[2 pr], x[2 pr + 1]) of one channel, reflect-padded per sample
  auto ldpair = [&](const ST* base, int pr) {
    return mk(ld_at(base, reflect_idx(2 * pr, T)), ld_at(base, reflect_idx(2 * pr + 1, T)));
  };
  auto ld4 = [&](int pr) {   // (L even, L odd, R even, R odd)
    const v2f a = ldpair(xL, pr), b = ldpair(xR, pr);
    return v4f{a.x, a.y, b.x, b.y};
  };
  v4f raw[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) raw[t] = v4f{0.f, 0.f, 0.f, 0.f};
  if (nfw > 0) {
    const int b0 = f0 * 256 - 512 + lane;   // pair index of column 0 (frame start = sample 512 f - 1024)
#pragma unroll
    for (int t = 0; t < 16; ++t) raw[t] = ld4(b0 + 64 * t);
  }
  __syncthreads();

  constexpr int kMixLead = 2;
#pragma unroll
  for (int k = 0; k < kMixLead; ++k) {   // mixture energy of the sub-run's first hops
    const int mp0 = (f0 + k) * 256 + 64 * stem + lane;
    if (k < nfw && 2 * mp0 < T) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        if (2 * mp0 + hh < T) {
          float c8[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) c8[c] = ld_at(chan(c), 2 * mp0 + hh);
          const float mL = ((c8[0] + c8[2]) + c8[4]) + c8[6];   // python sum(): ((v + b) + d) + o
          const float mR = ((c8[1] + c8[3]) + c8[5]) + c8[7];
          mixsq = fmaf(mL, mL, mixsq);
          mixsq = fmaf(mR, mR, mixsq);
        }
      }
    }
  }
  const int nblk = (p.fpw + BLK - 1) / BLK;
  float out[4][BLK];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < BLK; ++e) out[k][e] = 0.f;
#pragma unroll 1
  for (int blk = 0; blk < nblk; ++blk) {
    const int nv = max(0, min(BLK, nfw - blk * BLK));
#pragma unroll 1
    for (int i = 0; i < nv; ++i) {
      const int f = f0 + blk * BLK + i;
      // ---- window the even and the odd half, L/R balance
      v2f xe[16], xo[16];
      float ma = 0.f, mb = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const v2f w = s_win[lane + 64 * t];
        xe[t] = mk(raw[t].x * w.x, raw[t].z * w.x);
        xo[t] = mk(raw[t].y * w.y, raw[t].w * w.y);
        ma = fmaxf(ma, fmaxf(fabsf(xe[t].x), fabsf(xo[t].x)));
        mb = fmaxf(mb, fmaxf(fabsf(xe[t].y), fabsf(xo[t].y)));
      }
      const unsigned ua = wave_umax_uniform(__float_as_uint(ma)), ub = wave_umax_uniform(__float_as_uint(mb));
      int dep;   // opaque zero that depends on the reduction: keeps this frame's loads below the first use of the old ones
      asm volatile("s_mov_b32 %0, 0" : "=s"(dep) : "s"(ua), "s"(ub));
      // ---- the next frame's 256 new pairs per channel (consumed at the end of this frame)
      const bool more = blk * BLK + i + 1 < nfw;
      v4f nxt[4];
      {
        const int base2 = f * 256 + 512 + dep, b2 = base2 + lane;
        if (more) {
          if (2 * (base2 + 255) + 1 < T) {   // wave-uniform: interior
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int pr = b2 + 64 * j;
              nxt[j] = v4f{ld_at(xL, 2 * pr), ld_at(xL, 2 * pr + 1), ld_at(xR, 2 * pr), ld_at(xR, 2 * pr + 1)};
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) nxt[j] = ld4(b2 + 64 * j);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) nxt[j] = v4f{0.f, 0.f, 0.f, 0.f};
        }
      }
      int sh = 0;
      if (ua != 0u && ub != 0u) sh = max(-40, min(40, (int)(ua >> 23) - (int)(ub >> 23)));
      if (sh != 0) {
        const float sc = __uint_as_float((unsigned)(127 + sh) << 23);
#pragma unroll
        for (int t = 0; t < 16; ++t) xe[t].y *= sc, xo[t].y *= sc;
      }
      const float ia = ua != 0u ? 1.0f : 0.f;
      const float ib = ub != 0u ? __uint_as_float((unsigned)(127 - 2 * sh) << 23) : 0.f;
      // ---- waveform moments from the 512 samples this frame owns (columns 8..11, both halves)
      auto moments = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n0 = 2 * (f * 256 + lane + 64 * j);
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            const bool ok = n0 + hh < T;
            const float L = ok ? (hh ? raw[8 + j].y : raw[8 + j].x) : 0.f, R = ok ? (hh ? raw[8 + j].w : raw[8 + j].z) : 0.f;
            const float dL = ok ? L - pvL : 0.f, dR = ok ? R - pvR : 0.f;
            sqL = fmaf(L, L, sqL), sqR = fmaf(R, R, sqR);
            pkL = fmaxf(pkL, fabsf(L)), pkR = fmaxf(pkR, fabsf(R));
            dsL += dL, dsR += dR;
            dqL = fmaf(dL, dL, dqL), dqR = fmaf(dR, dR, dqR);
            cr = fmaf(dL, dR, cr);
            mid = fmaf(L + R, L + R, mid);
            side = fmaf(L - R, L - R, side);
          }
        }
      };
      // ---- E = FFT of the even samples, O = FFT of the odd samples
      fft1024(xe, scr, s_tw2, s_tw3, lane, moments);
      __builtin_amdgcn_wave_barrier();
      fft1024(xo, scr, s_tw2, s_tw3, lane);
      // ---- DIT combine, split into the two channels, power: P2[k] = (|L[k]|^2, |R[k]|^2), k = 0..1024
      __builtin_amdgcn_wave_barrier();
      {
        // xo <- W^k O (in place); D = E - W^k O.  Z[k] = E + W^k O is formed on the fly.
        v2f D[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          xo[t] = cmul(xo[t], s_tw4[t * 64 + lane]);
          D[t] = xe[t] - xo[t];
        }
        const v2f sc4 = mk(0.25f * ia, 0.25f * ib);
        v2f* P2 = scr;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const v2f za = xe[t] + xo[t], zb = xe[8 + t] + xo[8 + t];
          // mirror Z[2048 - k]: generic lanes pair butterfly a (index lane + 128 t) with b (index 128 - lane + 128 (7 - t));
          // lane 0 holds the self-paired butterflies 0 and 64
          const v2f ma0 = t == 0 ? za : D[(8 - t) & 7];
          const v2f zm_a = sel2(1ull, ma0, D[8 + 7 - t]);
          const v2f zm_b = sel2(1ull, D[8 + 7 - t], D[7 - t]);
          P2[lane + 128 * t] = pair_power4(za, zm_a) * sc4;
          P2[jb + 128 * t] = pair_power4(zb, zm_b) * sc4;
        }
        if (l0) P2[1024] = D[0] * D[0] * mk(ia, ib);    // Nyquist: Z[1024] = E[0] - O[0] = L + i s R with both real
        if (lane < 16) P2[1025 + lane] = mk(0.f, 0.f);  // the piece walks may run past bin 1024 (zero weights there)
      }
      // mixture quarter of this stem: pairs 256 f + 64 stem + lane of the 8 channels (latency hides behind the mel)
      // (of the hop the frame two ahead owns -- the pairs the stem waves are loading right now -- see melfeat_v2_frame.inc; the
      //  sub-run's first kMixLead hops are added up before the loop)
      float mx[16];
      const int mpair = blk * BLK + i + kMixLead < nfw ? (f + kMixLead) * 256 + 64 * stem + lane : T;
      {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          mx[2 * c] = ld_at(chan(c), min(2 * mpair, T - 1));
          mx[2 * c + 1] = ld_at(chan(c), min(2 * mpair + 1, T - 1));
        }
      }
      __builtin_amdgcn_wave_barrier();
      // ---- sparse mel by pieces of segments
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r < p.nslot) {
          v2f slo = mk(0.f, 0.f), shi = mk(0.f, 0.f);
          const v2f* pw = s_segw + p.goff[r] * 64 + lane;
          const v2f* pp = scr + pstart[r];
          const int n = p.glen[r];
#pragma unroll 2
          for (int k = 0; k < n; ++k) {
            const v2f w = pw[k * 64];
            const v2f q = pp[k];
            slo = bcast_fma(w.x, q, slo);
            shi = bcast_fma(w.y, q, shi);
          }
          scr[kEx4Hi + pid[r]] = shi;
          scr[kEx4Lo + pid[r]] = slo;
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int b = lane + 64 * r;
        const int fh = btab[r] & 255, ch = (btab[r] >> 8) & 255, fl = (btab[r] >> 16) & 255, cl = (btab[r] >> 24) & 255;
        v2f m = mk(0.f, 0.f);
        for (int q = 0; q < p.maxcnt; ++q) {
          const v2f a = scr[kEx4Hi + min(fh + q, 135)], c = scr[kEx4Lo + min(fl + q, 135)];
          m += (q < ch ? a : mk(0.f, 0.f)) + (q < cl ? c : mk(0.f, 0.f));
        }
        const bool ok = b < M;
        const float l0v = __log2f(m.x + 1e-10f) * kLn2, l1v = __log2f(m.y + 1e-10f) * kLn2;
        switch (i) {
#define MST_PUT(E) case E: out[2 * r][E] = l0v, out[2 * r + 1][E] = l1v; break;
          MST_PUT(0) MST_PUT(1) MST_PUT(2) MST_PUT(3)
#undef MST_PUT
        }
        if (ok) {
          acc_db[r] += l0v + l1v;
          acc_log += l0v + l1v;
          acc_lin += m.x + m.y;
          exch[(i * 4 + stem) * 128 + b] = 0.5f * (m.x + m.y);
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (2 * mpair < T) {   // mixture energy of this stem's quarter (python sum(): ((v + b) + d) + o)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          if (2 * mpair + hh < T) {
            const float mL = ((mx[hh] + mx[4 + hh]) + mx[8 + hh]) + mx[12 + hh];
            const float mR = ((mx[2 + hh] + mx[6 + hh]) + mx[10 + hh]) + mx[14 + hh];
            mixsq = fmaf(mL, mL, mixsq);
            mixsq = fmaf(mR, mR, mixsq);
          }
        }
      }
      // ---- slide the window by one hop (4 columns of pairs)
#pragma unroll
      for (int t = 0; t < 12; ++t) raw[t] = raw[t + 4];
#pragma unroll
      for (int j = 0; j < 4; ++j) raw[12 + j] = nxt[j];
    }
    // ---- the block's log-mel
    if (nv > 0 && p.logmel && !cm) {
      const int fb0 = f0 + blk * BLK;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int b = lane + 64 * r;
        if (b < M) {
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            float* dst = p.logmel + (((size_t)clip * 8 + 2 * stem + c) * M + b) * p.F + fb0;
            const float* o = out[2 * r + c];
            if (nv == 4) {
              *reinterpret_cast<f4u*>(dst) = f4u{o[0], o[1], o[2], o[3]};
            } else {
#pragma unroll
              for (int q = 0; q < 3; ++q)
                if (q < nv) dst[q] = o[q];
            }
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int b = lane + 64 * r;
      if (b < M) {
#pragma unroll 2
        for (int e = 0; e < nv; ++e) {
          float other = -INFINITY, own = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float sj = exch[(e * 4 + j) * 128 + b];
            other = (j != stem) ? fmaxf(other, sj) : other;
            own = (j == stem) ? sj : own;
          }
          acc_mask += __builtin_amdgcn_rcpf(1.0f + __expf(own - other));
        }
      }
    }
    // channel-minor output: transposed through the four stem waves' scratch (melfeat_v2.inc: cm_stage / cm_store)
    if (cm && p.absmax) block_absmax<2, BLK>(out, lane, nv, M, s_amax);
    if (cm && p.logmel) cm_stage<2, BLK, WPS, kScr4>(out, s_scr, h, stem, lane, nv, p.out_mode);
    __syncthreads();
    if (cm && p.logmel)
      cm_store<2, BLK>(scr, stem, lane, nv, ((size_t)clip * p.F + (f0 + blk * BLK)) * M, M, p.logmel, p.logmel_lo, p.out_mode);
  }
  if (cm) __syncthreads();   // the reduction below reuses the scratch: every wave has read its staged frames

  // ---- reductions -> partial record (same slots as melfeat_kernel)
  float* red = reinterpret_cast<float*>(s_scr);
#pragma unroll
  for (int r = 0; r < 2; ++r) red[(wave * 2 + r) * 64 + lane] = acc_db[r];
  float* red2 = red + kWaves * 2 * 64;
  {
    const float v[13] = {acc_log, acc_lin, sqL, sqR, dsL, dsR, dqL, dqR, cr, mid, side, mixsq, acc_mask};
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      const float r = mst::wave_sum(v[k]);
      if (lane == 0) red2[wave * 16 + k] = r;
    }
    const float a = mst::wave_max(pkL), b = mst::wave_max(pkR);
    if (lane == 0) red2[wave * 16 + 13] = a, red2[wave * 16 + 14] = b;
  }
  __syncthreads();
  float* part = p.partials + ((size_t)clip * p.runs_per_clip + run) * p.pstride;
  for (int i = tid; i < 4 * 128; i += kThreads) {
    const int s = i >> 7, b = i & 127;
    if (b < M) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < WPS; ++w) v += red[((WPS * s + w) * 2 + (b >> 6)) * 64 + (b & 63)];
      part[s * M + b] = v;
    }
  }
  if (tid < 4) {
    const int s = tid;
    float v[13], pk0 = 0.f, pk1 = 0.f;
#pragma unroll
    for (int k = 0; k < 13; ++k) v[k] = 0.f;
    for (int w = 0; w < WPS; ++w) {
      const float* a = red2 + (WPS * s + w) * 16;
#pragma unroll
      for (int k = 0; k < 13; ++k) v[k] += a[k];
      pk0 = fmaxf(pk0, a[13]), pk1 = fmaxf(pk1, a[14]);
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
    q[S_MASK + s] = v[12];
    q[S_PEAK + 2 * s] = pk0, q[S_PEAK + 2 * s + 1] = pk1;
    q[S_PIVOT + 2 * s] = Smp<ST>::ld(chan(2 * s) + o_piv), q[S_PIVOT + 2 * s + 1] = Smp<ST>::ld(chan(2 * s + 1) + o_piv);
  }
  if (cm && p.absmax && tid == 0) atomicMax(p.absmax + clip, *s_amax);
  if (tid == 8) {
    float mxs = 0.f;
    for (int w = 0; w < kWaves; ++w) mxs += red2[w * 16 + 11];
    part[4 * M + S_MIX] = mxs;
    part[4 * M + S_NSAMP] = (float)max(0, o_end - o_begin);
    part[4 * M + S_NFRAME] = (float)max(0, f_end - f_begin);
  }
}

template <typename ST>
int launch_melfeat_v2_2048(const K4Params& kp, int grid, hipStream_t st) {
  const size_t lds = V4Lds::bytes(kp.segw_count);
  return kp.out_mode != 0 ? launch_stage_a<melfeat_v2_2048_kernel<ST, true>>(kp, grid, 512, lds, st)
                          : launch_stage_a<melfeat_v2_2048_kernel<ST, false>>(kp, grid, 512, lds, st);
}
