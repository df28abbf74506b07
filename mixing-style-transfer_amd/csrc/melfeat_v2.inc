// Stage A, "sliding window" kernel for the standard configuration (n_fft 1024, hop 256, n_mels <= 128) -- included by
// melfeat.hip (shares KParams' conventions, Smp<>, the partial-record slots and the finalise kernel).
//
// Same work split as melfeat_spw_kernel (one workgroup = one clip x one run of frames, WPS waves per stem, a wave
// transforms the L and R channel of one frame as ONE 1024-point complex FFT), but built around what bounded that
// kernel -- exposed latency and instruction count, not bandwidth:
//   * a wave walks CONSECUTIVE frames and keeps the frame's 1024 un-windowed (L, R) samples in registers
//     (element n = lane + 64 t, 16 register pairs): the next frame re-uses 12 of the 16 (shift by 4) and loads only the
//     256 new samples per channel -- issued one whole frame ahead, so their latency hides behind the current FFT.
//     Every sample is fetched once per wave (4x fewer vector-memory instructions, no L1/L2 re-reads of the overlap);
//   * FFT on packed-fp32 VALU, radix 16 x 8 x 8 with two LDS exchanges, and a last pass that leaves X[k] and X[1024-k]
//     in the same lane (fft_pk.h): the two-real-channels split costs no cross-lane traffic;
//   * sparse mel by SEGMENT: the triangular filters overlap pairwise, so every bin feeds exactly two bands, the one
//     falling and the one rising over the segment [centre s-1, centre s] it lies in.  A lane owns up to three segments
//     (dealt by length so the trip counts are uniform and short: 14 + 4 + 1 bins at 128 mels instead of 27 + 18 per
//     band pair), accumulates both edge sums of both channels with two packed FMAs per bin, and band b is
//     rising(b) + falling(b + 1) after a 6-store / 4-load exchange inside the wave's scratch;
//   * log-mel output, two layouts (K2Params::out_mode):
//       0  the reference's (B, 8, M, F) (model.py:41-67): 16-byte stores of 4 consecutive frames per (channel, band) row
//          straight from the registers -- every store instruction scatters 64 lanes to 64 rows (what a caller of
//          MelSpectrogramPreprocessor.forward gets);
//       1  the encoder's internal CHANNEL-MINOR layout [B][F][M][8 ch] fp32 (32 bytes per (frame, band), 4 KB per frame) and
//       2  the same as float16 hi + lo planes [B][F][M][8 ch] (what the f16 / split-precision conv1 kernels read without
//          any conversion): a block's values are transposed through the FFT scratch of the block's four stem waves (free
//          between the frame loop and the next block) so that every store instruction writes 1 KB of contiguous bytes and
//          every 128-byte line is written whole, once;
//   * the mixture energy needs all four stems of a sample: the wave of stem s takes the s-th quarter of the 256 samples
//     a frame owns and loads the 8 channels of those 64 samples (issued before the FFT, consumed after it);
//   * inter-stem masking needs the 4 stems' channel-mean mel of the same (frame, band): exchanged through a small LDS
//     buffer once per block of 4 frames (two barriers per block; everything else in the frame loop is wave-private).
// Partial records are the same as melfeat_kernel's (same finalise kernel).

constexpr int kV2Slots = 6;   // (slot, lane) pairs a lane can own: ceil(pieces / 64) <= 6

struct K2Params {
  const void* stem[4];
  long long clip_stride;
  float* logmel;           // out_mode 0: [B][8][M][F]; 1: [B][F][M][8] fp32; 2: [B][F][M][8] float16 (high parts)
  void* logmel_lo;         // out_mode 2: low parts, same layout
  unsigned* absmax;        // optional [B]: max |log-mel| of the clip as float bits (atomicMax; the caller zeroes it)
  int out_mode;
  float* partials;
  const float* window;
  const float2* tw2;       // fft_pk pass-2 twiddles [7][64]
  const float2* tw3;       // fft_pk pass-3 twiddles [14][64]
  const float2* segw;      // [(goff[slot] + i) * 64 + lane] = (falling weight, rising weight) of bin segstart + i
  const int* segstart;     // [slot][64] first bin of the lane's PIECE in this slot (a piece = at most 16 bins of a segment)
  const int* segid;        // [slot][64] piece index (its slot in the exchange arrays); unused lanes point at the dump slot
  const int2* bandtab;     // [NBL][64] band lane + 64 r: (first rising piece | count << 16, first falling piece | count << 16)
  int B, T, F, M;
  int nslot, glen[kV2Slots], goff[kV2Slots], segw_count;
  int maxcnt;              // most pieces any segment has; 1 = every segment is one piece and piece index == segment index
  int fpw;                 // frames per wave; a run is WPS * fpw frames
  int runs_per_clip, pstride;
};

namespace v2 {
using namespace mstpk;

constexpr int kP2 = 0;          // v2f P2[k] = (|A[k]|^2, |B[k]|^2), k = 0..512, then 16 zeros
constexpr int kExN = 288;       // entries per piece-sum array (the last one, kExDump, is the dump slot of unused lanes)
constexpr int kExDump = kExN - 1;
constexpr int kExHi = 544;      // v2f rising-edge sums per piece
constexpr int kExLo = kExHi + kExN;
static_assert(kExLo + kExN <= kScr, "exchange areas must fit the FFT scratch");
static_assert(kExDump == stage_a::kV2Dump && kV2Slots == stage_a::kMaxSlots, "the piece table is built for these limits");

// |A|^2 and |s B|^2 (times 4) of bin k from Z[k] and Z[N-k]:  Z[k] + Z[N-k] = (2 Re A, 2 Re sB),
// Z[k] - Z[N-k] = (-2 Im sB, 2 Im A)
__device__ __forceinline__ v2f pair_power4(v2f zk, v2f zm) {
  const v2f s = zk + zm, d = zk - zm;
  const v2f q = s * s;
  v2f r;
  asm("v_pk_fma_f32 %0, %1, %1, %2 op_sel:[1,1,0] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(d), "v"(q));   // (d.y^2 + q.x, d.x^2 + q.y)
  return r;
}

// lane-mask select (mask bit set -> a).  Written as v_cndmask on purpose: `lane0 ? x[i] : x[j]` on register arrays
// is turned into a dynamic index by the optimiser, i.e. a 32-deep select chain per element.
__device__ __forceinline__ v2f sel2(unsigned long long m, v2f a, v2f b) {
  float rx, ry;
  const float ax = a.x, ay = a.y, bx = b.x, by = b.y;
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(rx) : "v"(bx), "v"(ax), "s"(m));
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(ry) : "v"(by), "v"(ay), "s"(m));
  return mk(rx, ry);
}

// element `idx` of a wave-uniform base pointer: the BYTE offset is formed in 32 bits, so the load takes the scalar-base +
// 32-bit lane offset form (global_load ... v_off, s[base]) instead of a 64-bit address per lane (2-3 VALU per load)
template <typename ST>
__device__ __forceinline__ float ld_at(const ST* base, int idx) {
  const unsigned boff = (unsigned)idx * (unsigned)sizeof(ST);
  return Smp<ST>::lds(reinterpret_cast<const ST*>(reinterpret_cast<const char*>(base) + boff));
}

__device__ __forceinline__ v2f bcast_fma(float w, v2f q, v2f acc) { return __builtin_elementwise_fma(mk(w, w), q, acc); }

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));

// ---- channel-minor log-mel output (out_mode 1: [B][F][M][8 ch] fp32; 2: float16 high and low planes of that shape).
// A block's values are transposed through the FFT scratch of the block's four stem waves, which is free between the frame
// loop and the next block.  A staged frame = 4 stem planes of MB (L, R) pairs; the plane pitch PSTR makes the 8-byte
// reads of the store step conflict-free (two planes are 2 * PSTR = 32 words mod 64 apart).
template <int NBL>
struct CmGeom {
  static constexpr int MB = 64 * NBL, PSTR = 2 * MB + 16, TILE = 4 * PSTR;   // 32-bit words
};
// max |log-mel| of a block's valid values -> one LDS word of the workgroup (bit patterns of non-negative floats order like
// unsigned integers); the range bound of the float16 convolutions, so that no separate pass has to read the log-mel
template <int NBL, int BLK>
__device__ __forceinline__ void block_absmax(const float (&out)[2 * NBL][BLK], int lane, int nv, int M, unsigned* s_amax) {
  float bm = 0.f;
#pragma unroll
  for (int r = 0; r < NBL; ++r)
#pragma unroll
    for (int e = 0; e < BLK; ++e)
      if (e < nv && lane + 64 * r < M) bm = fmaxf(bm, fmaxf(fabsf(out[2 * r][e]), fabsf(out[2 * r + 1][e])));
  bm = mst::wave_max(bm);
  if (lane == 0) atomicMax(s_amax, __float_as_uint(bm));
}
// step 1 (after the barrier that ends the frame loop): every stem wave hands its (L, R) pairs of frame e to the scratch of
// the wave of stem e & 3 of its sub-run h, one plane per stem -- contiguous 8-byte stores
template <int NBL, int BLK, int WPS, int SCR>
__device__ __forceinline__ void cm_stage(const float (&out)[2 * NBL][BLK], v2f* s_scr, int h, int stem, int lane, int nv, int out_mode) {
  using G = CmGeom<NBL>;
  static_assert((BLK / 4) * G::TILE <= 2 * SCR, "the staged frames of a wave must fit its FFT scratch");
#pragma unroll
  for (int e = 0; e < BLK; ++e) {
    if (e < nv) {   // wave-uniform
      float* tl = reinterpret_cast<float*>(s_scr + ((e & 3) * WPS + h) * SCR) + (e >> 2) * G::TILE + stem * G::PSTR;
#pragma unroll
      for (int r = 0; r < NBL; ++r) {
        const float vL = out[2 * r][e], vR = out[2 * r + 1][e];
        v2f val;
        if (out_mode == 2) {   // (hi L, hi R) and (lo L, lo R) as two packed float16 pairs: x ~ hi + lo, 22 significant bits
          const _Float16 hL = (_Float16)vL, hR = (_Float16)vR;
          const h16x2 hi = {hL, hR}, lo = {(_Float16)(vL - (float)hL), (_Float16)(vR - (float)hR)};
          val = mk(__builtin_bit_cast(float, hi), __builtin_bit_cast(float, lo));
        } else {
          val = mk(vL, vR);
        }
        *reinterpret_cast<v2f*>(tl + 2 * (lane + 64 * r)) = val;
      }
    }
  }
}
// step 2 (after the next barrier): the wave of stem w owns frames e = w, w + 4, .. of the block and writes them as whole
// 16-byte units of 4 (fp32) or 8 (float16) channels -- 1 KB of contiguous global memory per store instruction, every
// 128-byte line written whole and once.  frow0 = (clip * F + first frame of the block) * M, in units of 8 channels.
template <int NBL, int BLK>
__device__ __forceinline__ void cm_store(const v2f* scr, int stem, int lane, int nv, size_t frow0, int M, float* logmel, void* logmel_lo,
                                         int out_mode) {
  using G = CmGeom<NBL>;
#pragma unroll
  for (int q = 0; q < BLK / 4; ++q) {
    const int e = 4 * q + stem;
    if (e < nv) {   // wave-uniform
      const float* tl = reinterpret_cast<const float*>(scr) + q * G::TILE;
      const size_t frow = frow0 + (size_t)e * M;
      if (out_mode == 1) {
        f32x4v* dst = reinterpret_cast<f32x4v*>(logmel) + frow * 2;
#pragma unroll
        for (int it = 0; it < 2 * NBL; ++it) {
          const int g = 64 * it + lane, b = g >> 1, pp = g & 1;
          const v2f a0 = *reinterpret_cast<const v2f*>(tl + (2 * pp) * G::PSTR + 2 * b);
          const v2f a1 = *reinterpret_cast<const v2f*>(tl + (2 * pp + 1) * G::PSTR + 2 * b);
          if (b < M) dst[g] = f32x4v{a0.x, a0.y, a1.x, a1.y};
        }
      } else {
        f32x4v* dhi = reinterpret_cast<f32x4v*>(logmel) + frow;
        f32x4v* dlo = reinterpret_cast<f32x4v*>(logmel_lo) + frow;
#pragma unroll
        for (int it = 0; it < NBL; ++it) {
          const int b = 64 * it + lane;
          v2f a[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = *reinterpret_cast<const v2f*>(tl + j * G::PSTR + 2 * b);
          if (b < M) {
            dhi[b] = f32x4v{a[0].x, a[1].x, a[2].x, a[3].x};
            if (logmel_lo) dlo[b] = f32x4v{a[0].y, a[1].y, a[2].y, a[3].y};   // (NULL: the caller reads the high parts only)
          }
        }
      }
    }
  }
}


}  // namespace v2

// BLK = frames per block (log-mel leaves as BLK/4 16-byte stores per row; one masking exchange per block): 8 with two
// waves per SIMD (WPS = 2, 256 registers), 4 with three (WPS = 3, 168 registers).
// WIN_LDS: the lane's 16 window values are re-read from LDS every frame instead of living in 16 registers.
// SB = frames per log-mel STORE block (a row leaves the registers as SB/4 adjacent 16-byte stores).
template <int WPS> struct V2Geom {
  static constexpr int BLK = WPS == 2 ? 8 : 4;
  static constexpr int SB = BLK;
  static constexpr bool WIN_LDS = true;        // both builds: 16 registers buy more than 16 ds_read_b32 per frame cost
  static constexpr bool MIX_EARLY = WPS == 2;  // mixture loads issued before the FFT (8 registers across it)
};

// LDS of melfeat_v2_kernel<., WPS, NBL, ..>; a_*: from the end of segw[segw_count]
template <int WPS, int NBL>
struct V2Lds {
  static constexpr int BLK = NBL == 2 ? V2Geom<WPS>::BLK : 4, MB = 64 * NBL, WAVES = 4 * WPS;
  // v2f tw2[7 * 64], tw3[14 * 64], segw[segw_count] (even)
  static constexpr int tw2 = 0, tw3 = tw2 + mstpk::kTw2Rows * 64 * 8, segw = tw3 + mstpk::kTw3Rows * 64 * 8;
  // float win[1024] (only when the window does not live in registers), exch[WPS][BLK frames][4 stems][MB]
  static constexpr int a_win = 0, a_exch = a_win + (V2Geom<WPS>::WIN_LDS ? 1024 * 4 : 0);
  // v2f scr[WAVES][kScr] (FFT scratch, piece sums, channel-minor staging, final reduction); unsigned amax, padded to 16 bytes
  static constexpr int a_scr = a_exch + WPS * BLK * 4 * MB * 4, a_amax = a_scr + WAVES * mstpk::kScr * 8;
  static constexpr size_t bytes(int segw_count) { return (size_t)segw + (size_t)segw_count * 8 + a_amax + 16; }
  static_assert(WAVES * NBL * 64 + WAVES * 16 <= 2 * WAVES * mstpk::kScr, "the reduction buffer must fit the FFT scratch");
};

// NBL = bands per lane: 2 (n_mels <= 128) or 4 (n_mels <= 256, BASELINE configs[4]; two waves per SIMD only).
// CM: the channel-minor output build (out_mode 1 or 2, optional absmax); false: the reference layout (out_mode 0) -- two
// builds because the 168-register budget of three waves per SIMD holds either store path, not both.
// STD: the piece table is the one of the standard 128-mel filterbank at 44.1 kHz / n_fft 1024 (three slots of 14 + 3 + 0 bins,
// every segment one piece, both band rows full) -- checked on the host (v2_table_is_standard); its shape then is a set of
// compile-time constants: no table words in scalar registers, straight-line piece walks with all their LDS reads issued up
// front, no band-validity masks.
template <typename ST, int WPS, int NBL = 2, bool CM = false, bool STD = false>
__global__ __launch_bounds__(WPS * 256) void melfeat_v2_kernel(const K2Params p) {
  // No implicit mul + add contraction in this kernel: its instantiations (rolled / unrolled frames, either output layout) must
  // return the SAME feature bits for the same clip, and which a * b + c the optimiser fuses depends on the code around it.
  // (Every fused multiply-add that is meant is spelled fmaf / __builtin_elementwise_fma / v_pk_fma.)
#pragma clang fp contract(off)
  using namespace mstpk;
  using namespace v2;
  using L = V2Lds<WPS, NBL>;
  constexpr int kWaves = L::WAVES, kThreads = kWaves * 64, BLK = L::BLK, MB = L::MB;
  constexpr bool kUnrollBlock = STD && BLK == 4;   // the standard-table build walks its 4-frame blocks unrolled (melfeat_v2_frame.inc)
  constexpr bool WIN_LDS = V2Geom<WPS>::WIN_LDS, MIX_EARLY = V2Geom<WPS>::MIX_EARLY;
  constexpr int SB = BLK;
  constexpr float kLn2 = 0.69314718055994530942f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  v2f* s_tw2 = reinterpret_cast<v2f*>(smem + L::tw2);
  v2f* s_tw3 = reinterpret_cast<v2f*>(smem + L::tw3);
  v2f* s_segw = reinterpret_cast<v2f*>(smem + L::segw);
  unsigned char* after_segw = reinterpret_cast<unsigned char*>(s_segw + p.segw_count);
  float* s_win = reinterpret_cast<float*>(after_segw + L::a_win);
  float* s_exch = reinterpret_cast<float*>(after_segw + L::a_exch);
  v2f* s_scr = reinterpret_cast<v2f*>(after_segw + L::a_scr);
  unsigned* s_amax = reinterpret_cast<unsigned*>(after_segw + L::a_amax);
  static_assert(!STD || NBL == 2, "the standard table has 128 bands");
  const int M = STD ? 128 : p.M, T = p.T;
  const int nslot = STD ? 3 : p.nslot, maxcnt = STD ? 1 : p.maxcnt;
  constexpr int kStdLen[3] = {14, 3, 0}, kStdOff[3] = {0, 14, 17};   // (slot 2: the 129th piece, an empty segment)
  constexpr bool cm = CM;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: keep it (and all the
  //                                                               frame bookkeeping derived from it) on the scalar unit
  const int work = mst::xcd_remap(blockIdx.x, gridDim.x);
  const int clip = work / p.runs_per_clip, run = work % p.runs_per_clip;
  const int fpr = WPS * p.fpw;
  const int f_begin = run * fpr;
  const int f_end = min(p.F, f_begin + fpr);
  {
    const v2f* g2 = reinterpret_cast<const v2f*>(p.tw2);
    const v2f* g3 = reinterpret_cast<const v2f*>(p.tw3);
    const v2f* gs = reinterpret_cast<const v2f*>(p.segw);
    for (int i = tid; i < kTw2Rows * 64; i += kThreads) s_tw2[i] = g2[i];
    for (int i = tid; i < kTw3Rows * 64; i += kThreads) s_tw3[i] = g3[i];
    for (int i = tid; i < p.segw_count; i += kThreads) s_segw[i] = gs[i];
    if (WIN_LDS)
      for (int i = tid; i < 1024; i += kThreads) s_win[i] = p.window[i];
    if (tid == 0) *s_amax = 0u;
  }
  const int stem = wave / WPS, h = wave % WPS;
  auto chan = [&](int c) {
    return static_cast<const ST*>(p.stem[c >> 1]) + (size_t)clip * p.clip_stride + (size_t)(c & 1) * T;
  };
  const ST* const xL = chan(2 * stem);
  const ST* const xR = chan(2 * stem + 1);
  const int o_begin = f_begin * 256;
  const int o_end = (f_end == p.F) ? T : min(T, f_end * 256);
  const int o_piv = min(o_begin, T - 1);
  const float pvL = Smp<ST>::ld(xL + o_piv), pvR = Smp<ST>::ld(xR + o_piv);
  v2f* scr = s_scr + wave * kScr;
  float* exch = s_exch + h * (BLK * 4 * MB);   // this sub-run's exchange block: [frame][stem][band]

  // window of the 16 elements this lane owns, as register pairs (w[2q], w[2q+1])
  v2f wp[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
    wp[q] = WIN_LDS ? mk(0.f, 0.f) : mk(p.window[lane + 64 * (2 * q)], p.window[lane + 64 * (2 * q + 1)]);
  constexpr int NSL = NBL == 2 ? 3 : kV2Slots;   // slots the kernel walks (n_mels <= 128: at most 3, checked on the host)
  int seg_start[NSL], seg_id[NSL];
#pragma unroll
  for (int r = 0; r < NSL; ++r) {
    seg_start[r] = r < nslot ? p.segstart[r * 64 + lane] : 0;
    seg_id[r] = r < nslot ? p.segid[r * 64 + lane] : kExDump;
  }
  int2 btab[NBL];
#pragma unroll
  for (int r = 0; r < NBL; ++r) btab[r] = p.bandtab[r * 64 + lane];
  const int jb = jb_of(lane);
  const bool l0 = lane == 0;

  float acc_db[NBL], acc_log = 0.f, acc_lin = 0.f, acc_mask = 0.f, mixsq = 0.f;
#pragma unroll
  for (int r = 0; r < NBL; ++r) acc_db[r] = 0.f;
  float sqL = 0.f, sqR = 0.f, pkL = 0.f, pkR = 0.f, dsL = 0.f, dsR = 0.f, dqL = 0.f, dqR = 0.f;
  float cr = 0.f, mid = 0.f, side = 0.f;

  const int f0 = f_begin + h * p.fpw;
  const int nfw = max(0, min(p.fpw, f_end - f0));   // frames of this wave (wave-uniform)
  auto ld2 = [&](int pos) {   // (L, R) at absolute sample position pos, reflect-padded
    const int q = reflect_idx(pos, T);
    return mk(ld_at(xL, q), ld_at(xR, q));
  };
  v2f raw[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) raw[t] = mk(0.f, 0.f);
  if (nfw > 0) {
    const int b0 = f0 * 256 - 512 + lane;
#pragma unroll
    for (int t = 0; t < 16; ++t) raw[t] = ld2(b0 + 64 * t);
  }
  __syncthreads();

  // mixture energy of the sub-run's first kMixLead hops (the frame loop takes hop f + kMixLead at frame f, see melfeat_v2_frame.inc)
  constexpr int kMixLead = 2;
#pragma unroll
  for (int k = 0; k < kMixLead; ++k) {
    const int mp0 = (f0 + k) * 256 + 64 * stem + lane;
    if (k < nfw && mp0 < T) {
      float c8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) c8[c] = ld_at(chan(c), mp0);
      const float mL = ((c8[0] + c8[2]) + c8[4]) + c8[6];   // python sum(): ((v + b) + d) + o
      const float mR = ((c8[1] + c8[3]) + c8[5]) + c8[7];
      mixsq = fmaf(mL, mL, mixsq);
      mixsq = fmaf(mR, mR, mixsq);
    }
  }

  const int nblk = (p.fpw + BLK - 1) / BLK;
  float out[2 * NBL][SB];   // [2 * r + c][frame of the store block]: log-mel of band lane + 64 r, channel c
#pragma unroll
  for (int k = 0; k < 2 * NBL; ++k)
#pragma unroll
    for (int e = 0; e < SB; ++e) out[k][e] = 0.f;
  auto store_block = [&](int fb0, int cnt) __attribute__((always_inline)) {
    if (!p.logmel || CM) return;
#pragma unroll
    for (int r = 0; r < NBL; ++r) {
      const int b = lane + 64 * r;
      if (b < M) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float* dst = p.logmel + (((size_t)clip * 8 + 2 * stem + c) * M + b) * p.F + fb0;
          const float* o = out[2 * r + c];
#pragma unroll
          for (int e = 0; e < SB; e += 4) {
            if (e + 4 <= cnt) {   // wave-uniform
              const f4u v4 = f4u{o[e], o[e + 1], o[e + 2], o[e + 3]};
              *reinterpret_cast<f4u*>(dst + e) = v4;
            } else {
#pragma unroll
              for (int q = 0; q < 3; ++q)
                if (e + q < cnt) dst[e + q] = o[e + q];
            }
          }
        }
      }
    }
  };
#pragma unroll 1
  for (int blk = 0; blk < nblk; ++blk) {
    const int nv = max(0, min(BLK, nfw - blk * BLK));   // valid frames of this block
    if constexpr (kUnrollBlock) {
      static_assert(!kUnrollBlock || (BLK == 4 && SB == 4), "the unrolled block rotates 16 registers in 4 frames");
#define MST_FRAME_STATIC 1
      if (0 < nv) {
#define MST_FRAME_I 0
#include "melfeat_v2_frame.inc"
#undef MST_FRAME_I
      }
      if (1 < nv) {
#define MST_FRAME_I 1
#include "melfeat_v2_frame.inc"
#undef MST_FRAME_I
      }
      if (2 < nv) {
#define MST_FRAME_I 2
#include "melfeat_v2_frame.inc"
#undef MST_FRAME_I
      }
      if (3 < nv) {
#define MST_FRAME_I 3
#include "melfeat_v2_frame.inc"
#undef MST_FRAME_I
      }
#undef MST_FRAME_STATIC
    } else {
#define MST_FRAME_STATIC 0
#define MST_FRAME_I fi
#pragma unroll 1
      for (int fi = 0; fi < nv; ++fi)
#include "melfeat_v2_frame.inc"
#undef MST_FRAME_I
#undef MST_FRAME_STATIC
    }
    // ---- log-mel stores: a store block of SB frames is complete (or the wave's ragged tail).  (Deferring them behind the
    //      next frame's loads, and pinning those loads below the window stage so that no vmcnt wait has to drain younger
    //      operations, both measured 2-7 % SLOWER than this plain order -- profiles/README.md, round 2.)
    {
      const int done = min(nfw, (blk + 1) * BLK);          // frames finished so far
      if (nv > 0 && (done % SB == 0 || done == nfw)) {
        const int cnt = (done - 1) % SB + 1;               // frames sitting in slots 0 .. cnt - 1
        store_block(f0 + done - cnt, cnt);
      }
    }
    __syncthreads();
    // inter-stem masking (mixing_utils.py:288-307) for the block's valid frames
#pragma unroll
    for (int r = 0; r < NBL; ++r) {
      const int b = lane + 64 * r;
      if (b < M) {
#pragma unroll 2
        for (int e = 0; e < nv; ++e) {
          float other = -INFINITY, own = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float sj = exch[(e * 4 + j) * MB + b];
            other = (j != stem) ? fmaxf(other, sj) : other;
            own = (j == stem) ? sj : own;
          }
          acc_mask += __builtin_amdgcn_rcpf(1.0f + __expf(own - other));   // sigmoid(other - own)
        }
      }
    }
    if (cm && p.absmax) block_absmax<NBL, BLK>(out, lane, nv, M, s_amax);
    if (cm && p.logmel) cm_stage<NBL, BLK, WPS, kScr>(out, s_scr, h, stem, lane, nv, p.out_mode);
    __syncthreads();
    if (cm && p.logmel)
      cm_store<NBL, BLK>(scr, stem, lane, nv, ((size_t)clip * p.F + (f0 + blk * BLK)) * M, M, p.logmel, p.logmel_lo, p.out_mode);
  }
  if (cm) __syncthreads();   // the reduction below reuses the scratch: every wave has read its staged frames

  // ---- reductions -> partial record (same slots as melfeat_kernel)
  float* red = reinterpret_cast<float*>(s_scr);   // [kWaves][NBL][64] band sums, then per-wave scalars [kWaves][16]
#pragma unroll
  for (int r = 0; r < NBL; ++r) red[(wave * NBL + r) * 64 + lane] = acc_db[r];
  float* red2 = red + kWaves * NBL * 64;
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
  for (int i = tid; i < 4 * MB; i += kThreads) {
    const int s = i / MB, b = i % MB;
    if (b < M) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < WPS; ++w) v += red[((WPS * s + w) * NBL + (b >> 6)) * 64 + (b & 63)];
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
  if (cm && p.absmax && tid == 0) atomicMax(p.absmax + clip, *s_amax);   // (the barrier above orders the waves' LDS maxima)
  if (tid == 8) {
    float mxs = 0.f;
    for (int w = 0; w < kWaves; ++w) mxs += red2[w * 16 + 11];
    part[4 * M + S_MIX] = mxs;
    part[4 * M + S_NSAMP] = (float)max(0, o_end - o_begin);
    part[4 * M + S_NFRAME] = (float)max(0, f_end - f_begin);
  }
}

// std_table: the plan's piece table has the standard shape (see STD above); used by the channel-minor builds of the 12-wave kernel
template <typename ST, int WPS, int NBL = 2>
int launch_melfeat_v2(const K2Params& kp, int grid, hipStream_t st, bool std_table = false) {
  const size_t lds = V2Lds<WPS, NBL>::bytes(kp.segw_count);
  if constexpr (WPS == 3 && NBL == 2)
    if (std_table && kp.out_mode != 0) return launch_stage_a<melfeat_v2_kernel<ST, WPS, NBL, true, true>>(kp, grid, WPS * 256, lds, st);
  return kp.out_mode != 0 ? launch_stage_a<melfeat_v2_kernel<ST, WPS, NBL, true>>(kp, grid, WPS * 256, lds, st)
                          : launch_stage_a<melfeat_v2_kernel<ST, WPS, NBL, false>>(kp, grid, WPS * 256, lds, st);
}
