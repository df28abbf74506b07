// Host-side tables of stage A (melfeat.hip): FFT twiddles, the lane-band form of the mel filterbank (melfeat_kernel,
// melfeat_spw_kernel) and its piece form (melfeat_v2_kernel, melfeat_v2_2048_kernel).  Plain C++17, no HIP include: the
// builders compile and run without a GPU (tests/test_stage_a_tables_cpu.py).  F2 is uploaded as float2, LaneBand as is.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace stage_a {

struct F2 { float x, y; };
struct LaneBand { int band, start; };   // a mel band owned by a lane: band id (-1 = none), first bin of its support
inline F2 unit(double a) { return F2{(float)std::cos(a), (float)std::sin(a)}; }

// pass twiddles of the NC-point wave FFT (fft_wave.h FftPlan<NC>); empty for other lengths
inline std::vector<F2> fft_twiddles(int NC) {
  static const int kPasses[3][5][2] = {{{4, 1}, {4, 4}, {4, 16}, {4, 64}}, {{8, 1}, {8, 8}, {8, 64}}, {{8, 1}, {8, 8}, {4, 64}, {4, 256}}};
  std::vector<F2> tw;
  if (NC != 256 && NC != 512 && NC != 1024) return tw;
  for (const int* pass = kPasses[NC / 512][0]; pass[0]; pass += 2) {   // (radix R, stride NS) per pass, zero-terminated
    const int R = pass[0], NS = pass[1];
    if (NS == 1) continue;
    const int nbf = NS <= 64 ? 1 : NC / R / 64;  // (lane + 64 u) % NS does not depend on u when NS divides 64
    for (int u = 0; u < nbf; ++u)
      for (int t = 1; t < R; ++t)
        for (int lane = 0; lane < 64; ++lane) tw.push_back(unit(-2.0 * M_PI * (double)((lane + 64 * u) % NS * t) / (double)(NS * R)));
  }
  return tw;
}

// W_n_fft^k, k < n_fft / 2: the real-FFT split of the even/odd packing
inline std::vector<F2> post_twiddles(int n_fft) {
  std::vector<F2> post((size_t)n_fft / 2);
  for (int k = 0; k < n_fft / 2; ++k) post[k] = unit(-2.0 * M_PI * (double)k / (double)n_fft);
  return post;
}
// melfeat_v2_2048_kernel: [16][64] W_2048^k, k = lane + 128 t (rows 0..7) and jb(lane) + 128 t (rows 8..15)
inline std::vector<F2> tw4_twiddles() {
  std::vector<F2> t4(16 * 64);
  for (int t = 0; t < 8; ++t)
    for (int lane = 0; lane < 64; ++lane)
      for (int u = 0; u < 2; ++u)
        t4[(size_t)(8 * u + t) * 64 + lane] = unit(-2.0 * M_PI * (double)((u ? (lane ? 128 - lane : 64) : lane) + 128 * t) / 2048.0);
  return t4;
}

// Lane-band form.  lane -> bands: slot r even: r/2*128 + lane ; r odd: (r/2)*128 + 127 - lane  (pairs a narrow low band with a
// wide high band).  Weights go into a zero-padded table melw[goff[r] + i*64 + lane], i < glen[r] = the longest support in
// slot r, so the gather loop has a uniform trip count and no divergence.
struct LaneBandTable {
  std::vector<LaneBand> lanebands;   // [nb][64]
  std::vector<float> melw;           // never empty (one zero when the filterbank is)
  int nnz = 0, glen[4] = {0, 0, 0, 0}, goff[4] = {0, 0, 0, 0};   // nnz: floats of melw in use
};
inline LaneBandTable build_lane_bands(const float* fb, int n_bins, int M, int nb) {
  std::vector<int> start(M, 0), len(M, 0);   // per band contiguous support [start, start+len)
  for (int m = 0; m < M; ++m) {
    int lo = -1, hi = -1;
    for (int k = 0; k < n_bins; ++k)
      if (fb[(size_t)k * M + m] != 0.0f) lo = lo < 0 ? k : lo, hi = k;
    if (lo >= 0) start[m] = lo, len[m] = hi - lo + 1;
  }
  LaneBandTable t;
  t.lanebands.resize((size_t)nb * 64);
  for (int r = 0; r < nb; ++r) {
    int gl = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const int m = (r / 2) * 128 + ((r & 1) ? 127 - lane : lane);
      t.lanebands[(size_t)r * 64 + lane] = (m < M) ? LaneBand{m, start[m]} : LaneBand{-1, 0};
      if (m < M) gl = std::max(gl, len[m]);
    }
    t.glen[r] = gl, t.goff[r] = (int)t.melw.size();
    t.melw.resize(t.melw.size() + (size_t)gl * 64, 0.f);
    for (int lane = 0; lane < 64; ++lane) {
      const int m = t.lanebands[(size_t)r * 64 + lane].band;
      for (int i = 0; m >= 0 && i < len[m]; ++i) t.melw[(size_t)t.goff[r] + (size_t)i * 64 + lane] = fb[(size_t)(start[m] + i) * M + m];
    }
  }
  t.nnz = (int)t.melw.size();
  if (t.melw.empty()) t.melw.push_back(0.f);
  return t;
}

// seg(k), falling weight wl(k) (band seg - 1) and rising weight wh(k) (band seg) of every bin; false unless every bin feeds
// at most two ADJACENT bands and the segments are contiguous bin ranges.
inline bool segment_bins(const float* fb, int n_bins, int M, std::vector<int>& seg, std::vector<float>& wl, std::vector<float>& wh) {
  std::vector<int> peak(M, -1);
  for (int m = 0; m < M; ++m) {
    float best = 0.f;
    for (int k = 0; k < n_bins; ++k)
      if (fb[(size_t)k * M + m] > best) best = fb[(size_t)k * M + m], peak[m] = k;
  }
  seg.assign(n_bins, 0), wl.assign(n_bins, 0.f), wh.assign(n_bins, 0.f);
  int prev = 0;
  for (int k = 0; k < n_bins; ++k) {
    int b0 = -1, b1 = -1, cnt = 0;
    for (int m = 0; m < M; ++m)
      if (fb[(size_t)k * M + m] != 0.0f) b0 = cnt++ ? b0 : m, b1 = m;
    if (cnt > 2 || (cnt == 2 && b1 != b0 + 1)) return false;
    int s = prev;
    if (cnt == 2) {
      s = b1, wl[k] = fb[(size_t)k * M + b0], wh[k] = fb[(size_t)k * M + b1];
    } else if (cnt == 1) {
      if (k <= peak[b0]) s = b0, wh[k] = fb[(size_t)k * M + b0];
      else s = b0 + 1, wl[k] = fb[(size_t)k * M + b0];
    }
    if (s < prev) return false;
    seg[k] = prev = s;
  }
  return true;
}

constexpr int kMaxSlots = 6;   // (slot, lane) pairs a lane can own
struct PieceOpts {   // what the two sliding-window kernels' piece tables differ in, beside the packing of the band table
  bool empty_piece;   // an empty segment becomes one empty piece (piece index == segment index while no segment is cut)
  int dump;           // piece id of unused lanes: the dump slot of the kernel's exchange arrays; pieces stay below it
  int max_slots;      // ceil(pieces / 64) the kernel walks
};
constexpr int kV2Dump = 287, kV4Dump = 135;   // (the kernels assert them against their exchange arrays)
inline PieceOpts v2_piece_opts(int M) { return PieceOpts{true, kV2Dump, M <= 128 ? 3 : kMaxSlots}; }   // n_fft 1024
inline PieceOpts v4_piece_opts() { return PieceOpts{false, kV4Dump, 4}; }                               // n_fft 2048
struct PieceTable {
  bool ok = false;               // false: the filterbank does not have the structure, or exceeds the kernel's limits
  std::vector<F2> segw;          // [(goff[slot] + i) * 64 + lane] = (falling, rising) weight of bin start + i; even length
  std::vector<int> start, id;    // [nslot][64] first bin and index of the lane's piece
  std::vector<int> first, cnt;   // [M + 1] pieces of segment s: first .. first + cnt - 1
  int nslot = 0, maxcnt = 0, glen[kMaxSlots] = {0}, goff[kMaxSlots] = {0};   // maxcnt: most pieces any segment has
};

// Bin k feeds the falling edge of band s-1 and the rising edge of band s, s = seg(k).  Segments are cut into pieces of at
// most 16 bins (numbered in segment order), pieces are dealt to (slot, lane) by length so that the trip counts are uniform
// and short, and band b sums the pieces of its rising segment (b) and of its falling segment (b + 1).
inline PieceTable build_pieces(const float* fb, int n_bins, int M, const PieceOpts& o) {
  PieceTable t;
  std::vector<int> seg;
  std::vector<float> wl, wh;
  if (!segment_bins(fb, n_bins, M, seg, wl, wh)) return t;
  const int nseg = M + 1;
  std::vector<int> start(nseg, 0), len(nseg, 0);
  for (int k = n_bins - 1; k >= 0; --k) start[seg[k]] = k, ++len[seg[k]];
  struct Piece { int start, len; };
  std::vector<Piece> pieces;
  t.first.assign(nseg, 0), t.cnt.assign(nseg, 0);
  for (int sg = 0; sg < nseg; ++sg) {
    t.first[sg] = (int)pieces.size();
    if (len[sg] == 0 && o.empty_piece) pieces.push_back({0, 0}), t.cnt[sg] = 1;
    for (int off = 0; off < len[sg]; off += 16) pieces.push_back({start[sg] + off, std::min(16, len[sg] - off)}), ++t.cnt[sg];
    t.maxcnt = std::max(t.maxcnt, t.cnt[sg]);
  }
  const int np = (int)pieces.size();
  std::vector<int> order(np);
  for (int i = 0; i < np; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pieces[a].len > pieces[b].len; });
  t.nslot = (np + 63) / 64;
  if (np > o.dump || t.nslot > o.max_slots) return t;
  t.start.assign((size_t)t.nslot * 64, 0);
  t.id.assign((size_t)t.nslot * 64, o.dump);
  int off = 0;
  for (int r = 0; r < t.nslot; ++r) {
    int gl = 0;
    for (int lane = 0; lane < 64 && r * 64 + lane < np; ++lane) gl = std::max(gl, pieces[order[r * 64 + lane]].len);
    t.glen[r] = gl, t.goff[r] = off;
    t.segw.resize((size_t)(off + gl) * 64, F2{0.f, 0.f});
    for (int lane = 0; lane < 64 && r * 64 + lane < np; ++lane) {
      const Piece pc = pieces[order[r * 64 + lane]];
      t.start[(size_t)r * 64 + lane] = pc.start, t.id[(size_t)r * 64 + lane] = order[r * 64 + lane];
      for (int i = 0; i < pc.len; ++i) t.segw[(size_t)(off + i) * 64 + lane] = F2{wl[pc.start + i], wh[pc.start + i]};
    }
    off += gl;
  }
  t.segw.resize(std::max<size_t>(2, t.segw.size() + (t.segw.size() & 1)), F2{0.f, 0.f});   // even, never empty
  t.ok = true;
  return t;
}

// Band tables: band b at [(b >> 6) * 64 + (b & 63)] holds the piece ranges of its rising and of its falling segment.
// melfeat_v2_kernel: int2 [4][64] (first rising | count << 16, first falling | count << 16); bands that do not exist: the dump slot
inline std::vector<int> pack_bands16(const PieceTable& t, int M, int dump) {
  std::vector<int> tab(2 * 256, dump);
  for (int b = 0; b < M; ++b) tab[2 * b] = t.first[b] | (t.cnt[b] << 16), tab[2 * b + 1] = t.first[b + 1] | (t.cnt[b + 1] << 16);
  return tab;
}
// melfeat_v2_2048_kernel: int [2][64] first rising | count << 8 | first falling << 16 | count << 24
inline std::vector<int> pack_bands8(const PieceTable& t, int M) {
  std::vector<int> tab(128, 0);
  for (int b = 0; b < M; ++b) tab[b] = t.first[b] | (t.cnt[b] << 8) | (t.first[b + 1] << 16) | (t.cnt[b + 1] << 24);
  return tab;
}

}  // namespace stage_a
