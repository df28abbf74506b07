// Stand-alone driver of csrc/stage_a_tables.h for test_stage_a_tables_cpu.py: builds every stage-A table of one filterbank
// and writes each as a raw file <prefix>.<name>.<f32|i32>.   usage: prog fb.f32 n_fft n_mels prefix
#include <cstdio>
#include <cstdlib>
#include <string>

#include "stage_a_tables.h"

static std::string g_pre;
template <typename T>
static void dump(const char* name, const T* d, size_t n) {
  FILE* f = fopen((g_pre + name).c_str(), "wb");
  if (!f || fwrite(d, sizeof(T), n, f) != n) exit(5);
  fclose(f);
}
template <typename T>
static void dump(const char* name, const std::vector<T>& v) { dump(name, v.data(), v.size()); }

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int n_fft = atoi(argv[2]), M = atoi(argv[3]), n_bins = n_fft / 2 + 1;
  g_pre = argv[4];
  std::vector<float> fb((size_t)n_bins * M);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(fb.data(), sizeof(float), fb.size(), f) != fb.size()) return 3;
  fclose(f);
  using namespace stage_a;
  const LaneBandTable g = build_lane_bands(fb.data(), n_bins, M, M <= 128 ? 2 : 4);
  const std::vector<F2> tw = fft_twiddles(n_fft / 2), tw2 = n_fft <= 1024 ? fft_twiddles(n_fft) : std::vector<F2>();
  dump(".lanebands.i32", g.lanebands), dump(".melw.f32", g.melw), dump(".tw.f32", tw), dump(".tw2.f32", tw2);
  dump(".post.f32", post_twiddles(n_fft));
  const int gsc[3] = {g.nnz, (int)tw.size(), (int)tw2.size()};
  dump(".gen_scalars.i32", gsc, 3), dump(".gen_glen.i32", g.glen, 4), dump(".gen_goff.i32", g.goff, 4);
  const bool v4 = n_fft == 2048;
  const PieceTable t = build_pieces(fb.data(), n_bins, M, v4 ? v4_piece_opts() : v2_piece_opts(M));
  if (!t.ok) return 4;
  dump(".segw.f32", t.segw), dump(".start.i32", t.start), dump(".id.i32", t.id), dump(".first.i32", t.first), dump(".cnt.i32", t.cnt);
  if (v4) dump(".bandtab.i32", pack_bands8(t, M)), dump(".tw4.f32", tw4_twiddles());
  else dump(".bandtab.i32", pack_bands16(t, M, kV2Dump));
  const int sc[3] = {t.nslot, (int)t.segw.size(), t.maxcnt};
  dump(".scalars.i32", sc, 3), dump(".glen.i32", t.glen, kMaxSlots), dump(".goff.i32", t.goff, kMaxSlots);
  return 0;
}
