// Host-only check of the lean conv kernel's tile tables (csrc/conv_lean.inc: lean_build_tiles), meant to run under the host sanitizers on a
// machine without a GPU -- no kernel is launched:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined -I ladiffcodec_amd/csrc tools/lean_tables_check.hip -o tools/bin/lean_tables_check && tools/bin/lean_tables_check
// (the second, plain -fsanitize is for the link; hipcc says that it ignores it for the device code, which is what is wanted: host code only)
// For every shape of tests/test_gpu_lean_kinds.py (and the bench grid's k = 4 / k = 7 launches) it builds the table as launch_fast_cfg +
// launch_lean would and checks what the kernel relies on: every (tile, split-K slice) appears exactly once, the slices of a tile partition
// the units in order, every window lies inside the input and fits the kind's LDS plane.
#define LDC_FAST_T __bf16
#define LDC_FAST_NS fast_check
#define LDC_FAST_ENTRY launch_conv_fast_check
#define LDC_FAST_RESIDENCY conv_wgs_per_cu_check
#include "conv_fast.inc"

#include <cstdio>
#include <set>

namespace ldc {
unsigned long long* g_conv_stamps = nullptr;
long long g_lean_launches[8] = {0, 0, 0, 0, 0, 0, 0, 0};
}  // namespace ldc

using namespace ldc;
using namespace ldc::fast_check;

struct Shape { int B, L_in, cin, cout, k, stride, ups, tm, ksplit; };

static int check(const Shape& sh) {
  const int bke = 32, BM = sh.tm * 64, BN = 64;
  ConvKArgs a;
  memset(&a, 0, sizeof(a));
  const int pad = (sh.k == 4 && sh.stride == 2) ? 1 : (sh.k - 1) / 2;
  const int L_out = sh.ups ? 2 * sh.L_in : (sh.stride == 2 ? (sh.L_in + 2 * pad - sh.k) / 2 + 1 : sh.L_in);
  a.C1 = sh.cin; a.n = sh.cout; a.n_pad = (sh.cout + BN - 1) / BN * BN;
  a.B = sh.B; a.L_in = sh.L_in; a.L_rows = L_out; a.taps = sh.k; a.wtaps = sh.k; a.stride = sh.stride; a.dil = 1; a.pad_left = pad; a.ups = sh.ups;
  a.ksplit = sh.ksplit;
  const int M = sh.B * L_out;
  FastGeom gm;
  memset(&gm, 0, sizeof(gm));
  gm.ngroups = sh.k == 7 ? 2 : 1;
  gm.ntn = a.n_pad / BN; gm.ntm = (M + BM - 1) / BM; gm.ntiles = gm.ntn * gm.ntm; gm.grid = gm.ntiles * a.ksplit;
  const int nl = a.ksplit == 4 ? 2 : (a.ksplit == 2 ? 4 : 0);
  gm.sk_xcd = (nl && gm.ntn % nl == 0) ? 1 : 0;
  const int upc = sh.k == 7 ? 2 : 1;
  std::vector<LeanTile> h;
  const int mx = lean_build_tiles(a, gm, BM, BN, 1, M, bke, upc, h);
  const int plane = sh.k == 4 ? (sh.tm == 2 ? LeanShape<2, LEAN_K4S2, false>::PLANE_ROWS : LeanShape<1, LEAN_K4S2, false>::PLANE_ROWS)
                              : (sh.tm == 2 ? LeanShape<2, LEAN_K3, false>::PLANE_ROWS : LeanShape<1, LEAN_K3, false>::PLANE_ROWS);
  const int nunits = sh.cin / bke * upc;
  int bad = 0;
  std::set<std::pair<int, int>> seen;
  std::vector<int> covered((size_t)gm.ntiles, 0);
  if ((int)h.size() != gm.grid) ++bad;
  for (const LeanTile& t : h) {
    if (t.m0 < 0 || t.m0 >= M || t.m0 % BM || t.n0 < 0 || t.n0 >= a.n_pad || t.n0 % BN) { ++bad; continue; }
    if (t.sk_tile < 0 || t.sk_tile >= gm.ntiles || t.sk_k < 0 || t.sk_k >= a.ksplit) { ++bad; continue; }
    if (!seen.insert({(t.m0 / BM) * gm.ntn + t.n0 / BN, t.sk_k}).second) ++bad;
    if (t.R_lo < 0 || t.nrows < 1 || t.R_lo + t.nrows > a.B * a.L_in || t.nrows > plane) ++bad;
    if (t.u_begin < 0 || t.u_begin >= t.u_end || t.u_end > nunits) ++bad;
    if (t.sk_k == 0 && t.u_begin != 0) ++bad;
    if (t.sk_k == a.ksplit - 1 && t.u_end != nunits) ++bad;
    covered[(size_t)t.sk_tile] += t.u_end - t.u_begin;
  }
  for (int c : covered) if (c != nunits) ++bad;
  if ((int)seen.size() != gm.grid) ++bad;
  printf("B %d L %d -> %d, %d -> %d, k %d s %d u %d, %d-row tiles, split %d: %d workgroups, largest window %d of %d rows: %s\n", sh.B, sh.L_in, L_out, sh.cin,
         sh.cout, sh.k, sh.stride, sh.ups, BM, sh.ksplit, gm.grid, mx, plane, bad ? "BAD" : "ok");
  return bad;
}

int main() {
  const Shape shapes[] = {
      {3, 75, 64, 64, 3, 1, 1, 2, 1},     {2, 40, 96, 64, 3, 1, 1, 2, 1},    {2, 40, 96, 128, 3, 1, 1, 1, 1},  {3, 150, 64, 128, 4, 2, 0, 1, 1},
      {3, 150, 64, 128, 4, 2, 0, 2, 1},   {1, 64, 96, 64, 4, 2, 0, 2, 1},    {2, 600, 64, 64, 4, 2, 0, 2, 1},  {2, 200, 128, 64, 7, 1, 0, 2, 1},
      {3, 75, 32, 64, 7, 1, 0, 2, 1},     {3, 75, 96, 128, 7, 1, 0, 1, 1},   {3, 75, 96, 128, 7, 1, 0, 2, 1},  {1, 150, 1024, 1024, 4, 2, 0, 1, 2},
      {1, 37, 1024, 1024, 3, 1, 1, 1, 2}, {1, 75, 1024, 128, 7, 1, 0, 1, 1},
      // the bench grid (one part of 16 items)
      {16, 1200, 256, 256, 4, 2, 0, 2, 1}, {16, 600, 256, 512, 4, 2, 0, 2, 1}, {16, 300, 512, 512, 4, 2, 0, 1, 1}, {16, 150, 512, 1024, 4, 2, 0, 1, 2},
      {16, 1200, 128, 256, 7, 1, 0, 2, 1},
  };
  int bad = 0;
  for (const Shape& s : shapes) bad += check(s);
  printf(bad ? "FAILED\n" : "all tables ok\n");
  return bad ? 1 : 0;
}
