// Host-only check of the window-group builder (csrc/ldc_windows.h: win_group_build), meant to run under the host sanitizers on a machine
// without a GPU -- nothing here touches HIP:
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I ladiffcodec_amd/csrc \
//           tools/window_group_check.cpp -o tools/bin/window_group_check && tools/bin/window_group_check
// For R = 1..32 recordings of mixed lengths (one-window recordings, lengths that are no multiple of the 32-frame tile, triple-covered
// tails, the 32-window cap) it builds the group and checks what the group kernels rely on: every recording's rows of the concatenated
// tables are win_layout_build's for it alone, bit for bit; w0 / off are the prefix sums; the tile table gives recording r exactly
// ceil(Ltot_r / 32) tiles in order and no tile spans two recordings; then it WALKS the tile table as the update kernel does -- tile
// entry -> recording entry -> cover -> start, weight -- on exact-size buffers: every (window, row) a tile addresses lies inside a window of
// the tile's own recording, every element of the packed state and every row of every window has exactly one writer, frames behind a
// recording's end are stored nowhere; and the gather's source of every window row lies inside its recording's block.  Then the refusal
// edges: R 0 and 33, 33 windows in all, a recording shorter than the window, and win_layout_build's own refusals with the recording named.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ldc_windows.h"

using namespace ldc;

static int bad = 0, groups = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_group(const std::vector<int>& Ltot, int Lw, int O, int up) {
  const int R = (int)Ltot.size();
  WinGroup g;
  std::string err;
  const int rc = win_group_build(R, Ltot.data(), Lw, O, up, &g, &err);
  EXPECT(rc == 0, "R %d (Lw %d, O %d): refused: %s", R, Lw, O, err.c_str());
  if (rc) return;
  ++groups;
  EXPECT(g.R == R && g.Lw == Lw && g.O == O && (int)g.w0.size() == R + 1 && (int)g.off.size() == R + 1 && (int)g.rec.size() == R, "R %d: sizes", R);
  int wsum = 0, lsum = 0;
  size_t ntile = 0;
  for (int r = 0; r < R; ++r) {
    WinLayout lay;
    EXPECT(win_layout_build(Ltot[r], Lw, O, up, kWinPerPart, &lay, &err) == 0, "recording %d alone: %s", r, err.c_str());
    EXPECT(g.w0[r] == wsum && g.off[r] == lsum, "recording %d: w0 %d (want %d), off %d (want %d)", r, g.w0[r], wsum, g.off[r], lsum);
    const WinGroupRec& e = g.rec[r];
    EXPECT(e.Ltot == Ltot[r] && e.w0 == wsum && e.off == lsum && e.cover_off == lsum && e.W == lay.W && e.key_lo == 0 && e.key_hi == 0, "recording %d: table entry", r);
    EXPECT(wsum + lay.W <= (int)g.start.size() && lsum + Ltot[r] <= (int)g.cover.size(), "recording %d: its rows lie outside the tables", r);
    if (wsum + lay.W > (int)g.start.size() || lsum + Ltot[r] > (int)g.cover.size()) return;
    EXPECT(!memcmp(&g.start[wsum], lay.start.data(), lay.W * sizeof(int)), "recording %d: starts differ from its own layout", r);
    EXPECT(!memcmp(&g.cover[lsum], lay.cover.data(), Ltot[r] * sizeof(int)), "recording %d: cover differs from its own layout", r);
    EXPECT(!memcmp(&g.weight[(size_t)wsum * Lw], lay.weight.data(), (size_t)lay.W * Lw * sizeof(float)), "recording %d: weights differ from its own layout", r);
    for (int k = 0; k < lay.W; ++k) EXPECT(g.wrec[wsum + k] == r, "window %d belongs to recording %d, not %d", wsum + k, r, g.wrec[wsum + k]);
    for (int l0 = 0; l0 < Ltot[r]; l0 += kWinGroupTile, ++ntile) {
      EXPECT(ntile < g.tile.size() && g.tile[ntile].rec == r && g.tile[ntile].l0 == l0, "tile %zu: not {recording %d, l0 %d}", ntile, r, l0);
      if (ntile >= g.tile.size()) return;
    }
    wsum += lay.W;
    lsum += Ltot[r];
  }
  EXPECT(g.w0[R] == wsum && g.off[R] == lsum && g.W_sum == wsum && g.Lsum == lsum && wsum <= kWinPerPart, "R %d: totals (%d windows, %d frames)", R, wsum, lsum);
  EXPECT(ntile == g.tile.size(), "R %d: %zu tiles, expected %zu", R, g.tile.size(), ntile);
  EXPECT((int)g.start.size() == wsum && (int)g.wrec.size() == wsum && (int)g.cover.size() == lsum && g.weight.size() == (size_t)wsum * Lw, "R %d: table sizes", R);
  // the update kernel's walk, on exact-size buffers (one channel block: C = 3 of a 32-channel tile)
  const int C = 3;
  std::vector<unsigned char> x((size_t)C * lsum, 0), xcl((size_t)wsum * Lw * C, 0);
  for (size_t b = 0; b < g.tile.size(); ++b) {
    const WinGroupTile te = g.tile[b];
    const WinGroupRec rc2 = g.rec[(size_t)te.rec];
    const int* cover = g.cover.data() + rc2.cover_off;
    const size_t xo = (size_t)C * rc2.off;
    for (int i = 0; i < kWinGroupTile; ++i) {
      const int gf = te.l0 + i;
      const int cov = gf < rc2.Ltot ? cover[gf] : 0;
      const int first = rc2.w0 + (cov & 255), n = cov >> 8;
      EXPECT(gf < rc2.Ltot ? (n >= 1 && n <= 3) : n == 0, "tile %zu frame %d of recording %d: count %d", b, gf, te.rec, n);
      double sum = 0.0;
      for (int j = 0; j < n; ++j) {
        const int k = first + j;
        EXPECT(k >= rc2.w0 && k < rc2.w0 + rc2.W, "tile %zu frame %d: window %d is not one of recording %d", b, gf, k, te.rec);
        if (k < 0 || k >= wsum) continue;
        const int l = gf - g.start[(size_t)k];
        EXPECT(l >= 0 && l < Lw, "tile %zu frame %d: row %d of window %d", b, gf, l, k);
        if (l < 0 || l >= Lw) continue;
        sum += g.weight[(size_t)k * Lw + l];
        for (int c = 0; c < C; ++c) xcl[((size_t)k * Lw + l) * C + c] += 1;
      }
      if (gf < rc2.Ltot) {
        EXPECT(std::fabs(sum - 1.0) <= 1.2e-7, "tile %zu frame %d: weights sum to %.9g", b, gf, sum);
        for (int c = 0; c < C; ++c) x[xo + (size_t)c * rc2.Ltot + gf] += 1;
      }
    }
  }
  size_t wrong = 0;
  for (unsigned char v : x) wrong += v != 1;
  EXPECT(wrong == 0, "R %d: %zu elements of the packed state do not have exactly one writer", R, wrong);
  wrong = 0;
  for (unsigned char v : xcl) wrong += v != 1;
  EXPECT(wrong == 0, "R %d: %zu elements of the windows' rows do not have exactly one writer", R, wrong);
  // the gather's walk (div = 1 for the state, up for the raw condition)
  for (int div : {1, up}) {
    const int Cg = 2;
    std::vector<unsigned char> src((size_t)Cg * (lsum / div), 0);
    for (int k = 0; k < wsum; ++k) {
      const WinGroupRec rc2 = g.rec[(size_t)g.wrec[(size_t)k]];
      EXPECT(rc2.off % div == 0 && rc2.Ltot % div == 0 && g.start[(size_t)k] % div == 0 && Lw % div == 0, "window %d: not on the condition's frames", k);
      const int Lr = rc2.Ltot / div, s0 = g.start[(size_t)k] / div;
      const size_t xo = (size_t)Cg * (rc2.off / div);
      EXPECT(s0 + Lw / div <= Lr, "window %d: ends at %d of %d", k, s0 + Lw / div, Lr);
      for (int c = 0; c < Cg; ++c)
        for (int l = 0; l < Lw / div; ++l)
          if (s0 + l < Lr) src[xo + (size_t)c * Lr + s0 + l] |= 1;   // (the sanitizer sees the address)
    }
    wrong = 0;
    for (unsigned char v : src) wrong += v != 1;
    EXPECT(wrong == 0, "R %d div %d: %zu source elements are read by no window", R, div, wrong);
  }
}

static void refused(const std::vector<int>& Ltot, int R, int Lw, int O, int up, const char* word) {
  WinGroup g;
  std::string err;
  const int rc = win_group_build(R, Ltot.empty() ? nullptr : Ltot.data(), Lw, O, up, &g, &err);
  EXPECT(rc == 1 && err.find(word) != std::string::npos, "expected a refusal naming '%s', got rc %d '%s'", word, rc, err.c_str());
}

int main() {
  // Ltot that needs exactly W windows at (Lw, O) with a tail of `tail` frames on the last hop
  auto len = [](int W, int Lw, int O, int tail) { return W == 1 ? Lw : Lw + (W - 2) * (Lw - O) + tail; };
  for (int R = 1; R <= kWinPerPart; ++R) {
    check_group(std::vector<int>((size_t)R, 80), 80, 40, 10);            // R one-window recordings: an ordinary batch
    check_group(std::vector<int>((size_t)R, 160), 160, 40, 40);
    {   // mixed: the 32 windows dealt out over R recordings, short tails (triple cover, lengths off the 32-frame tile) and full ones
      std::vector<int> L;
      int left = kWinPerPart;
      for (int r = 0; r < R; ++r) {
        const int W = r + 1 == R ? left : std::max(1, std::min(left - (R - 1 - r), 1 + (r * 7 + R) % 5));
        L.push_back(len(W, 80, 40, r % 2 ? 20 : 40));
        left -= W;
      }
      check_group(L, 80, 40, 10);
      std::vector<int> L0;
      for (int r = 0; r < R; ++r) L0.push_back(80 * (1 + (r == 0 ? kWinPerPart - R : 0)));   // no overlap, the cap again
      check_group(L0, 80, 0, 10);
    }
  }
  check_group({180, 80, 240}, 80, 40, 10);                                // the GPU tests' groups
  check_group({400, 160}, 160, 40, 40);
  check_group(std::vector<int>(8, 180), 80, 40, 10);                      // 8 x 4 windows: the cap
  check_group({len(32, 80, 40, 20)}, 80, 40, 10);                         // one recording of 32 windows
  // refusals
  refused({}, 0, 80, 40, 10, "R 0");
  refused(std::vector<int>(33, 80), 33, 80, 40, 10, "R 33");
  refused({}, 2, 80, 40, 10, "null");
  refused(std::vector<int>(9, 180), 9, 80, 40, 10, "36 windows");         // a ninth recording: the sum is named
  refused({180, 80, 240, len(23, 80, 40, 40)}, 4, 80, 40, 10, "33 windows");
  refused({180, 70, 240}, 3, 80, 40, 10, "recording 1: Ltot 70");         // shorter than the window: index and value
  refused({180, 185}, 2, 80, 40, 10, "recording 1: Ltot 185");            // no multiple of up
  refused({180, 80}, 2, 80, 50, 10, "overlap 50");
  refused({180, 80}, 2, 80, 45, 10, "overlap 45");
  refused({180, 80}, 2, 85, 40, 10, "Lw 85");
  refused({180, 80}, 2, 80, 40, 0, "up 0");
  refused({80, len(33, 80, 40, 40)}, 2, 80, 40, 10, "recording 1");       // one recording alone beyond the cap
  // `single`, the group of a single-recording call: the same tables as the plain group of one; a recording shorter than the window is its
  // one window (the plain group at Lw = Ltot); refusals in win_layout_build's own words, on the caller's Lw
  for (int Ltot : {180, 80, 70}) {
    WinGroup a, b;
    std::string err;
    const int one[1] = {Ltot}, lw = std::min(80, Ltot);
    EXPECT(win_group_build(1, one, 80, 40, 10, &a, &err, true) == 0 && win_group_build(1, one, lw, 40 <= lw / 2 ? 40 : 0, 10, &b, &err) == 0,
           "single Ltot %d: refused: %s", Ltot, err.c_str());
    EXPECT(a.Lw == lw && a.W_sum == b.W_sum && a.Lsum == b.Lsum && a.w0 == b.w0 && a.off == b.off && a.start == b.start && a.cover == b.cover &&
               a.wrec == b.wrec && a.weight == b.weight && a.tile.size() == b.tile.size() && a.rec[0].Ltot == Ltot && a.rec[0].W == b.rec[0].W,
           "single Ltot %d: not the plain group of one", Ltot);
  }
  {
    WinGroup g;
    std::string err;
    const int one[1] = {180}, two[2] = {180, 80};
    EXPECT(win_group_build(1, one, 200, 110, 10, &g, &err, true) == 1 && err.rfind("overlap 110", 0) == 0 && err.find("Lw / 2 = 100") != std::string::npos,
           "single: expected the overlap refusal on the caller's Lw, got '%s'", err.c_str());
    EXPECT(win_group_build(2, two, 80, 40, 10, &g, &err, true) == 2, "single with R = 2 is an internal error, got '%s'", err.c_str());
  }
  printf(bad ? "FAILED (%d)\n" : "%d window groups ok (R = 1..%d, the cap, the refusals)\n", bad ? bad : groups, kWinPerPart);
  return bad ? 1 : 0;
}
