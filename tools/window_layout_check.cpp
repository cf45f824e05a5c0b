// Host-only check of the coupled-windows builders (csrc/ldc_windows.h: win_layout_build, win_parts_split, win_ptr_tables), meant to run
// under the host sanitizers on a machine without a GPU -- nothing here touches HIP:
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I ladiffcodec_amd/csrc \
//           tools/window_layout_check.cpp -o tools/bin/window_layout_check && tools/bin/window_layout_check
// For every W = 1..128 (several geometries, the triple-covered tail among them) and every part count it builds what a windows call in
// batch parts would build and checks what its update kernel would rely on: every frame is covered by 1..3 CONSECUTIVE windows whose weights sum to 1,
// the cover entry's first window fits its 8 bits, every (window, row) a tile addresses lies inside the window, the parts partition the
// windows by the floor rule with at most 32 each, and every window's base pointers land inside its own part's buffers, in order and
// without overlap.  Then the refusal edges: max_windows + 1 windows, max_windows outside [1, 128], parts 0 and 5, bad overlaps.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ldc_windows.h"

using namespace ldc;

static int bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_layout(int W, int Lw, int O, int up, int tail) {
  // Ltot that needs exactly W windows: W - 1 full hops and `tail` frames more (0 < tail <= H), or one window
  const int H = Lw - O;
  const int Ltot = W == 1 ? Lw : Lw + (W - 2) * H + tail;
  const int cap = std::max(1, std::min(kMaxWindows, (W + kWinPerPart - 1) / kWinPerPart * kWinPerPart));
  WinLayout lay;
  std::string err;
  const int rc = win_layout_build(Ltot, Lw, O, up, cap, &lay, &err);
  EXPECT(rc == 0, "W %d (Ltot %d, Lw %d, O %d): refused: %s", W, Ltot, Lw, O, err.c_str());
  if (rc) return;
  EXPECT(lay.W == W, "Ltot %d: %d windows, expected %d", Ltot, lay.W, W);
  EXPECT((int)lay.start.size() == W && (int)lay.cover.size() == Ltot && (int)lay.weight.size() == W * lay.Lw, "table sizes at W %d", W);
  EXPECT(lay.start[0] == 0 && lay.start[W - 1] + lay.Lw == Ltot, "W %d: the windows do not span the recording", W);
  for (int g = 0; g < Ltot; ++g) {
    const int first = lay.cover[g] & 255, n = lay.cover[g] >> 8;
    EXPECT(n >= 1 && n <= 3 && first + n <= W, "W %d frame %d: cover %d windows from %d", W, g, n, first);
    double sum = 0.0;
    for (int j = 0; j < n && first + j < W; ++j) {
      const int l = g - lay.start[first + j];
      EXPECT(l >= 0 && l < lay.Lw, "W %d frame %d: row %d of window %d", W, g, l, first + j);
      if (l >= 0 && l < lay.Lw) sum += lay.weight[(size_t)(first + j) * lay.Lw + l];
    }
    EXPECT(std::fabs(sum - 1.0) <= 1.2e-7, "W %d frame %d: weights sum to %.9g", W, g, sum);
    if (n == 1) EXPECT(lay.weight[(size_t)first * lay.Lw + (g - lay.start[first])] == 1.0f, "W %d frame %d: a lone window's weight is not 1.0f", W, g);
    if (first > 0) EXPECT(lay.start[first - 1] + lay.Lw <= g, "W %d frame %d: window %d covers it too", W, g, first - 1);
    if (first + n < W) EXPECT(lay.start[first + n] > g, "W %d frame %d: window %d covers it too", W, g, first + n);
  }
  // the partition and the pointer tables, for every part count that may hold W windows
  const int C = 5, esize = 2;
  for (int P = 1; P <= kWinMaxParts; ++P) {
    if (W > kWinPerPart * P) continue;
    int first[kWinMaxParts + 1];
    const int n = win_parts_split(W, P, first);
    EXPECT(n == std::min(P, W), "W %d P %d: %d parts", W, P, n);
    if (n < 1) continue;
    EXPECT(first[0] == 0 && first[n] == W, "W %d P %d: the ranges do not span the windows", W, P);
    std::vector<std::vector<char>> eps(n), xcl(n);
    const void* eb[kWinMaxParts];
    void* xb[kWinMaxParts];
    for (int p = 0; p < n; ++p) {
      EXPECT(first[p] == (int)((long long)p * W / n) && first[p + 1] > first[p] && first[p + 1] - first[p] <= kWinPerPart, "W %d P %d: part %d is [%d, %d)", W, P,
             p, first[p], first[p + 1]);
      const size_t bytes = (size_t)(first[p + 1] - first[p]) * lay.Lw * C * esize;
      eps[p].assign(bytes, 0);
      xcl[p].assign(bytes, 0);
      eb[p] = eps[p].data();
      xb[p] = xcl[p].data();
    }
    for (int p = n; p <= P; ++p) EXPECT(first[p] == W, "W %d P %d: entry %d behind the parts is %d", W, P, p, first[p]);
    std::vector<const void*> tab;
    EXPECT(win_ptr_tables(W, n, first, eb, xb, lay.Lw, C, esize, &tab) && (int)tab.size() == 2 * W, "W %d P %d: pointer tables", W, P);
    if ((int)tab.size() != 2 * W) continue;
    const size_t wbytes = (size_t)lay.Lw * C * esize;
    for (int p = 0; p < n; ++p)
      for (int k = first[p]; k < first[p + 1]; ++k) {
        const char* e = (const char*)tab[(size_t)k];
        char* x = (char*)tab[(size_t)W + k];
        EXPECT(e == eps[p].data() + (size_t)(k - first[p]) * wbytes && x == xcl[p].data() + (size_t)(k - first[p]) * wbytes, "W %d P %d: window %d points elsewhere",
               W, P, k);
        if (e >= eps[p].data() && e + wbytes <= eps[p].data() + eps[p].size()) (void)e[wbytes - 1];                  // (the sanitizer reads the row's ends)
        if (x >= xcl[p].data() && x + wbytes <= xcl[p].data() + xcl[p].size()) { x[0] += 1; x[wbytes - 1] += 1; }   // one writer per window: ends at 1
      }
    for (int p = 0; p < n; ++p)
      for (int k = first[p]; k < first[p + 1]; ++k) {
        const char* x = xcl[p].data() + (size_t)(k - first[p]) * wbytes;
        EXPECT(x[0] == 1 && x[wbytes - 1] == 1, "W %d P %d: window %d's rows were written %d times", W, P, k, x[0]);
      }
  }
}

static void check_refusals() {
  WinLayout lay;
  std::string err;
  int first[kWinMaxParts + 2];
  for (int cap : {1, 32, 33, 64, 128}) {   // max_windows + 1 windows: refused with both numbers named
    const int Ltot = 80 + cap * 40;
    err.clear();
    EXPECT(win_layout_build(Ltot, 80, 40, 10, cap, &lay, &err) == 1, "cap %d: %d windows were accepted", cap, cap + 1);
    char want[64];
    snprintf(want, sizeof want, "%d windows", cap + 1);
    EXPECT(err.find(want) != std::string::npos && err.find("at most " + std::to_string(cap)) != std::string::npos, "cap %d: '%s'", cap, err.c_str());
    EXPECT(win_layout_build(Ltot - 40, 80, 40, 10, cap, &lay, &err) == 0 && lay.W == cap, "cap %d: %d windows were refused: %s", cap, cap, err.c_str());
  }
  EXPECT(win_layout_build(160, 80, 40, 10, 0, &lay, &err) == 1 && err.find("max_windows 0") != std::string::npos, "max_windows 0: '%s'", err.c_str());
  EXPECT(win_layout_build(160, 80, 40, 10, 129, &lay, &err) == 1 && err.find("max_windows 129") != std::string::npos, "max_windows 129: '%s'", err.c_str());
  EXPECT(win_layout_build(160, 80, 50, 10, 32, &lay, &err) == 1 && err.find("overlap 50") != std::string::npos, "overlap 50: '%s'", err.c_str());
  EXPECT(win_layout_build(160, 80, 45, 10, 32, &lay, &err) == 1, "overlap 45 at up 10 was accepted");
  EXPECT(win_layout_build(165, 80, 40, 10, 32, &lay, &err) == 1 && err.find("Ltot 165") != std::string::npos, "Ltot 165: '%s'", err.c_str());
  EXPECT(win_layout_build(160, 80, 40, 0, 32, &lay, &err) == 1, "up 0 was accepted");
  EXPECT(win_parts_split(4, 0, first) == 0 && win_parts_split(4, 5, first) == 0 && win_parts_split(0, 2, first) == 0, "parts 0 / 5 or W 0 were accepted");
  EXPECT(win_parts_split(3, 4, first) == 3 && first[0] == 0 && first[1] == 1 && first[2] == 2 && first[3] == 3 && first[4] == 3, "(3, 4)");
  EXPECT(win_parts_split(4, 3, first) == 3 && first[1] == 1 && first[2] == 2 && first[3] == 4, "(4, 3)");
  EXPECT(win_parts_split(33, 2, first) == 2 && first[1] == 16 && first[2] == 33, "(33, 2)");
  EXPECT(win_parts_split(128, 4, first) == 4 && first[1] == 32 && first[2] == 64 && first[3] == 96 && first[4] == 128, "(128, 4)");
  std::vector<const void*> tab;
  char some[1] = {0};
  const void* eb[kWinMaxParts] = {some, some, some, some};
  void* xb[kWinMaxParts] = {some, some, some, some};
  const void* nb[kWinMaxParts] = {nullptr, nullptr, nullptr, nullptr};
  const int empty[3] = {0, 2, 2}, shortr[3] = {0, 2, 3}, good[3] = {0, 1, 2};
  EXPECT(!win_ptr_tables(2, 2, empty, eb, xb, 80, 4, 4, &tab), "an empty part was accepted");
  EXPECT(!win_ptr_tables(4, 2, shortr, eb, xb, 80, 4, 4, &tab), "ranges that stop short of W were accepted");
  EXPECT(!win_ptr_tables(2, 2, good, nb, xb, 80, 4, 4, &tab), "a part without a buffer was accepted");
}

int main() {
  for (int W = 1; W <= kMaxWindows; ++W) {
    check_layout(W, 80, 40, 10, 20);    // O = Lw / 2 with a short tail: the right-aligned last window makes the triple-covered stretch
    check_layout(W, 80, 40, 10, 40);    // ... a full last hop: cover <= 2
    check_layout(W, 160, 40, 40, 80);   // the r8 geometry
    check_layout(W, 80, 0, 10, 80);     // no overlap: cover 1 everywhere
  }
  check_refusals();
  printf(bad ? "FAILED (%d)\n" : "all layouts, partitions and pointer tables ok (W = 1..%d)\n", bad ? bad : kMaxWindows);
  return bad ? 1 : 0;
}
