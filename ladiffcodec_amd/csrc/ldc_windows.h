// Coupled windows: the host-only builders of a windows call -- the layout with its cover and weight tables, the
// partition of the windows into batch parts, the per-window base-pointer tables of a call in parts, and the tables of a window group
// (several recordings whose windows share one batch).  Pure functions of their arguments (no context, no HIP, no globals): ldc_api.cpp
// wraps them, tools/window_layout_check.cpp and tools/window_group_check.cpp run them under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace ldc {

static constexpr int kWinPerPart = 32;    // windows one batch part holds at most (the cap of a one-part call)
static constexpr int kWinMaxParts = 4;    // == kMaxParts (ldc_internal.h asserts it)
static constexpr int kMaxWindows = kWinPerPart * kWinMaxParts;   // the cover entry keeps the first window in 8 bits

struct WinLayout {
  int Ltot = 0, Lw = 0, O = 0, W = 0;
  std::vector<int> start, cover;   // cover[g] = first covering window | count << 8
  std::vector<float> weight;       // [W][Lw]
};

// The layout, the cover table and the weights (double, rounded once to float) of (Ltot, Lw, overlap) for at most max_windows windows.
// 0: ok; 1: refused (an argument; *err names its value); 2: internal.  max_windows must lie in [1, kMaxWindows].
inline int win_layout_build(int Ltot, int Lw, int O, int up, int max_windows, WinLayout* out, std::string* err) {
  char msg[256];
  auto refuse = [&](int code) { *err = msg; return code; };
  if (max_windows < 1 || max_windows > kMaxWindows) {
    snprintf(msg, sizeof msg, "max_windows %d: must be in [1, %d]", max_windows, kMaxWindows);
    return refuse(1);
  }
  if (up < 1) { snprintf(msg, sizeof msg, "up %d: the latent frames per condition frame must be >= 1", up); return refuse(1); }
  if (Ltot <= 0 || Ltot % up) { snprintf(msg, sizeof msg, "Ltot %d: must be a positive multiple of up = %d", Ltot, up); return refuse(1); }
  if (Lw <= 0 || Lw % up) { snprintf(msg, sizeof msg, "Lw %d: must be a positive multiple of up = %d", Lw, up); return refuse(1); }
  if (O < 0 || O % up || O > Lw / 2) {
    snprintf(msg, sizeof msg, "overlap %d: must be a multiple of up = %d in [0, Lw / 2 = %d]", O, up, Lw / 2);
    return refuse(1);
  }
  if (Ltot <= Lw) Lw = Ltot;   // one window: the recording itself
  const int H = Lw - O;
  const long long W = Ltot <= Lw ? 1 : 1 + ((long long)(Ltot - Lw) + H - 1) / H;
  if (W > max_windows) {
    snprintf(msg, sizeof msg, "Ltot %d needs %lld windows of %d frames at overlap %d: at most %d per call", Ltot, W, Lw, O, max_windows);
    return refuse(1);
  }
  out->Ltot = Ltot; out->Lw = Lw; out->O = O; out->W = (int)W;
  out->start.assign((size_t)W, 0);
  for (int k = 0; k < W; ++k) out->start[k] = (int)std::min<long long>((long long)k * H, Ltot - Lw);   // the last window is right-aligned
  std::vector<double> u((size_t)W * Lw);
  for (int k = 0; k < W; ++k) {
    const int Rl = k > 0 ? out->start[k - 1] + Lw - out->start[k] : 0, Rr = k + 1 < W ? out->start[k] + Lw - out->start[k + 1] : 0;
    for (int l = 0; l < Lw; ++l) {
      double v = 1.0;
      if (Rl > 0) v = std::min(v, (l + 0.5) / Rl);
      if (Rr > 0) v = std::min(v, (Lw - l - 0.5) / Rr);
      u[(size_t)k * Lw + l] = v;
    }
  }
  out->cover.assign((size_t)Ltot, 0);
  out->weight.assign((size_t)W * Lw, 0.f);
  int first = 0;
  for (int g = 0; g < Ltot; ++g) {
    while (out->start[first] + Lw <= g) ++first;   // (starts ascend, so the covering windows are consecutive from here)
    int n = 0;
    double sum = 0.0;
    while (first + n < W && out->start[first + n] <= g) { sum += u[(size_t)(first + n) * Lw + (g - out->start[first + n])]; ++n; }
    if (n < 1 || n > 3) { snprintf(msg, sizeof msg, "internal: frame %d is covered by %d windows", g, n); return refuse(2); }
    out->cover[g] = first | (n << 8);
    for (int j = 0; j < n; ++j) {
      const size_t i = (size_t)(first + j) * Lw + (g - out->start[first + j]);
      out->weight[i] = (float)(u[i] / sum);
    }
  }
  return 0;
}

// The batch parts of W windows at `parts` requested parts: P_eff = min(parts, W) contiguous ranges, part p holds the windows
// [floor(p W / P_eff), floor((p + 1) W / P_eff)); first_out[0 .. P_eff] are the range starts (first_out[P_eff] = W), entries behind
// them up to first_out[parts] are W (empty parts).  Returns P_eff, or 0 when W < 1 or parts lies outside [1, kWinMaxParts].
inline int win_parts_split(int W, int parts, int* first_out) {
  if (W < 1 || parts < 1 || parts > kWinMaxParts) return 0;
  const int P = std::min(parts, W);
  for (int p = 0; p <= parts; ++p) first_out[p] = p < P ? (int)((long long)p * W / P) : W;
  return P;
}

// The base pointers of the W windows' [Lw][C] rows, for an update kernel that finds a window through a table: window k of part p lives at that part's buffer + (k - first[p]) * Lw * C
// elements of esize bytes.  eps_base / xcl_base: the P parts' eps_cl / x_cl; first: win_parts_split's P + 1 range starts.
// out: [2 W] -- the eps pointers, then the input pointers.  false when a range is empty, descends or does not end at W.
inline bool win_ptr_tables(int W, int P, const int* first, const void* const* eps_base, void* const* xcl_base, int Lw, int C, size_t esize,
                           std::vector<const void*>* out) {
  if (W < 1 || P < 1 || P > kWinMaxParts || first[0] != 0 || first[P] != W) return false;
  for (int p = 0; p < P; ++p)
    if (first[p + 1] <= first[p] || first[p + 1] > W || !eps_base[p] || !xcl_base[p]) return false;
  out->assign((size_t)2 * W, nullptr);
  for (int p = 0; p < P; ++p) {
    for (int k = first[p]; k < first[p + 1]; ++k) {
      const size_t off = (size_t)(k - first[p]) * Lw * C * esize;
      (*out)[(size_t)k] = (const char*)eps_base[p] + off;
      (*out)[(size_t)W + k] = (const char*)xcl_base[p] + off;
    }
  }
  return true;
}

// ---- window groups ("Several recordings per call"): R recordings, the windows of all of them in ONE batch ----------
// Recording r keeps its own layout win_layout_build(Ltot_r, Lw, O, up); its windows take the batch indices w0[r] .. w0[r] + W_r - 1 in
// recording order, its [C][Ltot_r] blocks of the packed tensors begin at C * off[r] floats (off[r] = the frames of the recordings in
// front), its cover rows at off[r] of the concatenated table.  The update kernels walk a tile table: one entry per workgroup column,
// recording r owns ceil(Ltot_r / 32) tiles, so no tile spans two recordings.
struct WinGroupRec {    // one recording, as the kernels read it (device memory; 32 bytes)
  int Ltot;             // its latent frames
  int w0;               // batch index of its first window
  int off;              // frames in front of it on the packed axis: its state block begins at C * off floats
  int cover_off;        // its rows of the concatenated cover table begin here
  unsigned key_lo, key_hi;   // its Philox key (written on the stream in front of every loop, launch_windows_group_keys)
  int W, pad;
};
struct WinGroupTile { int rec, l0; };   // a workgroup column: 32 frames of recording rec from l0 (in the recording's own frames)

static constexpr int kWinGroupTile = 32;

struct WinGroup {
  int R = 0, Lw = 0, O = 0, W_sum = 0, Lsum = 0;
  std::vector<int> Ltot, w0, off;        // [R], [R + 1], [R + 1]
  std::vector<int> start, cover, wrec;   // [W_sum] in the recording's own frames; [Lsum] first window WITHIN the recording | count << 8; [W_sum] window -> recording
  std::vector<float> weight;             // [W_sum][Lw]
  std::vector<WinGroupRec> rec;          // [R] (keys zero)
  std::vector<WinGroupTile> tile;        // [sum ceil(Ltot_r / 32)]
};

// The group of R recordings of Ltot[r] frames at (Lw, overlap).  0: ok; 1: refused (*err names the value, and the recording where it is
// one's own); 2: internal.  Every recording must be at least one window long: a shorter one would shrink the window (win_layout_build's
// Ltot <= Lw case) and break the equal-length batch.
// single (R == 1 only): the group of a single-recording call -- win_layout_build's refusals in its own words (no "recording 0:"), and a
// recording shorter than Lw is its one window: out->Lw is then Ltot[0], the layout's effective window.
inline int win_group_build(int R, const int* Ltot, int Lw, int O, int up, WinGroup* out, std::string* err, bool single = false) {
  char msg[320];
  auto refuse = [&](int code) { *err = msg; return code; };
  if (R < 1 || R > kWinPerPart) { snprintf(msg, sizeof msg, "R %d: a window group holds 1 to %d recordings", R, kWinPerPart); return refuse(1); }
  if (!Ltot) { snprintf(msg, sizeof msg, "null list of lengths"); return refuse(1); }
  if (single && R != 1) { snprintf(msg, sizeof msg, "internal: a single-recording group of %d recordings", R); return refuse(2); }
  *out = WinGroup();
  out->R = R; out->Lw = Lw; out->O = O;
  out->Ltot.assign(Ltot, Ltot + R);
  out->w0.assign((size_t)R + 1, 0);
  out->off.assign((size_t)R + 1, 0);
  std::vector<WinLayout> lay((size_t)R);
  long long wsum = 0, lsum = 0;
  for (int r = 0; r < R; ++r) {
    std::string e1;
    const int rc = win_layout_build(Ltot[r], Lw, O, up, kWinPerPart, &lay[r], &e1);
    if (rc && single) { *err = e1; return rc; }
    if (rc) { snprintf(msg, sizeof msg, "recording %d: %s", r, e1.c_str()); return refuse(rc); }
    if (single) Lw = out->Lw = lay[r].Lw;
    if (Ltot[r] < Lw) {
      snprintf(msg, sizeof msg, "recording %d: Ltot %d is shorter than the window Lw = %d (every recording of a group is at least one window long)", r,
               Ltot[r], Lw);
      return refuse(1);
    }
    wsum += lay[r].W;
    lsum += Ltot[r];
    out->w0[r + 1] = (int)wsum;
    out->off[r + 1] = (int)lsum;   // (<= 32 recordings of <= 32 windows of Lw frames: far from 2^31 for every Lw the UNet takes; checked below)
  }
  if (wsum > kWinPerPart) {
    snprintf(msg, sizeof msg, "the %d recordings need %lld windows of %d frames at overlap %d in all: at most %d per call", R, wsum, Lw, O, kWinPerPart);
    return refuse(1);
  }
  if (lsum > 0x3fffffff) { snprintf(msg, sizeof msg, "the recordings hold %lld frames in all: too many for one call", lsum); return refuse(1); }
  out->W_sum = (int)wsum; out->Lsum = (int)lsum;
  out->start.reserve((size_t)wsum); out->wrec.reserve((size_t)wsum);
  out->cover.reserve((size_t)lsum); out->weight.reserve((size_t)wsum * Lw);
  out->rec.assign((size_t)R, WinGroupRec());
  for (int r = 0; r < R; ++r) {
    const WinLayout& l = lay[r];
    if (l.Lw != Lw) { snprintf(msg, sizeof msg, "internal: recording %d got windows of %d frames", r, l.Lw); return refuse(2); }
    out->start.insert(out->start.end(), l.start.begin(), l.start.end());
    out->cover.insert(out->cover.end(), l.cover.begin(), l.cover.end());
    out->weight.insert(out->weight.end(), l.weight.begin(), l.weight.end());
    out->wrec.insert(out->wrec.end(), (size_t)l.W, r);
    WinGroupRec& g = out->rec[r];
    g.Ltot = Ltot[r]; g.w0 = out->w0[r]; g.off = out->off[r]; g.cover_off = out->off[r]; g.W = l.W;
    for (int l0 = 0; l0 < Ltot[r]; l0 += kWinGroupTile) out->tile.push_back(WinGroupTile{r, l0});
  }
  return 0;
}

}  // namespace ldc
