// plan_passes.h -- the two things every UNet plan is built by, whether it is cached (unet_plan.cpp: get_plan) or private to a test hook
// (ldc_api_debug.cpp): the planning protocol that sizes, measures, allocates and builds a plan, and the layout of the region a step's
// first kernel clears.  Host-only and free of HIP (no context, no globals): tools/plan_passes_check.cpp runs both under the host
// sanitizers.  The protocol reports its one refusal through fail(), which the library defines in ldc_api.cpp and the check itself.
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/ladiffcodec.h"

int fail(int code, const char* fmt, ...);

struct Arena {   // bump allocator over one device buffer; base == nullptr measures only
  char* base = nullptr;
  size_t cap = 0, off = 0;
  void* alloc(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};

// The planning protocol.  build(arena) lays the plan out on an arena and returns an LDC_* code; it reads the plan's sk_floats (split-K
// workspace) and part_bytes (granule pool of the fused GroupNorm applies) and leaves what its convs asked for in sk_need_max / part_need.
// Two sizing passes on dry arenas carry those needs into the sizes (the second because convs fuse their GroupNorm apply only once the
// granule pool exists and then ask for more of it, and the split-K decisions feed back into what is folded), a measuring pass takes the
// plan's bytes, alloc(bytes, &base) provides them and the last pass builds the plan for real.  A plan that outgrows its measure is
// refused (a planner bug: a pass that plans other launch forms than the one before it).  Any failure ends the sequence; release(base)
// gives back what alloc handed out.  measure_only stops behind the measuring pass: the routes are planned, nothing is allocated.
template <class P, class Build, class Alloc, class Release>
int plan_passes(P* pl, bool measure_only, Build build, Alloc alloc, Release release, void** base_out = nullptr, size_t* bytes_out = nullptr) {
  for (int pass = 0; pass < 2; ++pass) {
    Arena dry;
    const int rc = build(dry);
    if (rc != LDC_OK) return rc;
    pl->sk_floats = std::max(pl->sk_floats, pl->sk_need_max);
    pl->part_bytes = std::max(pl->part_bytes, pl->part_need);
  }
  Arena measure;
  int rc = build(measure);
  if (rc != LDC_OK || measure_only) return rc;
  const size_t want = measure.off + 4096;
  void* base = nullptr;
  rc = alloc(want, &base);
  if (rc != LDC_OK) return rc;
  Arena real;
  real.base = (char*)base;
  real.cap = want;
  rc = build(real);
  if (rc == LDC_OK && real.off > want) rc = fail(LDC_E_STATE, "internal: the plan needs %zu bytes, its planning pass measured %zu", real.off, want);
  if (rc != LDC_OK) { release(base); return rc; }
  if (base_out) *base_out = base;
  if (bytes_out) *bytes_out = want;
  return LDC_OK;
}

// The region a step's first kernel clears (launch_step_begin), as byte offsets from its start:
//   GroupNorm sums [n_gn][B][groups][kGnSumFloats] | split-K arrival counters [kSkTilesCap] | granule pool of the fused GroupNorm applies
//   (rounded up to 64) | LinearAttention workspaces [n_lin] of lin_bytes each | per-item scale_x maxima.
// Workspaces that are not cleared (one shared workspace, k column max not fused) lie behind the cleared bytes: the scale_x maxima then
// start where that workspace does, and are dead by the time an attention block writes it.
static constexpr int kGnSumFloats = 16;    // == kGnPad (ldc_internal.h asserts it)
static constexpr int kSkTilesCap = 1024;   // split-K arrival counters of a plan
struct ZeroRegion {
  size_t sk_count = 0;               // (the GroupNorm sums are at 0)
  size_t part = 0, part_cap = 0;     // granule pool and its rounded size
  size_t lin = 0, sx = 0;
  size_t zero_bytes = 0;             // what the step clears
  size_t alloc_bytes = 0;            // what the region takes from the arena (uncleared workspaces and 64 bytes of slack included)
};
inline ZeroRegion zero_region_layout(int n_gn, int B, int groups, size_t granule_bytes, size_t n_lin, size_t lin_bytes, bool lin_cleared,
                                     size_t sx_bytes) {
  ZeroRegion z;
  z.sk_count = (size_t)n_gn * B * groups * kGnSumFloats * 4;
  z.part = z.sk_count + (size_t)kSkTilesCap * 4;
  z.part_cap = (granule_bytes + 63) / 64 * 64;
  z.lin = z.part + z.part_cap;
  z.sx = z.lin + (lin_cleared ? n_lin * lin_bytes : 0);
  z.zero_bytes = z.sx + sx_bytes;
  z.alloc_bytes = z.lin + n_lin * lin_bytes + sx_bytes + 64;
  return z;
}
