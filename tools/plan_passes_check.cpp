// Host-only check of the planning protocol and of the layout of the region a step clears (csrc/plan_passes.h: plan_passes,
// zero_region_layout), meant to run under the host sanitizers on a machine without a GPU -- nothing here touches HIP:
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I ladiffcodec_amd/csrc \
//           tools/plan_passes_check.cpp -o tools/bin/plan_passes_check && tools/bin/plan_passes_check
// The protocol, with fake plans and fake allocators: exactly two sizing passes on dry arenas, one measuring pass and one real pass on the
// allocator's memory, in that order; every pass sees the maxima of what the passes before it asked for (a fake whose second pass asks
// for more than its first, as the granule pool does); an error from any pass or from the allocator ends the sequence, and what the
// allocator handed out is given back; a real pass that ends beyond measured + 4096 is refused with the library's message; the
// route-only mode ends behind the measuring pass and never calls the allocator.  The layout, over a grid of inputs (no GroupNorm
// buffers, granule bytes 0 and not a multiple of 64, workspaces cleared and not, scale_x on and off): the offsets against the planner's
// former pointer arithmetic, restated below, their order, alignment and that no two cleared parts overlap.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "plan_passes.h"

static int bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static std::string last_error;
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error = buf;
  return code;
}

struct FakePlan {
  long long sk_floats = 0, sk_need_max = 0;
  size_t part_bytes = 0, part_need = 0;
};
struct Pass {   // what a build pass saw
  bool dry;
  size_t cap;
  long long sk_floats;
  size_t part_bytes;
};
struct Fake {
  FakePlan pl;
  std::vector<Pass> passes;
  std::vector<long long> sk_asks = {100, 300, 200, 200};   // per pass: what the plan's convs ask for
  std::vector<size_t> part_asks = {0, 640, 640, 640};      // (nothing fuses before the pool exists, then it does)
  std::vector<size_t> bytes = {1000, 1000, 1000, 1000};    // per pass: what the plan takes from its arena
  int fail_pass = -1, fail_alloc = 0;
  int allocs = 0, releases = 0;
  std::vector<char> mem;
  size_t alloc_bytes = 0;

  int build(Arena& ar) {
    const int n = (int)passes.size();
    passes.push_back({ar.base == nullptr, ar.cap, pl.sk_floats, pl.part_bytes});
    if (n == fail_pass) return LDC_E_INVALID;
    pl.sk_need_max = sk_asks[n];
    pl.part_need = part_asks[n];
    char* p = (char*)ar.alloc(bytes[n]);
    if (p && bytes[n] <= ar.cap) memset(p, 0x5a, bytes[n]);   // (a pass inside its arena writes it: the sanitizer watches)
    return LDC_OK;
  }
  int run(bool measure_only, void** base = nullptr, size_t* got = nullptr) {
    return plan_passes(&pl, measure_only, [&](Arena& ar) { return build(ar); },
                       [&](size_t n, void** out) {
                         ++allocs;
                         if (fail_alloc) return (int)LDC_E_NOMEM;
                         alloc_bytes = n;
                         mem.resize(n);
                         *out = mem.data();
                         return (int)LDC_OK;
                       },
                       [&](void* p) { ++releases; EXPECT(p == mem.data(), "released something the allocator did not hand out"); }, base, got);
  }
};

static void check_protocol() {
  {   // the whole sequence
    Fake f;
    void* base = nullptr;
    size_t got = 0;
    const int rc = f.run(false, &base, &got);
    EXPECT(rc == LDC_OK, "a plan that fits was refused (%d)", rc);
    EXPECT(f.passes.size() == 4, "%zu passes, expected 4", f.passes.size());
    if (f.passes.size() == 4) {
      EXPECT(f.passes[0].dry && f.passes[1].dry && f.passes[2].dry && !f.passes[3].dry, "order: dry, dry, measure, real");
      EXPECT(f.passes[0].sk_floats == 0 && f.passes[0].part_bytes == 0, "pass 0 saw sizes");
      EXPECT(f.passes[1].sk_floats == 100 && f.passes[1].part_bytes == 0, "pass 1 saw %lld / %zu", f.passes[1].sk_floats, f.passes[1].part_bytes);
      // (the measuring pass asks for less split-K workspace than the second sizing pass: the sizes stay at the maxima of the sizing passes)
      EXPECT(f.passes[2].sk_floats == 300 && f.passes[2].part_bytes == 640, "pass 2 saw %lld / %zu", f.passes[2].sk_floats, f.passes[2].part_bytes);
      EXPECT(f.passes[3].sk_floats == 300 && f.passes[3].part_bytes == 640, "pass 3 saw %lld / %zu", f.passes[3].sk_floats, f.passes[3].part_bytes);
      EXPECT(f.passes[3].cap == 1000 + 4096, "the real arena holds %zu bytes", f.passes[3].cap);
    }
    EXPECT(f.allocs == 1 && f.releases == 0 && f.alloc_bytes == 1000 + 4096, "allocator: %d calls, %d releases, %zu bytes", f.allocs, f.releases, f.alloc_bytes);
    EXPECT(base == f.mem.data() && got == 1000 + 4096, "base / bytes not handed to the caller");
  }
  {   // a first sizing pass that asks for MORE than the second: the maxima still hold
    Fake f;
    f.sk_asks = {500, 100, 100, 100};
    f.part_asks = {1280, 64, 64, 64};
    EXPECT(f.run(false) == LDC_OK, "refused");
    EXPECT(f.passes.size() == 4 && f.passes[2].sk_floats == 500 && f.passes[2].part_bytes == 1280 && f.passes[3].sk_floats == 500, "maxima lost");
  }
  for (int k = 0; k < 4; ++k) {   // an error from pass k ends the sequence there
    Fake f;
    f.fail_pass = k;
    const int rc = f.run(false);
    EXPECT(rc == LDC_E_INVALID, "pass %d failed, the protocol returned %d", k, rc);
    EXPECT((int)f.passes.size() == k + 1, "pass %d failed, %zu passes ran", k, f.passes.size());
    EXPECT(f.allocs == (k == 3) && f.releases == (k == 3), "pass %d failed: %d allocations, %d releases", k, f.allocs, f.releases);
  }
  {   // the allocator fails: no real pass, nothing to release
    Fake f;
    f.fail_alloc = 1;
    const int rc = f.run(false);
    EXPECT(rc == LDC_E_NOMEM && f.passes.size() == 3 && f.allocs == 1 && f.releases == 0, "allocator failure: rc %d, %zu passes, %d releases", rc, f.passes.size(), f.releases);
  }
  {   // a real pass that stays within the 4096 bytes of slack passes; one byte more is refused and its memory released
    Fake f;
    f.bytes = {1000, 1000, 1000, 1000 + 4096};
    EXPECT(f.run(false) == LDC_OK && f.releases == 0, "a real pass that ends at measured + 4096 was refused");
    Fake g;
    g.bytes = {1000, 1000, 1000, 1000 + 4097};
    void* base = nullptr;
    last_error.clear();
    const int rc = g.run(false, &base);
    EXPECT(rc == LDC_E_STATE && g.releases == 1 && base == nullptr, "overflow: rc %d, %d releases", rc, g.releases);
    EXPECT(last_error == "internal: the plan needs 5097 bytes, its planning pass measured 5096", "message: %s", last_error.c_str());
  }
  {   // route-only: three passes, no allocator
    Fake f;
    EXPECT(f.run(true) == LDC_OK && f.passes.size() == 3 && f.passes[2].dry && f.allocs == 0 && f.releases == 0, "route-only: %zu passes, %d allocations", f.passes.size(), f.allocs);
    Fake g;
    g.fail_pass = 2;
    EXPECT(g.run(true) == LDC_E_INVALID && g.allocs == 0, "route-only: a failing measuring pass");
  }
}

// The planner's arithmetic before there was a layout function (build_plan; the test hooks carved the same region for one block), on a
// float* stats_pool at 0: offsets in bytes
struct Former { size_t sk_count, part_pool, part_cap, linattn_ws, sx_max, alloc, stats_bytes; };
static Former former(int n_gn, int B, int groups, size_t plan_part_bytes, size_t n_lin, size_t ws_bytes, bool lin_zeroed, size_t sx_bytes) {
  const int kGnPad = 16;
  const size_t gn_bytes = (size_t)n_gn * B * groups * kGnPad * 4;
  const size_t lin_bytes = n_lin * ws_bytes;
  const int sk_tiles_cap = 1024;
  const size_t part_bytes = (plan_part_bytes + 63) / 64 * 64;
  const size_t sk_count_bytes = (size_t)sk_tiles_cap * 4 + part_bytes;
  Former f;
  f.alloc = gn_bytes + sk_count_bytes + lin_bytes + sx_bytes + 64;
  f.sk_count = gn_bytes / 4 * 4;                        // stats_pool + gn_bytes / 4
  f.part_pool = f.sk_count + (size_t)sk_tiles_cap * 4;  // sk_count + sk_tiles_cap
  f.part_cap = part_bytes;
  f.linattn_ws = (gn_bytes + sk_count_bytes) / 4 * 4;   // stats_pool + (gn_bytes + sk_count_bytes) / 4
  f.sx_max = f.linattn_ws + (lin_zeroed ? lin_bytes / 4 * 4 : 0);
  f.stats_bytes = gn_bytes + sk_count_bytes + (lin_zeroed ? lin_bytes : 0) + sx_bytes;
  return f;
}

static void check_layout() {
  int cases = 0;
  const size_t ws_item = (size_t)(4 * 32 + 4 * 32 * 32) * 4;   // a workspace of heads 4, dim_head 32 (any multiple of 4 serves)
  for (int n_gn : {0, 2, 46})
    for (int B : {1, 3, 16})
      for (int groups : {1, 8})
        for (size_t part : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)1000, (size_t)98304})
          for (size_t n_lin : {(size_t)1, (size_t)10})
            for (int cleared = 0; cleared < 2; ++cleared)
              for (int sx = 0; sx < 2; ++sx) {
                const size_t ws = (size_t)B * ws_item, sx_bytes = sx ? (size_t)B * 4 : 0;
                const ZeroRegion z = zero_region_layout(n_gn, B, groups, part, n_lin, ws, cleared != 0, sx_bytes);
                const Former f = former(n_gn, B, groups, part, n_lin, ws, cleared != 0, sx_bytes);
                ++cases;
                EXPECT(z.sk_count == f.sk_count && z.part == f.part_pool && z.part_cap == f.part_cap && z.lin == f.linattn_ws && z.sx == f.sx_max,
                       "offsets differ at n_gn %d B %d groups %d part %zu n_lin %zu cleared %d sx %d", n_gn, B, groups, part, n_lin, cleared, sx);
                EXPECT(z.zero_bytes == f.stats_bytes && z.alloc_bytes == f.alloc, "totals differ at n_gn %d B %d part %zu n_lin %zu cleared %d sx %d: %zu / %zu, %zu / %zu",
                       n_gn, B, part, n_lin, cleared, sx, z.zero_bytes, f.stats_bytes, z.alloc_bytes, f.alloc);
                // ordered, one behind the other: sums | counters | granules | (cleared workspaces) | maxima, then the end of what is cleared
                EXPECT(z.sk_count == (size_t)n_gn * B * groups * 16 * 4 && z.part == z.sk_count + 4096 && z.lin == z.part + z.part_cap, "order");
                EXPECT(z.part_cap % 64 == 0 && z.part_cap >= part && z.part_cap < part + 64, "granule pool %zu for %zu bytes", z.part_cap, part);
                EXPECT(z.sx == z.lin + (cleared ? n_lin * ws : 0) && z.zero_bytes == z.sx + sx_bytes, "the cleared bytes end behind the maxima");
                EXPECT(z.sk_count % 64 == 0 && z.part % 64 == 0 && z.lin % 64 == 0 && z.sx % 4 == 0, "alignment");
                // everything the builder addresses lies inside the allocation (the uncleared workspace too)
                EXPECT(z.lin + n_lin * ws <= z.alloc_bytes && z.zero_bytes + 64 <= z.alloc_bytes, "allocation");
              }
  printf("layout: %d cases\n", cases);
}

int main() {
  check_protocol();
  check_layout();
  if (bad) { printf("%d checks FAILED\n", bad); return 1; }
  printf("plan_passes_check: ok\n");
  return 0;
}
