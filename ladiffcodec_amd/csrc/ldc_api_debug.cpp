// ldc_api_debug.cpp -- test hooks of the UNet planner.  Host-side C++ only.
#include "ldc_internal.h"

extern "C" int ldc_unet_debug_tap(ldc_ctx* c, const char* name, float* out, int64_t capacity, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!name || !out) return fail(LDC_E_INVALID, "null argument");
  const Halves& h = c->last_halves;
  if (h.n == 0) return fail(LDC_E_STATE, "no UNet call has been made yet");
  int64_t need = 0;
  for (int k = 0; k < h.n; ++k) {
    auto it = h.p[k]->taps.find(name);
    if (it == h.p[k]->taps.end()) return fail(LDC_E_INVALID, "unknown tap '%s'", name);
    need += (int64_t)h.p[k]->B * it->second.C * it->second.L;
  }
  if (capacity < need) return fail(LDC_E_INVALID, "tap '%s' needs %lld elements", name, (long long)need);
  hipStream_t s = pick_stream(c, stream);
  for (int k = 0; k < h.n; ++k) {
    const Plan::Tap& tp = h.p[k]->taps.find(name)->second;
    HIPCHK(launch_from_cl(c->dt, tp.p, out + (size_t)h.b0[k] * tp.C * tp.L, h.p[k]->B, tp.C, tp.L, nullptr, 0, 0.f, s));
  }
  return finish_stream(c, stream);
}

// A block of the loaded UNet by the name the hooks take: down<i> / mid / up<i> is level i's attention block (r stays null); down<i>.1,
// down<i>.2, mid.1, mid.2, up<i>.1, up<i>.2 and final are ResnetBlocks, `a` the attention block that follows one in a step (down<i>.2,
// mid.1, up<i>.2).  Digits only, index in range; nothing set: no such block.
namespace {
struct UnetBlockRef {
  const ResnetW* r = nullptr;
  const LinAttnW* a = nullptr;
  bool linear = true, is_final = false;
};
UnetBlockRef find_unet_block(const UnetW& u, const std::string& n) {
  UnetBlockRef f;
  if (n == "final") { f.r = &u.fin; f.is_final = true; return f; }
  const size_t dot = n.find('.');
  const std::string head = n.substr(0, dot), which = dot == std::string::npos ? "" : n.substr(dot + 1);
  if (dot != std::string::npos && which != "1" && which != "2") return f;
  const ResnetW *b1 = nullptr, *b2 = nullptr;
  const LinAttnW* at = nullptr;
  bool attn_behind_b1 = false;
  auto level = [&](const char* pre, const std::vector<LevelW>& lv) {
    const size_t pl = strlen(pre);
    if (head.compare(0, pl, pre) != 0 || head.size() == pl || head.find_first_not_of("0123456789", pl) != std::string::npos) return;
    const size_t i = (size_t)atoi(head.c_str() + pl);
    if (i < lv.size()) { b1 = &lv[i].b1; b2 = &lv[i].b2; at = &lv[i].attn; }
  };
  if (head == "mid") { b1 = &u.mid1; b2 = &u.mid2; at = &u.mid_attn; f.linear = false; attn_behind_b1 = true; }
  else { level("down", u.downs); level("up", u.ups); }
  if (!at) return f;
  if (dot == std::string::npos) { f.a = at; return f; }
  f.r = which == "1" ? b1 : b2;
  f.a = (which == "1") == attn_behind_b1 ? at : nullptr;
  return f;
}

// A hook's private plan, never cached: built by the planning protocol of the cached plans (plan_passes.h) on memory of its own, which
// leaves with it -- as the fork / join events run_ops creates on a plan's first use (a cached plan frees them when it is evicted).
struct PrivatePlan {
  Plan pl;
  DevMem mem;
  ~PrivatePlan() {
    for (hipEvent_t e : pl.marker_events) (void)hipEventDestroy(e);
  }
  template <class Build>
  int build(bool route_only, Build body) {   // body(arena): one pass over the plan's content; route_only: planned, not allocated
    return plan_passes(&pl, route_only, [&](Arena& ar) { pl.reset_build(); return body(ar); },
                       [&](size_t bytes, void** base) { return mem.alloc(base, bytes); }, [](void*) {});
  }
};
}   // namespace

// Residual(PreNorm(LinearAttention | Attention)) of one block of the loaded UNet on caller data (tests).  The launches come from
// PlanBuilder::attention() itself, on a private plan that is never cached: every option (fold_ctx, fuse_attn_tail, fuse_kmax, fold_ln,
// conv_lean) routes as it does in a decode -- the PreNorm folded into to_qkv, the context fold, the tail.  What differs from a decode:
// no ResnetBlock in front, so a folded PreNorm computes its row statistics itself (as ldc_ln_fold_compare's out[0]) and an unfolded one
// is its own launch; the batch is one part.  Synchronous: the call waits for its stream and reports a device-side failure of its own
// launches.  Allocates and frees its workspace (hipFree waits for the device): not for the decode path.
extern "C" int ldc_debug_attention_block(ldc_ctx* c, const char* name, const float* x, int B, int L, float* out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!name || !x || !out || B <= 0 || L <= 0) return fail(LDC_E_INVALID, "bad arguments");
  const UnetW& u = c->unet;
  const UnetBlockRef blk = find_unet_block(u, name);
  const LinAttnW* a = blk.r ? nullptr : blk.a;
  if (!a) return fail(LDC_E_INVALID, "unknown attention block '%s' (down0..down%zu, mid, up0..up%zu)", name, u.downs.size() - 1, u.ups.size() - 1);
  hipStream_t s = pick_stream(c, stream);
  const int dt = c->dt, C = a->dim;
  const size_t es = dt_size(dt);
  PrivatePlan priv;
  Plan& pl = priv.pl;
  pl.B = B; pl.L = L;
  void *x_cl = nullptr, *y_cl = nullptr;
  LDCCHK(priv.build(false, [&](Arena& ar) {
    PlanBuilder pb{c, &pl, &ar, B, es};
    pb.take_zero_region(0, 1, true, 0);   // split-K arrival counters | LinearAttention workspace: what a step clears
    x_cl = pb.act(B * L, C);
    y_cl = pb.attention(*a, x_cl, L, blk.linear);
    return (int)LDC_OK;
  }));
  HIPCHK(hipMemsetAsync(pl.zero_ptr, 0, pl.zero_bytes, s));
  HIPCHK(launch_to_cl(dt, x, x_cl, B, C, L, nullptr, 0, 0.f, s));
  LDCCHK(run_ops(c, &pl, true, s));
  HIPCHK(launch_from_cl(dt, y_cl, out, B, C, L, nullptr, 0, 0.f, s));
  HIPCHK(hipStreamSynchronize(s));
  return check_dev_flag(c);
}

// One ResnetBlock of the loaded UNet on caller data (tests), optionally with the attention block that follows it in a step.  As
// ldc_debug_attention_block: a private plan that is never cached, the launches from PlanBuilder::resnet() (and attention()) themselves, so
// fuse_gn_epi, fuse_gn_stats, fold_res, fold_ln, fuse_ln and conv_lean route as in a decode.  The timestep is set as a step sets it
// (launch_step_set + launch_step_begin on the plan's zero region, or the item records + launch_step_begin_items), which also clears the
// GroupNorm sums, the split-K counters and the granule regions of the fused convs in front of the run.  `stats` are the sums the kernels
// themselves accumulated: the atomic / launch_gn_stats buffers, or the granules of the fused exchange read back and summed on the host.
extern "C" int ldc_debug_resnet_block(ldc_ctx* c, const char* name, const float* x1, const float* x2, int B, int L, int t, const int32_t* lens,
                                      int shift, const int32_t* t_items, int with_attention, float* out, float* mid, float* stats, float* attn_out,
                                      float* pre, int* info, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  const bool route_only = !out && !mid && !stats;   // planning on the host alone: info[0..9] of the run these arguments would make
  if (!name || !info || B <= 0 || L <= 0 || (!route_only && (!x1 || !out || !mid || !stats))) return fail(LDC_E_INVALID, "bad arguments");
  if (c->w8) return fail(LDC_E_INVALID, "ldc_debug_resnet_block does not support fp8 contexts (block1's output is stored in fp8 there)");
  const UnetW& u = c->unet;
  if (!t_items && (t < 0 || t >= u.timesteps)) return fail(LDC_E_INVALID, "t out of range");
  if (t_items && !lens) return fail(LDC_E_INVALID, "per-item timesteps need lengths (a per-item plan is a ragged plan)");
  if (!lens && shift != 0) return fail(LDC_E_INVALID, "shift without lengths");
  if (shift < 0 || shift > 8 || ((long long)L << shift) > (1ll << 30)) return fail(LDC_E_INVALID, "bad shift");
  for (int b = 0; lens && b < B; ++b) {
    if (lens[b] > (L << shift) || (lens[b] >> shift) < 1) return fail(LDC_E_INVALID, "length %d of item %d must leave 1..%d rows at shift %d", (int)lens[b], b, L, shift);
    if (t_items && (t_items[b] < 0 || t_items[b] >= u.timesteps)) return fail(LDC_E_INVALID, "t of item %d out of range", b);
  }
  // ---- which block ----
  const UnetBlockRef blk = find_unet_block(u, name);
  const ResnetW* r = blk.r;
  const LinAttnW* a = blk.a;   // the attention block that follows it in a step (down<i>.2, mid.1, up<i>.2)
  if (!r) return fail(LDC_E_INVALID, "unknown ResnetBlock '%s' (down<i>.1, down<i>.2, mid.1, mid.2, up<i>.1, up<i>.2, final)", name);
  if (!route_only && (r->cin2 > 0) != (x2 != nullptr)) return fail(LDC_E_INVALID, "block '%s' reads %s", name, r->cin2 > 0 ? "a concatenation: x2 is missing" : "one tensor: x2 must be null");
  if (with_attention && (!a || (!route_only && !attn_out))) return fail(LDC_E_INVALID, "with_attention: block '%s' has no attention block behind it, or attn_out is null", name);
  hipStream_t s = pick_stream(c, stream);
  const int dt = c->dt, g = u.groups, cout = r->cout;
  const size_t es = dt_size(dt);
  PrivatePlan priv;
  Plan& pl = priv.pl;
  pl.B = B; pl.L = lens ? L << shift : L;
  pl.ragged = lens != nullptr; pl.items = t_items != nullptr;
  PlanBuilder::ResnetTrace tr;
  void *x1_cl = nullptr, *x2_cl = nullptr, *y_cl = nullptr, *ya_cl = nullptr;
  const int rc = priv.build(route_only, [&](Arena& ar) {
    PlanBuilder pb{c, &pl, &ar, B, es};
    pb.trace = &tr;
    // GroupNorm sums | split-K arrival counters | granule regions | LinearAttention workspace: what a step's first kernel clears
    pb.take_zero_region(2, 1, true, 0);
    pl.step_state = (int*)ar.alloc(64);
    pl.cur_ss = (float*)ar.alloc((size_t)std::max(1, u.ss_stride) * 4);
    pl.item_state = pl.items ? (ItemState*)ar.alloc((size_t)B * sizeof(ItemState)) : nullptr;
    pl.lens = pl.ragged ? (int*)ar.alloc((size_t)B * 4) : nullptr;
    pl.flens = nullptr;
    x1_cl = pb.act(B * L, r->cin1);
    x2_cl = r->cin2 > 0 ? pb.act(B * L, r->cin2) : nullptr;
    ya_cl = nullptr;
    if (with_attention) ya_cl = pb.resnet_then_attention(*r, *a, x1_cl, x2_cl, L, blk.linear, &y_cl);   // as a step pairs them
    else if (blk.is_final) y_cl = pb.final_block(*r, x1_cl, x2_cl, L, false);                            // with the final block's tanh
    else y_cl = pb.resnet(*r, x1_cl, x2_cl, L);
    return (int)LDC_OK;
  });
  LDCCHK(rc);
  auto route = [&]() {
    info[0] = tr.epi1; info[1] = tr.epi2; info[2] = tr.folded; info[3] = tr.fuse_stats; info[4] = tr.xn; info[5] = tr.rowstat;
    info[6] = tr.t1[0]; info[7] = tr.t1[1]; info[8] = tr.t2[0]; info[9] = tr.t2[1];
    info[10] = info[11] = 0;
  };
  if (route_only) { route(); return LDC_OK; }
  HIPCHK(hipMemsetAsync(pl.step_state, 0, 64, s));   // (the epoch word)
  if (lens) HIPCHK(launch_lens_write(pl.lens, lens, B, s));
  HIPCHK(launch_to_cl(dt, x1, x1_cl, B, r->cin1, L, nullptr, 0, 0.f, s));
  if (x2_cl) HIPCHK(launch_to_cl(dt, x2, x2_cl, B, r->cin2, L, nullptr, 0, 0.f, s));
  if (lens) {   // the invariant a ragged plan gives its convs: zero behind every item's length
    HIPCHK(launch_mask_rows(dt, x1_cl, B, L, r->cin1, pl.lens, shift, s));
    if (x2_cl) HIPCHK(launch_mask_rows(dt, x2_cl, B, L, r->cin2, pl.lens, shift, s));
  }
  if (t_items) {
    std::vector<ItemState> recs(B);
    for (int b = 0; b < B; ++b) {
      ItemState it{};
      it.t = t_items[b]; it.remaining = 1; it.len = lens[b];
      recs[b] = it;
    }
    HIPCHK(launch_items_write(pl.item_state, recs.data(), B, pl.lens, nullptr, upsample_factor(c), s));
    HIPCHK(launch_step_begin_items(pl.item_state, B, pl.step_state, pl.zero_ptr, pl.zero_bytes, 0, s));
  } else {
    HIPCHK(launch_step_set(pl.step_state, t, 0, c->cur_key, s));
    HIPCHK(launch_step_begin(u.ss_table, u.ss_stride, pl.step_state, pl.cur_ss, nullptr, s, pl.zero_ptr, pl.zero_bytes));
  }
  LDCCHK(run_ops(c, &pl, true, s));
  HIPCHK(launch_from_cl(dt, y_cl, out, B, cout, L, nullptr, 0, 0.f, s));
  HIPCHK(launch_from_cl(dt, tr.b, mid, B, cout, L, nullptr, 0, 0.f, s));
  if (ya_cl) HIPCHK(launch_from_cl(dt, ya_cl, attn_out, B, a->dim, L, nullptr, 0, 0.f, s));
  for (int k = 0; pre && k < 2; ++k) {   // the conv outputs as stored, where the route stores them
    float* dst = pre + (size_t)k * B * cout * L;
    const void* src = k == 0 ? tr.a : tr.d;
    if (src) HIPCHK(launch_from_cl(dt, src, dst, B, cout, L, nullptr, 0, 0.f, s));
    else HIPCHK(hipMemsetAsync(dst, 0, (size_t)B * cout * L * 4, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  LDCCHK(check_dev_flag(c));
  // ---- the statistics as the kernels accumulated them ----
  int tags_ok = 1, stray = 0;
  const int cpg = cout / g;
  for (int k = 0; k < 2; ++k) {
    float* dst = stats + (size_t)k * B * g * 2;
    const bool fused = k == 0 ? tr.epi1 : tr.epi2;
    if (!fused) {
      std::vector<float> h((size_t)B * g * kGnPad);
      HIPCHK(hipMemcpy(h.data(), k == 0 ? tr.st1 : tr.st2, h.size() * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < B * g; ++i) { dst[2 * i] = h[(size_t)i * kGnPad]; dst[2 * i + 1] = h[(size_t)i * kGnPad + 1]; }
      continue;
    }
    // gn_part[item][M-tile slot][wave row][32-column block] x {tag, sum, tag, sumsq} (conv_device.h: epilogue_gn_fused)
    const int bm = (k == 0 ? tr.t1 : tr.t2)[0], wm = (k == 0 ? tr.t1 : tr.t2)[1], mslots = k == 0 ? tr.mslots1 : tr.mslots2;
    const int nc32 = cout / 32, sub_n = cpg / 32;
    if (bm <= 0 || wm <= 0 || sub_n <= 0) return fail(LDC_E_STATE, "internal: a fused conv without its tile shape");
    std::vector<uint32_t> h((size_t)B * mslots * wm * nc32 * 4);
    HIPCHK(hipMemcpy(h.data(), k == 0 ? tr.part1 : tr.part2, h.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
      const int lo = b * L, hi = lo + L;
      const int used = (hi - 1) / bm - lo / bm + 1;   // the M-tile slots `gather` reads for this item
      for (int gi = 0; gi < g; ++gi) { dst[((size_t)b * g + gi) * 2] = 0.f; dst[((size_t)b * g + gi) * 2 + 1] = 0.f; }
      for (int ms = 0; ms < mslots; ++ms)
        for (int w = 0; w < wm; ++w)
          for (int c32 = 0; c32 < nc32; ++c32) {
            const uint32_t* v = &h[((((size_t)b * mslots + ms) * wm + w) * nc32 + c32) * 4];
            if (ms >= used) { stray |= (v[0] | v[1] | v[2] | v[3]) != 0u; continue; }
            if (v[0] != 1u || v[2] != 1u) { tags_ok = 0; continue; }
            float sv, qv;
            memcpy(&sv, &v[1], 4); memcpy(&qv, &v[3], 4);
            dst[((size_t)b * g + c32 / sub_n) * 2] += sv;
            dst[((size_t)b * g + c32 / sub_n) * 2 + 1] += qv;
          }
    }
  }
  route();
  info[10] = tags_ok; info[11] = stray;
  return LDC_OK;
}