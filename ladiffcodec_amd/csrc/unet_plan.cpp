// unet_plan.cpp -- the UNet planner (unet_plan.h).  Host-side C++ only.
#include "ldc_internal.h"

bool gn_apply_fp8_ok(int C) { return C % 8 == 0 && C / 8 <= 256 && 256 % (C / 8) == 0 && C <= 2048; }

// ------------------------------------------------------------------------------------------------
// UNet plan
// ------------------------------------------------------------------------------------------------
void* PlanBuilder::act(int rows, int C) {
  pl->act_bytes += (double)rows * C * es;
  return ar->alloc((size_t)rows * C * es);
}
const int* PlanBuilder::lens() const { return pl->ragged ? (pl->lens ? pl->lens : reinterpret_cast<const int*>(16)) : nullptr; }
int PlanBuilder::level(int L) const {
  int sh = 0;
  while ((L << sh) < pl->L) ++sh;
  return sh;
}
void PlanBuilder::mask(void* y, int L, int C) {
  if (!pl->ragged) return;
  const int dt = c->dt, Bn = B, sh = level(L);
  const int* ln = pl->lens;
  info = "mask_rows_c" + std::to_string(C) + "_L" + std::to_string(L);
  add([=](hipStream_t s) { return launch_mask_rows(dt, y, Bn, L, C, ln, sh, s); }, false, 0, LDC_CLASS_ELEMENTWISE, 0);
}
void PlanBuilder::mark(int kind) {
  pl->step.push_back({[](hipStream_t) { return hipSuccess; }, kind, LDC_CLASS_OTHER, 0, 0, "-"});
}
void PlanBuilder::add(std::function<hipError_t(hipStream_t)> f, bool is_conv, double flops, int cls, double bytes) {
  pl->step.push_back({std::move(f), where, is_conv ? LDC_CLASS_CONV : cls, flops, bytes, info.empty() ? std::string("-") : info});
  info.clear();
  pl->flops += flops;
}
void PlanBuilder::conv_bm(const ConvLayer& ly, int L_in, int L_out, bool with_stats, int* out) {
  ConvCall d;
  d.B = B; d.L_in = L_in; d.L_rows = L_out; d.y_ld = ly.n; d.tune = &c->tune;
  d.sk_part = sk_part; d.sk_count = sk_count; d.sk_part_cap = sk_part_cap; d.sk_count_cap = sk_count_cap;
  if (with_stats) { d.gn_sum = stats_pool; d.gn_groups = c->unet.groups; }
  long long need = 0;
  out[0] = out[1] = 0; out[2] = 1; out[3] = 0;
  d.sk_need = &need; d.bm_out = out;
  // (a layer with a folded second conv is refused without its second output -- conv_kargs -- and the refusal reads as "generic kernel, no
  // fused epilogue": since round 5 asked for the folded layer's own tile shape, the nine folded block1 convs of a step had silently gone
  // back to conv + gn_apply pairs.  Nothing is written in a dry run.)
  if (ly.wtaps) d.y2 = reinterpret_cast<void*>(16);
  (void)launch_conv(ly, d, nullptr);
}
bool PlanBuilder::take_part(GnEpi* ge, int L, int bm, int wm, int n) {
  ge->mslots = (L + bm - 1) / bm + 1;
  const size_t bytes = (size_t)B * ge->mslots * wm * (n / 32) * 16;
  pl->part_need += bytes;
  if (!part_pool || part_used + bytes > part_cap) return false;
  ge->part = part_pool + part_used;
  part_used += bytes;
  return true;
}
void PlanBuilder::conv(const ConvLayer& ly, const void* x1, const void* x2, void* y, const void* residual, int L_in, int L_out, float* gn_sum,
                       unsigned* colmax, int cm_lo, int cm_hi, int cm_stride, const GnEpi* ge) {
  ConvCall cc;
  cc.B = B; cc.L_in = L_in; cc.L_rows = L_out; cc.x1 = x1; cc.x2 = x2; cc.y = y; cc.residual = residual; cc.y_ld = ly.n;
  cc.gn_sum = gn_sum; cc.gn_groups = gn_sum ? c->unet.groups : 0;
  cc.y2 = y2_next; y2_next = nullptr;
  cc.qkv_ctx_ws = qkv_ctx_next; cc.qkv_ctx_stride = qkv_ctx_stride_next; qkv_ctx_next = nullptr; qkv_ctx_stride_next = 0;
  cc.ln_rowstat = ly.ln_s ? ln_rowstat_next : nullptr; ln_rowstat_next = nullptr;
  if (pl->kst && pl->step.size() < (size_t)kKstOps) {
    cc.kst = pl->kst + pl->step.size() * 2; cc.kst_stride = kKstOps * 2; cc.kst_step = pl->step_state;
  }
  if (ge && ge->part) {
    cc.gn_groups = c->unet.groups;
    cc.rowstat_out = residual ? ge->rowstat : nullptr;
    cc.gn_part = ge->part; cc.gn_mslots = ge->mslots; cc.gn_gamma = ge->gamma; cc.gn_beta = ge->beta; cc.gn_ss = ge->ss; cc.gn_out = ge->out;
    cc.fail_flag = c->dev_flag_dev;
  }
  cc.colmax = colmax; cc.colmax_lo = cm_lo; cc.colmax_hi = cm_hi; cc.colmax_stride = cm_stride;
  cc.sk_part = sk_part; cc.sk_count = sk_count; cc.sk_part_cap = sk_part_cap; cc.sk_count_cap = sk_count_cap;
  cc.tune = &c->tune;
  {   // dry run of the launcher: how much split-K workspace would this conv use?
    ConvCall d = cc;
    long long need = 0;
    d.sk_need = &need;
    (void)launch_conv(ly, d, nullptr);
    pl->sk_need_max = std::max(pl->sk_need_max, need);
  }
  const ConvLayer* lp = &ly;
  {
    char buf[96];
    snprintf(buf, sizeof(buf), "k%d%s_s%d_u%d_c%d+%d->%d_L%d%s%s", ly.taps, ly.wtaps ? "+res" : "", ly.stride, ly.ups, ly.cin1, ly.cin2, ly.n, L_out,
             (ge && ge->part) ? (residual ? "_gnapply+res" : "_gnapply") : (gn_sum ? "_gn" : ""), colmax ? "_kmax" : (cc.qkv_ctx_ws ? "_ctx" : ""));
    info = buf;
  }
  const double cbytes = ((double)B * L_in * (ly.cin1 + ly.cin2) + (double)B * L_out * ly.n * (((ge && ge->part && residual) ? 2 : 1) + (ly.wtaps ? 1 : 0))) * es + (double)conv_packed_weight_bytes(ly);
  pl->conv_bytes += cbytes;
  add([lp, cc](hipStream_t s) { return launch_conv(*lp, cc, s); }, true, ly.flops_per_row * (double)B * L_out, LDC_CLASS_CONV, cbytes);
}
void* PlanBuilder::take_raw(size_t bytes) {
  bytes = (bytes + 63) / 64 * 64;
  pl->part_need += bytes;
  if (!part_pool || part_used + bytes > part_cap) return nullptr;
  void* p = part_pool + part_used;
  part_used += bytes;
  return p;
}
float* PlanBuilder::next_stats() {
  const int g = c->unet.groups;
  return stats_pool + (size_t)(stats_used++) * B * g * kGnPad;
}
void* PlanBuilder::resnet(const ResnetW& r, const void* x1, const void* x2, int L, const float* ln_g, void** xn_out, bool xn_fp8, int out_mode) {
  const int rows = B * L, dt = c->dt, g = c->unet.groups, Bn = B;
  const UnetW* u = &c->unet;
  const float* cur_ss = pl->cur_ss;
  // per-item plan: block1's gn_apply takes the (scale | shift) row of each item's own t from the table
  const int* item_t = pl->items ? &pl->item_state->t : nullptr;
  const float* ss_tab = u->ss_table + r.ss_off;
  const int ss_stride = u->ss_stride, n_t = u->timesteps;
  // fp8-weight context: block1's output feeds block2's conv alone, so it is produced in fp8 and that conv runs fp8 x fp8
  const bool f8 = c->w8 && c->fp8_act && r.c2_f8.w != nullptr;
  const int* ln = lens();   // ragged plan: conv -> gn_stats -> gn_apply, statistics over the valid rows, padding rows written as zero
  const int sh = ln ? level(L) : 0;
  void* b = f8 ? ar->alloc((size_t)rows * r.cout) : act(rows, r.cout);
  void* out = (out_mode & 1) ? ar->alloc((size_t)rows * r.cout) : act(rows, r.cout);
  float* st1 = next_stats();
  float* st2 = next_stats();
  const int cpg = r.cout / g;
  const bool fuse_stats = !ln && c->fuse_gn_stats && cpg >= 4 && (cpg & (cpg - 1)) == 0;   // (a conv's own sums run over every row)
  const bool rowstat_wanted = want_rowstat;
  want_rowstat = false;
  last_rowstat = nullptr;
  // GroupNorm apply inside the conv epilogue (in-launch per-item wait): the tile height must not exceed twice an item's rows
  // (a tile then straddles at most three items), and the output must be in the UNet dtype (fp8 outputs keep gn_apply)
  const bool epi_ok = !ln && c->fuse_gn_epi && cpg % 32 == 0 && r.cout % 32 == 0 && L >= c->gn_epi_min_l;
  bool epi1 = false, epi2 = false;
  GnEpi ge1, ge2;
  if (epi_ok) {
    int t1[4], t2[4];
    conv_bm(r.c1, L, L, false, t1);
    // (the tile shape of the layer that will be LAUNCHED: with res_conv folded in -- decided below by the same rule -- that is c1r,
    // which the 256 x 64 tiles do not take)
    if (r.has_res && c->fold_res && r.c1r.w && t1[0] > 0 && t1[2] == 1) conv_bm(r.c1r, L, L, false, t1);
    // Two gates on the tiles the dry run reports (BM x BN): (i) the launch as a whole stays within gn_epi_max_tiles (a performance gate:
    // beyond two rounds of workgroups the waiting tiles cost more than the gn_apply launch they replace); (ii) a SAFETY gate per item --
    // every tile spins until all tiles of its item(s) have published, and the dispatch order interleaves the items of a group of 8 M tiles,
    // so an item's tiles plus two dispatch groups (the one it sits in, the one a straddling tile reaches into) must be resident together
    // even while the other batch parts' launches hold their share of the chip (three workgroups of these kernels fit a CU: 41-51 KB of
    // ring, <= 168 registers; the parts run concurrently).  A long single file (sample.py's whole-file mode: B = 1, L = samples / hop)
    // fails (ii) and takes the conv + gn_apply pair instead of stalling every fused launch for its time-out.
    // The slots come from the occupancy query of the kernels these convs land on x the device's CUs (round 6; before: a constant 3 x 256).
    const int concurrent = std::max(2, c->split_batch);
    c->tune.ring3_cu_share = c->num_cus / concurrent * 8 / 10;   // (the launcher applies the same rule to the three-stage kernels' own slots: conv_lean.inc)
    const long resident_slots = (long)(c->w8 ? std::min(conv_fused_gn_wgs_per_cu(DT_BF16, true), conv_fused_gn_wgs_per_cu(DT_FP8, false)) : conv_fused_gn_wgs_per_cu(dt, false)) *
                                c->num_cus / concurrent * 8 / 10;
    auto few_tiles = [&](const int* t) {
      if (t[0] <= 0 || t[3] <= 0) return false;
      const long ntn = (r.cout + t[3] - 1) / t[3];
      const long launch_tiles = (long)((rows + t[0] - 1) / t[0]) * ntn;
      const long item_tiles = (long)((L + t[0] - 1) / t[0] + 1) * ntn;
      return launch_tiles <= c->gn_epi_max_tiles && (launch_tiles <= resident_slots || item_tiles + 16 * ntn <= resident_slots);
    };
    epi1 = (!f8 || dt == DT_BF16) && few_tiles(t1) && t1[0] <= 2 * L && take_part(&ge1, L, t1[0], t1[1], r.cout);   // f8: block1's output in fp8
    conv_bm(f8 ? r.c2_f8 : r.c2, L, L, false, t2);
    epi2 = (!(out_mode & 1) || dt == DT_BF16) && few_tiles(t2) && t2[0] <= 2 * L && take_part(&ge2, L, t2[0], t2[1], r.cout);
  }
  void* a = epi1 ? nullptr : act(rows, r.cout);   // un-normalised conv outputs exist only on the unfused path
  void* d = epi2 ? nullptr : act(rows, r.cout);
  // res_conv: folded into block1's conv where that conv runs on the pipelined kernel with an unsplit K (one launch and one
  // read of x less); otherwise its own launch (on the side stream when there is one: it only feeds the final add)
  const void* res = x1;
  bool folded = false;
  void* rr = r.has_res ? act(rows, r.cout) : nullptr;
  if (r.has_res && c->fold_res && r.c1r.w) {
    int t[4];
    conv_bm(r.c1, L, L, false, t);
    folded = t[0] > 0 && t[2] == 1;
  }
  if (r.has_res && !folded) {
    mark(2);
    where = 1;
    conv(r.res, x1, x2, rr, nullptr, L, L);
    where = 0;
  }
  if (r.has_res) res = rr;
  const ConvLayer& c1 = folded ? r.c1r : r.c1;
  const ResnetW* rp = &r;
  if (epi1) {   // block1: conv -> GroupNorm -> (scale + 1, shift) -> SiLU, one launch, one store
    ge1.gamma = r.g1; ge1.beta = r.b1; ge1.ss = cur_ss + r.ss_off; ge1.out = f8 ? 1 : 0;
    if (folded) y2_next = rr;
    conv(c1, x1, x2, b, nullptr, L, L, nullptr, nullptr, 0, 0, 0, &ge1);
  } else {
    if (folded) y2_next = rr;
    conv(c1, x1, x2, a, nullptr, L, L, fuse_stats ? st1 : nullptr);
    if (!fuse_stats) add([=](hipStream_t s) { return launch_gn_stats(dt, a, Bn, L, rp->cout, g, st1, s, ln, sh); });
    add([=](hipStream_t s) {
      if (item_t)
        return launch_gn_apply(dt, a, b, nullptr, Bn, L, rp->cout, g, st1, rp->g1, rp->b1, ss_tab, ss_stride, item_t, ACT_SILU, s, nullptr,
                               nullptr, 0, ln, sh, kItemStateInts, n_t);
      return launch_gn_apply(dt, a, b, nullptr, Bn, L, rp->cout, g, st1, rp->g1, rp->b1, cur_ss + rp->ss_off,
                             0, nullptr, ACT_SILU, s, nullptr, nullptr, f8 ? 1 : 0, ln, sh);
    }, false, 0, LDC_CLASS_GN_APPLY, (f8 ? 1.5 : 2.0) * Bn * L * rp->cout * es);
  }
  void* xn = nullptr;
  const bool xn_made = ln_g && xn_out && c->fuse_ln && !ln && gn_apply_ln_fusable(r.cout);
  if (xn_made) {
    xn = xn_fp8 ? ar->alloc((size_t)rows * r.cout) : act(rows, r.cout);
    *xn_out = xn;
  }
  if (trace) {
    ResnetTrace& tr = *trace;
    tr = ResnetTrace();
    tr.epi1 = epi1; tr.epi2 = epi2; tr.folded = folded; tr.fuse_stats = fuse_stats; tr.xn = xn_made;
    tr.rowstat = epi2 && rowstat_wanted && !f8;
    conv_bm(c1, L, L, false, tr.t1);   // (as the gate above asks: the tile shape of the launched layer)
    conv_bm(f8 ? r.c2_f8 : r.c2, L, L, false, tr.t2);
    tr.b = b; tr.a = a; tr.d = d; tr.st1 = st1; tr.st2 = st2;
    tr.part1 = (char*)ge1.part; tr.part2 = (char*)ge2.part; tr.mslots1 = ge1.mslots; tr.mslots2 = ge2.mslots;
  }
  if (epi2) {   // block2: conv -> GroupNorm -> SiLU -> + res (-> tanh), one launch; the PreNorm LayerNorm of a following attention block reads `out`
    ge2.gamma = r.g2; ge2.beta = r.b2; ge2.ss = nullptr; ge2.out = out_mode & 5;
    if (rowstat_wanted && !f8) ge2.rowstat = last_rowstat = (float*)ar->alloc((size_t)rows * (r.cout / 32) * 8);
    if (r.has_res && !folded) mark(3);
    conv(f8 ? r.c2_f8 : r.c2, b, nullptr, out, res, L, L, nullptr, nullptr, 0, 0, 0, &ge2);
    if (xn) {
      const int C = r.cout;
      add([=](hipStream_t s) { return launch_ln_rows(dt, out, xn, nullptr, ln_g, rows, C, s, xn_fp8 ? 1 : 0); }, false, 0, LDC_CLASS_LAYERNORM,
          (xn_fp8 ? 1.5 : 2.0) * rows * C * es);
    }
    return out;
  }
  conv(f8 ? r.c2_f8 : r.c2, b, nullptr, d, nullptr, L, L, fuse_stats ? st2 : nullptr);
  if (!fuse_stats) add([=](hipStream_t s) { return launch_gn_stats(dt, d, Bn, L, rp->cout, g, st2, s, ln, sh); });
  if (r.has_res && !folded) mark(3);
  const int out8_ln = ((xn && xn_fp8) ? 2 : 0) | (gn_apply_fp8_ok(r.cout) ? out_mode : 0);
  add([=](hipStream_t s) {
    return launch_gn_apply(dt, d, out, res, Bn, L, rp->cout, g, st2, rp->g2, rp->b2, nullptr, 0, nullptr, ACT_SILU, s, xn, ln_g, out8_ln, ln, sh);
  }, false, 0, LDC_CLASS_GN_APPLY, (xn ? 4.0 : 3.0) * Bn * L * rp->cout * es);
  return out;
}
bool PlanBuilder::qkv_fp8(const LinAttnW& a) const { return c->w8 && c->fp8_act && a.qkv_f8.w != nullptr; }
bool PlanBuilder::ln_foldable(const LinAttnW& a, int L) {
  if (pl->ragged || !c->fold_ln || !c->fuse_gn_epi || c->w8 || !a.qkv_ln.w || L < c->gn_epi_min_l) return false;
  int t[4];
  conv_bm(a.qkv_ln, L, L, false, t);
  return t[0] > 0;
}
void* PlanBuilder::attention(const LinAttnW& a, const void* x, int L, bool linear, void* xn_pre) {
  const int rows = B * L, dt = c->dt, Bn = B;
  const int H = c->unet.heads, Dh = c->unet.dim_head, hid = H * Dh;
  const bool f8 = qkv_fp8(a);
  const bool lnf = !xn_pre && ln_foldable(a, L);     // LayerNorm inside to_qkv: the conv reads x itself
  const float* rowstat = lnf ? last_rowstat : nullptr;   // (sum, sumsq) partials of x's rows left by the ResnetBlock in front, if it could
  last_rowstat = nullptr;
  void* xn = lnf ? const_cast<void*>(x) : (xn_pre ? xn_pre : (f8 ? ar->alloc((size_t)rows * a.dim) : act(rows, a.dim)));
  const ConvLayer& qkv_ly = lnf ? a.qkv_ln : (f8 ? a.qkv_f8 : a.qkv);
  void* qkv = act(rows, 3 * hid);
  void* o = act(rows, hid);
  void* out = act(rows, a.dim);
  const LinAttnW* ap = &a;
  const int* ln = lens();
  const int sh = ln ? level(L) : 0;
  // one workspace per LinearAttention layer when the k column-max is fused: all of them are zeroed by the
  // step's single memset (they sit behind the GroupNorm statistics)
  // (a ragged plan too: its workspaces are cleared with the step's accumulators, so that its step graphs hold kernel nodes only)
  float* ws = (linear && (c->fuse_kmax || ln)) ? linattn_ws + (size_t)(linattn_used++) * B * linattn_ws_floats_per_item(H, Dh) : linattn_ws;
  if (!xn_pre && !lnf)
    add([=](hipStream_t s) { return launch_ln_rows(dt, x, xn, nullptr, ap->norm_g, rows, ap->dim, s, f8 ? 1 : 0, ln, sh, L); }, false, 0, LDC_CLASS_LAYERNORM,
        2.0 * rows * a.dim * es);
  if (linear) {
    const size_t wss = linattn_ws_floats_per_item(H, Dh);
    if (!ln && c->fuse_kmax && c->fuse_attn_tail && !a.out.w8 && linattn_tail_supported(dt, H, Dh, a.dim)) {
      // three launches: qkv conv (+ k column max) -> context -> tail (out, to_out conv, LayerNorm, + x); round 6: TWO where to_qkv
      // accumulates the context itself (lean kernel, bf16, folded PreNorm: ConvCall::qkv_ctx_ws)
      ln_rowstat_next = rowstat;
      if (lnf && c->fold_ctx && c->tune.lean && !c->tune.force_generic && dt == DT_BF16 && a.qkv_ctx.w && hid == 128 && a.dim % 64 == 0) {
        qkv_ctx_next = ws; qkv_ctx_stride_next = (int)wss;
        conv(a.qkv_ctx, xn, nullptr, qkv, nullptr, L, L);
      } else {
        conv(qkv_ly, xn, nullptr, qkv, nullptr, L, L, nullptr, reinterpret_cast<unsigned*>(ws), hid, 2 * hid, (int)wss);
        add([=](hipStream_t s) { return launch_linattn_ctx(dt, qkv, ws, Bn, L, H, Dh, s); }, false, 0, LDC_CLASS_LINATTN, 2.0 * rows * hid * es);
      }
      const int dim = a.dim;
      info = "tail_c" + std::to_string(dim) + "_L" + std::to_string(L) + "_B" + std::to_string(B);
      unsigned* flag = c->dev_flag_dev;
      add([=](hipStream_t s) {
        return launch_linattn_tail(dt, qkv, ws, ap->out.w, ap->out.n_pad, ap->out.bias, ap->out_g, x, out, Bn, L, H, Dh, dim, flag, s);
      }, false, 2.0 * rows * hid * dim, LDC_CLASS_LINATTN, (1.0 * hid + 2.0 * dim) * rows * es);
      return out;
    }
    if (c->fuse_kmax && !ln) {
      ln_rowstat_next = rowstat;
      conv(qkv_ly, xn, nullptr, qkv, nullptr, L, L, nullptr, reinterpret_cast<unsigned*>(ws), hid, 2 * hid, (int)wss);
      add([=](hipStream_t s) { return launch_linattn(dt, qkv, o, ws, Bn, L, H, Dh, true, s); }, false, 0, LDC_CLASS_LINATTN,
          4.0 * rows * hid * es);
    } else {
      ln_rowstat_next = rowstat;
      conv(qkv_ly, xn, nullptr, qkv, nullptr, L, L);
      add([=](hipStream_t s) { return launch_linattn(dt, qkv, o, ws, Bn, L, H, Dh, false, s, ln, sh, ln != nullptr); }, false, 0, LDC_CLASS_LINATTN,
          5.0 * rows * hid * es);
    }
    void* t = act(rows, a.dim);
    conv(a.out, o, nullptr, t, nullptr, L, L);
    add([=](hipStream_t s) { return launch_ln_rows(dt, t, out, x, ap->out_g, rows, ap->dim, s, 0, ln, sh, L); }, false, 0, LDC_CLASS_LAYERNORM,
        3.0 * rows * a.dim * es);
  } else {
    ln_rowstat_next = rowstat;
    conv(qkv_ly, xn, nullptr, qkv, nullptr, L, L);
    add([=](hipStream_t s) { return launch_attn_full(dt, qkv, o, Bn, L, H, Dh, s, ln, sh); }, false, 0, LDC_CLASS_ATTN_FULL, 4.0 * rows * hid * es);
    conv(a.out, o, nullptr, out, x, L, L);   // + x in the epilogue
    mask(out, L, a.dim);                     // (to_out's bias)
  }
  return out;
}
void* PlanBuilder::resnet_then_attention(const ResnetW& r, const LinAttnW& a, const void* x1, const void* x2, int L, bool linear, void** resnet_out) {
  void* xn = nullptr;
  void* y;
  if (ln_foldable(a, L)) { want_rowstat = true; y = resnet(r, x1, x2, L); }
  else y = resnet(r, x1, x2, L, a.norm_g, &xn, qkv_fp8(a));
  if (resnet_out) *resnet_out = y;
  return attention(a, y, L, linear, xn);
}
void* PlanBuilder::final_block(const ResnetW& r, const void* x1, const void* x2, int L, bool f8) {
  const int dim = c->unet.dim, dt = c->dt;
  if (gn_apply_fp8_ok(dim)) return resnet(r, x1, x2, L, nullptr, nullptr, false, 4 | (f8 ? 1 : 0));
  const void* xin = resnet(r, x1, x2, L);
  void* tb = f8 ? ar->alloc((size_t)B * L * dim) : act(B * L, dim);
  const int64_t n = (int64_t)B * L * dim;
  const size_t esz = es;
  add([=](hipStream_t s) { return launch_act(dt, xin, tb, n, ACT_TANH, s, f8 ? 1 : 0); }, false, 0, LDC_CLASS_ELEMENTWISE, (f8 ? 1.5 : 2.0) * n * esz);
  return tb;
}
float* PlanBuilder::take_zero_region(int n_gn, size_t n_lin, bool lin_cleared, size_t sx_bytes) {
  const UnetW& u = c->unet;
  const ZeroRegion z = zero_region_layout(n_gn, B, u.groups, pl->part_bytes, n_lin, (size_t)B * linattn_ws_floats_per_item(u.heads, u.dim_head) * 4,
                                          lin_cleared, sx_bytes);
  char* base = (char*)ar->alloc(z.alloc_bytes);
  stats_pool = (float*)base;
  sk_count = reinterpret_cast<unsigned*>(base + z.sk_count);
  sk_count_cap = kSkTilesCap;
  part_pool = base + z.part;
  part_cap = z.part_cap;
  linattn_ws = reinterpret_cast<float*>(base + z.lin);
  pl->zero_ptr = base;   // cleared by the step's first kernel (launch_step_begin): no memset node of its own
  pl->zero_bytes = z.zero_bytes;
  sk_part_cap = pl->sk_floats;   // sized from the convs' own needs by the sizing passes (plan_passes)
  sk_part = (float*)ar->alloc((size_t)std::max<long long>(sk_part_cap, 4) * 4);
  return reinterpret_cast<float*>(base + z.sx);
}

int build_plan(ldc_ctx* c, Plan* pl, Arena& ar, int B, int L, int F) {
  const UnetW& u = c->unet;
  pl->B = B; pl->L = L; pl->F = F; pl->init_pc = nullptr;
  pl->reset_build();
  const int dt = c->dt;
  const size_t es = dt_size(dt);
  const int Cc = u.cond_channels, Cx = u.channels;
  PlanBuilder pb{c, pl, &ar, B, es};
  const int n_gn = 2 * (int)(2 * u.downs.size() + 2 + 2 * u.ups.size() + 1);
  const bool lin_zeroed = c->fuse_kmax || pl->ragged;   // one LinearAttention workspace per layer, inside the region the step's first kernel clears
  const size_t sx_bytes = c->cfg.unet_scale_x ? (size_t)B * 4 : 0;   // per-item max|cat(cond, x)| of --unet_scale_x
  float* sx_max = pb.take_zero_region(n_gn, lin_zeroed ? u.downs.size() + u.ups.size() : 1, lin_zeroed, sx_bytes);
  pl->maxabs = (float*)ar.alloc((size_t)B * 4);
  pl->step_state = (int*)ar.alloc(64);
  if (ar.base) pl->zero_once.push_back({pl->step_state, 64});   // [4] = the epoch of the UNet pass (launch_step_begin counts it up)
  pl->kst = c->kstamps ? (unsigned long long*)ar.alloc((size_t)2048 * kKstOps * 2 * 8) : nullptr;
  pl->cur_ss = (float*)ar.alloc((size_t)std::max(1, u.ss_stride) * 4);
  pl->x_cl = ar.alloc((size_t)B * L * Cx * es);
  pl->eps_cl = ar.alloc((size_t)B * L * Cx * es);
  pl->cond_cl = ar.alloc((size_t)B * L * Cc * es);
  if (pl->items && !pl->ragged) return fail(LDC_E_INVALID, "a per-item plan is a ragged plan");
  pl->item_state = pl->items ? (ItemState*)ar.alloc((size_t)B * sizeof(ItemState)) : nullptr;
  if (pl->ragged) {
    if (c->w8) return fail(LDC_E_INVALID, "ragged batches are not available on the fp8 engine (its fused forms have no length-aware variant): use dtype bf16 or f32");
    pl->lens = (int*)ar.alloc((size_t)B * 4);
    pl->flens = (int*)ar.alloc((size_t)B * 4);
  } else {
    pl->lens = pl->flens = nullptr;
  }
  // ---- process_cond (unet.py:407-420): fp32 upsampler, per-item max-abs, cast to the UNet dtype ----
  void* cond_in = ar.alloc((size_t)B * F * Cc * 4);
  pl->cond_in_cl = cond_in;
  {
    const void* x = cond_in;
    int Lc = F;
    const int Bn0 = B;
    const int *rl = pl->ragged ? pl->lens : nullptr, *rf = pl->ragged ? pl->flens : nullptr;
    // ragged: the upsampler sees zeros behind an item's last frame (whatever the caller's padding holds) ...
    if (rf) pl->cond_ops.push_back([=](hipStream_t s) { return launch_mask_rows(DT_F32, cond_in, Bn0, F, Cc, rf, 0, s); });
    for (const ConvLayer& ly : u.upsamplers) {
      ConvCall cc;
      cc.B = B; cc.L_in = Lc; cc.L_rows = Lc + 1; cc.L_final = Lc * ly.tr_stride; cc.y_ld = ly.tr_cout; cc.x1 = x; cc.tune = &c->tune;
      void* y = ar.alloc((size_t)B * cc.L_final * ly.tr_cout * 4);
      cc.y = y;
      const ConvLayer* lp = &ly;
      pl->cond_ops.push_back([lp, cc](hipStream_t s) { return launch_conv(*lp, cc, s); });
      // ... and EVERY layer's output is cut to the item's length: the upsampler's transposed convs are not causal (their trim is
      // symmetric), so what a layer leaves behind an item's end (its bias) would reach back into the item through the next layer.
      // An item's rows of a layer's output are F_b rows of (positions per frame x channels) values.  The per-item maximum below then
      // runs over the item's own frames, and the condition is zero in the padding
      if (rf) {
        const int row = cc.L_final / F * ly.tr_cout;
        pl->cond_ops.push_back([=](hipStream_t s) { return launch_mask_rows(DT_F32, y, Bn0, F, row, rf, 0, s); });
      }
      x = y;
      Lc = cc.L_final;
    }
    (void)rl;
    if (Lc != L) return fail(LDC_E_INVALID, "upsampled condition length %d != latent length %d (F=%d, upsampling product %d)", Lc, L, F, upsample_factor(c));
    float* mx = pl->maxabs;
    void* cond_cl = pl->cond_cl;
    const bool scale = c->cfg.unet_scale_cond != 0;
    const int Bn = B;
    const int64_t npi = (int64_t)L * Cc;
    // fp32 rows -> (scaled) rows in the UNet dtype.  A [rows][C] fp32 -> dt copy is a "transpose" of a
    // [B][C=1][L*C] tensor: reuse to_cl with C=1 (pure cast + scale).
    if (scale) {
      pl->cond_ops.push_back([=](hipStream_t s) { return hipMemsetAsync(mx, 0, (size_t)Bn * 4, s); });
      pl->cond_ops.push_back([=](hipStream_t s) { return launch_maxabs(DT_F32, x, Bn, npi, 1, mx, s); });
      pl->cond_ops.push_back([=](hipStream_t s) { return launch_to_cl(dt, (const float*)x, cond_cl, Bn, 1, (int)npi, mx, 1, 1e-20f, s); });
    } else {
      pl->cond_ops.push_back([=](hipStream_t s) { return launch_to_cl(dt, (const float*)x, cond_cl, Bn, 1, (int)npi, nullptr, 0, 0.f, s); });
    }
  }
  pl->taps["cond_proc"] = {pl->cond_cl, Cc, L};
  // ---- Unet1D.forward (unet.py:430-469) ----
  const void* in_cond = pl->cond_cl;
  const void* in_x = pl->x_cl;
  if (c->cfg.unet_scale_x) {
    // unet.py:432-433: x = cat(cond, x) / (max|.| per item + 1e-20).  The max runs over both halves of the concatenation;
    // the two scaled copies feed init_conv as its two inputs.
    void* cs = ar.alloc((size_t)B * L * Cc * es);
    void* xs = ar.alloc((size_t)B * L * Cx * es);
    const void* cin = pl->cond_cl; const void* xin = pl->x_cl;
    const int Bn = B;
    const int64_t nc = (int64_t)L * Cc, nx = (int64_t)L * Cx;
    pb.add([=](hipStream_t s) { return launch_maxabs(dt, cin, Bn, nc, 1, sx_max, s); });
    pb.add([=](hipStream_t s) { return launch_maxabs(dt, xin, Bn, nx, 1, sx_max, s); });
    pb.add([=](hipStream_t s) { return launch_scale_copy(dt, cin, cs, Bn, nc, sx_max, 1e-20f, s); }, false, 0, LDC_CLASS_ELEMENTWISE, 2.0 * B * nc * es);
    pb.add([=](hipStream_t s) { return launch_scale_copy(dt, xin, xs, Bn, nx, sx_max, 1e-20f, s); }, false, 0, LDC_CLASS_ELEMENTWISE, 2.0 * B * nx * es);
    in_cond = cs; in_x = xs;
  }
  void* x0 = pb.act(B * L, u.dim);
  if (c->split_init && !c->w8 && !c->cfg.unet_scale_x && u.init_c.w && u.init_x.w) {
    // the condition's half of init_conv once per sampler call (behind process_cond), the x half + that tensor every step
    void* pc = pb.act(B * L, u.dim);
    pl->init_pc = pc;
    {
      ConvCall cc;
      cc.B = B; cc.L_in = L; cc.L_rows = L; cc.x1 = pl->cond_cl; cc.y = pc; cc.y_ld = u.init_c.n; cc.tune = &c->tune;
      const ConvLayer* lp = &u.init_c;
      pl->cond_ops.push_back([lp, cc](hipStream_t s) { return launch_conv(*lp, cc, s); });
    }
    pb.conv(u.init_x, in_x, nullptr, x0, pc, L, L);
  } else {
    pb.conv(u.init, in_cond, in_x, x0, nullptr, L, L);
  }
  pb.mask(x0, L, u.dim);
  pl->taps["init"] = {x0, u.dim, L};
  const void* x = x0;
  int Lc = L;
  std::vector<std::pair<const void*, int>> hs;
  for (size_t i = 0; i < u.downs.size(); ++i) {
    const LevelW& lv = u.downs[i];
    x = pb.resnet(lv.b1, x, nullptr, Lc); hs.push_back({x, Lc});
    x = pb.resnet_then_attention(lv.b2, lv.attn, x, nullptr, Lc, true); hs.push_back({x, Lc});
    int Ln = Lc;
    if (lv.kind == 0) Ln = (Lc + 2 - 4) / 2 + 1;
    void* y = pb.act(B * Ln, lv.cout);
    pb.conv(lv.resample, x, nullptr, y, nullptr, Lc, Ln);
    pb.mask(y, Ln, lv.cout);
    x = y; Lc = Ln;
    pl->taps["down" + std::to_string(i)] = {y, lv.cout, Lc};
  }
  x = pb.resnet_then_attention(u.mid1, u.mid_attn, x, nullptr, Lc, false);
  x = pb.resnet(u.mid2, x, nullptr, Lc);
  pl->taps["mid"] = {const_cast<void*>(x), u.dims.back(), Lc};
  for (size_t i = 0; i < u.ups.size(); ++i) {
    const LevelW& lv = u.ups[i];
    if (hs.back().second != Lc) return fail(LDC_E_INVALID, "latent length %d is not divisible by 2^%zu", L, u.downs.size() - 1);
    x = pb.resnet(lv.b1, x, hs.back().first, Lc); hs.pop_back();
    x = pb.resnet_then_attention(lv.b2, lv.attn, x, hs.back().first, Lc, true); hs.pop_back();
    const int Ln = lv.kind == 1 ? 2 * Lc : Lc;
    void* y = pb.act(B * Ln, lv.cout);
    pb.conv(lv.resample, x, nullptr, y, nullptr, Lc, Ln);
    pb.mask(y, Ln, lv.cout);
    x = y; Lc = Ln;
    pl->taps["up" + std::to_string(i)] = {y, lv.cout, Lc};
  }
  if (Lc != L) return fail(LDC_E_INVALID, "latent length %d does not survive the down/up path (got %d)", L, Lc);
  {   // final ResnetBlock -> tanh -> final_conv (unet.py:465-469), the tanh in fp8 when final_conv runs fp8 x fp8
    const bool f8 = c->w8 && c->fp8_act && u.final_conv_f8.w != nullptr;
    const void* th = pb.final_block(u.fin, x, x0, L, f8);
    pb.conv(f8 ? u.final_conv_f8 : u.final_conv, th, nullptr, pl->eps_cl, nullptr, L, L);
  }
  return LDC_OK;
}

// Drop plan `idx` (and every captured graph of its (L, F)): waits for the device first, nothing of it may be running.
static void evict_plan(ldc_ctx* c, size_t idx) {
  (void)counted_device_sync();
  const Plan* pl = c->plans[idx].get();   // (its DPM and windows graphs carry the plan's L and F too)
  drop_step_graphs(c, [pl](const StepGraph& g) { return g.key.L == pl->L && g.key.F == pl->F && g.key.pool_id == pl->pool_id; });
  release_plan(c, idx);
}

int get_plan(ldc_ctx* c, int B, int L, int F, int slot, hipStream_t s, Plan** out, bool ragged, bool items, int pool_id, const std::vector<int>* win_lens,
             int win_O) {
  static const std::vector<int> no_group;
  const std::vector<int>& wgl = win_lens ? *win_lens : no_group;   // a windows plan: the ORDERED list of its recordings' lengths is part of the key (with L, its effective Lw)
  for (auto& p : c->plans)
    if (p->B == B && p->L == L && p->F == F && p->slot == slot && p->ragged == ragged && p->items == items && p->pool_id == pool_id &&
        p->win_O == win_O && p->win_group.Ltot == wgl) {
      p->last_use = ++c->use_tick;
      *out = p.get();
      return LDC_OK;
    }
  std::unique_ptr<Plan> pl(new Plan());
  pl->ragged = ragged;
  pl->items = items;
  pl->pool_id = pool_id;
  pl->win_O = win_O;
  pl->win_group.Ltot = wgl;   // (the rest of the group's tables: windows_prepare)
  for (int l : wgl) pl->win_Ltot += l;
  if (win_lens) pl->win_id = c->next_win_id++;
  auto alloc = [&](size_t want, void** base) {
    // LRU eviction: plans of the call being served (last_use > call_tick) are never candidates
    for (;;) {
      const bool over = c->plan_bytes + want > c->plan_bytes_cap || (int)c->plans.size() >= c->plan_count_cap;
      if (!over) break;
      size_t victim = c->plans.size();
      for (size_t i = 0; i < c->plans.size(); ++i)
        if (c->plans[i]->pool_id == 0 && c->plans[i]->last_use <= c->call_tick && (victim == c->plans.size() || c->plans[i]->last_use < c->plans[victim]->last_use)) victim = i;
      if (victim == c->plans.size()) break;   // everything cached belongs to this call: let hipMalloc decide
      evict_plan(c, victim);
    }
    hipError_t e = hipMalloc(base, want);
    if (e != hipSuccess) return fail(LDC_E_NOMEM, "hipMalloc(%zu) for the UNet workspace failed: %s", want, hipGetErrorString(e));
    return (int)LDC_OK;
  };
  void* base = nullptr;
  size_t want = 0;
  LDCCHK(plan_passes(pl.get(), false, [&](Arena& ar) { return build_plan(c, pl.get(), ar, B, L, F); }, alloc, [](void* p) { (void)hipFree(p); }, &base, &want));
  for (const auto& z : pl->zero_once) {   // the step state's epoch word: cleared once, before the plan's first use
    hipError_t ez = hipMemsetAsync(z.first, 0, z.second, s);
    if (ez != hipSuccess) { (void)hipFree(base); return fail(LDC_E_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(ez)); }
  }
  pl->arena_base = base;
  pl->arena_bytes = want;
  pl->slot = slot;
  pl->last_use = ++c->use_tick;
  c->plan_bytes += want;
  *out = pl.get();
  c->plans.push_back(std::move(pl));
  (void)s;
  return LDC_OK;
}

int run_ops(ldc_ctx* c, Plan* pl, bool is_step, hipStream_t s) {
  const bool use_side = is_step && !c->profile && c->side_streams;
  hipStream_t side = c->side_stream[pl->slot];
  if (use_side && pl->marker_events.empty()) {
    size_t nm = 0;
    for (const Plan::StepOp& op : pl->step) nm += (op.where >= 2);
    for (size_t k = 0; k < nm; ++k) {
      hipEvent_t e = nullptr;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      pl->marker_events.push_back(e);
    }
  }
  size_t marker = 0;
  const size_t n_ops = is_step ? pl->step.size() : pl->cond_ops.size();
  for (size_t i = 0; i < n_ops; ++i) {
    const bool prof = c->profile && is_step;
    const int where = is_step ? pl->step[i].where : 0;
    if (where == 2) {
      if (use_side) {
        hipEvent_t e = pl->marker_events[marker];
        HIPCHK(hipEventRecord(e, s));
        HIPCHK(hipStreamWaitEvent(side, e, 0));
      }
      ++marker;
      continue;
    }
    if (where == 3) {
      if (use_side) {
        hipEvent_t e = pl->marker_events[marker];
        HIPCHK(hipEventRecord(e, side));
        HIPCHK(hipStreamWaitEvent(s, e, 0));
      }
      ++marker;
      continue;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (prof) {
      HIPCHK(hipEventCreate(&e0));
      HIPCHK(hipEventCreate(&e1));
      HIPCHK(hipEventRecord(e0, s));
    }
    {
      const hipError_t oe = (is_step ? pl->step[i].fn : pl->cond_ops[i])((use_side && where == 1) ? side : s);
      if (oe != hipSuccess) {
        (void)hipGetLastError();
        return fail(LDC_E_HIP, "%s op %zu (%s) failed: %s", is_step ? "step" : "cond", i, is_step ? pl->step[i].info.c_str() : "-", hipGetErrorString(oe));
      }
    }
    if (prof) {
      HIPCHK(hipEventRecord(e1, s));
      c->prof_events.push_back({e0, e1});
      c->prof_event_flops.push_back(pl->step[i].flops);
      c->prof_event_class.push_back(pl->step[i].cls);
      c->prof_event_bytes.push_back(pl->step[i].bytes);
      c->prof_event_info.push_back(pl->step[i].info + "_B" + std::to_string(pl->B));
    }
  }
  return LDC_OK;
}
