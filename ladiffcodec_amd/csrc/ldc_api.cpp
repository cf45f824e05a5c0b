// ldc_api.cpp -- context, weight folding/packing, codec stages, the decode front ends and the C ABI (UNet plans: unet_plan.cpp)
// declared in include/ladiffcodec.h.  Host-side C++ only; every kernel lives in the .hip files.
//
// Mapping to the reference (haiciyang/LaDiffCodec):
//   Ctx::codec[*]    <- DiffAudioRep.encoder / .decoder / .quantizer      (srcs/model.py:52-66)
//   Ctx::unet        <- DiffAudioRep.diff_model = Unet1D                  (srcs/model.py:74, modules/unet.py:250-469)
//   Ctx::sched       <- GaussianDiffusion1D registered buffers            (srcs/losses/ddpm_loss.py:138-168)
//   ldc_denoise      <- GaussianDiffusion1D.halfway_sampling              (srcs/losses/ddpm_loss.py:370-385)
#include "ldc_internal.h"

long long g_device_syncs = 0;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char* ldc_last_error(void) { return g_err; }
extern "C" const char* ldc_version(void) { return "ladiffcodec-amd 0.1 (gfx950)"; }


// ------------------------------------------------------------------------------------------------
// weight access + folding
// ------------------------------------------------------------------------------------------------

// w = g * v / ||v||  per dim-0 slice  (torch weight_norm, dim=0; reference conv.py:27-30)
static std::vector<float> fold_weight_norm(const HostTensor& g, const HostTensor& v) {
  const size_t n0 = (size_t)v.shape[0], inner = v.numel() / n0;
  std::vector<float> w(v.numel());
  for (size_t i = 0; i < n0; ++i) {
    double s = 0;
    for (size_t j = 0; j < inner; ++j) s += (double)v.data[i * inner + j] * v.data[i * inner + j];
    const float nrm = (float)sqrt(s);
    const float sc = g.data[i] / nrm;
    for (size_t j = 0; j < inner; ++j) w[i * inner + j] = v.data[i * inner + j] * sc;
  }
  return w;
}

// weight standardisation, fp32 branch: (w - mean) * rsqrt(var + 1e-5), biased var per out channel (unet.py:73-78)
static std::vector<float> fold_weight_std(const HostTensor& wt) {
  const size_t n0 = (size_t)wt.shape[0], inner = wt.numel() / n0;
  std::vector<float> w(wt.numel());
  for (size_t i = 0; i < n0; ++i) {
    double s = 0;
    for (size_t j = 0; j < inner; ++j) s += wt.data[i * inner + j];
    const double mean = s / (double)inner;
    double v = 0;
    for (size_t j = 0; j < inner; ++j) {
      const double d = wt.data[i * inner + j] - mean;
      v += d * d;
    }
    const float fmean = (float)mean;
    const float rs = 1.0f / sqrtf((float)(v / (double)inner) + 1e-5f);
    for (size_t j = 0; j < inner; ++j) w[i * inner + j] = (wt.data[i * inner + j] - fmean) * rs;
  }
  return w;
}


// the column form of gn_apply (norm_act.hip) is the one that can write fp8

int make_conv(ldc_ctx* c, const ConvSpec& sp, const float* w_oik, const float* bias, ConvLayer* out) {
  ConvLayer ly;
  ly.dt = sp.dt;
  ly.cin1 = sp.cin1; ly.cin2 = sp.cin2;
  const int bke = 64 / (int)dt_size(sp.dt);
  if (sp.cin1 % bke || sp.cin2 % bke)
    return fail(LDC_E_INVALID, "conv input channels (%d,%d) must be multiples of %d for this dtype", sp.cin1, sp.cin2, bke);
  ly.n = sp.cout;
  ly.bn = conv_pick_bn(sp.cout);
  ly.n_pad = (sp.cout + ly.bn - 1) / ly.bn * ly.bn;
  ly.taps = sp.k; ly.stride = sp.stride; ly.dil = sp.dil; ly.pad_left = sp.pad_left; ly.ups = sp.ups;
  ly.pad_mode = sp.pad_mode; ly.pre_act = sp.pre_act; ly.post_act = sp.post_act;
  ly.flops_per_row = 2.0 * (sp.cin1 + sp.cin2) * sp.k * sp.cout;
  ly.w8 = (c->w8 && sp.dt == DT_BF16 && !sp.no_w8) ? 1 : 0;
  std::vector<char> packed(conv_packed_weight_bytes(ly));
  if (sp.dt == DT_FP8) {
    std::vector<float> scales((size_t)sp.cout);
    pack_conv_weights_fp8act(ly, w_oik, packed.data(), scales.data());
    LDCCHK(c->wmem.upload(&ly.wscale, scales));
  } else if (ly.w8) {
    std::vector<float> scales((size_t)sp.cout);
    pack_conv_weights_fp8(ly, w_oik, packed.data(), scales.data());
    LDCCHK(c->wmem.upload(&ly.wscale, scales));
  } else {
    pack_conv_weights(ly, w_oik, packed.data());
  }
  void* dw = nullptr;
  LDCCHK(c->wmem.alloc(&dw, packed.size()));
  HIPCHK(hipMemcpy(dw, packed.data(), packed.size(), hipMemcpyHostToDevice));
  ly.w = dw;
  if (bias) {
    std::vector<float> b(bias, bias + sp.cout);
    LDCCHK(c->wmem.upload(&ly.bias, b));
  }
  *out = ly;
  return LDC_OK;
}

// ConvTranspose1d(k = 2*stride) as a 2-tap conv over q with N = stride*Cout (see conv_gemm.hip)
int make_convtr(ldc_ctx* c, int dt, int cin, int cout, int stride, int trim_left, int pre_act, const float* w_iok,
                       const float* bias, ConvLayer* out) {
  ConvLayer ly;
  ly.dt = dt;
  ly.cin1 = cin; ly.cin2 = 0;
  const int bke = 64 / (int)dt_size(dt);
  if (cin % bke) return fail(LDC_E_INVALID, "convtr input channels %d must be a multiple of %d", cin, bke);
  ly.n = stride * cout;
  ly.bn = conv_pick_bn(ly.n);
  ly.n_pad = (ly.n + ly.bn - 1) / ly.bn * ly.bn;
  ly.taps = 2; ly.stride = 1; ly.dil = 1; ly.pad_left = 1; ly.ups = 0; ly.pad_mode = PAD_ZERO;
  ly.pre_act = pre_act; ly.post_act = ACT_NONE;
  ly.tr_stride = stride; ly.tr_cout = cout; ly.tr_trim_left = trim_left;
  ly.flops_per_row = 2.0 * cin * 2 * ly.n;
  std::vector<char> packed(conv_packed_weight_bytes(ly));
  pack_convtr_weights(ly, w_iok, cin, cout, stride, packed.data());
  void* dw = nullptr;
  LDCCHK(c->wmem.alloc(&dw, packed.size()));
  HIPCHK(hipMemcpy(dw, packed.data(), packed.size(), hipMemcpyHostToDevice));
  ly.w = dw;
  std::vector<float> b((size_t)ly.n, 0.f);
  if (bias)
    for (int p = 0; p < stride; ++p)
      for (int co = 0; co < cout; ++co) b[(size_t)p * cout + co] = bias[co];
  LDCCHK(c->wmem.upload(&ly.bias, b));
  *out = ly;
  return LDC_OK;
}

// ------------------------------------------------------------------------------------------------
// SEANet construction (reference srcs/modules/seanet.py:108-151, 200-244)
// ------------------------------------------------------------------------------------------------
static int build_wn_conv(ldc_ctx* c, WeightReader& wr, const std::string& p, int cin, int cout, int k, int stride, int dil,
                         int pre_act, ConvLayer* out) {
  HostTensor* b = wr.get(p + ".bias", {cout});
  HostTensor* g = wr.get(p + ".weight_g", {cout, 1, 1});
  HostTensor* v = wr.get(p + ".weight_v", {cout, cin, k});
  if (!b || !g || !v) return LDC_OK;   // reported later through wr.missing
  std::vector<float> w = fold_weight_norm(*g, *v);
  ConvSpec sp;
  sp.dt = DT_F32; sp.cin1 = cin; sp.cout = cout; sp.k = k; sp.stride = stride; sp.dil = dil;
  sp.pad_left = (k - 1) * dil - (stride - 1);   // causal: all padding on the left (conv.py:222-226)
  sp.pad_mode = PAD_REFLECT; sp.pre_act = pre_act;
  return make_conv(c, sp, w.data(), b->data.data(), out);
}

int build_lstm(ldc_ctx* c, WeightReader& wr, const std::string& p, int H, int layers, std::vector<LstmLayer>* out) {
  for (int n = 0; n < layers; ++n) {
    const std::string s = std::to_string(n);
    HostTensor* wih = wr.get(p + ".lstm.weight_ih_l" + s, {4 * H, H});
    HostTensor* whh = wr.get(p + ".lstm.weight_hh_l" + s, {4 * H, H});
    HostTensor* bih = wr.get(p + ".lstm.bias_ih_l" + s, {4 * H});
    HostTensor* bhh = wr.get(p + ".lstm.bias_hh_l" + s, {4 * H});
    if (!wih || !whh || !bih || !bhh) continue;
    LstmLayer L;
    std::vector<float> bias(4 * H);
    for (int i = 0; i < 4 * H; ++i) bias[i] = bih->data[i] + bhh->data[i];
    ConvSpec sp;
    sp.dt = DT_F32; sp.cin1 = H; sp.cout = 4 * H; sp.k = 1;
    LDCCHK(make_conv(c, sp, wih->data.data(), bias.data(), &L.in_proj));
    if (H == 64 || H == 128) {
      LDCCHK(c->wmem.upload(&L.w_hh, whh->data));
    } else {
      // k-major [H/4][4H][4] for the streaming kernel
      std::vector<float> km((size_t)4 * H * H);
      for (int row = 0; row < 4 * H; ++row)
        for (int k = 0; k < H; ++k) km[((size_t)(k / 4) * 4 * H + row) * 4 + (k % 4)] = whh->data[(size_t)row * H + k];
      LDCCHK(c->wmem.upload(&L.w_hh, km));
      if (lstm_coop_eligible(H)) LDCCHK(c->wmem.upload(&L.w_rm, whh->data));
    }
    out->push_back(L);
  }
  return LDC_OK;
}

static int build_res(ldc_ctx* c, WeightReader& wr, const std::string& p, int dim, int dil, SeaOp* op) {
  op->kind = SeaOp::RES;
  op->cin = op->cout = dim;
  op->hidden = dim / 2;
  LDCCHK(build_wn_conv(c, wr, p + ".block.1.conv.conv", dim, dim / 2, 3, 1, dil, ACT_ELU, &op->conv));
  LDCCHK(build_wn_conv(c, wr, p + ".block.3.conv.conv", dim / 2, dim, 1, 1, 1, ACT_ELU, &op->conv2));
  LDCCHK(build_wn_conv(c, wr, p + ".shortcut.conv.conv", dim, dim, 1, 1, 1, ACT_NONE, &op->shortcut));
  return LDC_OK;
}

static int build_codec(ldc_ctx* c, int which, const std::vector<int>& ratios, int n_q_layers, std::string* missing) {
  Codec& cd = c->codec[which];
  cd = Codec();
  cd.ratios = ratios;
  cd.hop = 1;
  for (int r : ratios) cd.hop *= r;
  const int nf = c->cfg.n_filters, D = c->cfg.rep_dims, nres = c->cfg.n_residual_layers, nl = c->cfg.lstm;
  WeightReader wr{c, which, ""};
  // ---- encoder ----
  {
    int idx = 0, mult = 1;
    SeaOp first;
    first.kind = SeaOp::CONV_CIN1; first.cin = 1; first.cout = nf; first.k = 7;
    {
      const std::string p = "encoder.model.0.conv.conv";
      HostTensor* b = wr.get(p + ".bias", {nf});
      HostTensor* g = wr.get(p + ".weight_g", {nf, 1, 1});
      HostTensor* v = wr.get(p + ".weight_v", {nf, 1, 7});
      if (b && g && v) {
        std::vector<float> w = fold_weight_norm(*g, *v);
        LDCCHK(c->wmem.upload(&first.w1, w));
        LDCCHK(c->wmem.upload(&first.b1, b->data));
      }
    }
    cd.enc.push_back(first);
    idx = 1;
    std::vector<int> rev(ratios.rbegin(), ratios.rend());
    for (int ratio : rev) {
      const int ch = mult * nf;
      for (int j = 0; j < nres; ++j) {
        SeaOp op;
        int dil = 1;
        for (int q = 0; q < j; ++q) dil *= 2;
        LDCCHK(build_res(c, wr, "encoder.model." + std::to_string(idx), ch, dil, &op));
        cd.enc.push_back(op);
        ++idx;
      }
      ++idx;   // ELU
      SeaOp op;
      op.kind = SeaOp::CONV; op.cin = ch; op.cout = 2 * ch; op.k = 2 * ratio; op.stride = ratio;
      LDCCHK(build_wn_conv(c, wr, "encoder.model." + std::to_string(idx) + ".conv.conv", ch, 2 * ch, 2 * ratio, ratio, 1,
                           ACT_ELU, &op.conv));
      cd.enc.push_back(op);
      ++idx;
      mult *= 2;
    }
    const int ch = mult * nf;
    bool pre = false;
    if (nl) {
      SeaOp op;
      op.kind = SeaOp::LSTM; op.cin = op.cout = ch;
      LDCCHK(build_lstm(c, wr, "encoder.model." + std::to_string(idx), ch, nl, &op.lstm));
      cd.enc.push_back(op);
      ++idx;
    }
    (void)pre;
    ++idx;   // ELU
    SeaOp op;
    op.kind = SeaOp::CONV; op.cin = ch; op.cout = D; op.k = 7;
    LDCCHK(build_wn_conv(c, wr, "encoder.model." + std::to_string(idx) + ".conv.conv", ch, D, 7, 1, 1, ACT_ELU, &op.conv));
    op.conv.post_act = c->enc_final_act;   // SEANetEncoder(final_activation=...) (seanet.py:144-149): both encoders get it
    cd.enc.push_back(op);
  }
  // ---- decoder ----
  {
    int idx = 0;
    int mult = 1 << ratios.size();
    SeaOp op0;
    op0.kind = SeaOp::CONV; op0.cin = D; op0.cout = mult * nf; op0.k = 7;
    LDCCHK(build_wn_conv(c, wr, "decoder.model.0.conv.conv", D, mult * nf, 7, 1, 1, ACT_NONE, &op0.conv));
    cd.dec.push_back(op0);
    idx = 1;
    if (nl) {
      SeaOp op;
      op.kind = SeaOp::LSTM; op.cin = op.cout = mult * nf;
      LDCCHK(build_lstm(c, wr, "decoder.model.1", mult * nf, nl, &op.lstm));
      cd.dec.push_back(op);
      idx = 2;
    }
    for (int ratio : ratios) {
      const int ch = mult * nf;
      ++idx;   // ELU
      SeaOp op;
      op.kind = SeaOp::CONVTR; op.cin = ch; op.cout = ch / 2; op.k = 2 * ratio; op.stride = ratio;
      {
        const std::string p = "decoder.model." + std::to_string(idx) + ".convtr.convtr";
        HostTensor* b = wr.get(p + ".bias", {ch / 2});
        HostTensor* g = wr.get(p + ".weight_g", {ch, 1, 1});
        HostTensor* v = wr.get(p + ".weight_v", {ch, ch / 2, 2 * ratio});
        if (b && g && v) {
          std::vector<float> w = fold_weight_norm(*g, *v);
          // causal: trim everything (k - s = s) on the right (conv.py:263-268) -> trim_left = 0
          LDCCHK(make_convtr(c, DT_F32, ch, ch / 2, ratio, 0, ACT_ELU, w.data(), b->data.data(), &op.conv));
        }
      }
      cd.dec.push_back(op);
      ++idx;
      for (int j = 0; j < nres; ++j) {
        SeaOp r;
        int dil = 1;
        for (int q = 0; q < j; ++q) dil *= 2;
        LDCCHK(build_res(c, wr, "decoder.model." + std::to_string(idx), ch / 2, dil, &r));
        cd.dec.push_back(r);
        ++idx;
      }
      mult /= 2;
    }
    ++idx;   // ELU
    SeaOp last;
    last.kind = SeaOp::CONV; last.cin = nf; last.cout = 1; last.k = 7;
    LDCCHK(build_wn_conv(c, wr, "decoder.model." + std::to_string(idx) + ".conv.conv", nf, 1, 7, 1, 1, ACT_ELU, &last.conv));
    cd.dec.push_back(last);
  }
  // ---- RVQ ----
  cd.n_q_layers = n_q_layers;
  if (n_q_layers > 0) {
    std::vector<float> all((size_t)n_q_layers * cd.bins * D);
    bool ok = true;
    for (int q = 0; q < n_q_layers; ++q) {
      const std::string p = "quantizer.vq.layers." + std::to_string(q) + "._codebook";
      HostTensor* e = wr.get(p + ".embed", {cd.bins, D});
      wr.get(p + ".inited", {1});
      wr.get(p + ".cluster_size", {cd.bins});
      wr.get(p + ".embed_avg", {cd.bins, D});
      if (!e) { ok = false; continue; }
      memcpy(all.data() + (size_t)q * cd.bins * D, e->data.data(), (size_t)cd.bins * D * sizeof(float));
    }
    if (ok) {
      LDCCHK(c->wmem.upload(&cd.codebooks, all));
      void* p = nullptr;
      LDCCHK(c->wmem.alloc(&p, (size_t)n_q_layers * cd.bins * sizeof(float)));
      cd.cb_sqnorm = reinterpret_cast<float*>(p);
      HIPCHK(launch_sqnorm_rows(cd.codebooks, n_q_layers * cd.bins, D, cd.cb_sqnorm, c->own_stream));
      HIPCHK(hipStreamSynchronize(c->own_stream));
    }
  }
  cd.present = true;
  *missing += wr.missing;
  return LDC_OK;
}

// ------------------------------------------------------------------------------------------------
// Unet1D construction (reference srcs/modules/unet.py:307-377)
// ------------------------------------------------------------------------------------------------
static int build_resnet(ldc_ctx* c, WeightReader& wr, const std::string& p, int cin1, int cin2, int cout, ResnetW* r) {
  const int cin = cin1 + cin2;
  r->cin1 = cin1; r->cin2 = cin2; r->cout = cout;
  HostTensor* w1 = wr.get(p + ".block1.proj.weight", {cout, cin, 3});
  HostTensor* b1 = wr.get(p + ".block1.proj.bias", {cout});
  HostTensor* g1 = wr.get(p + ".block1.norm.weight", {cout});
  HostTensor* be1 = wr.get(p + ".block1.norm.bias", {cout});
  HostTensor* w2 = wr.get(p + ".block2.proj.weight", {cout, cout, 3});
  HostTensor* b2 = wr.get(p + ".block2.proj.bias", {cout});
  HostTensor* g2 = wr.get(p + ".block2.norm.weight", {cout});
  HostTensor* be2 = wr.get(p + ".block2.norm.bias", {cout});
  wr.get(p + ".mlp.1.weight", {2 * cout, c->unet.time_dim});
  wr.get(p + ".mlp.1.bias", {2 * cout});
  r->has_res = cin != cout;
  HostTensor *wr_ = nullptr, *br_ = nullptr;
  if (r->has_res) {
    wr_ = wr.get(p + ".res_conv.weight", {cout, cin, 1});
    br_ = wr.get(p + ".res_conv.bias", {cout});
  }
  if (!w1 || !b1 || !g1 || !be1 || !w2 || !b2 || !g2 || !be2 || (r->has_res && (!wr_ || !br_))) return LDC_OK;
  ConvSpec sp;
  sp.dt = c->dt; sp.cin1 = cin1; sp.cin2 = cin2; sp.cout = cout; sp.k = 3; sp.pad_left = 1;
  {
    std::vector<float> w = fold_weight_std(*w1);
    LDCCHK(make_conv(c, sp, w.data(), b1->data.data(), &r->c1));
  }
  {
    std::vector<float> w = fold_weight_std(*w2);
    ConvSpec s2 = sp;
    s2.cin1 = cout; s2.cin2 = 0;
    LDCCHK(make_conv(c, s2, w.data(), b2->data.data(), &r->c2));
    if (c->w8 && c->fp8_act && c->dt == DT_BF16 && cout % 64 == 0 && gn_apply_fp8_ok(cout)) {
      s2.dt = DT_FP8; s2.act8 = 1;
      LDCCHK(make_conv(c, s2, w.data(), b2->data.data(), &r->c2_f8));
    }
  }
  if (r->has_res) {
    ConvSpec s3 = sp;
    s3.k = 1; s3.pad_left = 0;
    LDCCHK(make_conv(c, s3, wr_->data.data(), br_->data.data(), &r->res));
    if (!c->w8) {
      // res_conv folded into block1's conv (both read x, unet.py:171,189-192): a packed image with four slabs per channel
      // chunk -- the three taps of the standardised block1 weight and the 1x1 res_conv weight (ConvLayer::wtaps)
      const std::vector<float> w = fold_weight_std(*w1);
      std::vector<float> w4((size_t)cout * cin * 4);
      for (size_t oc = 0; oc < (size_t)cout * cin; ++oc) {
        w4[oc * 4 + 0] = w[oc * 3 + 0]; w4[oc * 4 + 1] = w[oc * 3 + 1]; w4[oc * 4 + 2] = w[oc * 3 + 2];
        w4[oc * 4 + 3] = wr_->data[oc];
      }
      ConvSpec s4 = sp;
      s4.k = 4;
      LDCCHK(make_conv(c, s4, w4.data(), b1->data.data(), &r->c1r));
      r->c1r.taps = 3; r->c1r.wtaps = 4; r->c1r.bias2 = r->res.bias;
      r->c1r.flops_per_row = r->c1.flops_per_row + r->res.flops_per_row;
    }
  }
  LDCCHK(c->wmem.upload(&r->g1, g1->data));
  LDCCHK(c->wmem.upload(&r->b1, be1->data));
  LDCCHK(c->wmem.upload(&r->g2, g2->data));
  LDCCHK(c->wmem.upload(&r->b2, be2->data));
  c->unet.weight_elems += (double)w1->numel() + w2->numel() + (wr_ ? wr_->numel() : 0);
  return LDC_OK;
}

static int build_attn(ldc_ctx* c, WeightReader& wr, const std::string& p, int dim, bool linear, LinAttnW* a) {
  const int hidden = c->unet.heads * c->unet.dim_head;
  a->dim = dim;
  HostTensor* ng = wr.get(p + ".fn.norm.g", {1, dim, 1});
  HostTensor* wq = wr.get(p + ".fn.fn.to_qkv.weight", {3 * hidden, dim, 1});
  HostTensor* wo = wr.get(p + (linear ? ".fn.fn.to_out.0.weight" : ".fn.fn.to_out.weight"), {dim, hidden, 1});
  HostTensor* bo = wr.get(p + (linear ? ".fn.fn.to_out.0.bias" : ".fn.fn.to_out.bias"), {dim});
  HostTensor* og = linear ? wr.get(p + ".fn.fn.to_out.1.g", {1, dim, 1}) : nullptr;
  if (!ng || !wq || !wo || !bo || (linear && !og)) return LDC_OK;
  ConvSpec sq;
  sq.dt = c->dt; sq.cin1 = dim; sq.cout = 3 * hidden; sq.k = 1;
  LDCCHK(make_conv(c, sq, wq->data.data(), nullptr, &a->qkv));
  if (c->w8 && c->fp8_act && c->dt == DT_BF16 && dim % 64 == 0 && dim <= 1024) {
    sq.dt = DT_FP8; sq.act8 = 1;
    LDCCHK(make_conv(c, sq, wq->data.data(), nullptr, &a->qkv_f8));
    sq.dt = c->dt; sq.act8 = 0;
  }
  if (!c->w8) {
    // PreNorm folded into to_qkv: W' = W diag(g); ln_s[n] = sum_c W'[n][c] of the weight AS THE MFMA SEES IT (bf16-rounded in the
    // bf16 engine), so that rstd * (W' x - mean * ln_s) equals W' ((x - mean) * rstd) up to fp32 rounding
    const int N3 = 3 * hidden;
    std::vector<float> w2((size_t)N3 * dim), sn((size_t)N3);
    auto as_packed = [&](float v) {
      if (c->dt != DT_BF16) return v;
      uint32_t u;
      memcpy(&u, &v, 4);
      u += 0x7fffu + ((u >> 16) & 1u);       // round to nearest even (finite weights)
      u &= 0xffff0000u;
      float r;
      memcpy(&r, &u, 4);
      return r;
    };
    for (int n = 0; n < N3; ++n) {
      double acc = 0;
      for (int k = 0; k < dim; ++k) {
        const float v = wq->data[(size_t)n * dim + k] * ng->data[k];
        w2[(size_t)n * dim + k] = v;
        acc += (double)as_packed(v);
      }
      sn[n] = (float)acc;
    }
    LDCCHK(make_conv(c, sq, w2.data(), nullptr, &a->qkv_ln));
    LDCCHK(c->wmem.upload(&a->qkv_ln.ln_s, sn));
    if (linear && c->dt == DT_BF16 && hidden == 128 && c->unet.dim_head == 32) {
      // the same layer with its output channels ordered q | (k_h v_h) x heads: a 64-column tile then holds k and v of ONE head (context fold)
      std::vector<float> wp((size_t)N3 * dim), sp((size_t)N3);
      for (int n = 0; n < N3; ++n) {
        int src = n;
        if (n >= hidden) {
          const int t = n - hidden, h = t / 64, w = t % 64;
          src = (w < 32 ? hidden : 2 * hidden) + h * 32 + (w & 31);
        }
        memcpy(&wp[(size_t)n * dim], &w2[(size_t)src * dim], (size_t)dim * sizeof(float));
        sp[n] = sn[src];
      }
      LDCCHK(make_conv(c, sq, wp.data(), nullptr, &a->qkv_ctx));
      LDCCHK(c->wmem.upload(&a->qkv_ctx.ln_s, sp));
    }
  }
  ConvSpec so;
  so.dt = c->dt; so.cin1 = hidden; so.cout = dim; so.k = 1;
  LDCCHK(make_conv(c, so, wo->data.data(), bo->data.data(), &a->out));
  LDCCHK(c->wmem.upload(&a->norm_g, ng->data));
  if (og) LDCCHK(c->wmem.upload(&a->out_g, og->data));
  c->unet.weight_elems += (double)wq->numel() + wo->numel();
  return LDC_OK;
}

static int build_plain_conv(ldc_ctx* c, WeightReader& wr, const std::string& p, int cin1, int cin2, int cout, int k,
                            int stride, int pad, int ups, ConvLayer* out) {
  HostTensor* w = wr.get(p + ".weight", {cout, cin1 + cin2, k});
  HostTensor* b = wr.get(p + ".bias", {cout});
  if (!w || !b) return LDC_OK;
  ConvSpec sp;
  sp.dt = c->dt; sp.cin1 = cin1; sp.cin2 = cin2; sp.cout = cout; sp.k = k; sp.stride = stride; sp.pad_left = pad; sp.ups = ups;
  c->unet.weight_elems += (double)w->numel();
  return make_conv(c, sp, w->data.data(), b->data.data(), out);
}

static int build_time_table(ldc_ctx* c, WeightReader& wr);

static int build_unet(ldc_ctx* c, std::string* missing) {
  UnetW& u = c->unet;
  u = UnetW();
  u.dim = c->cfg.diff_dims;
  u.time_dim = 4 * u.dim;
  u.channels = c->cfg.rep_dims;
  u.cond_channels = 128;
  static const int mults[5] = {1, 2, 2, 4, 4};   // DiffAudioRep fixes dim_mults=(1,2,2,4,4) (model.py:74)
  u.dims.push_back(u.dim);
  for (int m : mults) u.dims.push_back(u.dim * m);
  WeightReader wr{c, LDC_MODEL_MAIN, ""};
  const std::string P = "diff_model";
  LDCCHK(build_plain_conv(c, wr, P + ".init_conv", u.cond_channels, u.channels, u.dim, 7, 1, 3, 0, &u.init));
  {
    // init_conv(cat(cond, x)) = W_c * cond + b  +  W_x * x (unet.py:434): the processed condition does not change over the denoise steps, so its
    // half of the contraction is evaluated once per sampler call (init_c, with the bias) and every step runs only the x half (init_x) and adds it
    HostTensor* w = wr.get(P + ".init_conv.weight", {u.dim, u.cond_channels + u.channels, 7});
    HostTensor* b = wr.get(P + ".init_conv.bias", {u.dim});
    if (w && b) {
      const int Cc = u.cond_channels, Cx = u.channels, Ct = Cc + Cx;
      std::vector<float> wc((size_t)u.dim * Cc * 7), wx((size_t)u.dim * Cx * 7);
      for (int o = 0; o < u.dim; ++o) {
        for (int i = 0; i < Cc; ++i) for (int k = 0; k < 7; ++k) wc[((size_t)o * Cc + i) * 7 + k] = w->data[((size_t)o * Ct + i) * 7 + k];
        for (int i = 0; i < Cx; ++i) for (int k = 0; k < 7; ++k) wx[((size_t)o * Cx + i) * 7 + k] = w->data[((size_t)o * Ct + Cc + i) * 7 + k];
      }
      ConvSpec sc;
      sc.dt = c->dt; sc.cin1 = Cc; sc.cout = u.dim; sc.k = 7; sc.stride = 1; sc.pad_left = 3;
      LDCCHK(make_conv(c, sc, wc.data(), b->data.data(), &u.init_c));
      sc.cin1 = Cx;
      LDCCHK(make_conv(c, sc, wx.data(), nullptr, &u.init_x));
    }
  }
  const int nlev = (int)u.dims.size() - 1;
  int ss_off = 0;
  auto take_ss = [&](ResnetW& r) { r.ss_off = ss_off; ss_off += 2 * r.cout; };
  for (int i = 0; i < nlev; ++i) {
    const int din = u.dims[i], dout = u.dims[i + 1];
    const bool last = i >= nlev - 1;
    LevelW lv;
    const std::string p = P + ".downs." + std::to_string(i);
    LDCCHK(build_resnet(c, wr, p + ".0", din, 0, din, &lv.b1)); take_ss(lv.b1);
    LDCCHK(build_resnet(c, wr, p + ".1", din, 0, din, &lv.b2)); take_ss(lv.b2);
    LDCCHK(build_attn(c, wr, p + ".2", din, true, &lv.attn));
    lv.kind = last ? 2 : 0; lv.cin = din; lv.cout = dout;
    if (last) LDCCHK(build_plain_conv(c, wr, p + ".3", din, 0, dout, 3, 1, 1, 0, &lv.resample));
    else LDCCHK(build_plain_conv(c, wr, p + ".3", din, 0, dout, 4, 2, 1, 0, &lv.resample));
    u.downs.push_back(lv);
  }
  const int mid = u.dims.back();
  LDCCHK(build_resnet(c, wr, P + ".mid_block1", mid, 0, mid, &u.mid1)); take_ss(u.mid1);
  LDCCHK(build_attn(c, wr, P + ".mid_attn", mid, false, &u.mid_attn));
  LDCCHK(build_resnet(c, wr, P + ".mid_block2", mid, 0, mid, &u.mid2)); take_ss(u.mid2);
  for (int i = 0; i < nlev; ++i) {
    const int din = u.dims[nlev - 1 - i], dout = u.dims[nlev - i];
    const bool last = i == nlev - 1;
    LevelW lv;
    const std::string p = P + ".ups." + std::to_string(i);
    LDCCHK(build_resnet(c, wr, p + ".0", dout, din, dout, &lv.b1)); take_ss(lv.b1);
    LDCCHK(build_resnet(c, wr, p + ".1", dout, din, dout, &lv.b2)); take_ss(lv.b2);
    LDCCHK(build_attn(c, wr, p + ".2", dout, true, &lv.attn));
    lv.kind = last ? 2 : 1; lv.cin = dout; lv.cout = din;
    if (last) LDCCHK(build_plain_conv(c, wr, p + ".3", dout, 0, din, 3, 1, 1, 0, &lv.resample));
    else LDCCHK(build_plain_conv(c, wr, p + ".3.1", dout, 0, din, 3, 1, 1, 1, &lv.resample));
    u.ups.push_back(lv);
  }
  LDCCHK(build_resnet(c, wr, P + ".final_res_block", u.dim, u.dim, u.dim, &u.fin)); take_ss(u.fin);
  LDCCHK(build_plain_conv(c, wr, P + ".final_conv", u.dim, 0, u.channels, 1, 1, 0, 0, &u.final_conv));
  if (c->w8 && c->fp8_act && c->dt == DT_BF16 && u.dim % 64 == 0) {
    HostTensor* w = wr.get(P + ".final_conv.weight", {u.channels, u.dim, 1});
    HostTensor* b = wr.get(P + ".final_conv.bias", {u.channels});
    if (w && b) {
      ConvSpec sp;
      sp.dt = DT_FP8; sp.act8 = 1; sp.cin1 = u.dim; sp.cout = u.channels; sp.k = 1;
      LDCCHK(make_conv(c, sp, w->data.data(), b->data.data(), &u.final_conv_f8));
    }
  }
  u.ss_stride = ss_off;
  // cond upsampler: non-causal SConvTranspose1d(k=2r, s=r), no weight-norm (unet.py:372-377, conv.py:270-273)
  for (int i = 0; i < c->cfg.n_upsampling_ratios; ++i) {
    const int r = c->cfg.upsampling_ratios[i];
    const std::string p = P + ".upsampling_layers." + std::to_string(i) + ".convtr.convtr";
    HostTensor* w = wr.get(p + ".weight", {u.cond_channels, u.cond_channels, 2 * r});
    HostTensor* b = wr.get(p + ".bias", {u.cond_channels});
    u.up_ratios.push_back(r);
    if (!w || !b) continue;
    ConvLayer ly;
    const int padding_total = r, right = padding_total / 2, left = padding_total - right;
    LDCCHK(make_convtr(c, DT_F32, u.cond_channels, u.cond_channels, r, left, ACT_NONE, w->data.data(), b->data.data(), &ly));
    u.upsamplers.push_back(ly);
  }
  // schedule buffers come from the checkpoint (they are registered buffers, ddpm_loss.py:138-168)
  static const char* names[13] = {"betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                                  "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod",
                                  "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                                  "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
                                  "p2_loss_weight"};
  std::map<std::string, float*> dev;
  for (const char* n : names) {
    HostTensor* t = wr.get(std::string("diffusion.") + n, {u.timesteps});
    if (!t) continue;
    float* d = nullptr;
    LDCCHK(c->wmem.upload(&d, t->data));
    dev[n] = d;
    if (std::string(n) == "alphas_cumprod") c->alphas_cumprod = t->data;
    if (std::string(n) == "sqrt_recip_alphas_cumprod") c->sqrt_recip_ac = t->data;
    if (std::string(n) == "sqrt_recipm1_alphas_cumprod") c->sqrt_recipm1_ac = t->data;
  }
  c->sched.sqrt_recip_alphas_cumprod = dev["sqrt_recip_alphas_cumprod"];
  c->sched.sqrt_recipm1_alphas_cumprod = dev["sqrt_recipm1_alphas_cumprod"];
  c->sched.posterior_mean_coef1 = dev["posterior_mean_coef1"];
  c->sched.posterior_mean_coef2 = dev["posterior_mean_coef2"];
  c->sched.posterior_log_variance_clipped = dev["posterior_log_variance_clipped"];
  c->sqrt_alphas_cumprod = dev["sqrt_alphas_cumprod"];
  c->sqrt_one_minus_alphas_cumprod = dev["sqrt_one_minus_alphas_cumprod"];
  c->p2_loss_weight = dev["p2_loss_weight"];
  if (wr.missing.empty()) LDCCHK(build_time_table(c, wr));
  *missing += wr.missing;
  return LDC_OK;
}

// SinusoidalPosEmb + time_mlp + every ResnetBlock.mlp evaluated for all t = 0..T-1 at load time
// (they depend on t only; reference unet.py:109-116, 327-332, 162-165, 183-186).  fp32 on the GPU,
// through the same conv-GEMM kernel (a Linear is a k=1 conv over T "positions").
static int build_time_table(ldc_ctx* c, WeightReader& wr) {
  UnetW& u = c->unet;
  const int T = u.timesteps, dim = u.dim, td = u.time_dim;
  const std::string P = "diff_model";
  HostTensor* w1 = wr.get(P + ".time_mlp.1.weight", {td, dim});
  HostTensor* b1 = wr.get(P + ".time_mlp.1.bias", {td});
  HostTensor* w2 = wr.get(P + ".time_mlp.3.weight", {td, td});
  HostTensor* b2 = wr.get(P + ".time_mlp.3.bias", {td});
  if (!w1 || !b1 || !w2 || !b2) return LDC_OK;
  const int half = dim / 2;
  std::vector<float> emb((size_t)T * dim);
  const float lg = logf(10000.0f) / (float)(half - 1);
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < half; ++k) {
      const float f = expf((float)k * -lg);
      const float a = (float)t * f;
      emb[(size_t)t * dim + k] = sinf(a);
      emb[(size_t)t * dim + half + k] = cosf(a);
    }
  DevMem tmp;
  float *d_emb = nullptr, *d_h1 = nullptr, *d_h2 = nullptr;
  LDCCHK(tmp.upload(&d_emb, emb));
  void* p = nullptr;
  LDCCHK(tmp.alloc(&p, (size_t)T * td * 4)); d_h1 = (float*)p;
  LDCCHK(tmp.alloc(&p, (size_t)T * td * 4)); d_h2 = (float*)p;
  LDCCHK(c->wmem.alloc(&p, (size_t)T * u.ss_stride * 4));
  u.ss_table = (float*)p;
  LDCCHK(c->wmem.alloc(&p, (size_t)u.ss_stride * 4));
  u.cur_ss = (float*)p;
  hipStream_t s = c->own_stream;
  ConvLayer l1, l2;
  ConvSpec sp;
  sp.dt = DT_F32; sp.cin1 = dim; sp.cout = td; sp.k = 1; sp.post_act = ACT_GELU;
  LDCCHK(make_conv(c, sp, w1->data.data(), b1->data.data(), &l1));
  sp.cin1 = td; sp.post_act = ACT_SILU;   // SiLU of ResnetBlock.mlp[0] folded here: every block consumes SiLU(temb)
  LDCCHK(make_conv(c, sp, w2->data.data(), b2->data.data(), &l2));
  ConvCall cc;
  cc.B = 1; cc.L_in = T; cc.L_rows = T;
  cc.x1 = d_emb; cc.y = d_h1; cc.y_ld = td;
  HIPCHK(launch_conv(l1, cc, s));
  cc.x1 = d_h1; cc.y = d_h2;
  HIPCHK(launch_conv(l2, cc, s));
  std::vector<ResnetW*> blocks;
  for (auto& lv : u.downs) { blocks.push_back(&lv.b1); blocks.push_back(&lv.b2); }
  blocks.push_back(&u.mid1); blocks.push_back(&u.mid2);
  for (auto& lv : u.ups) { blocks.push_back(&lv.b1); blocks.push_back(&lv.b2); }
  blocks.push_back(&u.fin);
  std::vector<std::string> prefixes;
  for (size_t i = 0; i < u.downs.size(); ++i) { prefixes.push_back(P + ".downs." + std::to_string(i) + ".0"); prefixes.push_back(P + ".downs." + std::to_string(i) + ".1"); }
  prefixes.push_back(P + ".mid_block1"); prefixes.push_back(P + ".mid_block2");
  for (size_t i = 0; i < u.ups.size(); ++i) { prefixes.push_back(P + ".ups." + std::to_string(i) + ".0"); prefixes.push_back(P + ".ups." + std::to_string(i) + ".1"); }
  prefixes.push_back(P + ".final_res_block");
  for (size_t i = 0; i < blocks.size(); ++i) {
    ResnetW* r = blocks[i];
    HostTensor* wm = wr.get(prefixes[i] + ".mlp.1.weight", {2 * r->cout, td});
    HostTensor* bm = wr.get(prefixes[i] + ".mlp.1.bias", {2 * r->cout});
    if (!wm || !bm) continue;
    ConvLayer lm;
    ConvSpec sm;
    sm.dt = DT_F32; sm.cin1 = td; sm.cout = 2 * r->cout; sm.k = 1;
    LDCCHK(make_conv(c, sm, wm->data.data(), bm->data.data(), &lm));
    ConvCall cm;
    cm.B = 1; cm.L_in = T; cm.L_rows = T; cm.x1 = d_h2; cm.y = u.ss_table + r->ss_off; cm.y_ld = u.ss_stride;
    HIPCHK(launch_conv(lm, cm, s));
    u.weight_elems += (double)wm->numel();
  }
  HIPCHK(hipStreamSynchronize(s));
  return LDC_OK;
}

// ------------------------------------------------------------------------------------------------
// lifecycle
// ------------------------------------------------------------------------------------------------
extern "C" int ldc_create(const ldc_config* cfg, int device, ldc_ctx** out) {
  if (!cfg || !out) return fail(LDC_E_INVALID, "null argument");
  if (cfg->compute_dtype != LDC_F32 && cfg->compute_dtype != LDC_BF16 && cfg->compute_dtype != LDC_BF16_W8)
    return fail(LDC_E_INVALID, "compute_dtype must be LDC_F32, LDC_BF16 or LDC_BF16_W8");
  if (cfg->n_enc_ratios < 1 || cfg->n_enc_ratios > LDC_MAX_RATIOS || cfg->n_upsampling_ratios < 0 ||
      cfg->n_upsampling_ratios > LDC_MAX_RATIOS)
    return fail(LDC_E_INVALID, "bad ratio counts");
  if (cfg->rep_dims != 128) return fail(LDC_E_INVALID, "rep_dims must be 128 (RVQ / UNet channel width of the reference checkpoints)");
  if (cfg->diff_dims % 32 || cfg->diff_dims <= 0) return fail(LDC_E_INVALID, "diff_dims must be a positive multiple of 32");
  if (cfg->n_filters % 32) return fail(LDC_E_INVALID, "n_filters must be a multiple of 32");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(LDC_E_INVALID, "device %d out of range (%d visible)", device, ndev);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(LDC_E_INVALID, "this library is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
  std::unique_ptr<ldc_ctx> c(new ldc_ctx());
  c->cfg = *cfg;
  c->device = device;
  c->num_cus = prop.multiProcessorCount;
  c->dt = cfg->compute_dtype == LDC_F32 ? DT_F32 : DT_BF16;
  c->w8 = cfg->compute_dtype == LDC_BF16_W8;
  HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  for (int k = 0; k < kMaxParts; ++k)
    for (int e = 0; e <= ldc_ctx::kLstmChunks; ++e) HIPCHK(hipEventCreateWithFlags(&c->lstm_ev[k][e], hipEventDisableTiming));
  if (const char* ex = getenv("LDC_TEST_EXTRA_STREAMS")) {   // test hook: shift the stream -> hardware-queue mapping the way other libraries' streams would
    for (int i = 0; i < atoi(ex); ++i) { hipStream_t dummy = nullptr; HIPCHK(hipStreamCreateWithFlags(&dummy, hipStreamNonBlocking)); }
  }
  HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  for (auto& e : c->flow_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (int k = 1; k < kMaxParts; ++k) {
    HIPCHK(hipStreamCreateWithFlags(&c->aux_stream[k], hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_join[k], hipEventDisableTiming));
  }
  for (int k = 0; k < kMaxParts; ++k) {
    HIPCHK(hipStreamCreateWithFlags(&c->side_stream[k], hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_side_fork[k], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_side_join[k], hipEventDisableTiming));
  }
  // Every knob of the library is an OPTION (one table: find_option below; tools/README.md lists them): ldc_set_option at run time, or
  // LDC_OPTIONS="name=value,name=value" in the environment at ldc_create (round 6: ~50 separate LDC_* variables before).
  c->xcd_resident[0] = lstm_xcd_resident(256);
  c->xcd_resident[1] = lstm_xcd_resident(512);
  c->coop_resident[0] = lstm_coop_resident(256) ? 1 : 0;
  c->coop_resident[1] = lstm_coop_resident(512) ? 1 : 0;
  c->plan_bytes_cap = (size_t)48 << 30;
  c->plan_count_cap = 24;
  if (const char* mp = getenv("LDC_AUX_FROM_SIDE")) {   // diagnostics (hardware-queue mapping): part stream k = side stream digit k of the value ('-' keeps it)
    c->calib = 0;
    for (int k = 1; k < kMaxParts && mp[k - 1]; ++k)
      if (mp[k - 1] >= '0' && mp[k - 1] < '0' + kMaxParts) std::swap(c->aux_stream[k], c->side_stream[mp[k - 1] - '0']);
  }
  if (const char* ov = getenv("LDC_OPTIONS")) {
    std::string all(ov);
    size_t pos = 0;
    while (pos < all.size()) {
      size_t end = all.find_first_of(",; ", pos);
      if (end == std::string::npos) end = all.size();
      const std::string kv = all.substr(pos, end - pos);
      pos = end + 1;
      if (kv.empty()) continue;
      const size_t eq = kv.find('=');
      const std::string name = kv.substr(0, eq);
      const int value = eq == std::string::npos ? 1 : atoi(kv.c_str() + eq + 1);
      std::unique_ptr<ldc_ctx>& cc = c;
      const int rc = ldc_set_option(cc.get(), name.c_str(), value);
      if (rc != LDC_OK) return fail(LDC_E_INVALID, "LDC_OPTIONS: %s", ldc_last_error());
    }
  }
  switch (cfg->final_activation) {
    case LDC_ACT_NONE: c->enc_final_act = ACT_NONE; break;
    case LDC_ACT_TANH: c->enc_final_act = ACT_TANH; break;
    case LDC_ACT_SIGMOID: c->enc_final_act = ACT_SIGMOID; break;
    case LDC_ACT_ELU: c->enc_final_act = ACT_ELU; break;
    case LDC_ACT_SILU: c->enc_final_act = ACT_SILU; break;
    case LDC_ACT_GELU: c->enc_final_act = ACT_GELU; break;
    case LDC_ACT_RELU: c->enc_final_act = ACT_RELU; break;
    default: return fail(LDC_E_INVALID, "final_activation code %d is not one of LDC_ACT_*", cfg->final_activation);
  }
  {
    void* hp = nullptr;
    HIPCHK(hipHostMalloc(&hp, 64, hipHostMallocMapped));
    memset(hp, 0, 64);
    c->dev_flag_host = (unsigned*)hp;
    void* dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, hp, 0));
    c->dev_flag_dev = (unsigned*)dp;
  }
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, 4 * sizeof(int)));
  c->step_state = (int*)p;
  *out = c.release();
  return LDC_OK;
}

void free_plan_resources(Plan* pl) {
  for (hipEvent_t e : pl->marker_events) (void)hipEventDestroy(e);
  if (pl->arena_base) (void)hipFree(pl->arena_base);
  if (pl->x0_prev) (void)hipFree(pl->x0_prev);     // (every captured DPM graph of the plan has gone before)
  if (pl->item_keys) (void)hipFree(pl->item_keys); // (likewise every seeded graph)
  if (pl->win_base) (void)hipFree(pl->win_base);   // (likewise every windows graph)
}

void release_plan(ldc_ctx* c, size_t idx) {
  Plan* pl = c->plans[idx].get();
  for (int k = 0; k < c->last_halves.n; ++k)
    if (c->last_halves.p[k] == pl) c->last_halves = Halves();
  free_plan_resources(pl);
  c->plan_bytes -= pl->arena_bytes;
  c->plans.erase(c->plans.begin() + idx);
}

void drop_plans(ldc_ctx* c) {
  (void)counted_device_sync();   // nothing captured or planned may still be running when it is destroyed
  drop_step_graphs(c, [](const StepGraph&) { return true; });
  for (auto& pl : c->plans) free_plan_resources(pl.get());
  c->plans.clear();
  c->plan_bytes = 0;
  c->last_halves = Halves();
}

extern "C" int ldc_destroy(ldc_ctx* c) {
  if (!c) return LDC_OK;
  (void)hipSetDevice(c->device);
  (void)counted_device_sync();
  drop_plans(c);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->outnorm_ws) (void)hipFree(c->outnorm_ws);
  if (c->state_buf) (void)hipFree(c->state_buf);
  if (c->ddim_table) (void)hipFree(c->ddim_table);
  if (c->dpm_table) (void)hipFree(c->dpm_table);
  if (c->step_state) (void)hipFree(c->step_state);
  if (c->dev_flag_host) (void)hipHostFree(c->dev_flag_host);
  if (c->tl_buf) (void)hipFree(c->tl_buf);
  for (auto& e : c->prof_events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  for (int k = 0; k < kMaxParts; ++k) {
    for (int e = 0; e <= ldc_ctx::kLstmChunks; ++e)
      if (c->lstm_ev[k][e]) (void)hipEventDestroy(c->lstm_ev[k][e]);
  }
  for (auto& e : c->flow_ev) if (e) (void)hipEventDestroy(e);
  for (int k = 1; k < kMaxParts; ++k) {
    if (c->ev_join[k]) (void)hipEventDestroy(c->ev_join[k]);
    if (c->aux_stream[k]) (void)hipStreamDestroy(c->aux_stream[k]);
  }
  for (int k = 0; k < kMaxParts; ++k) {
    if (c->ev_side_fork[k]) (void)hipEventDestroy(c->ev_side_fork[k]);
    if (c->ev_side_join[k]) (void)hipEventDestroy(c->ev_side_join[k]);
    if (c->side_stream[k]) (void)hipStreamDestroy(c->side_stream[k]);
  }
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return LDC_OK;
}

// OCP e4m3 quantisation exactly as the fp8 weight packer applies it (host function: testable without a GPU)
extern "C" void ldc_quantize_e4m3(const float* in, int64_t n, uint8_t* out_codes, float* out_values) {
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t q = host_f32_to_e4m3(in[i]);
    if (out_codes) out_codes[i] = q;
    if (out_values) out_values[i] = host_e4m3_to_f32(q);
  }
}

// ---- options: ONE table for ldc_set_option and LDC_OPTIONS (no os.environ mutation around ldc_create; VERDICT r5: ~70 LDC_* switches) ----
// replan: cached plans / graphs depend on the value and are dropped when it changes.  tools/README.md documents every name.
struct OptRef { int* p; bool replan; int lo, hi; };
static bool find_option(ldc_ctx* c, const std::string& n, OptRef* r) {
#define LDC_OPT(NAME, FIELD, REPLAN, LO, HI) if (n == NAME) { r->p = &(FIELD); r->replan = REPLAN; r->lo = LO; r->hi = HI; return true; }
  // launch structure of a decode
  LDC_OPT("split", c->split_batch, true, 1, kMaxParts)            // independent chains a batch is decoded as
  LDC_OPT("part_graphs", c->part_graphs, false, 0, 2)             // 0 one fork / join graph | 1 one single-stream graph per part (two parts) | 2 also for 3 / 4 parts
  LDC_OPT("graph_steps", c->graph_steps, false, 0, 1000)          // steps per replayed graph (0: by chain count)
  LDC_OPT("flow_depth", c->flow_depth, false, 0, (int)ldc_ctx::kFlowRing - 1)
  LDC_OPT("split_ends", c->split_ends, false, 0, 1)               // codec front / back ends per batch part on the parts' streams
  LDC_OPT("ends_join", c->ends_join, false, 0, 1)
  LDC_OPT("split_init", c->split_init, true, 0, 1)                // init_conv's condition half once per sampler call
  LDC_OPT("side_streams", c->side_streams, true, 0, 1)            // res_conv on a side stream (single chain only)
  LDC_OPT("serial_parts", c->serial_parts, false, 0, 1)           // diagnostics: parts back to back, eager
  LDC_OPT("stream_calib", c->calib, false, 0, 1)                  // choose the part streams by measured overlap
  LDC_OPT("merge_advance", c->merge_advance, true, 0, 1)          // the step state advances in the step's first kernel
  // fusions of the UNet step
  LDC_OPT("fuse_gn_stats", c->fuse_gn_stats, true, 0, 1)
  LDC_OPT("fuse_gn_epi", c->fuse_gn_epi, true, 0, 1)              // GroupNorm apply in the conv epilogue; 0 is the fallback after a [gn_wait] failure
  LDC_OPT("gn_epi_min_l", c->gn_epi_min_l, true, 0, 1 << 30)
  LDC_OPT("gn_epi_max_tiles", c->gn_epi_max_tiles, true, 0, 1 << 30)
  LDC_OPT("fold_res", c->fold_res, true, 0, 1)
  LDC_OPT("fold_ln", c->fold_ln, true, 0, 1)
  LDC_OPT("fuse_kmax", c->fuse_kmax, true, 0, 1)
  LDC_OPT("fuse_ln", c->fuse_ln, true, 0, 1)
  LDC_OPT("fuse_attn_tail", c->fuse_attn_tail, true, 0, 1)
  LDC_OPT("fold_ctx", c->fold_ctx, true, 0, 1)                     // LinearAttention context inside to_qkv's epilogue (lean kernel, bf16)
  // conv launchers (ConvTune)
  LDC_OPT("conv_lean", c->tune.lean, true, 0, 1)                  // conv_lean_kernel where its shapes allow; 0 = conv_fast_kernel (A/B)
  LDC_OPT("lean_all", c->tune.lean_all, true, 0, 1)               // ... also for k = 4 stride 2 and k = 7 (bf16); 0 = conv_fast_kernel for those (A/B)
  LDC_OPT("ring3_tiles", c->tune.ring3_tiles, true, 0, 1 << 30)   // three-stage ring of conv_lean_kernel for launches of at most this many workgroups; 0 = off (A/B)
  LDC_OPT("ring3_wgs", c->tune.ring3_wgs, true, 1, 3)             // ... where this many three-stage workgroups still fit a CU's LDS (1 = every tile)
  LDC_OPT("ring3_window", c->tune.ring3_window, true, 0, 1)       // ... and where they do not but as many window rings do (k = 3, 128-row tile), the window ring; 0 = two stages (A/B)
  LDC_OPT("ring3_window_tiles", c->tune.ring3_window_tiles, true, 0, 1 << 30)   // ... for launches of at most this many workgroups
  LDC_OPT("conv_generic", c->tune.force_generic, true, 0, 1)      // every conv on the generic kernel
  LDC_OPT("conv_small_tiles", c->tune.small_max, true, 0, 1 << 30)
  LDC_OPT("conv_splitk", c->tune.splitk, true, 0, 4)
  LDC_OPT("sk_tiles", c->tune.sk_tiles, true, 0, 1 << 30)
  LDC_OPT("sk_u2", c->tune.sk_u2, true, 0, 1 << 30)
  LDC_OPT("sk_u3", c->tune.sk_u3, true, 0, 1 << 30)
  LDC_OPT("conv_mfast", c->tune.m_fastest, true, 0, 2)
  LDC_OPT("conv_debug", c->tune.debug, true, 0, 255)              // ablation bits (conv_lean.inc / conv_fast.inc)
  LDC_OPT("conv_tile", c->tune.force_tile, true, -1, 1)
  LDC_OPT("conv_xcd_order", c->tune.xcd_order, true, 0, 8)
  LDC_OPT("gn_nap", c->tune.gn_nap, true, 0, 4096)
  LDC_OPT("gn_nap0", c->tune.gn_nap0, true, 0, 4096)
  // codec ends
  LDC_OPT("lstm_stream", c->lstm_stream_only, false, 0, 1)        // never the cooperative LSTM kernel
  LDC_OPT("lstm_xcd", c->lstm_xcd, false, 0, 1)
  LDC_OPT("lstm_pipe", c->lstm_pipe, false, 0, 1)
  LDC_OPT("coop_launch", c->coop_launch, false, 0, 1)
  LDC_OPT("sea_splitk", c->sea_splitk, false, 0, 1)
  LDC_OPT("rvq_tiled", c->rvq_tiled, false, 0, 1)
  // process-wide training switches
  LDC_OPT("train_bf16", g_train_bf16, false, 0, 1)
  LDC_OPT("train_fp32_mfma", g_train_fp32_mfma, false, 0, 1)
  LDC_OPT("train_valu", g_train_valu, false, 0, 1)
  LDC_OPT("train_dw_side", g_train_dw_side, false, 0, 1)
#undef LDC_OPT
  return false;
}

extern "C" int ldc_set_option(ldc_ctx* c, const char* name, int value) {
  if (!c || !name) return fail(LDC_E_INVALID, "null context or option name");
  const std::string n(name);
  if (n == "fp8_act") {   // fp8-weight contexts: fp8 x fp8 MFMA where a tensor's only consumer is a conv (decided when the weights are packed)
    if (c->finalized) return fail(LDC_E_STATE, "fp8_act must be set before ldc_finalize_weights");
    c->fp8_act = value ? 1 : 0;
    return LDC_OK;
  }
  if (n == "plan_cache_gb") { c->plan_bytes_cap = (size_t)std::max(1, value) << 30; return LDC_OK; }
  if (n == "plan_cache_n") { c->plan_count_cap = std::max(2 * kMaxParts, value); return LDC_OK; }
  OptRef r;
  if (!find_option(c, n, &r)) return fail(LDC_E_INVALID, "unknown option '%s' (tools/README.md lists the options)", name);
  if (value < r.lo || value > r.hi) return fail(LDC_E_INVALID, "option %s must be in %d..%d", name, r.lo, r.hi);
  if (n == "side_streams" && value && c->split_batch != 1) return fail(LDC_E_INVALID, "side streams need a single chain (split 1)");
  if (value == *r.p) return LDC_OK;
  if (r.replan && c->live_pools > 0)
    return fail(LDC_E_STATE, "option %s rebuilds every plan, and %d decode pool(s) keep their items' state in theirs: destroy the pools first", name, c->live_pools);
  if (r.replan && !c->plans.empty()) { HIPCHK(hipSetDevice(c->device)); drop_plans(c); }   // plans of one shape differ by the value: start clean
  *r.p = value;
  if (n == "split" && value != 1) c->side_streams = 0;
  return LDC_OK;
}

// device-wide synchronisations issued by this library in this process so far (documented cold paths only: plan eviction, re-capture,
// option changes, profiling / tuning reads)
extern "C" long long ldc_debug_sync_count(void) { return g_device_syncs; }

// debug hook: raise the device-side failure flag as a kernel that gave up would (1 = cooperative LSTM, 2 = fused GroupNorm wait,
// 4 = LinearAttention context fold outside its valid k range; 3 is the RVQ bad-code report, which has no hook)
extern "C" int ldc_debug_raise_failure(ldc_ctx* c, int code) {
  if (!c || !c->dev_flag_host || (code != 1 && code != 2 && code != (int)kDevFailCtxRange)) return fail(LDC_E_INVALID, "bad arguments");
  *reinterpret_cast<volatile unsigned*>(c->dev_flag_host) = (unsigned)code;
  return LDC_OK;
}

extern "C" int ldc_reseed(ldc_ctx* c, uint64_t seed) {
  if (!c) return fail(LDC_E_INVALID, "null ctx");
  c->cfg.noise_seed = seed;
  c->noise_epoch = 0;
  return LDC_OK;
}

extern "C" int ldc_set_weight(ldc_ctx* c, int which, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!c || !key || !data || (ndim > 0 && !shape)) return fail(LDC_E_INVALID, "null argument");
  if (which != LDC_MODEL_MAIN && which != LDC_MODEL_COND) return fail(LDC_E_INVALID, "which must be LDC_MODEL_MAIN or LDC_MODEL_COND");
  if (c->finalized) return fail(LDC_E_STATE, "weights already finalized");
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  t.data.assign(data, data + t.numel());
  c->raw[which][key] = std::move(t);
  return LDC_OK;
}

extern "C" int ldc_finalize_weights(ldc_ctx* c, int strict) {
  if (!c) return fail(LDC_E_INVALID, "null ctx");
  if (c->finalized) return fail(LDC_E_STATE, "already finalized");
  HIPCHK(hipSetDevice(c->device));
  std::string missing;
  std::vector<int> main_ratios(c->cfg.enc_ratios, c->cfg.enc_ratios + c->cfg.n_enc_ratios);
  LDCCHK(build_codec(c, LDC_MODEL_MAIN, main_ratios, 0, &missing));
  LDCCHK(build_unet(c, &missing));
  if (c->cfg.has_cond_model) {
    // quirk Q1: the cond codec is always built with the default ratios [8,5,4,2] (sample.py:63, model.py:34)
    const int frame_rate_ceil = 50;
    const int n_q = (int)floor(1000.0 * c->cfg.cond_bandwidth / (frame_rate_ceil * 10));   // model.py:65
    LDCCHK(build_codec(c, LDC_MODEL_COND, {8, 5, 4, 2}, n_q, &missing));
  }
  if (!missing.empty()) return fail(LDC_E_MISSING, "missing or mis-shaped keys in state_dict: %s", missing.c_str());
  if (strict) {
    std::string unexpected;
    for (int w = 0; w < 2; ++w)
      for (auto& kv : c->raw[w])
        if (!kv.second.used) {
          // the UNet is registered twice (diff_model.* and diffusion.model.*): either alias satisfies the other
          const std::string& k = kv.first;
          std::string alias;
          if (k.rfind("diffusion.model.", 0) == 0) alias = "diff_model." + k.substr(16);
          else if (k.rfind("diff_model.", 0) == 0) alias = "diffusion.model." + k.substr(11);
          auto it = alias.empty() ? c->raw[w].end() : c->raw[w].find(alias);
          if (it != c->raw[w].end() && it->second.used && it->second.shape == kv.second.shape) continue;
          if (unexpected.size() < 600) unexpected += k + " ";
        }
    if (!unexpected.empty()) return fail(LDC_E_MISSING, "unexpected keys in state_dict: %s", unexpected.c_str());
  }
  c->raw[0].clear();
  c->raw[1].clear();
  c->finalized = true;
  return LDC_OK;
}

// ------------------------------------------------------------------------------------------------
// scratch
// ------------------------------------------------------------------------------------------------
// Growth of a context-owned workspace is the one place a stage call waits for the device (the old buffer may still be
// in use by earlier asynchronous calls); steady-state calls never do (include/ladiffcodec.h documents this).
int ensure_scratch(ldc_ctx* c, size_t bytes, hipStream_t s) {
  if (bytes <= c->scratch_cap) return LDC_OK;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(counted_device_sync());
  if (c->scratch) HIPCHK(hipFree(c->scratch));
  c->scratch = nullptr;
  c->scratch_cap = 0;
  void* p = nullptr;
  const size_t want = bytes + bytes / 4;
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) return fail(LDC_E_NOMEM, "hipMalloc(%zu) for scratch failed: %s", want, hipGetErrorString(e));
  c->scratch = (char*)p;
  c->scratch_cap = want;
  return LDC_OK;
}

// ------------------------------------------------------------------------------------------------
// SEANet execution (codec dtype = fp32, channels-last)
// ------------------------------------------------------------------------------------------------
int conv_out_len(const ConvLayer& ly, int L) {
  // SConv1d output length with the reference's extra right padding (conv.py:56-63): ceil(L / stride)
  const int eff_k = (ly.taps - 1) * ly.dil + 1;
  const int padding_total = eff_k - ly.stride;
  const double n_frames = (double)(L - eff_k + padding_total) / ly.stride + 1.0;
  return (int)ceil(n_frames);
}


// stream session: the conv's context entry, or null when the layer never reads before its chunk (k = 1)
static int stream_conv_state(SeaRun& R, int rows, int ch, StreamConvState** out) {
  *out = nullptr;
  if (!R.st || rows <= 0) return LDC_OK;
  if (R.st->conv_at >= R.st->convs.size() || R.st->convs[R.st->conv_at].rows != rows || R.st->convs[R.st->conv_at].ch != ch)
    return fail(LDC_E_STATE, "stream state does not match the layer table (conv %zu: %d rows x %d channels)", R.st->conv_at, rows, ch);
  *out = &R.st->convs[R.st->conv_at++];
  return LDC_OK;
}

// A conv of a stream session: the launch sees (context | chunk) per item and pads nothing itself; the context of the next chunk is
// written to the other buffer by a copy launch of its own
static int sea_conv_stream(SeaRun& R, const ConvLayer& ly, StreamConvState& cs, const void* x, const void* residual, int L_in, void** y, int* L_out, int cout) {
  if (!ly.tr_stride && L_in % ly.stride) return fail(LDC_E_INVALID, "stream chunk of %d rows is not a multiple of the layer's stride %d", L_in, ly.stride);
  ConvLayer lv = ly;
  lv.pad_left = 0;
  ConvCall cc;
  cc.B = R.B; cc.L_in = L_in + cs.rows; cc.x1 = x; cc.residual = residual; cc.tune = &R.c->tune; cc.route_out = R.route;
  cc.ctx = cs.buf[R.st->parity]; cc.ctx_fresh = R.st->fresh_dev; cc.ctx_rows = cs.rows; cc.ctx_zero = ly.tr_stride ? 1 : 0;
  if (ly.tr_stride) {   // row q of the 2-tap GEMM reads virtual rows q (the previous input row) and q + 1; the row the whole-sequence call trims is never formed
    cc.L_rows = L_in;
    cc.L_final = L_in * ly.tr_stride;
    *L_out = cc.L_final;
    cc.y_ld = ly.tr_cout;
  } else {
    cc.L_rows = L_in / ly.stride;
    *L_out = cc.L_rows;
    cc.y_ld = cout;
  }
  *y = R.ar->alloc((size_t)R.B * (*L_out) * cc.y_ld * 4);
  cc.y = *y;
  if (R.c->sea_splitk) {
    const long long fl = conv_generic_splitk_floats(lv, cc);
    if (fl > 0) {
      cc.sk_part = (float*)R.ar->alloc((size_t)fl * 4);
      cc.sk_part_cap = fl;
      cc.generic_split = 1;
    }
  }
  if (R.dry) {   // refused here, before any GPU work of the call: a launch whose tiles cross so many item seams that its LDS window does not fit
    ConvCall chk = cc;
    chk.check_only = 1; chk.route_out = nullptr;
    if (launch_conv(lv, chk, R.s) != hipSuccess)
      return fail(LDC_E_INVALID, "stream chunk of %d rows x B = %d items: the LDS window of a layer (%d context rows per item, stride %d) does not fit; "
                                 "use longer chunks or fewer items per session", L_in, R.B, cs.rows, ly.stride);
  } else {
    HIPCHK(launch_conv(lv, cc, R.s));
    HIPCHK(launch_stream_ctx_update((const float*)x, cs.buf[R.st->parity], cs.buf[R.st->parity ^ 1], R.st->fresh_dev, R.B, L_in, cs.rows, cs.ch, cc.ctx_zero, R.s));
  }
  return LDC_OK;
}

int sea_conv(SeaRun& R, const ConvLayer& ly, const void* x, const void* residual, int L_in, void** y, int* L_out, int cout) {
  StreamConvState* cs = nullptr;
  LDCCHK(stream_conv_state(R, ly.tr_stride ? 1 : ly.pad_left, ly.cin1, &cs));
  if (cs) return sea_conv_stream(R, ly, *cs, x, residual, L_in, y, L_out, cout);
  ConvCall cc;
  cc.B = R.B; cc.L_in = L_in; cc.x1 = x; cc.residual = residual; cc.tune = &R.c->tune; cc.route_out = R.route;
  if (ly.tr_stride) {
    cc.L_rows = L_in + 1;
    cc.L_final = L_in * ly.tr_stride;
    *L_out = cc.L_final;
    cc.y_ld = ly.tr_cout;
  } else {
    cc.L_rows = conv_out_len(ly, L_in);
    *L_out = cc.L_rows;
    cc.y_ld = cout;
  }
  *y = R.ar->alloc((size_t)R.B * (*L_out) * cc.y_ld * 4);
  cc.y = *y;
  if (R.c->sea_splitk) {   // few-tile long-K layers: split-K partial sums in the run's arena
    const long long fl = conv_generic_splitk_floats(ly, cc);
    if (fl > 0) {
      cc.sk_part = (float*)R.ar->alloc((size_t)fl * 4);
      cc.sk_part_cap = fl;
      cc.generic_split = 1;
    }
  }
  if (!R.dry) HIPCHK(launch_conv(ly, cc, R.s));
  return LDC_OK;
}

int run_seanet(SeaRun& R, const std::vector<SeaOp>& ops, const void* x_in, int L, void** out, int* L_out, int* C_out) {
  const void* x = x_in;
  int C = 0;
  for (const SeaOp& op : ops) {
    void* y = nullptr;
    int Ln = L;
    switch (op.kind) {
      case SeaOp::CONV_CIN1: {
        if (L <= op.k - 1) return fail(LDC_E_INVALID, "input no longer than the first conv's reflect padding is not supported (L=%d pad=%d)", L, op.k - 1);
        y = R.ar->alloc((size_t)R.B * L * op.cout * 4);
        StreamConvState* cs = nullptr;
        LDCCHK(stream_conv_state(R, op.k - 1, 1, &cs));
        if (!R.dry && cs) {
          HIPCHK(launch_conv_cin1(DT_F32, (const float*)x, y, op.w1, op.b1, R.B, L, op.cout, op.k, R.s, nullptr, cs->buf[R.st->parity], R.st->fresh_dev));
          HIPCHK(launch_stream_ctx_update((const float*)x, cs->buf[R.st->parity], cs->buf[R.st->parity ^ 1], R.st->fresh_dev, R.B, L, cs->rows, 1, 0, R.s));
        } else if (!R.dry) HIPCHK(launch_conv_cin1(DT_F32, (const float*)x, y, op.w1, op.b1, R.B, L, op.cout, op.k, R.s));
        C = op.cout;
        break;
      }
      case SeaOp::CONV:
      case SeaOp::CONVTR:
        LDCCHK(sea_conv(R, op.conv, x, nullptr, L, &y, &Ln, op.cout));
        C = op.cout;
        break;
      case SeaOp::RES: {
        void *sc = nullptr, *h = nullptr;
        int l1 = L, l2 = L, l3 = L;
        LDCCHK(sea_conv(R, op.shortcut, x, nullptr, L, &sc, &l1, op.cout));
        LDCCHK(sea_conv(R, op.conv, x, nullptr, L, &h, &l2, op.hidden));
        LDCCHK(sea_conv(R, op.conv2, h, sc, l2, &y, &l3, op.cout));
        Ln = l3;
        C = op.cout;
        break;
      }
      case SeaOp::LSTM: {
        const int H = op.cout;
        const void* in = x;
        // Two-layer register LSTM (the main codec's decoder: 1 200 steps x 2 layers, one workgroup per item) as a TWO-STAGE PIPELINE over
        // time chunks: layer 0 writes its chunk time-major, the side stream runs layer 1's input GEMM over exactly those rows (contiguous
        // in that layout) and layer 1's chunk while layer 0 is on its next one; the recurrent state travels through [B][2H] buffers.
        // 5 chunk times instead of 8 on paper; measured (tools/lstm_pipe_time.py) it does not pay on this runtime -- see ldc_ctx::lstm_pipe -- and is off.
        const bool pipe = !R.st && R.c->lstm_pipe && R.side >= 0 && R.side < 2 && R.c->aux_stream[2 + R.side] && op.lstm.size() == 2 && lstm_seq_supported(H) && !op.lstm[0].w_rm && !op.lstm[1].w_rm &&
                          L >= 64 * ldc_ctx::kLstmChunks;
        if (pipe) {
          constexpr int NCH = ldc_ctx::kLstmChunks;
          void* pre0 = R.ar->alloc((size_t)R.B * L * 4 * H * 4);
          void* o0 = R.ar->alloc((size_t)R.B * L * H * 4);         // time-major [L][B][H]
          void* pre1 = R.ar->alloc((size_t)R.B * L * 4 * H * 4);   // time-major [L][B][4H]
          void* o1 = R.ar->alloc((size_t)R.B * L * H * 4);
          float* st0 = (float*)R.ar->alloc((size_t)R.B * 2 * H * 4);
          float* st1 = (float*)R.ar->alloc((size_t)R.B * 2 * H * 4);
          if (!R.dry) {
            hipStream_t s2 = R.c->aux_stream[2 + R.side];
            hipEvent_t* ev = R.c->lstm_ev[R.side];
            ConvCall cc;
            cc.B = R.B; cc.L_in = L; cc.L_rows = L; cc.x1 = in; cc.y = pre0; cc.y_ld = 4 * H; cc.tune = &R.c->tune;
            HIPCHK(launch_conv(op.lstm[0].in_proj, cc, R.s));
            for (int k = 0; k < NCH; ++k) {
              const int t0 = (int)((long long)L * k / NCH), t1 = (int)((long long)L * (k + 1) / NCH);
              LstmSeq q0;
              q0.t0 = t0; q0.t1 = t1; q0.pre_bs = L; q0.pre_ts = 1; q0.out_bs = 1; q0.out_ts = R.B; q0.state = st0;
              HIPCHK(launch_lstm_seq(DT_F32, pre0, op.lstm[0].w_hh, o0, nullptr, R.B, H, q0, R.s));
              HIPCHK(hipEventRecord(ev[k], R.s));
              HIPCHK(hipStreamWaitEvent(s2, ev[k], 0));
              ConvCall c1;
              c1.B = 1; c1.L_in = (t1 - t0) * R.B; c1.L_rows = c1.L_in; c1.tune = &R.c->tune; c1.y_ld = 4 * H;
              c1.x1 = (const char*)o0 + (size_t)t0 * R.B * H * 4;
              c1.y = (char*)pre1 + (size_t)t0 * R.B * 4 * H * 4;
              HIPCHK(launch_conv(op.lstm[1].in_proj, c1, s2));
              LstmSeq q1;
              q1.t0 = t0; q1.t1 = t1; q1.pre_bs = 1; q1.pre_ts = R.B; q1.out_bs = L; q1.out_ts = 1; q1.skip_bs = L; q1.skip_ts = 1; q1.state = st1;
              HIPCHK(launch_lstm_seq(DT_F32, pre1, op.lstm[1].w_hh, o1, x, R.B, H, q1, s2));
            }
            HIPCHK(hipEventRecord(ev[NCH], s2));
            HIPCHK(hipStreamWaitEvent(R.s, ev[NCH], 0));
          }
          y = o1;
          C = H;
          break;
        }
        for (size_t n = 0; n < op.lstm.size(); ++n) {
          void* pre = R.ar->alloc((size_t)R.B * L * 4 * H * 4);
          void* o = R.ar->alloc((size_t)R.B * L * H * 4);
          const bool coop = op.lstm[n].w_rm && !R.c->lstm_stream_only && R.c->coop_resident[H == 512 ? 1 : 0];
          void* lws = coop ? R.ar->alloc(lstm_coop_ws_bytes(H)) : nullptr;
          LstmCarry carry;   // stream session: (h | c) in and out; the kernel is picked per chunk by the same rule as for a whole sequence
          if (R.st) {
            if (R.st->lstm_at >= R.st->lstm.size()) return fail(LDC_E_STATE, "stream state does not match the layer table (LSTM layer %zu)", R.st->lstm_at);
            carry.state = R.st->lstm[R.st->lstm_at++];
            carry.fresh = R.st->fresh_dev;
          }
          if (!R.dry) {
            ConvCall cc;
            cc.B = R.B; cc.L_in = L; cc.L_rows = L; cc.x1 = in; cc.y = pre; cc.y_ld = 4 * H; cc.tune = &R.c->tune;
            HIPCHK(launch_conv(op.lstm[n].in_proj, cc, R.s));
            const bool lastl = n + 1 == op.lstm.size();
            hipError_t le = hipErrorCooperativeLaunchTooLarge;
            if (coop) le = launch_lstm_coop(DT_F32, pre, op.lstm[n].w_rm, o, lastl ? x : nullptr, R.B, L, H, lws, R.c->dev_flag_dev, (R.c->lstm_xcd && R.c->xcd_resident[H == 512 ? 1 : 0] >= 2 * R.teams) ? 2 : R.c->coop_launch, R.s, carry);
            if (le == hipErrorCooperativeLaunchTooLarge) {   // (or not eligible): one workgroup per item, W_hh streamed from L2
              (void)hipGetLastError();
              le = launch_lstm_layer(DT_F32, pre, op.lstm[n].w_hh, o, lastl ? x : nullptr, R.B, L, H, R.s, carry);
            }
            HIPCHK(le);
          }
          in = o;
          y = o;
        }
        C = H;
        break;
      }
    }
    x = y;
    L = Ln;
  }
  *out = const_cast<void*>(x);
  *L_out = L;
  *C_out = C;
  return LDC_OK;
}


int check_ready(ldc_ctx* c, int which, bool need_cond_codec) {
  if (!c) return fail(LDC_E_INVALID, "null ctx");
  if (!c->finalized) return fail(LDC_E_STATE, "ldc_finalize_weights has not been called");
  if (which != LDC_MODEL_MAIN && which != LDC_MODEL_COND) return fail(LDC_E_INVALID, "bad model selector");
  if ((which == LDC_MODEL_COND || need_cond_codec) && !c->codec[LDC_MODEL_COND].present)
    return fail(LDC_E_STATE, "no cond model configured (has_cond_model = 0)");
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(LDC_E_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
  return check_dev_flag(c);
}

extern "C" int ldc_seanet_encode(ldc_ctx* c, int which, const float* wav, int B, int T, float* z_out, void* stream) {
  LDCCHK(check_ready(c, which));
  if (!wav || !z_out || B <= 0 || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  hipStream_t s = pick_stream(c, stream);
  const Codec& cd = c->codec[which];
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    SeaRun R{c, &ar, s, dry, B};
    void* z = nullptr;
    int L = 0, C = 0;
    LDCCHK(run_seanet(R, cd.enc, wav, T, &z, &L, &C));
    if (!dry) HIPCHK(launch_from_cl(DT_F32, z, z_out, B, C, L, nullptr, 0, 0.f, s));
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

extern "C" int ldc_seanet_decode(ldc_ctx* c, int which, const float* z, int B, int L, float* wav_out, void* stream) {
  LDCCHK(check_ready(c, which));
  if (!z || !wav_out || B <= 0 || L <= 0) return fail(LDC_E_INVALID, "bad arguments");
  hipStream_t s = pick_stream(c, stream);
  const Codec& cd = c->codec[which];
  const int D = c->cfg.rep_dims;
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    SeaRun R{c, &ar, s, dry, B};
    R.side = 0;
    void* zc = ar.alloc((size_t)B * L * D * 4);
    if (!dry) HIPCHK(launch_to_cl(DT_F32, z, zc, B, D, L, nullptr, 0, 0.f, s));
    void* y = nullptr;
    int Lo = 0, C = 0;
    LDCCHK(run_seanet(R, cd.dec, zc, L, &y, &Lo, &C));
    // last conv has Cout = 1: channels-last [B*T][1] is already [B,1,T]
    if (!dry) HIPCHK(hipMemcpyAsync(wav_out, y, (size_t)B * Lo * 4, hipMemcpyDeviceToDevice, s));
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

// ------------------------------------------------------------------------------------------------
// RVQ
// ------------------------------------------------------------------------------------------------
int rvq_rows(ldc_ctx* c, const float* z_rows, int rows, int n_q, int64_t* codes, float* q_rows, Arena& ar, bool dry,
                    hipStream_t s) {
  const Codec& cd = c->codec[LDC_MODEL_COND];
  int64_t* cw = codes;
  if (!cw) cw = (int64_t*)ar.alloc((size_t)n_q * rows * sizeof(int64_t));
  if (!dry) HIPCHK(launch_rvq(z_rows, rows, c->cfg.rep_dims, cd.codebooks, cd.cb_sqnorm, cd.bins, n_q, cw, q_rows, s, c->rvq_tiled));
  return LDC_OK;
}

int n_q_for_bandwidth(ldc_ctx* c, float bandwidth) {
  // vq.py:86-98 with frame_rate = 16000/320 = 50: bw_per_q = log2(1024)*50/1000 = 0.5
  const Codec& cd = c->codec[LDC_MODEL_COND];
  const double bw = bandwidth > 0 ? bandwidth : c->cfg.cond_bandwidth;
  const double bw_per_q = log2((double)cd.bins) * (16000.0 / cd.hop) / 1000.0;
  int n_q = cd.n_q_layers;
  if (bw > 0) n_q = (int)std::max(1.0, floor(bw / bw_per_q));
  return std::min(n_q, cd.n_q_layers);
}

extern "C" int ldc_rvq_encode(ldc_ctx* c, const float* z, int B, int F, int n_q, int64_t* codes_out, float* quantized_out,
                              void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_COND));
  const Codec& cd = c->codec[LDC_MODEL_COND];
  if (!z || !quantized_out || B <= 0 || F <= 0 || n_q < 1 || n_q > cd.n_q_layers)
    return fail(LDC_E_INVALID, "bad arguments (n_q must be in [1,%d])", cd.n_q_layers);
  hipStream_t s = pick_stream(c, stream);
  const int D = c->cfg.rep_dims;
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    float* zr = (float*)ar.alloc((size_t)B * F * D * 4);
    float* qr = (float*)ar.alloc((size_t)B * F * D * 4);
    if (!dry) HIPCHK(launch_to_cl(DT_F32, z, zr, B, D, F, nullptr, 0, 0.f, s));
    LDCCHK(rvq_rows(c, zr, B * F, n_q, codes_out, qr, ar, dry, s));
    if (!dry) HIPCHK(launch_from_cl(DT_F32, qr, quantized_out, B, D, F, nullptr, 0, 0.f, s));
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

extern "C" int ldc_rvq_decode(ldc_ctx* c, const int64_t* codes, int B, int F, int n_q, float* quantized_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_COND));
  const Codec& cd = c->codec[LDC_MODEL_COND];
  if (!codes || !quantized_out || B <= 0 || F <= 0 || n_q < 1 || n_q > cd.n_q_layers) return fail(LDC_E_INVALID, "bad arguments");
  hipStream_t s = pick_stream(c, stream);
  const int D = c->cfg.rep_dims;
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    float* qr = (float*)ar.alloc((size_t)B * F * D * 4);
    if (!dry) {
      HIPCHK(launch_rvq_dequant(codes, nullptr, 0, 0, n_q, B, 0, B, F, cd.codebooks, cd.bins, D, qr, c->dev_flag_dev, s));
      HIPCHK(launch_from_cl(DT_F32, qr, quantized_out, B, D, F, nullptr, 0, 0.f, s));
    }
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

// encoder -> RVQ, rows stay channels-last in between; returns the quantized rows pointer (scratch)
static int get_cond_rows(ldc_ctx* c, const float* wav, int B, int T, float bandwidth, Arena& ar, bool dry, hipStream_t s,
                         float** q_rows, int* F_out, int64_t* codes_out, int teams = 1) {
  const Codec& cd = c->codec[LDC_MODEL_COND];
  SeaRun R{c, &ar, s, dry, B};
  R.teams = teams;
  void* z = nullptr;
  int F = 0, C = 0;
  LDCCHK(run_seanet(R, cd.enc, wav, T, &z, &F, &C));
  float* qr = (float*)ar.alloc((size_t)B * F * C * 4);
  LDCCHK(rvq_rows(c, (const float*)z, B * F, n_q_for_bandwidth(c, bandwidth), codes_out, qr, ar, dry, s));
  *q_rows = qr;
  *F_out = F;
  return LDC_OK;
}

extern "C" int ldc_get_cond(ldc_ctx* c, const float* wav, int B, int T, float bandwidth, float* cond_out, int64_t* codes_out,
                            void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_COND));
  if (!wav || !cond_out || B <= 0 || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  hipStream_t s = pick_stream(c, stream);
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    float* qr = nullptr;
    int F = 0;
    LDCCHK(get_cond_rows(c, wav, B, T, bandwidth, ar, dry, s, &qr, &F, codes_out));
    if (!dry) HIPCHK(launch_from_cl(DT_F32, qr, cond_out, B, c->cfg.rep_dims, F, nullptr, 0, 0.f, s));
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

// ------------------------------------------------------------------------------------------------
// cond upsampler (fp32): rows [B*F][C] -> rows [B*L][C]
// ------------------------------------------------------------------------------------------------
// flens (ragged batches): condition frames per item; every layer's output is cut to the item's length (see build_plan)
static int upsample_rows(ldc_ctx* c, const void* rows_in, int B, int F, Arena& ar, bool dry, hipStream_t s, void** out,
                         int* L_out, const int* flens = nullptr) {
  const UnetW& u = c->unet;
  const void* x = rows_in;
  int L = F;
  for (const ConvLayer& ly : u.upsamplers) {
    ConvCall cc;
    cc.B = B; cc.L_in = L; cc.L_rows = L + 1; cc.L_final = L * ly.tr_stride; cc.y_ld = ly.tr_cout; cc.x1 = x; cc.tune = &c->tune;
    void* y = ar.alloc((size_t)B * cc.L_final * ly.tr_cout * 4);
    cc.y = y;
    if (!dry) HIPCHK(launch_conv(ly, cc, s));
    if (!dry && flens) HIPCHK(launch_mask_rows(DT_F32, y, B, F, cc.L_final / F * ly.tr_cout, flens, 0, s));
    x = y;
    L = cc.L_final;
  }
  *out = const_cast<void*>(x);
  *L_out = L;
  return LDC_OK;
}

int upsample_factor(const ldc_ctx* c) {
  int f = 1;
  for (int r : c->unet.up_ratios) f *= r;
  return f;
}

extern "C" int ldc_cond_upsample(ldc_ctx* c, const float* cond, int B, int F, int normalise, float* img_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!cond || !img_out || B <= 0 || F <= 0 || normalise < 0 || normalise > 2) return fail(LDC_E_INVALID, "bad arguments");
  hipStream_t s = pick_stream(c, stream);
  const int C = c->unet.cond_channels;
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    void* rows = ar.alloc((size_t)B * F * C * 4);
    float* mx = (float*)ar.alloc((size_t)B * 4);
    if (!dry) HIPCHK(launch_to_cl(DT_F32, cond, rows, B, C, F, nullptr, 0, 0.f, s));
    void* up = nullptr;
    int L = 0;
    LDCCHK(upsample_rows(c, rows, B, F, ar, dry, s, &up, &L));
    if (!dry) {
      if (normalise) {
        HIPCHK(hipMemsetAsync(mx, 0, (size_t)B * 4, s));
        HIPCHK(launch_maxabs(DT_F32, up, B, (int64_t)L * C, normalise == 2, mx, s));
        HIPCHK(launch_from_cl(DT_F32, up, img_out, B, C, L, mx, normalise == 2, 1e-8f, s));
      } else {
        HIPCHK(launch_from_cl(DT_F32, up, img_out, B, C, L, nullptr, 0, 0.f, s));
      }
    }
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

// The batch parts run as chains on streams of this context next to the caller's stream s.  HIP serves a process's streams from four
// hardware queues and two streams that share one run their graphs back to back (measured: 229 instead of 143 ms per decode with part 1 on
// such a stream; which streams share depends on what else the process created before -- torch's pool, RCCL, other contexts).  So the part
// streams are CHOSEN, once per caller stream: a candidate is accepted when a 150 us single-workgroup spin on it and on every stream
// accepted so far takes one spin, not two.  ~2 ms, the first time a batch is decoded in parts on a stream; never inside a capture.
int calibrate_part_streams(ldc_ctx* c, hipStream_t s) {
  if (!c->calib || (c->calibrated && c->calib_stream == s)) return LDC_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return LDC_OK; }
  std::vector<hipStream_t*> cand;
  for (int k = 1; k < kMaxParts; ++k) cand.push_back(&c->aux_stream[k]);
  for (int k = 0; k < kMaxParts; ++k) cand.push_back(&c->side_stream[k]);
  for (const auto& e : c->calib_cache)
    if (e.s == s && e.order.size() == cand.size()) {   // measured before against this caller stream: re-apply, no synchronisation
      for (size_t i = 0; i < cand.size(); ++i) *cand[i] = e.order[i];
      c->calib_good = e.good; c->calib_cand = e.cand; c->calib_one_ms = e.one_ms; c->calib_all_ms = e.all_ms;
      c->calib_stream = s; c->calibrated = true;
      return LDC_OK;
    }
  std::vector<hipStream_t> chosen{s};
  auto timed = [&](const std::vector<hipStream_t>& set, double* ms) -> int {
    double best = 1e30;
    for (int rep = 0; rep < 4; ++rep) {   // (best of four: host wall time, a loaded host inflates single samples)
      for (hipStream_t q : set) HIPCHK(hipStreamSynchronize(q));
      const auto t0 = std::chrono::steady_clock::now();
      for (hipStream_t q : set) HIPCHK(launch_spin_us(150, q));
      for (hipStream_t q : set) HIPCHK(hipStreamSynchronize(q));
      best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    *ms = best;
    return LDC_OK;
  };
  double base = 0;
  LDCCHK(timed(chosen, &base));   // (also loads the kernel)
  LDCCHK(timed(chosen, &base));
  std::vector<hipStream_t> good, rest;
  for (hipStream_t* p : cand) {
    if ((int)good.size() >= kMaxParts - 1) { rest.push_back(*p); continue; }
    std::vector<hipStream_t> set = chosen;
    set.push_back(*p);
    double ms = 0;
    LDCCHK(timed(set, &ms));
    if (ms < base + 0.09) { good.push_back(*p); chosen.push_back(*p); }   // one 0.15 ms spin more = a shared queue
    else rest.push_back(*p);
  }
  if (getenv("LDC_VERBOSE")) fprintf(stderr, "[ldc] part streams: %zu of %zu candidates overlap with the caller's stream and each other (one spin: %.3f ms)\n", good.size(), cand.size(), base);
  std::vector<hipStream_t> order = good;
  order.insert(order.end(), rest.begin(), rest.end());
  for (size_t i = 0; i < cand.size(); ++i) *cand[i] = order[i];
  double all_ms = base;
  if (!good.empty()) LDCCHK(timed(chosen, &all_ms));   // the caller's stream and every accepted stream spinning together: one spin when they overlap
  c->calib_good = (int)good.size(); c->calib_cand = (int)cand.size(); c->calib_one_ms = base; c->calib_all_ms = all_ms;
  if (c->calib_cache.size() >= 8) c->calib_cache.erase(c->calib_cache.begin());
  c->calib_cache.push_back({s, order, c->calib_good, c->calib_cand, base, all_ms});
  c->calib_stream = s;
  c->calibrated = true;
  return LDC_OK;
}

int get_halves(ldc_ctx* c, int B, int L, int F, hipStream_t s, Halves* h, bool ragged, bool items, int pool_id) {
  *h = Halves();
  c->call_tick = c->use_tick;   // plans touched from here on belong to the call being served (not evictable)
  // Independent chains the batch is decoded as (utterances never interact inside the UNet).  A chain is a
  // dependent sequence of ~155 launches per step whose cost is mostly per-launch floor, so chains side by side hide each
  // other's floors.  Measured on one box (32 x 2.4 s): 2 x 16 items 503 audio-s/s, 3 chains 505, 4 x 8 items 510 -- but
  // the convs of a 4 x 8 decode run at 209 instead of 344 TFLOP/s per launch, so two chains stay the default (LDC_SPLIT).
  h->n = std::max(1, std::min(c->split_batch, B));
  if (h->n >= 2) LDCCHK(calibrate_part_streams(c, s));
  for (int k = 0; k < h->n; ++k) {
    const int lo = (int)((long long)B * k / h->n), hi = (int)((long long)B * (k + 1) / h->n);
    h->b0[k] = lo;
    LDCCHK(get_plan(c, hi - lo, L, F, k, s, &h->p[k], ragged, items, pool_id));
  }
  c->last_halves = *h;
  return LDC_OK;
}

int load_cond(ldc_ctx* c, const Halves& h, const float* cond, hipStream_t s) {
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    const float* src = cond + (size_t)h.b0[k] * c->unet.cond_channels * pl->F;
    HIPCHK(launch_to_cl(DT_F32, src, pl->cond_in_cl, pl->B, c->unet.cond_channels, pl->F, nullptr, 0, 0.f, s));
    LDCCHK(run_ops(c, pl, false, s));
  }
  return LDC_OK;
}

int load_x(ldc_ctx* c, const Halves& h, const float* x, hipStream_t s) {
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    HIPCHK(launch_to_cl(c->dt, x + (size_t)h.b0[k] * c->unet.channels * pl->L, pl->x_cl, pl->B, c->unet.channels, pl->L, nullptr,
                        0, 0.f, s));
  }
  return LDC_OK;
}

int check_unet_args(ldc_ctx* c, int B, int L, int F) {
  if (B <= 0 || L <= 0 || F <= 0) return fail(LDC_E_INVALID, "bad sizes");
  // upsampling_ratios=None (unet.py:411): process_cond only scales, so the condition must already have the latent length
  if (F * upsample_factor(c) != L) return fail(LDC_E_INVALID, "L (%d) must equal F (%d) x prod(upsampling_ratios) (%d)", L, F, upsample_factor(c));
  return LDC_OK;
}

extern "C" int ldc_unet_forward(ldc_ctx* c, const float* x, int t, const float* cond, int B, int L, int F, float* eps_out,
                                void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!x || !cond || !eps_out) return fail(LDC_E_INVALID, "null tensor");
  if (t < 0 || t >= c->unet.timesteps) return fail(LDC_E_INVALID, "t out of range");
  LDCCHK(check_unet_args(c, B, L, F));
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(load_cond(c, h, cond, s));
  LDCCHK(load_x(c, h, x, s));
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    HIPCHK(launch_step_set(pl->step_state, t, 0, c->cur_key, s));
    HIPCHK(launch_step_begin(c->unet.ss_table, c->unet.ss_stride, pl->step_state, pl->cur_ss, nullptr, s, pl->zero_ptr, pl->zero_bytes));
    LDCCHK(run_ops(c, pl, true, s));
    HIPCHK(launch_from_cl(c->dt, pl->eps_cl, eps_out + (size_t)h.b0[k] * c->unet.channels * L, pl->B, c->unet.channels, L, nullptr,
                          0, 0.f, s));
  }
  return finish_stream(c, stream);
}

// ---- ragged batches: items of different lengths in one [B, Lmax] layout ----
// halvings of the UNet's down path: a latent length must survive them
static int unet_halvings(const ldc_ctx* c) {
  int n = 0;
  for (const LevelW& lv : c->unet.downs) n += lv.kind == 0;
  return n;
}
static long long lcm_ll(long long a, long long b) {
  long long x = a, y = b;
  while (y) { const long long t = x % y; x = y; y = t; }
  return a / x * b;
}
// latent frames an item's length must be a multiple of: whole condition frames and the halvings
int ragged_latent_quantum(const ldc_ctx* c) { return (int)lcm_ll(upsample_factor(c), 1ll << unet_halvings(c)); }
// every length of a ragged call, before any GPU work: `unit` is what the lengths count (latent frames or samples)
static int check_ragged_lengths(const int32_t* lens, int B, int maxlen, long long quantum, const char* unit) {
  if (!lens) return fail(LDC_E_INVALID, "null lengths");
  if (maxlen <= 0 || maxlen % quantum) return fail(LDC_E_INVALID, "the padded length %d is not a positive multiple of %lld %s", maxlen, quantum, unit);
  for (int b = 0; b < B; ++b)
    if (lens[b] <= 0 || lens[b] > maxlen || lens[b] % quantum)
      return fail(LDC_E_INVALID, "length %d of item %d must be a multiple of %lld %s in (0, %d]", (int)lens[b], b, quantum, unit, maxlen);
  return LDC_OK;
}
// the parts' own slices of the lengths into their plans, ordered on s (every part's stream forks from s behind it)
static int write_plan_lens(ldc_ctx* c, const Halves& h, const std::vector<int>& lat, hipStream_t s) {
  const int up = upsample_factor(c);
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    std::vector<int> fr(pl->B);
    for (int b = 0; b < pl->B; ++b) fr[b] = lat[h.b0[k] + b] / up;
    HIPCHK(launch_lens_write(pl->lens, lat.data() + h.b0[k], pl->B, s));
    HIPCHK(launch_lens_write(pl->flens, fr.data(), pl->B, s));
  }
  return LDC_OK;
}

extern "C" int ldc_unet_forward_ragged(ldc_ctx* c, const float* x, int t, const float* cond, const int32_t* latent_lens_host, int B, int Lmax,
                                       int Fmax, float* eps_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!x || !cond || !eps_out) return fail(LDC_E_INVALID, "null tensor");
  if (t < 0 || t >= c->unet.timesteps) return fail(LDC_E_INVALID, "t out of range");
  LDCCHK(check_unet_args(c, B, Lmax, Fmax));
  LDCCHK(check_ragged_lengths(latent_lens_host, B, Lmax, ragged_latent_quantum(c), "latent frames"));
  if (c->w8) return fail(LDC_E_INVALID, "ragged batches are not available on the fp8 engine (its fused forms have no length-aware variant): use dtype bf16 or f32");
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(get_halves(c, B, Lmax, Fmax, s, &h, true));
  LDCCHK(write_plan_lens(c, h, std::vector<int>(latent_lens_host, latent_lens_host + B), s));
  LDCCHK(load_cond(c, h, cond, s));
  LDCCHK(load_x(c, h, x, s));
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    HIPCHK(launch_mask_rows(c->dt, pl->x_cl, pl->B, Lmax, c->unet.channels, pl->lens, 0, s));   // (whatever the caller's padding holds)
    HIPCHK(launch_step_set(pl->step_state, t, 0, c->cur_key, s));
    HIPCHK(launch_step_begin(c->unet.ss_table, c->unet.ss_stride, pl->step_state, pl->cur_ss, nullptr, s, pl->zero_ptr, pl->zero_bytes));
    LDCCHK(run_ops(c, pl, true, s));
    HIPCHK(launch_mask_rows(c->dt, pl->eps_cl, pl->B, Lmax, c->unet.channels, pl->lens, 0, s));   // (final_conv's bias)
    HIPCHK(launch_from_cl(c->dt, pl->eps_cl, eps_out + (size_t)h.b0[k] * c->unet.channels * Lmax, pl->B, c->unet.channels, Lmax, nullptr,
                          0, 0.f, s));
  }
  return finish_stream(c, stream);
}

static int ensure_outnorm(ldc_ctx* c, int B) {
  const size_t need = output_normalise_ws_bytes(B);
  if (need <= c->outnorm_ws_bytes) return LDC_OK;
  HIPCHK(counted_device_sync());
  if (c->outnorm_ws) HIPCHK(hipFree(c->outnorm_ws));
  c->outnorm_ws = nullptr;
  HIPCHK(hipMalloc(&c->outnorm_ws, need * 2));
  c->outnorm_ws_bytes = need * 2;
  return LDC_OK;
}

extern "C" int ldc_output_normalise(ldc_ctx* c, float* wav, int B, int T, int per_item, void* stream) {
  if (!c) return fail(LDC_E_INVALID, "null ctx");
  if (!wav || B <= 0 || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  HIPCHK(hipSetDevice(c->device));
  LDCCHK(ensure_outnorm(c, B));
  hipStream_t s = pick_stream(c, stream);
  HIPCHK(launch_output_normalise(wav, B, T, per_item ? 1 : 0, c->outnorm_ws, s));
  return finish_stream(c, stream);
}

// synthesis() body for one resident batch (sample.py:94-134): ldc_decode (DDPM halfway sampling, ddim = false) and ldc_decode_ddim
// (n_steps DDIM iterations on the schedule ddim_schedule left in c->ddim_host; draws: some of them add noise)
// the front end's source: a waveform [B,1,T] (cond encoder -> RVQ) or RVQ codes (dequantisation only; one of codes / packed)
struct FrontSrc {
  const float* wav = nullptr;
  const int64_t* codes = nullptr;
  const uint8_t* packed = nullptr;
  int64_t packed_stride = 0;
  int bits = 0, n_q = 0;
};

// The sender's front end of a right-padded batch (ldc_decode_ragged, ldc_get_cond_ragged): cond encoder -> RVQ -> mask over items
// b0 .. b0 + Bk - 1 of `wav` [B][T] (zero behind every item).  lens: the whole batch's lengths in samples (host); flens_dev: its
// condition frames per item (device).  The rows (scratch, [Bk * F][D]) and the codes ([n_q][B][F]; only with b0 = 0, Bk = B) of an
// item are those of get_cond_rows on the item alone, and 0 behind its last frame (RVQ is per frame).
static int ragged_cond_rows(ldc_ctx* c, const float* wav, int B, int b0, int Bk, int T, const int32_t* lens, const int* flens_dev,
                            float bandwidth, Arena& ar, bool dry, hipStream_t sk, float** q_rows, int* F_out, int64_t* codes_out,
                            int teams) {
  const Codec& cc = c->codec[LDC_MODEL_COND];
  const int F = T / cc.hop, D = c->cfg.rep_dims, n_q = n_q_for_bandwidth(c, bandwidth);
  if (codes_out && (b0 != 0 || Bk != B)) return fail(LDC_E_INVALID, "internal: the codes of a ragged batch are written for the whole batch");
  float* qr = nullptr;
  int Fq = 0;
  LDCCHK(get_cond_rows(c, wav + (size_t)b0 * T, Bk, T, bandwidth, ar, dry, sk, &qr, &Fq, codes_out, teams));
  if (!dry && Fq != F) return fail(LDC_E_INVALID, "internal: encoder produced %d frames, expected %d", Fq, F);
  // an item with no more frames than the encoder's last conv pads on the left (k - 1 = 6) is NOT a prefix of its padded self -- the
  // reference's reflect padding falls back to zeros plus a shorter reflection when the input is that short (conv.py:81-98) -- so such
  // an item is encoded once more on its own and its rows and codes replace the batch's
  const int short_max = cc.enc.empty() ? 0 : cc.enc.back().k - 1;
  for (int b = b0; b < b0 + Bk; ++b) {
    const int Fb = lens[b] / cc.hop;
    if (Fb > short_max) continue;
    float* q1 = nullptr;
    int F1 = 0;
    int64_t* codes1 = codes_out ? (int64_t*)ar.alloc((size_t)n_q * Fb * 8) : nullptr;
    LDCCHK(get_cond_rows(c, wav + (size_t)b * T, 1, lens[b], bandwidth, ar, dry, sk, &q1, &F1, codes1, teams));
    if (dry) continue;
    HIPCHK(hipMemcpyAsync(qr + (size_t)(b - b0) * F * D, q1, (size_t)F1 * D * 4, hipMemcpyDeviceToDevice, sk));
    if (codes_out)
      HIPCHK(hipMemcpy2DAsync(codes_out + (size_t)b * F, (size_t)B * F * 8, codes1, (size_t)F1 * 8, (size_t)F1 * 8, n_q, hipMemcpyDeviceToDevice, sk));
  }
  if (!dry) {   // codes and condition behind an item's last frame are 0
    if (codes_out) HIPCHK(launch_mask_codes(codes_out, n_q, Bk, F, flens_dev + b0, sk));
    HIPCHK(launch_mask_rows(DT_F32, qr, Bk, F, D, flens_dev + b0, 0, sk));
  }
  *q_rows = qr;
  *F_out = F;
  return LDC_OK;
}

// rag (ldc_decode_ragged, ldc_decode_codes_ragged): the items' own lengths in samples (host, validated); T is then the padded length
// seeds (ldc_decode_seeded, ldc_decode_codes_seeded; [B], host): item b draws under seeds[b] as if alone ("Item seeds");
// noise is null and per_item 1, the context's noise epoch is neither read nor advanced
// sampler: SAMPLER_DDPM, SAMPLER_DDIM (the schedule in c->ddim_host) or SAMPLER_DPM (c->dpm_host; draws false, noise null)
static int decode_body(ldc_ctx* c, const FrontSrc& src, int B, int T, int n_steps, int sampler, bool draws, const float* noise, int per_item,
                       float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream, const int32_t* rag = nullptr,
                       const uint64_t* seeds = nullptr) {
  const Codec& cc = c->codec[LDC_MODEL_COND];
  const Codec& mc = c->codec[LDC_MODEL_MAIN];
  if (T % cc.hop || T % mc.hop) return fail(LDC_E_INVALID, "T must be a multiple of %d and %d (sample.py:87 trims to 640)", cc.hop, mc.hop);
  const int F = T / cc.hop, L = T / mc.hop, D = c->cfg.rep_dims;
  LDCCHK(check_unet_args(c, B, L, F));
  LDCCHK(ensure_outnorm(c, B));
  hipStream_t s = pick_stream(c, stream);
  if (sampler == SAMPLER_DDIM) LDCCHK(ddim_upload(c, s));   // (in front of everything: the parts' streams fork from s behind it)
  if (sampler == SAMPLER_DPM) LDCCHK(dpm_upload(c, s));
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h, rag != nullptr));
  if (sampler == SAMPLER_DPM) LDCCHK(ensure_history(c, h));
  std::vector<int> rag_lat, rag_fr;   // ragged: latent / condition frames per item
  if (rag) {
    for (int b = 0; b < B; ++b) { rag_lat.push_back(rag[b] / mc.hop); rag_fr.push_back(rag[b] / cc.hop); }
    LDCCHK(write_plan_lens(c, h, rag_lat, s));
  }
  if (seeds) LDCCHK(write_item_keys(c, h, seeds, s));   // (on s, in front of the parts' forks and of the loop)
  // The codec front end (cond encoder -> RVQ -> upsampler -> start image) and back end (decoder) are chains of ~40 latency-bound
  // launches each (fp32 convs on a fraction of the CUs, LSTM recurrences): with per-utterance normalisation nothing couples the
  // items, so every batch part runs its own front / back end on its own stream, like its denoise steps, and the parts' chains fill
  // each other's gaps (round 5; `split_ends` 0 / LDC_NO_SPLIT_ENDS restores the whole-batch ends).  The RVQ codes are written
  // [n_q][B][F]: a caller that wants them gets the whole-batch path.
  const bool split_ends = c->split_ends && per_item && !codes_out && h.n >= 2 && parts_parallel(c, h);
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    float* x = latents_out ? latents_out : (float*)ar.alloc((size_t)B * D * L * 4);
    float* mx = (float*)ar.alloc((size_t)B * 4);
    // ragged: the whole batch's lengths for the codec ends (a part reads its slice), and a copy of the waveform whose padding is zero.
    // Encoder and decoder are causal (left reflect padding, forward LSTM, transposed convs trimmed on the right), so an item's first
    // F_b frames / T_b samples in the padded layout are what it gives alone; everything behind them is cut off below.
    int *lens_all = nullptr, *flens_all = nullptr;
    const float* wav_in = src.wav;
    if (rag) {
      lens_all = (int*)ar.alloc((size_t)B * 4);
      flens_all = (int*)ar.alloc((size_t)B * 4);
      float* wm = src.wav ? (float*)ar.alloc((size_t)B * T * 4) : nullptr;
      if (!dry) {
        HIPCHK(launch_lens_write(lens_all, rag_lat.data(), B, s));
        HIPCHK(launch_lens_write(flens_all, rag_fr.data(), B, s));
        if (wm) {
          HIPCHK(hipMemcpyAsync(wm, src.wav, (size_t)B * T * 4, hipMemcpyDeviceToDevice, s));
          HIPCHK(launch_mask_rows(DT_F32, wm, B, L, mc.hop, lens_all, 0, s));
        }
      }
      wav_in = wm;
    }
    if (!dry && split_ends) LDCCHK(fork_parts(c, h, s));
    const int n_front = split_ends ? h.n : 1;
    // From here to the final join the parts' streams carry work that only join_parts orders against the caller's stream (and against the
    // scratch arena the next call reuses): the forked regions collect their first error and the call joins before it reports it.
    bool parts_open = !dry && split_ends;
    auto bail = [&](int rc) -> int {
      if (parts_open) (void)join_parts(c, h, s);
      parts_open = false;
      return rc;
    };
    auto front_end = [&]() -> int {
    for (int k = 0; k < n_front; ++k) {
      hipStream_t sk = (split_ends && k > 0) ? c->aux_stream[k] : s;
      const int b0 = split_ends ? h.b0[k] : 0, Bk = split_ends ? h.p[k]->B : B;
      float* qr = nullptr;
      int Fq = 0;
      if (src.wav) {
        if (rag) LDCCHK(ragged_cond_rows(c, wav_in, B, b0, Bk, T, rag, flens_all, 0.f, ar, dry, sk, &qr, &Fq, codes_out, n_front));
        else LDCCHK(get_cond_rows(c, wav_in + (size_t)b0 * T, Bk, T, 0.f, ar, dry, sk, &qr, &Fq, codes_out, n_front));
      } else {
        qr = (float*)ar.alloc((size_t)Bk * F * D * 4);
        Fq = F;
        // ragged: rows behind an item's frames are 0 and their codes are never read (a packed item ends after its own bytes)
        if (!dry)
          HIPCHK(launch_rvq_dequant(src.codes, src.packed, src.packed_stride, src.bits, src.n_q, B, b0, Bk, F, cc.codebooks, cc.bins, D, qr,
                                    c->dev_flag_dev, sk, rag ? flens_all + b0 : nullptr));
      }
      if (!dry && Fq != F) return fail(LDC_E_INVALID, "internal: encoder produced %d frames, expected %d", Fq, F);
      // start image: upsample, /= max|.|+1e-8 (sample.py:125-129)
      void* up = nullptr;
      int Lu = 0;
      LDCCHK(upsample_rows(c, qr, Bk, F, ar, dry, sk, &up, &Lu, rag ? flens_all + b0 : nullptr));   // ragged: the start image is zero in the padding, its maximum the item's own
      if (dry) continue;
      if (cond_out) HIPCHK(launch_from_cl(DT_F32, qr, cond_out + (size_t)b0 * D * F, Bk, D, F, nullptr, 0, 0.f, sk));
      HIPCHK(hipMemsetAsync(mx + b0, 0, (size_t)Bk * 4, sk));
      HIPCHK(launch_maxabs(DT_F32, up, Bk, (int64_t)L * D, per_item ? 1 : 0, mx + b0, sk));
      HIPCHK(launch_from_cl(DT_F32, up, x + (size_t)b0 * D * L, Bk, D, L, mx + b0, per_item ? 1 : 0, 1e-8f, sk));
      // process_cond for the UNet (rows are already channels-last fp32)
      for (int kk = 0; kk < h.n; ++kk) {
        if (split_ends && kk != k) continue;
        Plan* pl = h.p[kk];
        HIPCHK(hipMemcpyAsync(pl->cond_in_cl, qr + (size_t)(h.b0[kk] - b0) * F * D, (size_t)pl->B * F * D * 4, hipMemcpyDeviceToDevice, sk));
        LDCCHK(run_ops(c, pl, false, sk));
        HIPCHK(launch_to_cl(c->dt, x + (size_t)h.b0[kk] * c->unet.channels * pl->L, pl->x_cl, pl->B, c->unet.channels, pl->L, nullptr, 0, 0.f, sk));
      }
    }
    return LDC_OK;
    };
    { const int fr = front_end(); if (fr != LDC_OK) return bail(fr); }
    if (!dry) {
      // The parts stay on their streams from the front end to the back end (no join in front of the loop: it forks the part streams behind
      // part 0's front end itself; none behind it when the per-part replay path ran): they de-phase by the front ends' serialised pieces
      // (the cooperative LSTMs), and one part's latency-bound back end then runs under the other's last denoise steps.
      // (c->ends_join / LDC_ENDS_JOIN: both joins as before, for A/B runs)
      if (split_ends && c->ends_join) { parts_open = false; LDCCHK(join_parts(c, h, s)); }
      if (!seeds) next_noise_key(c, noise == nullptr && draws);
      bool forked = false;
      StepSampler sm;
      sm.kind = sampler;
      sm.item_seeds = seeds != nullptr;
      sm.ddim = sampler == SAMPLER_DDIM ? c->ddim_table : nullptr;
      sm.dpm = sampler == SAMPLER_DPM ? c->dpm_table : nullptr;
      const int dr = denoise_loop(c, h, B, x, noise, n_steps, s, (split_ends && !c->ends_join) ? &forked : nullptr, sm);
      if (dr != LDC_OK) return bail(dr);
      if (split_ends && !forked) { parts_open = false; LDCCHK(fork_parts(c, h, s)); }   // (the loop joined, or never left s)
      parts_open = split_ends;
    }
    // decoder (quirk Q3: no x18 un-scaling on this path, sample.py:131)
    int Lo_all = T;
    auto back_end = [&]() -> int {
    for (int k = 0; k < n_front; ++k) {
      hipStream_t sk = (split_ends && k > 0) ? c->aux_stream[k] : s;
      const int b0 = split_ends ? h.b0[k] : 0, Bk = split_ends ? h.p[k]->B : B;
      SeaRun R{c, &ar, sk, dry, Bk};
      R.side = h.n <= 2 ? k : -1;   // (aux_stream[2], [3] are free when the batch has at most two parts)
      R.teams = h.n;
      void* zc = ar.alloc((size_t)Bk * L * D * 4);
      if (!dry) HIPCHK(launch_to_cl(DT_F32, x + (size_t)b0 * D * L, zc, Bk, D, L, nullptr, 0, 0.f, sk));
      void* y = nullptr;
      int Lo = 0, Cd = 0;
      LDCCHK(run_seanet(R, mc.dec, zc, L, &y, &Lo, &Cd));
      if (!dry) HIPCHK(hipMemcpyAsync(wav_out + (size_t)b0 * Lo, y, (size_t)Bk * Lo * 4, hipMemcpyDeviceToDevice, sk));
      Lo_all = Lo;
    }
    return LDC_OK;
    };
    { const int br = back_end(); if (br != LDC_OK) return bail(br); }
    if (!dry) {
      if (split_ends) { parts_open = false; LDCCHK(join_parts(c, h, s)); }
      if (rag && Lo_all != T) return fail(LDC_E_INVALID, "internal: decoder produced %d samples, expected %d", Lo_all, T);
      HIPCHK(launch_output_normalise(wav_out, B, Lo_all, per_item ? 1 : 0, c->outnorm_ws, s, lens_all, mc.hop));
    }
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

extern "C" int ldc_decode(ldc_ctx* c, const float* wav, int B, int T, int n_steps, const float* noise, int per_item,
                          float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (!wav || !wav_out || B <= 0 || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  if (n_steps < 1 || n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps must be in [1,%d]", c->unet.timesteps);
  FrontSrc src;
  src.wav = wav;
  return decode_body(c, src, B, T, n_steps, SAMPLER_DDPM, true, noise, per_item, wav_out, latents_out, cond_out, codes_out, stream);
}

// the decode with DDIM sampling from t_start (the DDIM counterpart of halfway_sampling: the start image is the upsampled,
// max-normalised condition, as in ldc_decode); noise (optional) [n_steps][B][C][L]
extern "C" int ldc_decode_ddim(ldc_ctx* c, const float* wav, int B, int T, int t_start, int n_steps, float eta, const float* noise,
                               int per_item, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (!wav || !wav_out || B <= 0 || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  bool draws = false;
  LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  FrontSrc src;
  src.wav = wav;
  return decode_body(c, src, B, T, n_steps, SAMPLER_DDIM, draws, noise, per_item, wav_out, latents_out, cond_out, codes_out, stream);
}

// ldc_decode / ldc_decode_ddim on a batch of items of different lengths (right-padded to Tmax): one call, every item as if alone
static int decode_ragged_impl(ldc_ctx* c, const float* wav, const int32_t* lengths_host, int B, int Tmax, int t_start, int n_steps, float eta,
                              const float* noise, const uint64_t* seeds, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out,
                              void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (!wav || !wav_out || B <= 0 || Tmax <= 0) return fail(LDC_E_INVALID, "bad arguments");
  if (t_start < 0) return fail(LDC_E_INVALID, "t_start must be >= 0 (0: DDPM halfway sampling)");
  const long long quantum = lcm_ll(c->codec[LDC_MODEL_COND].hop, (long long)c->codec[LDC_MODEL_MAIN].hop << unet_halvings(c));
  LDCCHK(check_ragged_lengths(lengths_host, B, Tmax, quantum, "samples"));
  if (c->w8) return fail(LDC_E_INVALID, "ragged batches are not available on the fp8 engine (its fused forms have no length-aware variant): use dtype bf16 or f32");
  bool draws = true;
  if (t_start > 0) LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  else if (n_steps < 1 || n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps must be in [1,%d]", c->unet.timesteps);
  FrontSrc src;
  src.wav = wav;
  return decode_body(c, src, B, Tmax, n_steps, t_start > 0 ? SAMPLER_DDIM : SAMPLER_DDPM, draws, noise, 1, wav_out, latents_out, cond_out, codes_out,
                     stream, lengths_host, seeds);
}
extern "C" int ldc_decode_ragged(ldc_ctx* c, const float* wav, const int32_t* lengths_host, int B, int Tmax, int t_start, int n_steps, float eta,
                                 const float* noise, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  return decode_ragged_impl(c, wav, lengths_host, B, Tmax, t_start, n_steps, eta, noise, nullptr, wav_out, latents_out, cond_out, codes_out, stream);
}

// ldc_get_cond on a right-padded batch (the sender side of ragged batches): every item's rows and codes as if encoded alone, 0 behind
// its lengths[b] / hop frames.  Lengths are positive multiples of the cond hop: nothing here needs the UNet's quantum.
extern "C" int ldc_get_cond_ragged(ldc_ctx* c, const float* wav, const int32_t* lengths_host, int B, int Tmax, float bandwidth, float* cond_out,
                                   int64_t* codes_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_COND));
  if (!wav || !cond_out || B <= 0 || Tmax <= 0) return fail(LDC_E_INVALID, "bad arguments");
  const Codec& cc = c->codec[LDC_MODEL_COND];
  LDCCHK(check_ragged_lengths(lengths_host, B, Tmax, cc.hop, "samples"));
  hipStream_t s = pick_stream(c, stream);
  const int F = Tmax / cc.hop, D = c->cfg.rep_dims;
  std::vector<int> fr(B);
  for (int b = 0; b < B; ++b) fr[b] = lengths_host[b] / cc.hop;
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    int* flens = (int*)ar.alloc((size_t)B * 4);
    float* wm = (float*)ar.alloc((size_t)B * Tmax * 4);   // the waveform with zeros behind every item
    if (!dry) {
      HIPCHK(launch_lens_write(flens, fr.data(), B, s));
      HIPCHK(hipMemcpyAsync(wm, wav, (size_t)B * Tmax * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(launch_mask_rows(DT_F32, wm, B, F, cc.hop, flens, 0, s));
    }
    float* qr = nullptr;
    int Fq = 0;
    LDCCHK(ragged_cond_rows(c, wm, B, 0, B, Tmax, lengths_host, flens, bandwidth, ar, dry, s, &qr, &Fq, codes_out, 1));
    if (!dry) HIPCHK(launch_from_cl(DT_F32, qr, cond_out, B, D, F, nullptr, 0, 0.f, s));
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

// the receiver side: ldc_decode / ldc_decode_ddim from RVQ codes.  The context-free refusals come first (a NULL context sees them
// too); then those that need the codec; bad code VALUES are found on the device (LDC_E_INVALID "[bad_code]", see check_dev_flag).
static int codes_args(const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B, int F,
                      const float* wav_out) {
  if ((codes == nullptr) == (packed == nullptr)) return fail(LDC_E_INVALID, "exactly one of codes / packed must be given");
  if (!wav_out || B <= 0 || F <= 0) return fail(LDC_E_INVALID, "bad arguments");
  if (n_q < 1) return fail(LDC_E_INVALID, "n_q must be >= 1");
  if (packed && (bits < 1 || bits > 16)) return fail(LDC_E_INVALID, "bits must be in [1,16]");
  if (packed && packed_stride < ldc_packed_bytes(n_q, F, bits))
    return fail(LDC_E_INVALID, "packed_stride %lld < %lld packed bytes per item", (long long)packed_stride, (long long)ldc_packed_bytes(n_q, F, bits));
  return LDC_OK;
}

static int codes_src(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int F, FrontSrc* src,
                     int* T) {
  const Codec& cd = c->codec[LDC_MODEL_COND];
  if (n_q > cd.n_q_layers) return fail(LDC_E_INVALID, "n_q must be in [1,%d]", cd.n_q_layers);
  if (packed) {
    int need = 0;
    while ((1ll << need) < cd.bins) ++need;
    if (bits < need) return fail(LDC_E_INVALID, "bits must be in [%d,16] for %d bins", need, cd.bins);
  }
  if ((int64_t)F * cd.hop > INT32_MAX) return fail(LDC_E_INVALID, "F too large");
  *T = F * cd.hop;
  src->codes = codes;
  src->packed = packed;
  src->packed_stride = packed_stride;
  src->bits = bits;
  src->n_q = n_q;
  return LDC_OK;
}

extern "C" int ldc_decode_codes(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B,
                                int F, int n_steps, const float* noise, int per_item, float* wav_out, float* latents_out, float* cond_out,
                                void* stream) {
  LDCCHK(codes_args(codes, packed, packed_stride, bits, n_q, B, F, wav_out));
  if (n_steps < 1) return fail(LDC_E_INVALID, "n_steps must be >= 1");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps must be in [1,%d]", c->unet.timesteps);
  FrontSrc src;
  int T = 0;
  LDCCHK(codes_src(c, codes, packed, packed_stride, bits, n_q, F, &src, &T));
  return decode_body(c, src, B, T, n_steps, SAMPLER_DDPM, true, noise, per_item, wav_out, latents_out, cond_out, nullptr, stream);
}

extern "C" int ldc_decode_codes_ddim(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q,
                                     int B, int F, int t_start, int n_steps, float eta, const float* noise, int per_item, float* wav_out,
                                     float* latents_out, float* cond_out, void* stream) {
  LDCCHK(codes_args(codes, packed, packed_stride, bits, n_q, B, F, wav_out));
  if (!(eta >= 0.0f && eta <= 1.0f)) return fail(LDC_E_INVALID, "eta must be a finite value in [0, 1]");
  if (t_start < 1) return fail(LDC_E_INVALID, "t_start must be >= 1");
  if (n_steps < 1 || n_steps > t_start) return fail(LDC_E_INVALID, "n_steps must be in [1, t_start = %d] (more would repeat timesteps)", t_start);
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  FrontSrc src;
  int T = 0;
  LDCCHK(codes_src(c, codes, packed, packed_stride, bits, n_q, F, &src, &T));
  bool draws = false;
  LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  return decode_body(c, src, B, T, n_steps, SAMPLER_DDIM, draws, noise, per_item, wav_out, latents_out, cond_out, nullptr, stream);
}
// ldc_decode_codes / ldc_decode_codes_ddim with the length semantics of ldc_decode_ragged: frames_host[b] frames of item b are its own
// (multiples of the ragged quantum / 320), the codes behind them are never read, a packed item's stream is ldc_packed_bytes(n_q,
// frames_host[b], bits) long; t_start 0: DDPM halfway sampling, > 0: DDIM; per-item normalisation; outputs 0 beyond an item's length.
static int decode_codes_ragged_impl(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B,
                                    int Fmax, const int32_t* frames_host, int t_start, int n_steps, float eta, const float* noise,
                                    const uint64_t* seeds, float* wav_out, float* latents_out, float* cond_out, void* stream) {
  if ((codes == nullptr) == (packed == nullptr)) return fail(LDC_E_INVALID, "exactly one of codes / packed must be given");
  if (!wav_out || B <= 0 || Fmax <= 0) return fail(LDC_E_INVALID, "bad arguments");
  if (!frames_host) return fail(LDC_E_INVALID, "null lengths");
  if (n_q < 1) return fail(LDC_E_INVALID, "n_q must be >= 1");
  if (packed && (bits < 1 || bits > 16)) return fail(LDC_E_INVALID, "bits must be in [1,16]");
  if (t_start < 0) return fail(LDC_E_INVALID, "t_start must be >= 0 (0: DDPM halfway sampling)");
  if (n_steps < 1) return fail(LDC_E_INVALID, "n_steps must be >= 1");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  const Codec& cc = c->codec[LDC_MODEL_COND];
  const long long quantum = lcm_ll(cc.hop, (long long)c->codec[LDC_MODEL_MAIN].hop << unet_halvings(c)) / cc.hop;
  LDCCHK(check_ragged_lengths(frames_host, B, Fmax, quantum, "condition frames"));
  if (packed) {   // a row holds its longest item; shorter items end sooner
    int64_t need = 0;
    for (int b = 0; b < B; ++b) need = std::max(need, (int64_t)ldc_packed_bytes(n_q, frames_host[b], bits));
    if (packed_stride < need) return fail(LDC_E_INVALID, "packed_stride %lld < %lld packed bytes of the longest item", (long long)packed_stride, (long long)need);
  }
  if (c->w8) return fail(LDC_E_INVALID, "ragged batches are not available on the fp8 engine (its fused forms have no length-aware variant): use dtype bf16 or f32");
  FrontSrc src;
  int T = 0;
  LDCCHK(codes_src(c, codes, packed, packed_stride, bits, n_q, Fmax, &src, &T));
  bool draws = true;
  if (t_start > 0) LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  else if (n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps must be in [1,%d]", c->unet.timesteps);
  std::vector<int32_t> lens(B);
  for (int b = 0; b < B; ++b) lens[b] = frames_host[b] * cc.hop;
  return decode_body(c, src, B, T, n_steps, t_start > 0 ? SAMPLER_DDIM : SAMPLER_DDPM, draws, noise, 1, wav_out, latents_out, cond_out, nullptr, stream,
                     lens.data(), seeds);
}
extern "C" int ldc_decode_codes_ragged(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B,
                                       int Fmax, const int32_t* frames_host, int t_start, int n_steps, float eta, const float* noise,
                                       float* wav_out, float* latents_out, float* cond_out, void* stream) {
  return decode_codes_ragged_impl(c, codes, packed, packed_stride, bits, n_q, B, Fmax, frames_host, t_start, n_steps, eta, noise, nullptr, wav_out,
                                  latents_out, cond_out, stream);
}

// ---- item seeds ("Item seeds"): the decodes above with one Philox seed per item; item b draws what reseed(seeds[b])
// followed by the unseeded entry at B = 1 on the item's own length draws.  Per-item normalisation at both ends, always.  The two
// context-free refusals of every seeded entry come first (a NULL context sees them too).
int seeded_args(int sampler, const uint64_t* seeds) {
  if (sampler != SAMPLER_DDPM && sampler != SAMPLER_DDIM)
    return fail(LDC_E_INVALID, "sampler %d: a seeded call takes 0 (DDPM) or 1 (DDIM) (DPM-Solver++ draws nothing: there is nothing to seed)", sampler);
  if (!seeds) return fail(LDC_E_INVALID, "seeds NULL: a seeded call takes one seed per item");
  return LDC_OK;
}

extern "C" int ldc_decode_seeded(ldc_ctx* c, const float* wav, const int32_t* lengths_host, int B, int Tmax, int sampler, int t_start, int n_steps,
                                 float eta, const uint64_t* seeds, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out,
                                 void* stream) {
  LDCCHK(seeded_args(sampler, seeds));
  if (sampler == SAMPLER_DDIM && t_start < 1) return fail(LDC_E_INVALID, "t_start %d: must be >= 1 with sampler 1 (DDIM)", t_start);
  if (lengths_host)   // (t_start 0 is the ragged entries' word for DDPM)
    return decode_ragged_impl(c, wav, lengths_host, B, Tmax, sampler == SAMPLER_DDIM ? t_start : 0, n_steps, eta, nullptr, seeds, wav_out, latents_out,
                              cond_out, codes_out, stream);
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (!wav || !wav_out || B <= 0 || Tmax <= 0) return fail(LDC_E_INVALID, "bad arguments");
  bool draws = true;
  if (sampler == SAMPLER_DDIM) LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  else if (n_steps < 1 || n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps must be in [1,%d]", c->unet.timesteps);
  FrontSrc src;
  src.wav = wav;
  return decode_body(c, src, B, Tmax, n_steps, sampler, draws, nullptr, 1, wav_out, latents_out, cond_out, codes_out, stream, nullptr, seeds);
}

extern "C" int ldc_decode_codes_seeded(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B,
                                       int Fmax, const int32_t* frames_host, int sampler, int t_start, int n_steps, float eta, const uint64_t* seeds,
                                       float* wav_out, float* latents_out, float* cond_out, void* stream) {
  LDCCHK(seeded_args(sampler, seeds));
  if (sampler == SAMPLER_DDIM && t_start < 1) return fail(LDC_E_INVALID, "t_start %d: must be >= 1 with sampler 1 (DDIM)", t_start);
  if (frames_host)
    return decode_codes_ragged_impl(c, codes, packed, packed_stride, bits, n_q, B, Fmax, frames_host, sampler == SAMPLER_DDIM ? t_start : 0, n_steps,
                                    eta, nullptr, seeds, wav_out, latents_out, cond_out, stream);
  LDCCHK(codes_args(codes, packed, packed_stride, bits, n_q, B, Fmax, wav_out));
  if (sampler == SAMPLER_DDIM) {   // (the context-free refusals of ldc_decode_codes_ddim)
    if (!(eta >= 0.0f && eta <= 1.0f)) return fail(LDC_E_INVALID, "eta must be a finite value in [0, 1]");
    if (n_steps < 1 || n_steps > t_start) return fail(LDC_E_INVALID, "n_steps must be in [1, t_start = %d] (more would repeat timesteps)", t_start);
  } else if (n_steps < 1) return fail(LDC_E_INVALID, "n_steps must be >= 1");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (sampler == SAMPLER_DDPM && n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps must be in [1,%d]", c->unet.timesteps);
  FrontSrc src;
  int T = 0;
  LDCCHK(codes_src(c, codes, packed, packed_stride, bits, n_q, Fmax, &src, &T));
  bool draws = true;
  if (sampler == SAMPLER_DDIM) LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  return decode_body(c, src, B, T, n_steps, sampler, draws, nullptr, 1, wav_out, latents_out, cond_out, nullptr, stream, nullptr, seeds);
}

// ---- the decodes with DPM-Solver++(2M) sampling from t_start: ldc_decode_ddim / ldc_decode_ragged / ldc_decode_codes_ddim without eta
// and noise.  The context-free refusals come first (a NULL context sees them too).
static int dpm_front_args(int t_start, int n_steps) {
  if (t_start < 1) return fail(LDC_E_INVALID, "t_start %d: must be >= 1", t_start);
  if (n_steps < 1 || n_steps > t_start) return fail(LDC_E_INVALID, "n_steps %d: must be in [1, t_start = %d] (more would repeat timesteps)", n_steps, t_start);
  return LDC_OK;
}

extern "C" int ldc_decode_dpm(ldc_ctx* c, const float* wav, int B, int T, int t_start, int n_steps, int per_item, float* wav_out,
                              float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  LDCCHK(dpm_front_args(t_start, n_steps));
  if (!wav || !wav_out || B <= 0 || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  LDCCHK(dpm_schedule(c, t_start, n_steps));
  FrontSrc src;
  src.wav = wav;
  return decode_body(c, src, B, T, n_steps, SAMPLER_DPM, false, nullptr, per_item, wav_out, latents_out, cond_out, codes_out, stream);
}

extern "C" int ldc_decode_ragged_dpm(ldc_ctx* c, const float* wav, const int32_t* lengths_host, int B, int Tmax, int t_start, int n_steps,
                                     float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  LDCCHK(dpm_front_args(t_start, n_steps));
  if (!wav || !wav_out || B <= 0 || Tmax <= 0) return fail(LDC_E_INVALID, "bad arguments");
  if (!lengths_host) return fail(LDC_E_INVALID, "null lengths");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  const long long quantum = lcm_ll(c->codec[LDC_MODEL_COND].hop, (long long)c->codec[LDC_MODEL_MAIN].hop << unet_halvings(c));
  LDCCHK(check_ragged_lengths(lengths_host, B, Tmax, quantum, "samples"));
  if (c->w8) return fail(LDC_E_INVALID, "ragged batches are not available on the fp8 engine (its fused forms have no length-aware variant): use dtype bf16 or f32");
  LDCCHK(dpm_schedule(c, t_start, n_steps));
  FrontSrc src;
  src.wav = wav;
  return decode_body(c, src, B, Tmax, n_steps, SAMPLER_DPM, false, nullptr, 1, wav_out, latents_out, cond_out, codes_out, stream, lengths_host);
}

extern "C" int ldc_decode_codes_dpm(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B,
                                    int F, int t_start, int n_steps, int per_item, float* wav_out, float* latents_out, float* cond_out,
                                    void* stream) {
  LDCCHK(codes_args(codes, packed, packed_stride, bits, n_q, B, F, wav_out));
  LDCCHK(dpm_front_args(t_start, n_steps));
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  FrontSrc src;
  int T = 0;
  LDCCHK(codes_src(c, codes, packed, packed_stride, bits, n_q, F, &src, &T));
  LDCCHK(dpm_schedule(c, t_start, n_steps));
  return decode_body(c, src, B, T, n_steps, SAMPLER_DPM, false, nullptr, per_item, wav_out, latents_out, cond_out, nullptr, stream);
}


// ---- coupled windows: recordings longer than the UNet's window, each decoded on ONE shared latent -----------------
// The overlapping windows of R recordings are the items of an ordinary equal-length batch; after every UNet pass their eps are blended per
// global frame of their recording and the recording's single fp32 state is updated from the blend (windows_group_update_kernel, in place of
// the update launch).  Every recording keeps its own layout, state block, noise and (DPM) x0 history; the timestep and the schedule are the
// call's.  x, eps, the history and every step of a tape are packed: recording r's [C][Ltot_r] block at C * off_r floats (off_r: the frames
// of the recordings in front), the raw condition's [Cc][Ftot_r] block at Cc * off_r / up.  A single-recording call (ldc_*_windows) is the
// group of one: it differs in its refusals' words, in its one-window case (Ltot <= Lw) and in drawing under the context's Philox epoch.
// (the builders are the pure functions of ldc_windows.h: WinLayout, win_layout_build, win_parts_split, win_ptr_tables, win_group_build)
// the layout, the cover table and the weights (double, rounded once to float) of (Ltot, Lw, overlap); every refusal names its value
static int window_layout(int Ltot, int Lw, int O, int up, int max_windows, WinLayout* out) {
  std::string err;
  const int rc = win_layout_build(Ltot, Lw, O, up, max_windows, out, &err);
  if (rc) return fail(rc == 1 ? LDC_E_INVALID : LDC_E_STATE, "%s", err.c_str());
  return LDC_OK;
}

// The layout for up to max_windows (<= 128) windows: starts_out [max_windows], zero behind W.  Host-only: needs no context.  (The calls
// with a context take 32 windows.)
extern "C" int ldc_window_layout_n(int Ltot, int Lw, int overlap, int up, int max_windows, int* starts_out, float* weights_out) {
  WinLayout lay;
  LDCCHK(window_layout(Ltot, Lw, overlap, up, max_windows, &lay));
  if (starts_out)
    for (int k = 0; k < max_windows; ++k) starts_out[k] = k < lay.W ? lay.start[k] : 0;
  if (weights_out) std::copy(lay.weight.begin(), lay.weight.end(), weights_out);
  return lay.W;
}

extern "C" int ldc_window_layout(int Ltot, int Lw, int overlap, int up, int* starts_out, float* weights_out) {
  return ldc_window_layout_n(Ltot, Lw, overlap, up, kWinPerPart, starts_out, weights_out);
}

// The partition of W windows into `parts` batch parts of contiguous windows: returns P_eff = min(parts, W) and writes first_out
// [parts + 1], the range starts (part p holds the windows [first_out[p], first_out[p + 1]); entries behind P_eff are W).  Host-only.
extern "C" int ldc_window_parts(int W, int parts, int* first_out) {
  if (!first_out) return fail(LDC_E_INVALID, "null output");
  if (W < 1 || W > kMaxWindows) return fail(LDC_E_INVALID, "W %d: must be in [1, %d]", W, kMaxWindows);
  if (parts < 1 || parts > kMaxParts) return fail(LDC_E_INVALID, "parts %d: must be in [1, %d]", parts, kMaxParts);
  if (W > kWinPerPart * parts) return fail(LDC_E_INVALID, "W %d: %d part(s) hold at most %d windows", W, parts, kWinPerPart * parts);
  return win_parts_split(W, parts, first_out);
}

static int window_group(int R, const int* Ltot, int Lw, int O, int up, WinGroup* out, bool single = false) {
  std::string err;
  const int rc = win_group_build(R, Ltot, Lw, O, up, out, &err, single);
  if (rc) return fail(rc == 1 ? LDC_E_INVALID : LDC_E_STATE, "%s", err.c_str());
  return LDC_OK;
}

// Host-only: w0_out [R + 1] (recording r's windows are the batch items w0_out[r] .. w0_out[r + 1] - 1), starts_out [32] in each
// recording's own frames (zero behind W_sum), weights_out [W_sum][Lw] or null.  Returns W_sum.
extern "C" int ldc_window_group_layout(int R, const int* Ltot, int Lw, int overlap, int up, int* w0_out, int* starts_out, float* weights_out) {
  WinGroup g;
  LDCCHK(window_group(R, Ltot, Lw, overlap, up, &g));
  if (w0_out) std::copy(g.w0.begin(), g.w0.end(), w0_out);
  if (starts_out)
    for (int k = 0; k < kWinPerPart; ++k) starts_out[k] = k < g.W_sum ? g.start[k] : 0;
  if (weights_out) std::copy(g.weight.begin(), g.weight.end(), weights_out);
  return g.W_sum;
}

// everything a windows call refuses, before any GPU work (on the caller's Lw and overlap, in the words of a single-recording call where
// `single`); then the plan of the layout -- the windows plan at B = W_sum with the packed state, the tables, the recording table and the
// tile table in its one allocation (made and uploaded on s on its first use) -- as a one-part Halves: the blend couples every window at
// every step, whatever `split` says
static int windows_prepare(ldc_ctx* c, int R, const int* Ltot, const int* Ftot, int Lw, int O, hipStream_t s, Halves* h, bool single) {
  if (c->w8) return fail(LDC_E_INVALID, "coupled windows are not available on the fp8 engine: use dtype bf16 or f32");
  if (R < 1 || R > kWinPerPart) return fail(LDC_E_INVALID, "R %d: a window group holds 1 to %d recordings", R, kWinPerPart);
  if (!Ltot || !Ftot) return fail(LDC_E_INVALID, "null list of lengths");
  const int up = upsample_factor(c), q = ragged_latent_quantum(c);
  bool longer = false;
  for (int r = 0; r < R; ++r) {
    if (Ltot[r] <= 0 || Ftot[r] <= 0 || (long long)Ftot[r] * up != Ltot[r]) {
      if (single) return fail(LDC_E_INVALID, "Ltot (%d) must equal Ftot (%d) x prod(upsampling_ratios) (%d)", Ltot[r], Ftot[r], up);
      return fail(LDC_E_INVALID, "recording %d: Ltot (%d) must equal Ftot (%d) x prod(upsampling_ratios) (%d)", r, Ltot[r], Ftot[r], up);
    }
    longer = longer || Ltot[r] > Lw;
  }
  if (longer && (Lw <= 0 || Lw % q)) return fail(LDC_E_INVALID, "Lw %d: a window must be a positive multiple of %d latent frames (the chunk quantum)", Lw, q);
  WinGroup g;
  LDCCHK(window_group(R, Ltot, Lw, O, up, &g, single));
  Lw = g.Lw;   // (a single recording no longer than the window is its one window)
  *h = Halves();
  c->call_tick = c->use_tick;
  Plan* pl = nullptr;
  LDCCHK(get_plan(c, g.W_sum, Lw, Lw / up, 0, s, &pl, false, false, 0, &g.Ltot, O));
  if (!pl->win_base) {
    const int C = c->unet.channels;
    auto pad = [](size_t n) { return (n + 255) / 256 * 256; };
    const size_t nx = pad((size_t)C * g.Lsum * 4), nc = pad((size_t)g.Lsum * 4), nw = pad((size_t)g.W_sum * Lw * 4), ns = pad((size_t)g.W_sum * 4);
    const size_t nr = pad((size_t)R * sizeof(WinGroupRec)), nt = pad(g.tile.size() * sizeof(WinGroupTile));
    const size_t total = nx + nc + nw + 2 * ns + nr + nt;
    void* base = nullptr;
    hipError_t e = hipMalloc(&base, total);
    if (e != hipSuccess) return fail(LDC_E_NOMEM, "hipMalloc(%zu) for the windows state failed: %s", total, hipGetErrorString(e));
    pl->win_base = base;
    pl->win_x = (float*)base;
    char* p = (char*)base + nx;
    int* cover = (int*)p; p += nc;
    float* weight = (float*)p; p += nw;
    int* start = (int*)p; p += ns;
    int* wrec = (int*)p; p += ns;
    WinGroupRec* rec = (WinGroupRec*)p; p += nr;
    WinGroupTile* tile = (WinGroupTile*)p;
    pl->win_group = std::move(g);   // (the host copies stay alive with the plan: the upload is asynchronous)
    const WinGroup& wg = pl->win_group;
    HIPCHK(hipMemcpyAsync(cover, wg.cover.data(), wg.cover.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(weight, wg.weight.data(), wg.weight.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(start, wg.start.data(), wg.start.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(wrec, wg.wrec.data(), wg.wrec.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(rec, wg.rec.data(), wg.rec.size() * sizeof(WinGroupRec), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(tile, wg.tile.data(), wg.tile.size() * sizeof(WinGroupTile), hipMemcpyHostToDevice, s));
    pl->wg = WinGroupTables{tile, rec, cover, weight, start, wrec, (int)wg.tile.size(), R, Lw};
    pl->wg_rec = rec;
  }
  h->n = 1;
  h->p[0] = pl;
  h->b0[0] = 0;
  c->last_halves = *h;
  return LDC_OK;
}

// The DPM-Solver++(2M) history of a windows plan: ONE x0_prev [channels][Ltot_r] fp32 block per recording, in the layout of win_x (not one
// per window).  Like the parts' histories (ensure_history) it is made by the first DPM call on the plan, outside of any capture, kept in
// pl->x0_prev until the plan goes -- behind the plan's graphs (evict_plan, drop_plans) -- and never cleared: the first iteration does not load it.
static int ensure_windows_history(ldc_ctx* c, Plan* pl) {
  if (pl->x0_prev) return LDC_OK;
  void* p = nullptr;
  const size_t bytes = (size_t)c->unet.channels * pl->win_Ltot * 4;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return fail(LDC_E_NOMEM, "hipMalloc(%zu) for the windows DPM history failed: %s", bytes, hipGetErrorString(e));
  pl->x0_prev = (float*)p;
  return LDC_OK;
}

// the sampler of a windows loop: the schedule the caller left in c->ddim_host / c->dpm_host goes to the device in front of everything else
// (before any capture), a DPM loop gets the plan's history
static int windows_sampler(ldc_ctx* c, Plan* pl, int sampler, hipStream_t s, StepSampler* sm) {
  if (sampler == SAMPLER_DDIM) LDCCHK(ddim_upload(c, s));
  if (sampler == SAMPLER_DPM) {
    LDCCHK(dpm_upload(c, s));
    LDCCHK(ensure_windows_history(c, pl));
  }
  sm->kind = sampler;
  sm->ddim = sampler == SAMPLER_DDIM ? c->ddim_table : nullptr;
  sm->dpm = sampler == SAMPLER_DPM ? c->dpm_table : nullptr;
  return LDC_OK;
}

// the windows' condition slices from the packed cond ([Cc][Ftot_r] blocks) through process_cond, as ldc_unet_forward does at B = W_sum
static int windows_load_cond(ldc_ctx* c, Plan* pl, const float* cond, hipStream_t s) {
  HIPCHK(launch_windows_group_gather(DT_F32, cond, pl->cond_in_cl, pl->B, c->unet.cond_channels, pl->F, pl->wg, upsample_factor(c), s));
  return run_ops(c, pl, false, s);
}
// the windows' input rows from the recordings' packed state
static int windows_load_x(ldc_ctx* c, Plan* pl, const float* x, hipStream_t s) {
  HIPCHK(launch_windows_group_gather(c->dt, x, pl->x_cl, pl->B, c->unet.channels, pl->L, pl->wg, 1, s));
  return LDC_OK;
}

// one UNet pass over the windows and the blend of their eps: x, eps_out packed [C][Ltot_r] blocks, cond packed [Cc][Ftot_r] blocks
static int unet_forward_windows(ldc_ctx* c, const float* x, int t, const float* cond, int R, const int* Ltot, const int* Ftot, int Lw, int overlap,
                                float* eps_out, void* stream, bool single) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!x || !cond || !eps_out) return fail(LDC_E_INVALID, "null tensor");
  if (t < 0 || t >= c->unet.timesteps) return fail(LDC_E_INVALID, "t %d: out of range [0, %d)", t, c->unet.timesteps);
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(windows_prepare(c, R, Ltot, Ftot, Lw, overlap, s, &h, single));
  Plan* pl = h.p[0];
  LDCCHK(windows_load_cond(c, pl, cond, s));
  LDCCHK(windows_load_x(c, pl, x, s));
  HIPCHK(launch_step_set(pl->step_state, t, 0, c->cur_key, s));
  HIPCHK(launch_step_begin(c->unet.ss_table, c->unet.ss_stride, pl->step_state, pl->cur_ss, nullptr, s, pl->zero_ptr, pl->zero_bytes));
  LDCCHK(run_ops(c, pl, true, s));
  HIPCHK(launch_windows_group_update(c->dt, WIN_BLEND, nullptr, pl->eps_cl, nullptr, 0, nullptr, eps_out, c->unet.channels, pl->wg, c->sched, nullptr,
                                     nullptr, s));
  return finish_stream(c, stream);
}

extern "C" int ldc_unet_forward_windows(ldc_ctx* c, const float* x, int t, const float* cond, int Ltot, int Ftot, int Lw, int overlap,
                                        float* eps_out, void* stream) {
  return unet_forward_windows(c, x, t, cond, 1, &Ltot, &Ftot, Lw, overlap, eps_out, stream, true);
}

extern "C" int ldc_unet_forward_windows_group(ldc_ctx* c, const float* x, int t, const float* cond, int R, const int* Ltot, const int* Ftot, int Lw,
                                              int overlap, float* eps_out, void* stream) {
  return unet_forward_windows(c, x, t, cond, R, Ltot, Ftot, Lw, overlap, eps_out, stream, false);
}

// the coupled loop on the plan's packed state; the update kernels draw under the recording table's keys, which go in on the stream in
// front of the loop.  A single-recording call (`single`) draws as ldc_denoise at B = 1 does: under the key of the context's Philox epoch,
// which a drawing call without a tape advances (`draws`).  A group call neither reads nor advances the epoch (as decode pools, section
// 5e): recording r draws under seeds[r] at epoch 0, and a call with a tape leaves the keys zero.
static int windows_loop(ldc_ctx* c, const Halves& h, const StepSampler& sm, const float* noise, const uint64_t* seeds, bool single, bool draws,
                        int n_steps, hipStream_t s) {
  Plan* pl = h.p[0];
  if (single) next_noise_key(c, noise == nullptr && draws);
  HIPCHK(launch_windows_group_keys(pl->wg_rec, single ? &c->cur_key : (noise ? nullptr : seeds), pl->wg.R, s));
  return denoise_loop(c, h, pl->B, pl->win_x, noise, n_steps, s, nullptr, sm);
}

// img (packed [C][Ltot_r] blocks) in, the coupled loop on the plan's own state, img out
static int windows_sample(ldc_ctx* c, float* img, const float* cond, const float* noise, const uint64_t* seeds, int n_steps, int sampler, bool draws,
                          int R, const int* Ltot, const int* Ftot, int Lw, int overlap, void* stream, bool single) {
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(windows_prepare(c, R, Ltot, Ftot, Lw, overlap, s, &h, single));   // (every refusal, before any GPU work)
  Plan* pl = h.p[0];
  StepSampler sm;
  LDCCHK(windows_sampler(c, pl, sampler, s, &sm));   // c->ddim_host / c->dpm_host, filled by the caller
  LDCCHK(windows_load_cond(c, pl, cond, s));
  const size_t nbytes = (size_t)c->unet.channels * pl->win_Ltot * 4;
  HIPCHK(hipMemcpyAsync(pl->win_x, img, nbytes, hipMemcpyDeviceToDevice, s));
  LDCCHK(windows_load_x(c, pl, pl->win_x, s));
  LDCCHK(windows_loop(c, h, sm, noise, seeds, single, draws, n_steps, s));
  HIPCHK(hipMemcpyAsync(img, pl->win_x, nbytes, hipMemcpyDeviceToDevice, s));
  return finish_stream(c, stream);
}

extern "C" int ldc_denoise_windows(ldc_ctx* c, float* img, const float* cond, const float* noise, int n_steps, int Ltot, int Ftot, int Lw,
                                   int overlap, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  if (n_steps < 1 || n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps %d: must be in [1,%d]", n_steps, c->unet.timesteps);
  return windows_sample(c, img, cond, noise, nullptr, n_steps, SAMPLER_DDPM, true, 1, &Ltot, &Ftot, Lw, overlap, stream, true);
}

extern "C" int ldc_ddim_sample_windows(ldc_ctx* c, float* img, const float* cond, const float* noise, int t_start, int n_steps, float eta,
                                       int Ltot, int Ftot, int Lw, int overlap, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  bool draws = false;
  LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  return windows_sample(c, img, cond, noise, nullptr, n_steps, SAMPLER_DDIM, draws, 1, &Ltot, &Ftot, Lw, overlap, stream, true);
}

// DPM-Solver++(2M) on coupled windows, as ldc_dpm_sample at B = 1: deterministic, nothing is drawn, the Philox epoch stays where it is
extern "C" int ldc_dpm_sample_windows(ldc_ctx* c, float* img, const float* cond, int t_start, int n_steps, int Ltot, int Ftot, int Lw, int overlap,
                                      void* stream) {
  LDCCHK(dpm_front_args(t_start, n_steps));
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  LDCCHK(dpm_schedule(c, t_start, n_steps));
  return windows_sample(c, img, cond, nullptr, nullptr, n_steps, SAMPLER_DPM, false, 1, &Ltot, &Ftot, Lw, overlap, stream, true);
}

// ldc_decode / ldc_decode_ddim / ldc_decode_dpm (src.wav) or ldc_decode_codes / _ddim / _dpm (src.codes | src.packed; R = 1 only) with the
// denoise loop replaced by ONE coupled loop over the windows of R recordings.  The codec ends run per recording: the condition rows
// (get_cond_rows at B = 1, or the dequantised codes) and the start image normalised over that recording, the SEANet decoder over that
// recording's latent, output_normalise for that recording.  src.wav and wav_out are packed (recording r's T[r] samples behind those in
// front), latents_out [D][Ltot_r] blocks, cond_out [D][Ftot_r] blocks, codes_out [n_q][Ftot_r] blocks.
static int decode_windows_body(ldc_ctx* c, const FrontSrc& src, int R, const int* T, int n_steps, int sampler, bool draws, const float* noise,
                               const uint64_t* seeds, int Lw, int overlap, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out,
                               void* stream, bool single) {
  const Codec& cc = c->codec[LDC_MODEL_COND];
  const Codec& mc = c->codec[LDC_MODEL_MAIN];
  const int D = c->cfg.rep_dims;
  if (!src.wav && R != 1) return fail(LDC_E_STATE, "internal: the receiver's windows decode one recording");
  std::vector<int> Lr((size_t)R), Fr((size_t)R);
  std::vector<size_t> toff((size_t)R + 1, 0);
  for (int r = 0; r < R; ++r) {
    if (T[r] <= 0 || T[r] % cc.hop || T[r] % mc.hop) {
      if (single) return fail(LDC_E_INVALID, "T %d: must be a multiple of %d and %d (sample.py:87 trims to 640)", T[r], cc.hop, mc.hop);
      return fail(LDC_E_INVALID, "recording %d: T %d: must be a positive multiple of %d and %d (sample.py:87 trims to 640)", r, T[r], cc.hop, mc.hop);
    }
    Fr[r] = T[r] / cc.hop; Lr[r] = T[r] / mc.hop;
    LDCCHK(check_unet_args(c, 1, Lr[r], Fr[r]));
    toff[r + 1] = toff[r] + (size_t)T[r];
  }
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(windows_prepare(c, R, Lr.data(), Fr.data(), Lw, overlap, s, &h, single));   // (every refusal, before any GPU work)
  LDCCHK(ensure_outnorm(c, 1));
  Plan* pl = h.p[0];
  StepSampler sm;
  LDCCHK(windows_sampler(c, pl, sampler, s, &sm));
  const WinGroup& g = pl->win_group;
  const int n_q = n_q_for_bandwidth(c, 0.f);
  LDCCHK(with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    float* mx = (float*)ar.alloc((size_t)R * 4);
    const int Fw = pl->F, upf = upsample_factor(c);
    for (int r = 0; r < R; ++r) {
      const int F = Fr[r], L = Lr[r];
      const size_t foff = (size_t)g.off[r] / upf;
      float* qr = nullptr;
      int Fq = 0;
      if (src.wav) {
        LDCCHK(get_cond_rows(c, src.wav + toff[r], 1, T[r], 0.f, ar, dry, s, &qr, &Fq, codes_out ? codes_out + (size_t)n_q * foff : nullptr, 1));
      } else {   // the receiver: quantizer.decode(codes) over the whole recording, as decode_body at B = 1 (bad code values raise the device flag)
        qr = (float*)ar.alloc((size_t)F * D * 4);
        Fq = F;
        if (!dry)
          HIPCHK(launch_rvq_dequant(src.codes, src.packed, src.packed_stride, src.bits, src.n_q, 1, 0, 1, F, cc.codebooks, cc.bins, D, qr,
                                    c->dev_flag_dev, s, nullptr));
      }
      if (!dry && Fq != F) return fail(LDC_E_INVALID, "internal: encoder produced %d frames, expected %d", Fq, F);
      void* up = nullptr;
      int Lu = 0;
      LDCCHK(upsample_rows(c, qr, 1, F, ar, dry, s, &up, &Lu));
      if (!dry) {
        if (cond_out) HIPCHK(launch_from_cl(DT_F32, qr, cond_out + (size_t)D * foff, 1, D, F, nullptr, 0, 0.f, s));
        // start image: upsample, /= max|.|+1e-8 over the whole recording (sample.py:125-129), straight into the plan's state
        HIPCHK(hipMemsetAsync(mx + r, 0, 4, s));
        HIPCHK(launch_maxabs(DT_F32, up, 1, (int64_t)L * D, 0, mx + r, s));
        HIPCHK(launch_from_cl(DT_F32, up, pl->win_x + (size_t)D * g.off[r], 1, D, L, mx + r, 0, 1e-8f, s));
        // process_cond per window: the rows are channels-last fp32 already, a window's slice is one contiguous run of its recording's rows
        for (int k = g.w0[r]; k < g.w0[r + 1]; ++k)
          HIPCHK(hipMemcpyAsync((float*)pl->cond_in_cl + (size_t)k * Fw * D, qr + (size_t)(g.start[k] / upf) * D, (size_t)Fw * D * 4,
                                hipMemcpyDeviceToDevice, s));
      }
    }
    if (!dry) {
      LDCCHK(run_ops(c, pl, false, s));
      LDCCHK(windows_load_x(c, pl, pl->win_x, s));
      LDCCHK(windows_loop(c, h, sm, noise, seeds, single, draws, n_steps, s));
      if (latents_out) HIPCHK(hipMemcpyAsync(latents_out, pl->win_x, (size_t)D * g.Lsum * 4, hipMemcpyDeviceToDevice, s));
    }
    for (int r = 0; r < R; ++r) {   // decoder over each recording's latent (quirk Q3: no x18 un-scaling on this path, sample.py:131)
      const int L = Lr[r];
      SeaRun Rn{c, &ar, s, dry, 1};
      void* zc = ar.alloc((size_t)L * D * 4);
      if (!dry) HIPCHK(launch_to_cl(DT_F32, pl->win_x + (size_t)D * g.off[r], zc, 1, D, L, nullptr, 0, 0.f, s));
      void* y = nullptr;
      int Lo = 0, Cd = 0;
      LDCCHK(run_seanet(Rn, mc.dec, zc, L, &y, &Lo, &Cd));
      if (!dry) {
        if (Lo != T[r]) return fail(LDC_E_STATE, "internal: the decoder gave %d samples for recording %d of %d", Lo, r, T[r]);
        HIPCHK(hipMemcpyAsync(wav_out + toff[r], y, (size_t)Lo * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(launch_output_normalise(wav_out + toff[r], 1, Lo, 0, c->outnorm_ws, s, nullptr, mc.hop));
      }
    }
    return LDC_OK;
  }));
  return finish_stream(c, stream);
}

extern "C" int ldc_decode_windows(ldc_ctx* c, const float* wav, int T, int n_steps, const float* noise, int Lw, int overlap, float* wav_out,
                                  float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (!wav || !wav_out || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  if (n_steps < 1 || n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps %d: must be in [1,%d]", n_steps, c->unet.timesteps);
  FrontSrc src;
  src.wav = wav;
  return decode_windows_body(c, src, 1, &T, n_steps, SAMPLER_DDPM, true, noise, nullptr, Lw, overlap, wav_out, latents_out, cond_out, codes_out, stream,
                             true);
}

extern "C" int ldc_decode_ddim_windows(ldc_ctx* c, const float* wav, int T, int t_start, int n_steps, float eta, const float* noise, int Lw,
                                       int overlap, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  if (!wav || !wav_out || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  bool draws = false;
  LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  FrontSrc src;
  src.wav = wav;
  return decode_windows_body(c, src, 1, &T, n_steps, SAMPLER_DDIM, draws, noise, nullptr, Lw, overlap, wav_out, latents_out, cond_out, codes_out, stream,
                             true);
}

// ldc_decode_dpm of one recording with the loop on coupled windows: no eta, no noise, the Philox epoch stays where it is
extern "C" int ldc_decode_dpm_windows(ldc_ctx* c, const float* wav, int T, int t_start, int n_steps, int Lw, int overlap, float* wav_out,
                                      float* latents_out, float* cond_out, int64_t* codes_out, void* stream) {
  LDCCHK(dpm_front_args(t_start, n_steps));
  if (!wav || !wav_out || T <= 0) return fail(LDC_E_INVALID, "bad arguments");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  LDCCHK(dpm_schedule(c, t_start, n_steps));
  FrontSrc src;
  src.wav = wav;
  return decode_windows_body(c, src, 1, &T, n_steps, SAMPLER_DPM, false, nullptr, nullptr, Lw, overlap, wav_out, latents_out, cond_out, codes_out, stream,
                             true);
}

// The receiver on coupled windows: ldc_decode_windows / ldc_decode_ddim_windows from the RVQ codes of ONE recording of Ftot condition
// frames (int64 codes [n_q][1][Ftot] or the packed payload, as ldc_decode_codes).  t_start 0: DDPM halfway sampling of n_steps (eta is not
// used); > 0: DDIM -- the convention of ldc_decode_codes_ragged.  The context-free refusals come first (a NULL context sees them too).
extern "C" int ldc_decode_codes_windows(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int Ftot,
                                        int t_start, int n_steps, float eta, const float* noise, int Lw, int overlap, float* wav_out,
                                        float* latents_out, float* cond_out, void* stream) {
  LDCCHK(codes_args(codes, packed, packed_stride, bits, n_q, 1, Ftot, wav_out));
  if (!(eta >= 0.0f && eta <= 1.0f)) return fail(LDC_E_INVALID, "eta %g: must be a finite value in [0, 1]", (double)eta);
  if (t_start < 0) return fail(LDC_E_INVALID, "t_start %d: must be >= 0 (0: DDPM halfway sampling)", t_start);
  if (n_steps < 1) return fail(LDC_E_INVALID, "n_steps %d: must be >= 1", n_steps);
  if (t_start > 0 && n_steps > t_start)
    return fail(LDC_E_INVALID, "n_steps %d: must be in [1, t_start = %d] (more would repeat timesteps)", n_steps, t_start);
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  FrontSrc src;
  int T = 0;
  LDCCHK(codes_src(c, codes, packed, packed_stride, bits, n_q, Ftot, &src, &T));
  bool draws = true;
  if (t_start > 0) LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  else if (n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps %d: must be in [1,%d]", n_steps, c->unet.timesteps);
  return decode_windows_body(c, src, 1, &T, n_steps, t_start > 0 ? SAMPLER_DDIM : SAMPLER_DDPM, draws, noise, nullptr, Lw, overlap, wav_out, latents_out,
                             cond_out, nullptr, stream, true);
}

extern "C" int ldc_decode_codes_dpm_windows(ldc_ctx* c, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q,
                                            int Ftot, int t_start, int n_steps, int Lw, int overlap, float* wav_out, float* latents_out,
                                            float* cond_out, void* stream) {
  LDCCHK(codes_args(codes, packed, packed_stride, bits, n_q, 1, Ftot, wav_out));
  LDCCHK(dpm_front_args(t_start, n_steps));
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, true));
  FrontSrc src;
  int T = 0;
  LDCCHK(codes_src(c, codes, packed, packed_stride, bits, n_q, Ftot, &src, &T));
  LDCCHK(dpm_schedule(c, t_start, n_steps));
  return decode_windows_body(c, src, 1, &T, n_steps, SAMPLER_DPM, false, nullptr, nullptr, Lw, overlap, wav_out, latents_out, cond_out, nullptr, stream,
                             true);
}

// The front of a group sampler call, the refusals of ldc_denoise_windows / ldc_ddim_sample_windows / ldc_dpm_sample_windows in their order
// (sampler 0 DDPM: t_start and eta are not used; 1 DDIM; 2 DPM: eta, noise and seeds are not used).  Leaves the schedule in c->ddim_host /
// c->dpm_host.  A sampler that draws needs a tape or the recordings' seeds.
static int windows_group_front(ldc_ctx* c, int sampler, int t_start, int n_steps, float eta, const float* noise, const uint64_t* seeds, bool tensors,
                               bool codec, bool* draws) {
  if (sampler != SAMPLER_DDPM && sampler != SAMPLER_DDIM && sampler != SAMPLER_DPM)
    return fail(LDC_E_INVALID, "sampler %d: must be 0 (DDPM), 1 (DDIM) or 2 (DPM-Solver++)", sampler);
  *draws = false;
  if (sampler == SAMPLER_DPM) {
    LDCCHK(dpm_front_args(t_start, n_steps));
    if (!tensors) return fail(LDC_E_INVALID, codec ? "bad arguments" : "null tensor");
    LDCCHK(check_ready(c, LDC_MODEL_MAIN, codec));
    LDCCHK(dpm_schedule(c, t_start, n_steps));
    return LDC_OK;
  }
  LDCCHK(check_ready(c, LDC_MODEL_MAIN, codec));
  if (!tensors) return fail(LDC_E_INVALID, codec ? "bad arguments" : "null tensor");
  if (sampler == SAMPLER_DDPM) {
    if (n_steps < 1 || n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps %d: must be in [1,%d]", n_steps, c->unet.timesteps);
    *draws = true;
  } else {
    LDCCHK(ddim_schedule(c, t_start, n_steps, eta, draws));
  }
  if (*draws && !noise && !seeds)
    return fail(LDC_E_INVALID, "seeds NULL: a group call that draws takes a noise tape or one seed per recording (it never reads the context's epoch)");
  return LDC_OK;
}

extern "C" int ldc_sample_windows_group(ldc_ctx* c, float* img, const float* cond, int sampler, int t_start, int n_steps, float eta, const float* noise,
                                        const uint64_t* seeds, int R, const int* Ltot, const int* Ftot, int Lw, int overlap, void* stream) {
  bool draws = false;
  LDCCHK(windows_group_front(c, sampler, t_start, n_steps, eta, noise, seeds, img && cond, false, &draws));
  return windows_sample(c, img, cond, sampler == SAMPLER_DPM ? nullptr : noise, seeds, n_steps, sampler, draws, R, Ltot, Ftot, Lw, overlap, stream, false);
}

// ldc_decode_windows / _ddim_windows / _dpm_windows of R recordings with ONE loop (decode_windows_body's packed layouts)
extern "C" int ldc_decode_windows_group(ldc_ctx* c, const float* wav, int R, const int* T, int sampler, int t_start, int n_steps, float eta,
                                        const float* noise, const uint64_t* seeds, int Lw, int overlap, float* wav_out, float* latents_out,
                                        float* cond_out, int64_t* codes_out, void* stream) {
  bool draws = false;
  LDCCHK(windows_group_front(c, sampler, t_start, n_steps, eta, noise, seeds, wav && wav_out && T && R >= 1, true, &draws));
  if (R > kWinPerPart) return fail(LDC_E_INVALID, "R %d: a window group holds 1 to %d recordings", R, kWinPerPart);
  FrontSrc src;
  src.wav = wav;
  return decode_windows_body(c, src, R, T, n_steps, sampler, draws, sampler == SAMPLER_DPM ? nullptr : noise, seeds, Lw, overlap, wav_out, latents_out,
                             cond_out, codes_out, stream, false);
}

int check_dev(ldc_ctx* c) {
  if (!c) return fail(LDC_E_INVALID, "null ctx");
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(LDC_E_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
  return LDC_OK;
}
