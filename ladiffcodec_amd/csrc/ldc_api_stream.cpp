// ldc_api_stream.cpp -- stream sessions over the SEANet codec ends: chunked encode / decode / get_cond whose joined outputs are the
// whole-sequence call's (include/ladiffcodec.h, "stream sessions").  Host-side C++ only: the state lives in
// ldc_stream (ldc_internal.h), the kernels read it through ConvCall::ctx, launch_conv_cin1's ctx and LstmCarry.
#include "ldc_internal.h"

namespace {

// One entry per conv of a SEANet stack that pads on the left (reference srcs/modules/seanet.py:108-151, 200-244; conv.py:217-232):
// `pad` = (k - 1) dil - (stride - 1) rows, read from an input that is n * num / den rows long when the stack's input is n units long.
// A host-only entry point has no built layers to read, so the table is generated from the configuration with the SEANet constants this
// library builds every codec with (build_codec): kernel_size = last_kernel_size = 7, residual_kernel_size = 3, dilation_base = 2,
// strided / transposed kernels of 2 * ratio, and the cond codec's ratios 8 5 4 2.  ldc_stream_create holds it to the built layers.
struct PadEntry { int pad, num, den; };

std::vector<PadEntry> pad_table(const std::vector<int>& ratios, int n_residual, int side) {
  std::vector<PadEntry> t;
  if (side == LDC_STREAM_ENCODER) {
    int den = 1;
    t.push_back({7 - 1, 1, den});
    for (auto it = ratios.rbegin(); it != ratios.rend(); ++it) {
      for (int j = 0; j < n_residual; ++j) t.push_back({(3 - 1) << j, 1, den});
      t.push_back({(2 * *it - 1) - (*it - 1), 1, den});
      den *= *it;
    }
    t.push_back({7 - 1, 1, den});
  } else {
    int num = 1;
    t.push_back({7 - 1, num, 1});
    for (int r : ratios) {
      num *= r;   // (the transposed conv pads nothing: it sees no previous row at the start of a sequence)
      for (int j = 0; j < n_residual; ++j) t.push_back({(3 - 1) << j, num, 1});
    }
    t.push_back({7 - 1, num, 1});
  }
  return t;
}

int min_first_of(const std::vector<PadEntry>& t, int unit) {
  for (int n = unit;; n += unit) {
    bool ok = true;
    for (const PadEntry& e : t) ok = ok && (long long)n * e.num / e.den > e.pad;
    if (ok) return n;
  }
}

// the same table read off the built layers: what ldc_stream_create allocates, and a check of pad_table against the real stack
std::vector<StreamConvState> state_table(const std::vector<SeaOp>& ops, std::vector<int>* pads, std::vector<int>* lstm_h) {
  std::vector<StreamConvState> v;
  auto conv = [&](const ConvLayer& ly) {
    const int rows = ly.tr_stride ? 1 : ly.pad_left;
    if (rows <= 0) return;
    StreamConvState cs;
    cs.rows = rows; cs.ch = ly.cin1;
    v.push_back(cs);
    if (!ly.tr_stride) pads->push_back(rows);
  };
  for (const SeaOp& op : ops) switch (op.kind) {
      case SeaOp::CONV_CIN1: {
        StreamConvState cs;
        cs.rows = op.k - 1; cs.ch = 1;
        v.push_back(cs);
        pads->push_back(cs.rows);
        break;
      }
      case SeaOp::CONV:
      case SeaOp::CONVTR: conv(op.conv); break;
      case SeaOp::RES: conv(op.shortcut); conv(op.conv); conv(op.conv2); break;   // (run_seanet's order)
      case SeaOp::LSTM:
        for (size_t n = 0; n < op.lstm.size(); ++n) lstm_h->push_back(op.cout);
        break;
    }
  return v;
}

int check_stream(ldc_ctx* c, ldc_stream* st, int which_side, const char* entry) {
  if (!c) return fail(LDC_E_INVALID, "%s: null pointer: ctx", entry);
  if (!st) return fail(LDC_E_INVALID, "%s: null pointer: stream object", entry);
  if (st->ctx != c) return fail(LDC_E_INVALID, "%s: the stream object belongs to another context (%p, not %p)", entry, (void*)st->ctx, (void*)c);
  if (st->poisoned)
    return fail(LDC_E_STATE, "%s: an earlier call on this stream object failed after its GPU work had started, its state is inconsistent: "
                             "ldc_stream_reset with a NULL mask (every item) makes it usable again", entry);
  if (st->side != which_side)
    return fail(LDC_E_INVALID, "%s: the stream object is of side %d (%s), this call needs side %d", entry, st->side,
                st->side == LDC_STREAM_ENCODER ? "LDC_STREAM_ENCODER" : "LDC_STREAM_DECODER", which_side);
  return LDC_OK;
}

// n: the chunk length in input units; unit: hop (encoder) or 1 (decoder)
int check_chunk(ldc_stream* st, int n, int unit, const char* what, const char* entry) {
  if (n <= 0 || n % unit) return fail(LDC_E_INVALID, "%s: %s = %d is not a positive multiple of %d", entry, what, n, unit);
  if (n < st->min_first)
    for (int b = 0; b < st->B; ++b)
      if (st->fresh_host[b])
        return fail(LDC_E_INVALID, "%s: item %d is fresh and %s = %d is below the first-chunk minimum %d (ldc_stream_min_first)", entry, b, what, n,
                    st->min_first);
  return LDC_OK;
}

void begin_pass(ldc_stream* st, bool dry) {
  st->conv_at = st->lstm_at = 0;
  st->touched = !dry;
}

// a call that failed before its GPU work (refusals, the measuring pass) leaves the session as it was; one that failed later poisons it
int finish_call(ldc_stream* st, int rc) {
  if (rc != LDC_OK && st->touched) st->poisoned = true;
  st->touched = false;
  return rc;
}

// after the launches of a call: every item now has history; the next call reads what this one wrote
int end_call(ldc_stream* st, hipStream_t s) {
  st->last_stream = s;
  HIPCHK(hipMemsetAsync(st->fresh_dev, 0, (size_t)st->B * sizeof(int), s));
  std::fill(st->fresh_host.begin(), st->fresh_host.end(), 0);
  st->parity ^= 1;
  return LDC_OK;
}

}  // namespace

extern "C" int ldc_stream_min_first(const ldc_config* cfg, int which, int side) {
  if (!cfg) return fail(LDC_E_INVALID, "ldc_stream_min_first: null pointer: cfg");
  if (which != LDC_MODEL_MAIN && which != LDC_MODEL_COND) return fail(LDC_E_INVALID, "ldc_stream_min_first: which = %d is neither LDC_MODEL_MAIN nor LDC_MODEL_COND", which);
  if (side != LDC_STREAM_ENCODER && side != LDC_STREAM_DECODER) return fail(LDC_E_INVALID, "ldc_stream_min_first: side = %d is neither LDC_STREAM_ENCODER nor LDC_STREAM_DECODER", side);
  std::vector<int> ratios = {8, 5, 4, 2};   // the cond codec (quirk Q1)
  if (which == LDC_MODEL_MAIN) {
    if (cfg->n_enc_ratios < 1 || cfg->n_enc_ratios > LDC_MAX_RATIOS) return fail(LDC_E_INVALID, "ldc_stream_min_first: n_enc_ratios = %d", cfg->n_enc_ratios);
    ratios.assign(cfg->enc_ratios, cfg->enc_ratios + cfg->n_enc_ratios);
  }
  int hop = 1;
  for (int r : ratios) {
    if (r < 1) return fail(LDC_E_INVALID, "ldc_stream_min_first: ratio %d", r);
    hop *= r;
  }
  if (cfg->n_residual_layers < 0 || cfg->n_residual_layers > 16) return fail(LDC_E_INVALID, "ldc_stream_min_first: n_residual_layers = %d", cfg->n_residual_layers);
  return min_first_of(pad_table(ratios, cfg->n_residual_layers, side), side == LDC_STREAM_ENCODER ? hop : 1);
}

extern "C" int ldc_stream_create(ldc_ctx* c, int which, int side, int B, ldc_stream** out) {
  if (!c) return fail(LDC_E_INVALID, "ldc_stream_create: null pointer: ctx");
  if (!out) return fail(LDC_E_INVALID, "ldc_stream_create: null pointer: out");
  *out = nullptr;
  if (side != LDC_STREAM_ENCODER && side != LDC_STREAM_DECODER) return fail(LDC_E_INVALID, "ldc_stream_create: side = %d is neither LDC_STREAM_ENCODER nor LDC_STREAM_DECODER", side);
  if (B <= 0) return fail(LDC_E_INVALID, "ldc_stream_create: B = %d must be positive", B);
  LDCCHK(check_ready(c, which));
  const Codec& cd = c->codec[which];
  std::unique_ptr<ldc_stream> st(new ldc_stream());
  st->ctx = c; st->which = which; st->side = side; st->B = B; st->hop = cd.hop;
  std::vector<int> pads, lstm_h;
  st->convs = state_table(side == LDC_STREAM_ENCODER ? cd.enc : cd.dec, &pads, &lstm_h);
  {   // the host-only table must describe the stack that was built
    const std::vector<PadEntry> t = pad_table(cd.ratios, c->cfg.n_residual_layers, side);
    bool same = t.size() == pads.size();
    for (size_t i = 0; same && i < t.size(); ++i) same = t[i].pad == pads[i];
    if (!same) return fail(LDC_E_STATE, "ldc_stream_create: the layer table of ldc_stream_min_first does not describe this codec");
    st->min_first = min_first_of(t, side == LDC_STREAM_ENCODER ? cd.hop : 1);
  }
  for (StreamConvState& cs : st->convs)
    for (int k = 0; k < 2; ++k) {
      void* p = nullptr;
      LDCCHK(st->mem.alloc(&p, (size_t)B * cs.rows * cs.ch * sizeof(float)));
      cs.buf[k] = reinterpret_cast<float*>(p);
    }
  for (int H : lstm_h) {
    void* p = nullptr;
    LDCCHK(st->mem.alloc(&p, (size_t)B * 2 * H * sizeof(float)));
    st->lstm.push_back(reinterpret_cast<float*>(p));
  }
  void* p = nullptr;
  LDCCHK(st->mem.alloc(&p, (size_t)B * sizeof(int)));
  st->fresh_dev = reinterpret_cast<int*>(p);
  st->fresh_host.assign((size_t)B, 1);
  HIPCHK(launch_lens_write(st->fresh_dev, st->fresh_host.data(), B, c->own_stream));
  HIPCHK(hipStreamSynchronize(c->own_stream));
  *out = st.release();
  return LDC_OK;
}

extern "C" int ldc_stream_reset(ldc_stream* st, const uint8_t* item_mask_host, void* stream) {
  if (!st) return fail(LDC_E_INVALID, "ldc_stream_reset: null pointer: stream object");
  ldc_ctx* c = st->ctx;
  LDCCHK(check_dev(c));
  bool all = true;
  for (int b = 0; b < st->B; ++b) all = all && (!item_mask_host || item_mask_host[b]);
  if (st->poisoned && !all)
    return fail(LDC_E_STATE, "ldc_stream_reset: a call on this stream object failed midway; only a reset of every item (NULL mask) makes it usable again");
  for (int b = 0; b < st->B; ++b)
    if (!item_mask_host || item_mask_host[b]) st->fresh_host[b] = 1;
  st->poisoned = false;   // (every item fresh: nothing of the old state is read again)
  hipStream_t s = pick_stream(c, stream);
  st->last_stream = s;
  HIPCHK(launch_lens_write(st->fresh_dev, st->fresh_host.data(), st->B, s));   // (nothing else to clear: a fresh item reads no state)
  return finish_stream(c, stream);
}

extern "C" int ldc_stream_destroy(ldc_stream* st) {
  if (!st) return LDC_OK;
  if (st->ctx) {
    (void)hipSetDevice(st->ctx->device);
    // the state may still be in use by asynchronous calls: calls on one session go in order on one stream, so its last stream is enough
    // (a session whose last call failed midway waits for the whole device)
    if (st->poisoned) (void)hipDeviceSynchronize();
    else (void)hipStreamSynchronize(st->last_stream ? st->last_stream : st->ctx->own_stream);
  }
  delete st;
  return LDC_OK;
}

extern "C" int ldc_seanet_encode_stream(ldc_ctx* c, ldc_stream* st, const float* wav, int T, float* z_out, void* stream) {
  const char* me = "ldc_seanet_encode_stream";
  LDCCHK(check_stream(c, st, LDC_STREAM_ENCODER, me));
  if (!wav) return fail(LDC_E_INVALID, "%s: null pointer: wav", me);
  if (!z_out) return fail(LDC_E_INVALID, "%s: null pointer: z_out", me);
  LDCCHK(check_chunk(st, T, st->hop, "T", me));
  LDCCHK(check_ready(c, st->which));
  hipStream_t s = pick_stream(c, stream);
  const Codec& cd = c->codec[st->which];
  const int B = st->B;
  int rc = with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    SeaRun R{c, &ar, s, dry, B};
    R.st = st;
    begin_pass(st, dry);
    void* z = nullptr;
    int L = 0, C = 0;
    LDCCHK(run_seanet(R, cd.enc, wav, T, &z, &L, &C));
    if (!dry) HIPCHK(launch_from_cl(DT_F32, z, z_out, B, C, L, nullptr, 0, 0.f, s));
    return LDC_OK;
  });
  if (rc == LDC_OK) rc = end_call(st, s);
  if (rc == LDC_OK) rc = finish_stream(c, stream);
  return finish_call(st, rc);
}

extern "C" int ldc_seanet_decode_stream(ldc_ctx* c, ldc_stream* st, const float* z, int L, float* wav_out, void* stream) {
  const char* me = "ldc_seanet_decode_stream";
  LDCCHK(check_stream(c, st, LDC_STREAM_DECODER, me));
  if (!z) return fail(LDC_E_INVALID, "%s: null pointer: z", me);
  if (!wav_out) return fail(LDC_E_INVALID, "%s: null pointer: wav_out", me);
  LDCCHK(check_chunk(st, L, 1, "L", me));
  LDCCHK(check_ready(c, st->which));
  hipStream_t s = pick_stream(c, stream);
  const Codec& cd = c->codec[st->which];
  const int B = st->B, D = c->cfg.rep_dims;
  int rc = with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    SeaRun R{c, &ar, s, dry, B};
    R.st = st;
    begin_pass(st, dry);
    void* zc = ar.alloc((size_t)B * L * D * 4);
    if (!dry) HIPCHK(launch_to_cl(DT_F32, z, zc, B, D, L, nullptr, 0, 0.f, s));
    void* y = nullptr;
    int Lo = 0, C = 0;
    LDCCHK(run_seanet(R, cd.dec, zc, L, &y, &Lo, &C));
    if (!dry) HIPCHK(hipMemcpyAsync(wav_out, y, (size_t)B * Lo * 4, hipMemcpyDeviceToDevice, s));   // Cout = 1: [B*T][1] is [B,1,T]
    return LDC_OK;
  });
  if (rc == LDC_OK) rc = end_call(st, s);
  if (rc == LDC_OK) rc = finish_stream(c, stream);
  return finish_call(st, rc);
}

extern "C" int ldc_get_cond_stream(ldc_ctx* c, ldc_stream* st, const float* wav, int T, float bandwidth, float* cond_out, int64_t* codes_out,
                                   void* stream) {
  const char* me = "ldc_get_cond_stream";
  LDCCHK(check_stream(c, st, LDC_STREAM_ENCODER, me));
  if (st->which != LDC_MODEL_COND) return fail(LDC_E_INVALID, "%s: the stream object is of codec %d, not the cond codec (LDC_MODEL_COND)", me, st->which);
  if (!wav) return fail(LDC_E_INVALID, "%s: null pointer: wav", me);
  if (!cond_out) return fail(LDC_E_INVALID, "%s: null pointer: cond_out", me);
  LDCCHK(check_chunk(st, T, st->hop, "T", me));
  LDCCHK(check_ready(c, LDC_MODEL_COND));
  hipStream_t s = pick_stream(c, stream);
  const Codec& cd = c->codec[LDC_MODEL_COND];
  const int B = st->B;
  int rc = with_scratch(c, s, [&](Arena& ar, bool dry) -> int {
    SeaRun R{c, &ar, s, dry, B};
    R.st = st;
    begin_pass(st, dry);
    void* z = nullptr;
    int F = 0, C = 0;
    LDCCHK(run_seanet(R, cd.enc, wav, T, &z, &F, &C));
    float* qr = (float*)ar.alloc((size_t)B * F * C * 4);
    LDCCHK(rvq_rows(c, (const float*)z, B * F, n_q_for_bandwidth(c, bandwidth), codes_out, qr, ar, dry, s));   // (frame by frame: no state)
    if (!dry) HIPCHK(launch_from_cl(DT_F32, qr, cond_out, B, c->cfg.rep_dims, F, nullptr, 0, 0.f, s));
    return LDC_OK;
  });
  if (rc == LDC_OK) rc = end_call(st, s);
  if (rc == LDC_OK) rc = finish_stream(c, stream);
  return finish_call(st, rc);
}
