/*
 * ladiffcodec.h  --  C ABI of the MI355X-native LaDiffCodec decode path (libladiffcodec.so).
 *
 * The reference (haiciyang/LaDiffCodec) is pure Python/PyTorch and exposes no plugin / FFI layer;
 * its hot path is `nn.Module` calls made by `synthesis()` (srcs/sample.py:50-136).  Each entry point
 * below replaces one of those calls; the reference call site it stands in for is cited next to it.
 * The Python host in `ladiffcodec_amd/` binds these with ctypes and mirrors the reference's module
 * attributes (`get_cond`, `diff_model.upsampling_layers`, `diffusion.halfway_sampling`, `decoder`).
 *
 * Conventions
 *   - Every function returns 0 on success or a negative LDC_E_* code; `ldc_last_error()` returns a
 *     thread-local human-readable message for the last failure.  No C++ exception crosses the ABI.
 *   - Tensor arguments are DEVICE pointers owned by the caller, contiguous, in the reference's own
 *     layouts: activations [B, C, L] float32, RVQ codes [n_q, B, F] int64.  The caller keeps them
 *     alive until `stream` has been synchronised.  `stream` is a hipStream_t passed as void*.
 *     stream != NULL: all work is queued asynchronously on that stream.  stream == NULL: the call runs
 *     on the context's own (non-blocking) stream and returns after synchronising it.
 *   - Device-wide synchronisation happens only in three documented places, never in the steady
 *     state: (1) when a context-owned workspace has to grow (first call at a larger shape),
 *     (2) when a captured step graph is replaced or evicted (a new (B, L, F), a new noise pointer,
 *     the LRU plan cache bound, see LDC_PLAN_CACHE_GB / LDC_PLAN_CACHE_N), (3) in ldc_destroy.
 *     Besides those, a sampler call may wait ON THE HOST for an earlier step-graph replay of the same
 *     context (bounded look-ahead, LDC_FLOW_DEPTH = 8 replays; an event wait, not a device sync).
 *   - Several contexts may be used side by side on one device (one per stream of work): two batches
 *     in flight, each decoded by its own context on its own stream, is how `python -m srcs.sample`
 *     and `bench.py --in-flight 2` raise throughput.
 *   - Reproducibility: GroupNorm statistics and the fused column maxima are accumulated with fp32
 *     atomics, so two identical UNet calls agree to rounding (~1e-6 relative), not bit for bit; the
 *     split-K reduction order is fixed.  The codec stages (SEANet, LSTM, RVQ) use no atomics: RVQ code
 *     indices are bit-reproducible.
 *   - An asynchronous device-side failure (the cooperative LSTM's bounded spin timing out) is
 *     reported as LDC_E_HIP by the synchronous call that hit it or by the next call on the context.
 *   - Weights are handed over on the HOST (float32, the `.amlt` state-dict tensors,
 *     srcs/utils.py:98-108), one call per state-dict key, then folded / packed / uploaded by
 *     `ldc_finalize_weights`.
 *   - A context is bound to one device and is not thread-safe (one context per rank / stream).
 *   - Internally activations are channels-last [B, L, C] in the context's compute dtype
 *     (LDC_F32: exact-fp32 MFMA path for parity; LDC_BF16: bf16 storage + bf16 MFMA, fp32
 *     accumulation, fp32 diffusion state).
 */
#ifndef LADIFFCODEC_H_
#define LADIFFCODEC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDC_OK 0
#define LDC_E_INVALID -1   /* bad argument / unsupported configuration          */
#define LDC_E_STATE -2     /* call out of order (e.g. stage before finalize)    */
#define LDC_E_MISSING -3   /* strict load: missing / unexpected / mis-shaped key */
#define LDC_E_HIP -4       /* a HIP runtime call failed                          */
#define LDC_E_NOMEM -5

#define LDC_F32 0
#define LDC_BF16 1
#define LDC_BF16_W8 2   /* bf16 activations, UNet conv weights stored as OCP fp8 e4m3 + one fp32 scale per output channel
                          (BASELINE config 5); codec stages stay fp32 */

/* which of the two DiffAudioRep instances a call addresses (srcs/sample.py:56 and :63) */
#define LDC_MODEL_MAIN 0   /* --model_path      : autoencoder [enc_ratios] + Unet1D + diffusion */
#define LDC_MODEL_COND 1   /* --model_for_cond  : EnCodec-style codec, always ratios [8,5,4,2] (quirk Q1) */

#define LDC_MAX_RATIOS 8

typedef struct ldc_ctx ldc_ctx;

/* Mirrors the argparse flags of srcs/sample.py:141-201 that shape the two models. */
typedef struct ldc_config {
  int32_t compute_dtype;                 /* LDC_F32 | LDC_BF16 | LDC_BF16_W8 */
  /* shared SEANet hyper-parameters (model.py:52-55) */
  int32_t rep_dims;                      /* --rep_dims            (128) */
  int32_t n_filters;                     /* --n_filters           (32)  */
  int32_t n_residual_layers;             /* --n_residual_layers   (1)   */
  int32_t lstm;                          /* --lstm                (2)   */
  /* main model */
  int32_t n_enc_ratios;                  /* --enc_ratios          ([8]) */
  int32_t enc_ratios[LDC_MAX_RATIOS];
  int32_t diff_dims;                     /* --diff_dims           (256) */
  int32_t n_upsampling_ratios;           /* --upsampling_ratios   ([5,4,2]); 0 = None */
  int32_t upsampling_ratios[LDC_MAX_RATIOS];
  int32_t unet_scale_cond;               /* --unet_scale_cond */
  int32_t unet_scale_x;                  /* --unet_scale_x    */
  /* cond model */
  int32_t has_cond_model;                /* --model_for_cond given */
  float cond_bandwidth;                  /* --cond_bandwidth      (3.0): builds floor(1000*bw / (50*10)) codebooks */
  /* capacity hints (workspaces are sized lazily; these only pre-size) */
  int32_t max_batch;
  int32_t max_latent_len;
  uint64_t noise_seed;                   /* device Philox stream used when noise == NULL */
  int32_t final_activation;              /* --final_activation: LDC_ACT_* applied after both encoders' last conv */
  int32_t reserved_;
} ldc_config;

/* --final_activation names (getattr(nn, name)() with default arguments, seanet.py:144-149) */
#define LDC_ACT_NONE 0
#define LDC_ACT_TANH 1
#define LDC_ACT_SIGMOID 2
#define LDC_ACT_ELU 3
#define LDC_ACT_SILU 4
#define LDC_ACT_GELU 5
#define LDC_ACT_RELU 6

const char* ldc_last_error(void);
const char* ldc_version(void);

/* lifecycle ---------------------------------------------------------------------------------- */
int ldc_create(const ldc_config* cfg, int device, ldc_ctx** out);
int ldc_destroy(ldc_ctx* ctx);

/* Per-context run-time options (instead of environment variables read at ldc_create): "split" = independent chains a batch is
 * decoded as (1..4, default 2; the reference has no counterpart: utterances never interact inside the UNet), "lstm_stream" =
 * 1: never use the cooperative (co-resident workgroups) LSTM kernel, "side_streams" = 1: res_conv on a side stream (split 1
 * only), "fp8_act" (fp8 contexts, before ldc_finalize_weights), "train_fp32_mfma" = 1: the training GEMMs on the exact-fp32
 * MFMA (round-2 kernels) instead of the split-bf16 ones (three bf16 MFMAs per product, 2^-16-class: csrc/train_mm3.hip) -- this
 * one is process-wide, like "train_bf16" = 1: one bf16 MFMA per product in the training GEMMs (autocast-class numerics, opt-in).
 * Launch structure of the UNet step (round 4; each keeps the reference's arithmetic, unet.py:137-246): "fuse_gn_epi" (default 1) = the
 * GroupNorm apply of a ResnetBlock's Block inside the producing conv, behind an in-launch exchange of per-wave statistics -- 0 restores
 * the conv + gn_apply launch pairs and is the fallback when a "[gn_wait]" device-side failure is reported; "fold_res" (1) = res_conv as a
 * fourth weight slab of block1's conv; "fold_ln" (1) = the attention blocks' PreNorm LayerNorm inside to_qkv.
 * Round 6: "conv_lean" (1) = the instruction-diet conv kernel (csrc/conv_lean.inc) where its shapes allow, 0 = conv_fast_kernel
 * everywhere (same tiles, same results: for A/B runs); "part_graphs" (1) = one single-stream step graph per batch part (two parts),
 * 0 = one fork / join graph, 2 = per-part graphs for three / four parts as well.  (Removed in round 6, measured slower in rounds 4-5:
 * "chain_convs" -- block1's and block2's convs as one launch -- and "xcd_teams" -- runs of convs as persistent XCD-team launches;
 * profiles/r04_fusion_experiments.md, profiles/r05_team_chain_experiments.md keep the numbers.)
 * "conv_xcd_order" (1) = the lean kernel's dispatch order as an xm x xn arrangement of the eight XCDs chosen per launch by operand
 * bytes (0 = conv_fast_kernel's order; 2 / 4 / 8 = xn forced); "fold_ctx" (1) = the LinearAttention context inside to_qkv's epilogue.
 * The whole table (name, default, effect) is in tools/README.md; LDC_OPTIONS="name=value,..." in the environment sets the same
 * names at ldc_create.  Cached plans and graphs are dropped when a value changes. */
int ldc_set_option(ldc_ctx* ctx, const char* name, int value);

/* Device-drawn noise (noise == NULL): Philox4x32-10 keyed by (noise_seed, call counter); every sampler call that
 * draws advances the counter, as every torch.randn_like of the reference (ddpm_loss.py:249) advances the global
 * generator.  ldc_reseed sets the seed and rewinds the counter (the counterpart of torch.manual_seed). */
int ldc_reseed(ldc_ctx* ctx, uint64_t seed);
/* The fp8 weight packer's rounding (OCP e4m3fn, nearest even, saturating at 448), host-side: codes and/or decoded values. */
void ldc_quantize_e4m3(const float* in, int64_t n, uint8_t* out_codes, float* out_values);

/* load_model(model, path, strict) -- srcs/utils.py:98-108.  One call per state-dict entry (after
 * the caller stripped any `module.` prefix).  `data` is a host float32 buffer of prod(shape)
 * elements.  Keys under `diffusion.model.*` alias `diff_model.*` and may be passed or skipped. */
int ldc_set_weight(ldc_ctx* ctx, int which, const char* key, const float* data, const int64_t* shape, int ndim);
/* strict != 0 reproduces load_state_dict(strict=True): every expected key present with the expected
 * shape, no unexpected key.  Folds weight-norm (conv.py:27-30) and weight-standardisation
 * (unet.py:73-78, eps 1e-5, fp32) once, packs for MFMA, builds the timestep scale/shift table. */
int ldc_finalize_weights(ldc_ctx* ctx, int strict);

/* stages ---------------------------------------------------------------------------------------- */
/* model.encoder(wav)  (seanet.py:153)            wav [B,1,T] -> z [B,rep_dims,T/hop]            */
int ldc_seanet_encode(ldc_ctx* ctx, int which, const float* wav, int B, int T, float* z_out, void* stream);
/* model.decoder(z)    (seanet.py:246; sample.py:131)   z [B,rep_dims,L] -> wav [B,1,L*hop]      */
int ldc_seanet_decode(ldc_ctx* ctx, int which, const float* z, int B, int L, float* wav_out, void* stream);
/* model.quantizer(z, frame_rate, bandwidth) in eval (vq.py:69-84, core_vq.py:324-342).
 * n_q = number of codebooks used.  codes_out [n_q,B,F] int64 (may be NULL), quantized_out [B,D,F]. */
int ldc_rvq_encode(ldc_ctx* ctx, const float* z, int B, int F, int n_q, int64_t* codes_out, float* quantized_out,
                   void* stream);
/* quantizer.decode(codes) (core_vq.py:356-362); a code outside [0, bins) is refused ("[bad_code]", see ldc_decode_codes) */
int ldc_rvq_decode(ldc_ctx* ctx, const int64_t* codes, int B, int F, int n_q, float* quantized_out, void* stream);
/* model_for_cond.get_cond(wav) (model.py:223-231) = encode + rvq, fused on one stream.
 * codes_out may be NULL.  bandwidth <= 0 means the configured cond_bandwidth. */
int ldc_get_cond(ldc_ctx* ctx, const float* wav, int B, int T, float bandwidth, float* cond_out, int64_t* codes_out,
                 void* stream);
/* ldc_get_cond on a right-padded batch (the sender side of a mixed-length batch): wav [B,1,Tmax], lengths_host[B] samples per item
 * (host memory), positive multiples of the cond hop (320), none above Tmax, Tmax itself such a multiple: LDC_E_INVALID otherwise,
 * before any GPU work.  Every item's codes and condition rows are those of ldc_get_cond on the item alone (items of at most
 * 6 frames, where the encoder's reflect padding changes form, are encoded on their own inside the call); codes_out [n_q,B,Fmax]
 * and cond_out [B,D,Fmax] are zero behind lengths_host[b] / 320 frames.  What the padding of wav holds is never read into a value. */
int ldc_get_cond_ragged(ldc_ctx* ctx, const float* wav, const int32_t* lengths_host, int B, int Tmax, float bandwidth,
                        float* cond_out, int64_t* codes_out, void* stream);
/* stream sessions ------------------------------------------------------------------------------
 * Both SEANet codecs are causal, so their ends can run chunk by chunk.  A stream object holds, for B independent streams of one
 * (codec, side), what a chunk needs from the past: every conv's most recent input rows, the transposed convs' previous input row
 * and the LSTM layers' (h, c).  Contract: split a sequence into chunks any way you like and push them through one item of a
 * stream -- the item's concatenated outputs are what ldc_seanet_encode / ldc_seanet_decode / ldc_get_cond return for the whole
 * sequence (same fp32 arithmetic; a chunk may take another split-K factor or LSTM kernel than the whole call, which moves
 * values in the last bits only).  An item is FRESH after create / reset: its next chunk starts a sequence (left reflect padding as
 * in the whole-sequence call, no previous transposed-conv row, h = c = 0).  Fresh items and items with history may share a call;
 * all items advance by the same T (or L).  Refused with LDC_E_INVALID before any GPU work, ldc_last_error() naming the value: a T
 * that is not a positive multiple of the codec's hop (an L <= 0), a call with a fresh item whose length is below
 * ldc_stream_min_first, a stream object of the other side / another context, ldc_get_cond_stream on anything but the cond encoder's
 * stream, a null pointer, B <= 0, and a (B, chunk) whose conv launches would not fit their LDS window (one-row chunks of thousands of
 * items).  Calls on one stream object must be issued in order on one HIP stream.  A call that fails AFTER its GPU work has started
 * (LDC_E_HIP, LDC_E_NOMEM) leaves part of the state advanced: the object then refuses every call with LDC_E_STATE until
 * ldc_stream_reset with a NULL mask. */
typedef struct ldc_stream ldc_stream;
#define LDC_STREAM_ENCODER 0
#define LDC_STREAM_DECODER 1
/* host-only, no context or GPU needed (like ldc_ddim_times): smallest length of the FIRST chunk of a stream, in input units
 * (samples for an encoder, latent frames for a decoder), for the codec described by cfg: the smallest multiple of the hop at which
 * no conv of that side reads an input no longer than its left padding (below it the reference's pad1d zero-extends before it
 * reflects and the result depends on what follows).  2240 samples = 7 frames for the cond encoder.  Negative: LDC_E_*. */
int ldc_stream_min_first(const ldc_config* cfg, int which, int side);
int ldc_stream_create(ldc_ctx* ctx, int which, int side, int B, ldc_stream** out);     /* B independent streams, all fresh */
int ldc_stream_reset(ldc_stream* st, const uint8_t* item_mask_host /* [B], NULL = all */, void* stream);
int ldc_stream_destroy(ldc_stream* st);   /* waits for the stream of the session's last call */
/* wav [B,1,T] -> z_out [B,rep_dims,T/hop] */
int ldc_seanet_encode_stream(ldc_ctx* ctx, ldc_stream* st, const float* wav, int T, float* z_out, void* stream);
/* z [B,rep_dims,L] -> wav_out [B,1,L*hop] */
int ldc_seanet_decode_stream(ldc_ctx* ctx, ldc_stream* st, const float* z, int L, float* wav_out, void* stream);
/* the cond encoder's stream only: wav [B,1,T] -> cond_out [B,rep_dims,T/320], codes_out [n_q,B,T/320] (may be NULL) */
int ldc_get_cond_stream(ldc_ctx* ctx, ldc_stream* st, const float* wav, int T, float bandwidth, float* cond_out, int64_t* codes_out,
                        void* stream);
/* for layer in diff_model.upsampling_layers: img = layer(img)   (sample.py:125-128, unet.py:372-377)
 * normalise: 0 = raw; 1 = img /= max|img|+1e-8 over the whole tensor (sample.py:129);
 *            2 = the same per batch item (a batch of independent utterances). cond [B,C,F] -> [B,C,L] */
int ldc_cond_upsample(ldc_ctx* ctx, const float* cond, int B, int F, int normalise, float* img_out, void* stream);
/* diff_model(x, t, cond)  (Unet1D.forward, unet.py:422-469).  cond is the RAW condition [B,C,F]
 * (process_cond runs inside, as in the reference).  t is one timestep for the whole batch: the sampler
 * only ever calls the model with torch.full((b,), t) (ddpm_loss.py:247); ldc_unet_forward_items takes one per item. */
int ldc_unet_forward(ldc_ctx* ctx, const float* x, int t, const float* cond, int B, int L, int F, float* eps_out,
                     void* stream);
/* diffusion.p_sample(x, t, cond) (ddpm_loss.py:244-251).  noise [B,C,L] or NULL (NULL: Philox draw;
 * ignored when t == 0). x is updated in place. */
int ldc_p_sample(ldc_ctx* ctx, float* x_inout, int t, const float* cond, const float* noise, int B, int L, int F,
                 void* stream);
/* diffusion.halfway_sampling(img, t=n_steps, condition=cond) (ddpm_loss.py:370-385): t = n_steps-1..0.
 * noise [n_steps,B,C,L] (entry j is consumed at iteration j; the last is unused) or NULL.
 * Five steps of every batch part are captured in one hipGraph keyed by (B, L, F) and replayed; the loop runs on a
 * context-owned copy of img, so a new tensor per call does not force a re-capture (a new noise pointer does). */
int ldc_denoise(ldc_ctx* ctx, float* img_inout, const float* cond, const float* noise, int n_steps, int B, int L,
                int F, void* stream);
/* SURVEY.md section 8(f) row 1 -- the two alternative decode modes left commented in sample.py:96-122; same kernels,
 * different loop driver.
 * diffusion.p_sample_loop(shape, condition) (ddpm_loss.py:253-266): ancestral sampling over all timesteps.
 * fill_start != 0: img is drawn ~N(0,1) on the device first (ddpm_loss.py:257); 0: img already holds the start image.
 * noise [timesteps,B,C,L] or NULL as for ldc_denoise. */
int ldc_p_sample_loop(ldc_ctx* ctx, float* img_inout, const float* cond, const float* noise, int fill_start, int B, int L,
                      int F, void* stream);
/* diffusion.infilling(infill_img, condition, midway_t, lam=lam) (ddpm_loss.py:331-367): per t = midway_t-1..0
 *   img <- p_sample(img,t); img <- (1-lam) img + lam infill; infill <- p_sample(infill,t); img <- (1-lam) img + lam infill.
 * Both img and infill_img are updated in place (the reference returns img).  fill_start != 0: img is drawn ~U[0,1) first
 * (ddpm_loss.py:336).  noise [2*midway_t,B,C,L] (draw 2i for img, 2i+1 for infill at iteration i) or NULL. */
int ldc_infilling(ldc_ctx* ctx, float* img_inout, float* infill_inout, const float* cond, int midway_t, const float* noise,
                  float lam, int fill_start, int B, int L, int F, void* stream);
/* sample.py:133-134: x /= std(x)+1e-8 ; x /= max|x|+1e-8.  per_item: 0 whole tensor, 1 per item. */
int ldc_output_normalise(ldc_ctx* ctx, float* wav_inout, int B, int T, int per_item, void* stream);
/* The whole per-batch body of synthesis() (sample.py:94-134) on resident buffers:
 * wav [B,1,T] -> wav_out [B,1,T]; optional stage outputs may be NULL. per_item as above. */
int ldc_decode(ldc_ctx* ctx, const float* wav, int B, int T, int n_steps, const float* noise, int per_item,
               float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream);

/* DDIM sampling: diffusion.ddim_sample (ddpm_loss.py:268-303) with clip_denoised, started at any t_start <= timesteps.
 * times = reversed(torch.linspace(-1, t_start - 1, n_steps + 1).int()); per pair (t, t_next):
 *   x0 = clamp(sqrt_recip_ac[t] img - sqrt_recipm1_ac[t] eps, -1, 1); img = x0 if t_next < 0, else
 *   img = x0 sqrt(ac[t_next]) + c eps + sigma z,  sigma = eta sqrt((1 - a / a_next)(1 - a_next) / (1 - a)), c = sqrt(1 - a_next - sigma^2).
 * sigma and c are computed on the host in float32; z is drawn only where sigma > 0.  Refused: n_steps outside [1, t_start],
 * t_start outside [1, timesteps], eta outside [0, 1] or not finite.
 * ldc_ddim_times: the reference's list of n_steps + 1 timesteps (the last is -1); host-only, needs no context or GPU. */
int ldc_ddim_times(int t_start, int n_steps, int* times_out);
/* t_start = timesteps with an N(0,1) start image is the reference's ddim_sample.  fill_start != 0: img is drawn ~N(0,1) on the
 * device first; 0: img holds the start image.  noise [n_steps,B,C,L] (entry j at iteration j; the last is unused) or NULL.
 * The steps replay captured graphs as ldc_denoise's do, keyed by (B, L, F) and the sampler kind: any n_steps and eta reuse them. */
int ldc_ddim_sample(ldc_ctx* ctx, float* img_inout, const float* cond, const float* noise, int fill_start, int t_start,
                    int n_steps, float eta, int B, int L, int F, void* stream);
/* ldc_decode with DDIM sampling from t_start (the start image is the upsampled, max-normalised condition, as in ldc_decode's
 * halfway sampling).  noise [n_steps,B,C,L] or NULL. */
int ldc_decode_ddim(ldc_ctx* ctx, const float* wav, int B, int T, int t_start, int n_steps, float eta, const float* noise,
                    int per_item, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream);

/* ldc_decode / ldc_decode_ddim on a batch of items of different lengths: wav [B,1,Tmax], lengths_host[B] samples per item
 * (host memory).  Every item is decoded as if alone (per-item normalisation).  t_start == 0: halfway DDPM sampling of
 * n_steps (eta ignored); t_start > 0: DDIM as ldc_decode_ddim.  noise [n_steps,B,C,Lmax] or NULL; item b consumes
 * noise[:, b, :, :L_b].  Outputs are zero beyond an item's length; what the padding of wav and noise holds is never read
 * into a valid value.  Every length and Tmax must be a positive multiple of lcm(cond hop, main hop * 2^halvings) samples
 * (2560 for enc_ratios 8 4, 640 for 8) and no length may exceed Tmax: LDC_E_INVALID otherwise, before any GPU work; the
 * fp8 engine refuses ragged calls the same way.  The lengths live in device memory, so the step graph captured for
 * (B, Tmax) is replayed for every set of lengths. */
int ldc_decode_ragged(ldc_ctx* ctx, const float* wav, const int32_t* lengths_host, int B, int Tmax, int t_start, int n_steps,
                      float eta, const float* noise, float* wav_out, float* latents_out, float* cond_out,
                      int64_t* codes_out, void* stream);
/* Item seeds: the samplers and decodes above with one Philox seed per item, seeds[B] uint64 in host memory.
 * Item b, with its own latent length len_b (L of a rectangular call, its own length in a ragged one), draws at iteration j under key
 * (lo(seeds[b]), hi(seeds[b])), counter (lo(g), hi(g), j, 0x4c444323), g = c_first * len_b + l, output (c mod 32) div 8: what
 * ldc_reseed(seeds[b]) followed by the unseeded entry at B = 1 on the item's own length draws.  Neither the item's position in the batch,
 * the padded length nor the batch part it lands in enter the draw; positions behind an item's length get no noise and stay zero; the
 * context's noise epoch is neither read nor advanced.  sampler: 0 DDPM (n_steps steps from t = n_steps - 1; t_start and eta are not read),
 * 1 DDIM (t_start, n_steps, eta as ldc_ddim_sample; draws only where the iteration is not the last and sigma > 0; eta == 0 accepts seeds
 * and draws nothing).  The seeds are data: a step graph captured under one set serves any other.
 * Refused with LDC_E_INVALID before any GPU work, the value named: seeds == NULL, a sampler other than 0 / 1 (DPM-Solver++ draws nothing,
 * so there is nothing to seed) -- both also with a NULL context --, and everything the unseeded entry refuses.
 * ldc_sample_seeded: ldc_denoise / ldc_ddim_sample on the given start image, rectangular. */
int ldc_sample_seeded(ldc_ctx* ctx, float* img_inout, const float* cond, int sampler, int t_start, int n_steps, float eta,
                      const uint64_t* seeds, int B, int L, int F, void* stream);
/* ldc_decode / ldc_decode_ddim (lengths_host NULL: rectangular, T = Tmax) or ldc_decode_ragged (lengths_host[B] samples, with all its
 * refusals, the fp8 engine's included) under item seeds.  The normalisation is per item at both ends, always: the start image is
 * max-normalised over the item and so is the output -- otherwise "as if alone" would be false. */
int ldc_decode_seeded(ldc_ctx* ctx, const float* wav, const int32_t* lengths_host /*[B] or NULL*/, int B, int Tmax, int sampler, int t_start,
                      int n_steps, float eta, const uint64_t* seeds, float* wav_out, float* latents_out, float* cond_out,
                      int64_t* codes_out, void* stream);
/* ldc_decode_codes / ldc_decode_codes_ddim (frames_host NULL: every item Fmax frames) or ldc_decode_codes_ragged (frames_host[B]) under
 * item seeds; per-item normalisation, as ldc_decode_seeded. */
int ldc_decode_codes_seeded(ldc_ctx* ctx, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B,
                            int Fmax, const int32_t* frames_host /*[B] or NULL*/, int sampler, int t_start, int n_steps, float eta,
                            const uint64_t* seeds, float* wav_out, float* latents_out, float* cond_out, void* stream);
/* Unet1D.forward with per-item latent lengths (test hook and building block): x [B,C,Lmax], cond [B,C,Fmax];
 * latent_lens_host[B] in latent frames, multiples of lcm(prod(upsampling_ratios), 2^halvings).  eps_out is zero beyond
 * an item's length. */
int ldc_unet_forward_ragged(ldc_ctx* ctx, const float* x, int t, const float* cond, const int32_t* latent_lens_host,
                            int B, int Lmax, int Fmax, float* eps_out, void* stream);
/* Unet1D.forward with a timestep per item (unet.py:422-437); latent_lens_host NULL = every item Lmax long (still the per-item plan).
 * With NULL lengths Lmax need not be on the ragged quantum: it must equal Fmax x prod(upsampling_ratios) and survive the UNet's
 * halvings, as for ldc_unet_forward.
 * t_host[B] (host memory), each in [0, timesteps).  The per-item plan is the ragged plan with the items' timesteps in device memory
 * too: eps_out of item b is what ldc_unet_forward gives for it alone at t_host[b], within rounding, and zero beyond its length. */
int ldc_unet_forward_items(ldc_ctx* ctx, const float* x, const int32_t* t_host /*[B]*/, const float* cond,
                           const int32_t* latent_lens_host, int B, int Lmax, int Fmax, float* eps_out, void* stream);

/* decode pools -----------------------------------------------------------------------------------
 * A pool is a fixed set of slots that step together on one captured step graph per batch part, while every slot keeps its own
 * sampler, timestep, iteration, noise (tape or Philox key), length and "is running" flag in device memory.  Items are admitted into
 * free slots and taken out of finished ones while the others keep stepping.
 * The sampler is a property of an item, not of the pool: ldc_pool_admit admits a halfway-DDPM item, ldc_pool_admit_ddim a DDIM item
 * with a schedule (t_start, n_steps, eta) of its own, ldc_pool_admit_dpm a DPM-Solver++(2M) item with a schedule (t_start, n_steps),
 * into the same pool, in any mix; an 8-iteration DDIM or DPM item leaves its slot while a 50-step DDPM neighbour keeps going.  The
 * pool owns one schedule row per slot (timesteps entries, 32 KB) and one x0 history block per slot (the size of its latents), both
 * allocated with the pool; the history is never cleared, an item's first iteration does not read it.
 * Contract: a DDPM item's latents are those of ldc_denoise(img, cond, noise, n_steps, B = 1, L, F) on the item alone, a DDIM item's
 * those of ldc_ddim_sample(img, cond, noise, fill_start = 0, t_start, n_steps, eta, B = 1, L, F), a DPM item's those of
 * ldc_dpm_sample(img, cond, t_start, n_steps, B = 1, L, F) -- whatever the other slots hold
 * (any sampler, any schedule), whenever it was admitted, whichever slot it sits in -- within rounding (the unfused GroupNorm
 * statistics are summed with atomics: the contract of ldc_decode_ragged, not bit identity).
 * What stays out of a pool: the fp8 engine, the fused GroupNorm and attention launch forms (a per-item plan takes the unfused ones),
 * and fill_start (a start image drawn on the device: the caller passes img).
 * An idle slot (free, or finished and not yet taken) is computed on and discarded: its latents are not stored, so a finished item
 * keeps its latents bit for bit until it is taken, and its noise tape is not read after its last step.
 * The step graphs are keyed by (slots, Lmax, Fmax, pool) in the context's plan and graph caches and replayed for every state; the
 * pool's plans hold its state and are never evicted (an option that rebuilds every plan is refused with LDC_E_STATE while a pool
 * lives).  Admit, take and evict are small stream-ordered writes and copies (admit also runs process_cond for the one item);
 * warm calls issue no device-wide synchronisation.  Calls on one pool must be issued in order on one HIP stream; stream == NULL
 * makes a call synchronous on the context's own stream.  Destroy a context's pools before the context.
 * Refused with LDC_E_INVALID before any GPU work, ldc_last_error() naming the value: a slot outside [0, slots); admit into a slot
 * that is not free; L off the ragged latent quantum or above Lmax; n_steps outside [1, timesteps]; n <= 0; slots <= 0; a pool of
 * another context; a null pointer; an fp8 engine; for a DDIM or DPM item t_start outside [1, timesteps], n_steps outside
 * [1, t_start]; for a DDIM item eta outside [0, 1] or not finite.  ldc_pool_take of a slot that is not finished: LDC_E_STATE.  After a refusal the
 * pool goes on as if the call had not been made.  A call that fails AFTER its GPU work began (LDC_E_HIP, LDC_E_NOMEM) marks the
 * pool: it then refuses with LDC_E_STATE until every slot has been evicted. */
typedef struct ldc_pool ldc_pool;
int ldc_pool_create(ldc_ctx* ctx, int slots, int Lmax, ldc_pool** out);      /* all slots free; Lmax on the ragged latent quantum */
int ldc_pool_destroy(ldc_pool* pool);                                         /* waits for the stream of the pool's last call */
/* img [1,C,L] start image, cond [1,C,F] raw condition (F = L / prod(upsampling_ratios)), L on the ragged latent quantum, <= Lmax;
 * n_steps in [1, timesteps]: the item will run t = n_steps-1 .. 0.  noise [n_steps,1,C,L] (device; kept alive by the caller until the
 * item has finished) or NULL: Philox with key = seed, i.e. the tape ldc_reseed(ctx, seed) gives the first ldc_denoise at B = 1. */
int ldc_pool_admit(ldc_ctx* ctx, ldc_pool* pool, int slot, const float* img, const float* cond, int L, int n_steps,
                   const float* noise, uint64_t seed, void* stream);
/* A DDIM item: n_steps iterations on the timesteps ldc_ddim_times(t_start, n_steps) with the coefficients of ldc_ddim_sample.  noise
 * [n_steps,1,C,L], entry j at iteration j (the last entry is never read, none is at eta == 0), or NULL: Philox with key = seed, i.e.
 * what ldc_reseed(ctx, seed) gives the first ldc_ddim_sample at B = 1.  ldc_pool_remaining counts its iterations. */
int ldc_pool_admit_ddim(ldc_ctx* ctx, ldc_pool* pool, int slot, const float* img, const float* cond, int L, int t_start, int n_steps,
                        float eta, const float* noise, uint64_t seed, void* stream);
/* A DPM-Solver++(2M) item: n_steps iterations on the timesteps ldc_ddim_times(t_start, n_steps) with the coefficients of
 * ldc_dpm_schedule, i.e. ldc_dpm_sample at B = 1.  Deterministic: no noise, seed or eta, nothing is drawn.  The item's x0 history is its
 * slot's; what an earlier item left there is never read.  ldc_pool_remaining counts its iterations. */
int ldc_pool_admit_dpm(ldc_ctx* ctx, ldc_pool* pool, int slot, const float* img, const float* cond, int L, int t_start, int n_steps,
                       void* stream);
int ldc_pool_step(ldc_ctx* ctx, ldc_pool* pool, int n, void* stream);         /* n steps of every running slot; a slot stops behind its last step */
int ldc_pool_remaining(const ldc_pool* pool, int32_t* remaining_host /*[slots]*/);   /* host mirror, no GPU work: -1 free, 0 finished, k > 0 running */
int ldc_pool_take(ldc_ctx* ctx, ldc_pool* pool, int slot, float* latents_out /*[1,C,L]*/, void* stream);   /* finished slots only; frees the slot */
int ldc_pool_peek(ldc_ctx* ctx, ldc_pool* pool, int slot, float* latents_out /*[1,C,L]*/, void* stream);   /* ldc_pool_take without freeing the slot */
int ldc_pool_evict(ldc_pool* pool, int slot);                                 /* drop a running or finished item; frees the slot (a free slot: no-op) */

/* ---- Coupled windows: one recording longer than the UNet's window, decoded on ONE shared latent -------------
 * The recording's latent [1,C,Ltot] is covered by W windows of Lw frames that overlap by `overlap`; the windows are the items of an
 * ordinary equal-length batch (B = W, L = Lw, F = Lw / up; up = prod(upsampling_ratios)), process_cond runs per window on its slice
 * of the raw condition, and after every UNet pass the windows' eps are blended per global frame -- ebar(g) = sum_k w_k(g) eps_k(g - s_k),
 * fp32, in window order -- and the ONE state is updated from ebar by the sampler's own arithmetic at B = 1, L = Ltot.  Noise is that
 * of the B = 1, L = Ltot call: a tape [n_steps,1,C,Ltot], or Philox with the key and epoch rule of ldc_denoise / ldc_ddim_sample.
 * A W = 1 call is ldc_denoise at B = 1; an overlap-0 call is the batch of W independent chunks.
 * Layout (ldc_window_layout: host-only, needs no context or GPU; returns W or an error): Ltot <= Lw: one window of Ltot frames; else
 * H = Lw - overlap, W = 1 + ceil((Ltot - Lw) / H), s_k = min(k H, Ltot - Lw) (the last window is right-aligned).  Weights, in double
 * and rounded once to float: u_k(l) = min(1, (l + 0.5) / Rl_k, (Lw - l - 0.5) / Rr_k) over the terms whose overlap Rl_k (with the
 * predecessor) / Rr_k (with the successor) is > 0, w_k(g) = u_k(g - s_k) / sum_j u_j(g - s_j): exactly 1.0f on a singly covered frame,
 * a linear cross-fade on a plain overlap; a frame is covered by at most three windows.  starts_out [32]; weights_out [W][Lw] or NULL.
 * Refused (LDC_E_INVALID, before any GPU work, ldc_last_error() naming the value): Ltot, Lw or overlap not a multiple of up, overlap
 * outside [0, Lw / 2], more than 32 windows; by the calls with a context also Ltot != Ftot * up, Lw (when Ltot > Lw) not a multiple of
 * the latent chunk quantum lcm(up, 2^halvings), the fp8 engine, and what ldc_denoise / ldc_ddim_sample / ldc_decode refuse.
 * A windows plan is one batch part on one stream whatever `split` says; its cache key holds (Ltot, Lw, overlap), so its step graphs are
 * its own.  Warm calls allocate nothing and never synchronise the device.
 * ldc_window_layout_n: ldc_window_layout for up to max_windows (<= 128) windows, starts_out [max_windows]; bit-identical to it for
 * W <= 32.  ldc_window_parts: P_eff = min(parts, W) and the range starts first_out [parts + 1] of W windows (W <= 32 parts) cut into
 * `parts` (<= 4) contiguous batch parts, part p holding [floor(p W / P_eff), floor((p + 1) W / P_eff)).  Both host-only; they lay the
 * ground for a windows call in batch parts, which no call with a context offers yet.
 * DPM-Solver++(2M) on windows (ldc_dpm_sample_windows, ldc_decode_dpm_windows, ldc_decode_codes_dpm_windows): iteration j blends the
 * windows' eps as above and applies the update documented at ldc_dpm_schedule to the ONE state with ONE history x0_{j-1} [1,C,Ltot] (not
 * one per window), which lives with the windows plan.  Nothing is drawn and the noise epoch stays where it is; the steps replay graphs
 * keyed by the layout and the sampler kind (5 steps per graph, single-step remainders), never a DDPM or DDIM graph.  A W = 1 call is
 * ldc_dpm_sample at B = 1, an overlap-0 call the batch of independent chunks.
 * The receiver (ldc_decode_codes_windows, ldc_decode_codes_dpm_windows): the same decodes from the RVQ codes of ONE recording of Ftot
 * condition frames -- quantizer.decode(codes), the start image normalised over the whole recording, per-window condition slices, the
 * coupled loop, the decoder over the whole latent.  For the codes ldc_decode_windows returns, cond_out is bit-identical to its cond_out.
 * Sources, packed layout and the "[bad_code]" refusal are those of ldc_decode_codes at B = 1, F = Ftot.
 * Window groups (the *_windows_group entries): R >= 1 recordings in one call, the windows of all of them -- W_sum = sum W_r <= 32 -- the
 * items of ONE equal-length batch at (B = W_sum, L = Lw, F = Lw / up).  Recording r keeps the layout ldc_window_layout(Ltot_r, Lw,
 * overlap, up) gives it alone, its windows take the batch items w0_r .. w0_r + W_r - 1 (w0_r = sum_{q<r} W_q) in recording order, its own
 * fp32 state, noise and (DPM) x0 history, and its eps are blended from its own windows only; the timestep and the schedule are the
 * call's.  Each recording comes out as the single-recording call gives it alone.  Packed tensors: with off_r = sum_{q<r} Ltot_q and Lsum
 * = sum Ltot_r, the state, eps_out and every step of a tape [n_steps][C * Lsum] hold recording r's [C][Ltot_r] block at float offset
 * C * off_r (inside a block: the B = 1, L = Ltot_r layout); the raw condition holds [Cc][Ftot_r] at Cc * off_r / up; waveforms lie one
 * behind the other, codes_out holds [n_q][Ftot_r] blocks.  Ltot, Ftot, T and seeds are HOST arrays of R entries.  Noise: a tape, or Philox
 * with seeds[R] -- recording r draws what ldc_denoise_windows / ldc_ddim_sample_windows draws for it alone right after
 * ldc_reseed(seeds[r]) (key seeds[r], epoch 0).  A group call never reads or advances the context's noise epoch; a sampler that draws with
 * neither a tape nor seeds is refused; DPM takes neither.  Refused besides what the single-recording calls refuse: R outside [1, 32], a
 * recording shorter than Lw (index and value named: it would shrink the window and break the equal-length batch), W_sum > 32 (the sum
 * named).  An R = 1 group is the single-recording call, a group of R one-window recordings an ordinary B = R batch.  The group's plan and
 * step graphs are keyed by the ORDERED list of lengths, Lw and overlap: neither a single-recording call nor a group of other lengths
 * replays them.  One part on one stream whatever `split` says; warm calls allocate nothing and never synchronise the device.
 * Not available: decode pools, batch parts, more than 32 windows per call, ragged window lengths; for window groups also the receiver
 * (decoding from codes) and the fp8 engine.  Nothing here is a claim about perceived quality. */
int ldc_window_layout(int Ltot, int Lw, int overlap, int up, int* starts_out /*[32]*/, float* weights_out /*[W*Lw] or NULL*/);
int ldc_window_layout_n(int Ltot, int Lw, int overlap, int up, int max_windows, int* starts_out /*[max_windows]*/, float* weights_out /*[W*Lw] or NULL*/);
int ldc_window_parts(int W, int parts, int* first_out /*[parts + 1]*/);
/* the blended eps of one UNet pass at timestep t: x [1,C,Ltot], cond [1,Cc,Ftot] (raw), eps_out [1,C,Ltot] */
int ldc_unet_forward_windows(ldc_ctx* ctx, const float* x, int t, const float* cond, int Ltot, int Ftot, int Lw, int overlap,
                             float* eps_out, void* stream);
/* ldc_denoise / ldc_ddim_sample (img holds the start image) of the recording on coupled windows */
int ldc_denoise_windows(ldc_ctx* ctx, float* img_inout, const float* cond, const float* noise, int n_steps, int Ltot, int Ftot, int Lw,
                        int overlap, void* stream);
int ldc_ddim_sample_windows(ldc_ctx* ctx, float* img_inout, const float* cond, const float* noise, int t_start, int n_steps, float eta,
                            int Ltot, int Ftot, int Lw, int overlap, void* stream);
/* ldc_decode / ldc_decode_ddim at B = 1 with the denoise loop replaced: get_cond and the normalised start image over the whole
 * recording wav [1,1,T], the coupled loop, the decoder over the whole latent, output normalisation.  Lw, overlap in latent frames. */
int ldc_decode_windows(ldc_ctx* ctx, const float* wav, int T, int n_steps, const float* noise, int Lw, int overlap, float* wav_out,
                       float* latents_out, float* cond_out, int64_t* codes_out, void* stream);
int ldc_decode_ddim_windows(ldc_ctx* ctx, const float* wav, int T, int t_start, int n_steps, float eta, const float* noise, int Lw,
                            int overlap, float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream);
/* ldc_dpm_sample / ldc_decode_dpm of the recording on coupled windows.  Refused first, also with a NULL context: t_start < 1, n_steps
 * outside [1, t_start]; then what the DDIM windows call refuses. */
int ldc_dpm_sample_windows(ldc_ctx* ctx, float* img_inout, const float* cond, int t_start, int n_steps, int Ltot, int Ftot, int Lw,
                           int overlap, void* stream);
int ldc_decode_dpm_windows(ldc_ctx* ctx, const float* wav, int T, int t_start, int n_steps, int Lw, int overlap, float* wav_out,
                           float* latents_out, float* cond_out, int64_t* codes_out, void* stream);
/* The receiver on coupled windows.  codes [n_q,1,Ftot] int64 or packed (exactly one non-NULL); wav_out [1,1,Ftot*320].
 * ldc_decode_codes_windows: t_start == 0 is halfway DDPM sampling of n_steps (eta unused), t_start > 0 is DDIM -- the convention of
 * ldc_decode_codes_ragged; noise as in ldc_decode_windows / ldc_decode_ddim_windows.  Refused first, also with a NULL context: both
 * sources or neither, Ftot or n_q < 1, bits, packed_stride, eta outside [0, 1], t_start < 0 (DPM: < 1), n_steps < 1 or > t_start; then
 * what ldc_decode_codes at B = 1 and the windows calls refuse. */
int ldc_decode_codes_windows(ldc_ctx* ctx, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int Ftot,
                             int t_start, int n_steps, float eta, const float* noise, int Lw, int overlap, float* wav_out,
                             float* latents_out, float* cond_out, void* stream);
int ldc_decode_codes_dpm_windows(ldc_ctx* ctx, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q,
                                 int Ftot, int t_start, int n_steps, int Lw, int overlap, float* wav_out, float* latents_out,
                                 float* cond_out, void* stream);
/* Window groups.  ldc_window_group_layout (host-only): w0_out [R + 1], starts_out [32] in each recording's own frames (zero behind
 * W_sum), weights_out [W_sum][Lw] or NULL; returns W_sum. */
int ldc_window_group_layout(int R, const int* Ltot /*[R]*/, int Lw, int overlap, int up, int* w0_out /*[R + 1]*/, int* starts_out /*[32]*/,
                            float* weights_out /*[W_sum*Lw] or NULL*/);
/* ldc_unet_forward_windows of every recording in one UNet pass: x, eps_out packed [C][Ltot_r] blocks, cond packed [Cc][Ftot_r] blocks */
int ldc_unet_forward_windows_group(ldc_ctx* ctx, const float* x, int t, const float* cond, int R, const int* Ltot /*[R]*/,
                                   const int* Ftot /*[R]*/, int Lw, int overlap, float* eps_out, void* stream);
/* sampler 0: ldc_denoise_windows (t_start, eta unused); 1: ldc_ddim_sample_windows; 2: ldc_dpm_sample_windows (eta, noise, seeds unused)
 * of every recording in one loop; refusals of that call in its order.  img_inout, cond and noise [n_steps][C * Lsum] packed. */
int ldc_sample_windows_group(ldc_ctx* ctx, float* img_inout, const float* cond, int sampler, int t_start, int n_steps, float eta,
                             const float* noise, const uint64_t* seeds /*[R] or NULL*/, int R, const int* Ltot /*[R]*/,
                             const int* Ftot /*[R]*/, int Lw, int overlap, void* stream);
/* ldc_decode_windows / _ddim_windows / _dpm_windows of every recording with ONE loop; the codec ends run per recording (get_cond, the
 * start image normalised over that recording, the decoder, output normalisation).  wav, wav_out: T[r] samples each, one behind the other. */
int ldc_decode_windows_group(ldc_ctx* ctx, const float* wav, int R, const int* T /*[R]*/, int sampler, int t_start, int n_steps, float eta,
                             const float* noise, const uint64_t* seeds /*[R] or NULL*/, int Lw, int overlap, float* wav_out,
                             float* latents_out, float* cond_out, int64_t* codes_out, void* stream);

/* The decode of ldc_decode / ldc_decode_ddim started from RVQ codes instead of a waveform (the receiver side):
 * quantizer.decode(codes) -> upsample, /= max|.| -> sampling -> decoder -> output normalisation.
 * Exactly one of codes ([n_q,B,F] int64, device) / packed ([B][packed_stride] bytes, device, `bits` per code in
 * compress.py's push order: for t: for k, LSB first, as ldc_pack_codes writes them) is non-NULL.  wav_out [B,1,F*320];
 * cond_out [B,D,F] (the dequantised condition), latents_out [B,D,F*320/hop]; optional stage outputs may be NULL.
 * For the codes get_cond returns, the condition is bit-identical to the waveform decode's, and so is everything after it.
 * Refused (LDC_E_INVALID, before any GPU work): both sources or neither, n_q outside [1, n_q_layers], an F whose T = F*320
 * ldc_decode would refuse, bits outside [ceil(log2(bins)), 16], packed_stride < ldc_packed_bytes(n_q, F, bits), and the
 * n_steps / t_start / eta refusals of ldc_decode / ldc_decode_ddim.  A code VALUE outside [0, bins) is found on the device:
 * its condition row is NaN (never an out-of-bounds read) and the call -- or, with a non-NULL stream, the next call on the
 * context -- fails with LDC_E_INVALID and "[bad_code]" in ldc_last_error(), naming a codebook, item and frame.
 * ldc_rvq_decode validates its codes the same way. */
int ldc_decode_codes(ldc_ctx* ctx, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits,
                     int n_q, int B, int F, int n_steps, const float* noise, int per_item,
                     float* wav_out, float* latents_out, float* cond_out, void* stream);
int ldc_decode_codes_ddim(ldc_ctx* ctx, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits,
                          int n_q, int B, int F, int t_start, int n_steps, float eta, const float* noise, int per_item,
                          float* wav_out, float* latents_out, float* cond_out, void* stream);
/* ldc_decode_codes / ldc_decode_codes_ddim with the length semantics of ldc_decode_ragged (the receiver of containers of
 * different lengths): frames_host[B] (host memory) condition frames of item b are its own.  codes [n_q,B,Fmax] or packed
 * [B][packed_stride]: the codes behind an item's frames are neither read nor validated, and a packed item's stream is
 * ldc_packed_bytes(n_q, frames_host[b], bits) bytes long -- nothing behind that byte of its row is read, so payloads of unequal
 * containers go in as they are.  Within an item's frames the condition rows are bit-identical to ldc_rvq_decode of the item alone
 * and a code outside [0, bins) is refused as in ldc_decode_codes ("[bad_code]" names its codebook, item and frame); rows behind
 * them are zero.  t_start == 0: halfway DDPM sampling of n_steps; t_start > 0: DDIM.  Per-item normalisation; wav_out
 * [B,1,Fmax*320], latents_out, cond_out are zero beyond an item's length; noise as in ldc_decode_ragged.
 * Refused (LDC_E_INVALID, before any GPU work): what ldc_decode_codes refuses; a frames_host[b] that is not a positive multiple
 * of the ragged quantum / 320 (8 frames for enc_ratios 8 4, 2 for 8) or exceeds Fmax; packed_stride below the packed bytes of
 * the longest item; the fp8 engine.  The step graph captured for (B, Fmax) is the one ldc_decode_ragged replays at
 * (B, Fmax * 320): it serves every set of lengths. */
int ldc_decode_codes_ragged(ldc_ctx* ctx, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q,
                            int B, int Fmax, const int32_t* frames_host, int t_start, int n_steps, float eta, const float* noise,
                            float* wav_out, float* latents_out, float* cond_out, void* stream);

/* DPM-Solver++(2M) sampling, data-prediction form (Lu et al. 2022): the second-order multistep solver on DDIM's timestep list and
 * DDIM's clipped x0.  Deterministic: no noise argument, nothing is drawn, the noise epoch of the context is not advanced.
 * Per timestep t, from the checkpoint's float32 tables promoted to double: R = sqrt_recip_alphas_cumprod[t] (1 / alpha),
 * M = sqrt_recipm1_alphas_cumprod[t] (sigma / alpha), alpha = 1 / R, sigma = M / R, lambda = -ln M.
 * times = ldc_ddim_times(t_start, n_steps); iteration j, (t, tn) = (times[j], times[j + 1]):
 *   x0_j = clamp(R_t img - M_t eps(img, t, cond), -1, 1)
 *   tn < 0 (the final iteration): img = x0_j, the history is not read; else
 *   h = lambda_tn - lambda_t, phi = -alpha_tn expm1(-h), a = sigma_tn / sigma_t,
 *   j == 0: img = a img + phi x0_0;  j >= 1: r = (lambda_t - lambda_times[j-1]) / h,
 *                                            img = a img + phi (1 + 1/(2r)) x0_j - (phi / (2r)) x0_{j-1}.
 * The coefficients are computed on the host in double and rounded once to float; the update runs in float32.
 * ldc_dpm_schedule: that table for any pair of tables of `timesteps` entries; host-only, needs no context or GPU (like ldc_ddim_times).
 * t_out [n_steps]; coef_out [n_steps][3], rows (a, b0, b1) of img = a img + b0 x0_j + b1 x0_{j-1}: b1 == 0 on row 0, the final row
 * is (0, 1, 0).
 * Refused by every call here (LDC_E_INVALID, before any GPU work, ldc_last_error() naming the value; a NULL context sees the
 * context-free ones): t_start outside [1, timesteps], n_steps outside [1, t_start], null pointers, and the shape refusals of the
 * DDIM call each one mirrors.  The steps replay captured graphs keyed by (B, L, F) and the sampler kind: every n_steps reuses them,
 * and no call replays a DDPM or DDIM graph.  The x0 history lives with the cached plan of each batch part.
 * On coupled windows: ldc_dpm_sample_windows and its decodes, above.  In decode pools: ldc_pool_admit_dpm, above.
 * Not available: ldc_decode_codes_ragged, the SDE and third-order variants. */
int ldc_dpm_schedule(const float* sqrt_recip, const float* sqrt_recipm1, int timesteps, int t_start, int n_steps, int* t_out,
                     float* coef_out);
/* ldc_ddim_sample's arguments without noise, fill_start and eta: img holds the start image. */
int ldc_dpm_sample(ldc_ctx* ctx, float* img_inout, const float* cond, int t_start, int n_steps, int B, int L, int F, void* stream);
/* ldc_decode_ddim / ldc_decode_codes_ddim / ldc_decode_ragged (the fp8 engine refused, as for every ragged call) with this sampler. */
int ldc_decode_dpm(ldc_ctx* ctx, const float* wav, int B, int T, int t_start, int n_steps, int per_item, float* wav_out,
                   float* latents_out, float* cond_out, int64_t* codes_out, void* stream);
int ldc_decode_codes_dpm(ldc_ctx* ctx, const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B,
                         int F, int t_start, int n_steps, int per_item, float* wav_out, float* latents_out, float* cond_out,
                         void* stream);
int ldc_decode_ragged_dpm(ldc_ctx* ctx, const float* wav, const int32_t* lengths_host, int B, int Tmax, int t_start, int n_steps,
                          float* wav_out, float* latents_out, float* cond_out, int64_t* codes_out, void* stream);

/* bit-stream layer: the on-wire format between ldc_rvq_encode and ldc_rvq_decode -- SURVEY.md section 8(f) row 3 ------------
 * Every batch item is an independent stream.  All results are bit-exact with the reference classes.  These calls need no
 * weights (any context of the device).
 * BitPacker / BitUnpacker (srcs/encodec/binary.py:55-118) over a frame's codes in compress.py's push order
 * (srcs/encodec/compress.py:74-84: for t: for k: codes[k][t]); `bits` per code (10 for the 1024-entry codebooks).
 * codes [n_q,B,F] int64 (device) <-> out [B][out_stride] bytes (device), ldc_packed_bytes() of them used per item. */
int64_t ldc_packed_bytes(int n_q, int F, int bits);
int ldc_pack_codes(ldc_ctx* ctx, const int64_t* codes, int n_q, int B, int F, int bits, uint8_t* out, int64_t out_stride, void* stream);
int ldc_unpack_codes(ldc_ctx* ctx, const uint8_t* in, int64_t in_stride, int n_q, int B, int F, int bits, int64_t* codes_out,
                     void* stream);
/* build_stable_quantized_cdf (srcs/quantization/ac.py:18-53): pdf [rows][card] float32 -> cdf [rows][card] int32. */
int ldc_ac_build_cdf(ldc_ctx* ctx, const float* pdf, int rows, int card, int total_range_bits, float roundoff, int min_range,
                     int32_t* cdf_out, void* stream);
/* ArithmeticCoder.push ... flush (ac.py:131-174) of S symbols per stream.  symbols [B][S] int32.  n_static == 0: cdf is
 * [B][S][card] (a table per step, as an LM would provide, compress.py:79-82); n_static > 0: cdf is [n_static][card] and
 * symbol s uses table s % n_static (one static table per codebook).  nbytes_out[b] = bytes written, -1 = out_stride too
 * small or a symbol outside its table. */
int ldc_ac_encode(ldc_ctx* ctx, const int32_t* symbols, const int32_t* cdf, int B, int S, int card, int n_static, int total_range_bits,
                  uint8_t* out, int64_t out_stride, int64_t* nbytes_out, void* stream);
/* ArithmeticDecoder.pull x S (ac.py:218-260).  status_out[b]: 0 ok, 1 stream exhausted (pull returned None), 2 search failed. */
int ldc_ac_decode(ldc_ctx* ctx, const uint8_t* in, int64_t in_stride, const int64_t* nbytes, const int32_t* cdf, int B, int S, int card,
                  int n_static, int total_range_bits, int32_t* symbols_out, int32_t* status_out, void* stream);
/* The two calls above with a symbol count per stream: n_sym [B] int32 (device), 0 <= n_sym[b] <= S.  Stream b codes the first
 * n_sym[b] symbols of its row of symbols [B][S] (tables: row b*S + s of cdf [B][S][card], or the static ones) and flushes there:
 * its bytes are those of ldc_ac_encode on the item alone with S = n_sym[b].  The decoder writes 0 behind n_sym[b] symbols.
 * A count outside [0, S]: nbytes_out[b] = -1 / status_out[b] = 3. */
int ldc_ac_encode_ragged(ldc_ctx* ctx, const int32_t* symbols, const int32_t* n_sym, const int32_t* cdf, int B, int S, int card,
                         int n_static, int total_range_bits, uint8_t* out, int64_t out_stride, int64_t* nbytes_out, void* stream);
int ldc_ac_decode_ragged(ldc_ctx* ctx, const uint8_t* in, int64_t in_stride, const int64_t* nbytes, const int32_t* n_sym,
                         const int32_t* cdf, int B, int S, int card, int n_static, int total_range_bits, int32_t* symbols_out,
                         int32_t* status_out, void* stream);

/* audio front end -- SURVEY.md section 8(f) row 4: torchaudio.functional.resample(wav, orig_freq, new_freq) with its defaults
 * (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), the call at srcs/sample.py:84.  wav [C][T] -> out [C][ldc_resample_out_len]. */
int64_t ldc_resample_out_len(int64_t T, int orig_freq, int new_freq);
int ldc_resample(ldc_ctx* ctx, const float* wav, int C, int64_t T, int orig_freq, int new_freq, float* out, void* stream);

/* training step of the diffusion UNet -- SURVEY.md section 8(f) row 2 (BASELINE config 4); fp32 correctness path, reference layouts [B,C,L]
 * diffusion.q_sample(x_start, t, noise) (ddpm_loss.py:386-392); t [B] int64 (device). */
int ldc_train_q_sample(ldc_ctx* ctx, const float* x_start, const int64_t* t, const float* noise, int B, int C, int L, float* x_t,
                       void* stream);
/* Number of diffusion timesteps T of the loaded schedule (len(diffusion.betas)); device-side t is clamped to [0, T). */
int ldc_train_num_timesteps(ldc_ctx* ctx);
/* predicted_x_start of p_losses (ddpm_loss.py:416-420 -> :175-179, no clamp): x0 = sqrt(1/abar_t) x_t - sqrt(1/abar_t - 1) eps. */
int ldc_train_predict_x_start(ldc_ctx* ctx, const float* x_t, const float* eps, const int64_t* t, int B, int C, int L, float* x0_out,
                              void* stream);
/* Monitoring loss of DiffAudioRep.forward (model.py:194): per item clamp(-SD-SDR(est, tgt), min clip_min) -- ClippedSDR
 * (losses_fn.py:56-66) over asteroid 0.6.0's MultiSrcNegSDR("sdsdr"), one source; the reference calls it as (x, x_hat). */
int ldc_train_neg_sdsdr(ldc_ctx* ctx, const float* est, const float* tgt, int B, int64_t n_per_item, float clip_min, float* per_item_out,
                        void* stream);

/* The objective of p_losses (ddpm_loss.py:434-438, loss_type l1): loss = mean_b(p2_loss_weight[t_b] * mean_{c,l}|out - target|);
 * loss_out [1]; grad_out (nullable) = d loss / d model_out. */
int ldc_train_l1_loss(ldc_ctx* ctx, const float* model_out, const float* target, const int64_t* t, int B, int C, int L, float* loss_out,
                      float* grad_out, void* stream);
/* Block (unet.py:137-154): y = SiLU(GroupNorm(conv_k3(x; WS(w), bias)) * (scale + 1) + shift), weights as trained (raw `w`
 * [Cout,Cin,3]: the weight standardisation of unet.py:73-78 is part of the graph).  scale_shift [B][2*Cout] (scale | shift)
 * or NULL.  `ws`: ldc_train_block_ws_floats() floats of device scratch that carry the saved tensors from forward to backward. */
int64_t ldc_train_block_ws_floats(int B, int Cin, int Cout, int L, int groups);
int ldc_train_block_forward(ldc_ctx* ctx, const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                            const float* scale_shift, int B, int Cin, int Cout, int L, int groups, float* y, float* ws, void* stream);
/* gradients of everything: dx [B,Cin,L] (nullable), dw [Cout,Cin,3], db / dgamma / dbeta [Cout], dscale_shift [B][2*Cout]. */
int ldc_train_block_backward(ldc_ctx* ctx, const float* dy, const float* x, const float* gamma, const float* beta,
                             const float* scale_shift, int B, int Cin, int Cout, int L, int groups, float* ws, float* dx, float* dw,
                             float* db, float* dgamma, float* dbeta, float* dscale_shift, void* stream);

/* Channel LayerNorm of the UNet's attention blocks (srcs/modules/unet.py:82-101), forward and backward, [B, C, L] float32:
 * y = (x - mean_c) * rsqrt(var_c + 1e-5) * g.  `stats`: [B, L, 2] floats written by the forward pass (mean, 1/std), read by the
 * backward pass, which returns dx and dg [C]. */
int ldc_train_layernorm_forward(ldc_ctx* ctx, const float* x, const float* g, int B, int C, int L, float* y, float* stats, void* stream);
int ldc_train_layernorm_backward(ldc_ctx* ctx, const float* dy, const float* x, const float* g, const float* stats, int B, int C, int L,
                                 float* dx, float* dg, void* stream);

/* y[b, o, l] = bias[o] + sum_i w[o, i] * a(x[b, i, l]) on [B, C, L] float32, a = identity or SiLU (`pre_silu`): the 1x1 res_conv of a
 * ResnetBlock (srcs/modules/unet.py:171,192) and, with L = 1, its time-embedding MLP SiLU -> Linear (unet.py:163-166); backward
 * returns dx (may be NULL), dw [Cout, Cin] and db (may be NULL).  With ldc_train_block_* this is a whole ResnetBlock. */
int ldc_train_pointwise_forward(ldc_ctx* ctx, const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int L, int pre_silu,
                                float* y, void* stream);
int ldc_train_pointwise_backward(ldc_ctx* ctx, const float* dy, const float* x, const float* w, int B, int Cin, int Cout, int L, int pre_silu,
                                 float* dx, float* dw, float* db, void* stream);

/* LinearAttention core (srcs/modules/unet.py:208-221: both softmaxes and both einsums, between to_qkv and to_out), forward and backward.
 * qkv [B, 3*heads*dim_head, N] float32 = [q | k | v] (the to_qkv output), out [B, heads*dim_head, N]; `ws`:
 * ldc_train_linattn_ws_floats() floats carrying the saved softmaxes and context to the backward pass; dqkv in the layout of qkv. */
int64_t ldc_train_linattn_ws_floats(int B, int heads, int dim_head, int N);
int ldc_train_linattn_forward(ldc_ctx* ctx, const float* qkv, int B, int heads, int dim_head, int N, float* out, float* ws, void* stream);
int ldc_train_linattn_backward(ldc_ctx* ctx, const float* dout, const float* qkv, int B, int heads, int dim_head, int N, float* ws, float* dqkv,
                               void* stream);

/* The remaining layers of Unet1D (srcs/modules/unet.py:248-470) for the assembled forward / backward, [B, C, L] float32:
 * plain Conv1d with any kernel size / stride / zero padding (init_conv k7 p3 :307, Downsample k4 s2 p1 :64-65, the k3 p1 convs of
 * Upsample :58-62 and of the last levels, final_conv k1 :372); nearest x2 upsampling and its adjoint; tanh / GELU / SiLU
 * (`kind` 0 / 1 / 2; dy == NULL: out = f(x), else out = dy * f'(x)); the bottleneck softmax Attention core (:234-245) with
 * the [B, heads, N, N] attention matrix kept in `ws` (2 * B * heads * N * N floats) for the backward pass. */
int ldc_train_conv_forward(ldc_ctx* ctx, const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int Lin, int K, int stride,
                           int pad, float* y, void* stream);
int ldc_train_conv_backward(ldc_ctx* ctx, const float* dy, const float* x, const float* w, int B, int Cin, int Cout, int Lin, int K, int stride,
                            int pad, float* dx, float* dw, float* db, void* stream);
/* Option "train_dw_side" (process-wide, 0 / 1, default 0; DiffusionTrainer sets it around its backward pass): ldc_train_block_backward puts
 * the weight-gradient GEMM of the Block (and what hangs on it: the ordered reduction of its parts, the bias gradient, the
 * weight-standardisation backward) on an internal side stream behind an event, the caller's stream goes on with dX.  ldc_train_join makes
 * `stream` wait for everything the side stream holds: call it between the backward pass and the first use of a parameter gradient.  The
 * caller keeps the Block's workspace and saved input alive until then.  (The reference's autograd engine does the same thing with its
 * own streams; srcs/train.py:150-158 is `loss.backward()`.) */
int ldc_train_join(ldc_ctx* ctx, void* stream);
/* Round 6 (second half): ldc_train_conv_backward, ldc_train_pointwise_backward (L > 1) and ldc_train_layernorm_backward put their parameter
 * gradients on the side stream as well; those read `dy`, which the caller therefore keeps alive until ldc_train_join -- a torch caller marks
 * it with dy.record_stream(torch.cuda.ExternalStream(handle)), handle from ldc_train_side_stream. */
int ldc_train_side_stream(ldc_ctx* ctx, void** stream_out);
int ldc_train_upsample2(ldc_ctx* ctx, const float* in, int64_t rows, int L, int backward, float* out, void* stream);
int ldc_train_activation(ldc_ctx* ctx, const float* x, const float* dy, int64_t n, int kind, float* out, void* stream);
int64_t ldc_train_attn_ws_floats(int B, int heads, int N);
int ldc_train_attn_forward(ldc_ctx* ctx, const float* qkv, int B, int heads, int dim_head, int N, float* out, float* ws, void* stream);
int ldc_train_attn_backward(ldc_ctx* ctx, const float* dout, const float* qkv, int B, int heads, int dim_head, int N, float* ws, float* dqkv,
                            void* stream);

/* Unet1D.process_cond for training (srcs/modules/unet.py:372-377,401-420): the condition upsampler SConvTranspose1d(C, C, 2 * ratio,
 * stride ratio, non-causal; srcs/modules/conv.py:235-274) forward / backward on [B, C, L] -> [B, C, L * ratio] (weight [Cin, Cout,
 * 2 * ratio]), and the per-item max-abs scaling x / (max|x| + 1e-20): dy == NULL forward, else the gradient w.r.t. x. */
int ldc_train_convtr_forward(ldc_ctx* ctx, const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int L, int ratio, float* y,
                             void* stream);
int ldc_train_convtr_backward(ldc_ctx* ctx, const float* dy, const float* x, const float* w, int B, int Cin, int Cout, int L, int ratio, float* dx,
                              float* dw, float* db, void* stream);
int ldc_train_maxscale(ldc_ctx* ctx, const float* x, const float* dy, int B, int64_t n_per_item, float* out, void* stream);

/* One Adam step over flat device buffers, in place (srcs/train.py:365-371: optim.Adam(params, lr); torch's defaults are
 * beta1 0.9, beta2 0.999, eps 1e-8, no weight decay, no amsgrad).  `step` counts from 1 (bias correction). */
int ldc_train_adam_step(ldc_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr,
                        float beta1, float beta2, float eps, void* stream);
/* The same with the step count in device memory (*step_dev is counted up first, then used): the form a captured (hipGraph) optimisation
 * step needs -- a host-side count would be frozen into the graph. */
int ldc_train_adam_step_dev(ldc_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step_dev,
                            float lr, float beta1, float beta2, float eps, void* stream);

/* L1 primitives (reference srcs/modules/conv.py, lstm.py), exposed for the parity tests ---------- */
/* SConv1d.forward (conv.py:217-232), reflect padding.  w [Cout,Cin,k] (already weight-norm folded),
 * all HOST float32; x/y DEVICE [B,Cin,L] / [B,Cout,Lout].  pre_elu applies ELU to the input.
 * This hook is stricter than the encode / decode path: it refuses L <= pad_left (LDC_E_INVALID), while sea_conv (and
 * ldc_debug_sea_conv, which runs through it) computes such inputs as the reference's pad1d does. */
int ldc_sconv1d(ldc_ctx* ctx, const float* x, int B, int Cin, int L, const float* w_host, const float* b_host,
                int Cout, int k, int stride, int dilation, int causal, int pre_elu, float* y, void* stream);
/* SConvTranspose1d.forward (conv.py:252-274), w [Cin,Cout,k] host. */
int ldc_sconvtr1d(ldc_ctx* ctx, const float* x, int B, int Cin, int L, const float* w_host, const float* b_host,
                  int Cout, int k, int stride, int causal, float* y, void* stream);
/* SLSTM.forward (lstm.py:22-28): weights host, PyTorch layout [4H,H] / [4H] per layer, order
 * w_ih, w_hh, b_ih, b_hh for layer 0 then layer 1 ... */
int ldc_slstm(ldc_ctx* ctx, const float* x, int B, int H, int T, const float* const* weights_host, int layers,
              float* y, void* stream);

/* introspection ------------------------------------------------------------------------------- */
/* Copy a named intermediate of the last ldc_unet_forward (channels-last -> [B,C,L] fp32).
 * Names: "cond_proc", "init", "down0".."downN", "mid", "up0".."upN".  For tests. */
int ldc_unet_debug_tap(ldc_ctx* ctx, const char* name, float* out, int64_t capacity_elems, void* stream);
/* Algorithmic work of one UNet step for (B, L): flops and bytes (activations + weights, compute dtype). */
int ldc_unet_step_cost(ldc_ctx* ctx, int B, int L, double* flops, double* bytes);
/* Timing of the dominant kernel class, measured with hipEvents on the launch stream when enabled.
 * ldc_profile_enable(ctx, 1) makes ldc_denoise bracket every conv-GEMM launch (eager, no graph). */
int ldc_profile_enable(ldc_ctx* ctx, int on);
/* Tuning aid: histogram of the XCC (die) ids `wgs` workgroups land on when launched on a stream created with the given CU mask
 * (n_words 32-bit words; NULL: unmasked). */
int ldc_xcc_census(ldc_ctx* ctx, const uint32_t* mask, int n_words, int wgs, int* hist16);

/* Test hook: one attention core (4 heads x 32) on caller data, in the context's UNet dtype.  qkv: [B, 384, L] fp32 on the device
 * (q | k | v, head-major), converted to channels-last rows as ldc_unet_forward converts its inputs; then exactly the launches a
 * plan makes.  kind 0: LinearAttention core with its own column-maximum pass; 1: the same with the maxima prepared in the
 * workspace as to_qkv's fused epilogue leaves them; 2: context + fused tail (to_out 1x1 conv, LayerNorm, + residual; bf16 contexts,
 * C in {256, 512, 1024}; w_out [C, 128], b_out [C], gain [C] in host memory, resid [B, C, L] fp32 on the device); 3: the
 * bottleneck's softmax attention core.  out: [B, 128, L] fp32 on the device ([B, C, L] for kind 2).  The arguments of kind 2 are
 * ignored otherwise.  Synchronous (waits for its stream); reports a device-side failure of its own launches. */
int ldc_debug_attn_core(ldc_ctx* ctx, int kind, const float* qkv, int B, int L, const float* w_out, const float* b_out,
                        const float* gain, const float* resid, int C, float* out, void* stream);
/* Test hook: Residual(PreNorm(LinearAttention)) of level "down<i>" / "up<i>", or Residual(PreNorm(Attention)) of "mid", of the
 * loaded UNet on x [B, C, L] fp32 (device) -> out [B, C, L].  The launches come from the plan builder itself, so every option
 * (fold_ctx, fuse_attn_tail, fuse_kmax, fold_ln, conv_lean) routes as in a decode.  Synchronous; honours the device-side failure
 * flag (LDC_E_HIP, "device-side failure [ctx_range]" when the context fold met k values outside its valid range). */
int ldc_debug_attention_block(ldc_ctx* ctx, const char* name, const float* x, int B, int L, float* out, void* stream);
/* Test hook: one ResnetBlock of the loaded UNet on caller data, launched by the plan builder itself, so every option (fuse_gn_epi,
 * fuse_gn_stats, fold_res, fold_ln, fuse_ln, conv_lean) routes as in a decode.  name: "down<i>.1", "down<i>.2", "mid.1", "mid.2",
 * "up<i>.1", "up<i>.2" or "final" (which runs with the output mode of a step: tanh included).  x1 [B, cin1, L] and, for the blocks that
 * read a concatenation (the up levels and "final"), x2 [B, cin2, L]: fp32 on the device; x2 is NULL otherwise (a mismatch is
 * LDC_E_INVALID).  t: the timestep, set as a step sets it (which also clears the GroupNorm sums, the split-K counters and the granule
 * regions of the fused exchange in front of the run).  lens (host, NULL: equal lengths) with shift: a ragged plan of B items whose
 * lengths are given in rows of level 0, this block sitting `shift` halvings below it (an item has lens[b] >> shift of the L rows); x1
 * and x2 are masked to zero behind each item's length first, the invariant a ragged plan gives its convs.  t_items (host, NULL; needs
 * lens): a per-item plan, one timestep per item, t is ignored.  with_attention (only "down<i>.2", "mid.1", "up<i>.2"): the block and the
 * attention block behind it are built as a step pairs them (the PreNorm folded into to_qkv on the block's row partials, or written by
 * the block's last kernel), and attn_out [B, cout, L] receives the attention block's output.
 * out [B, cout, L]; mid [B, cout, L]: block1's stored output (so fp8 contexts are refused: LDC_E_INVALID); stats float [2][B][groups][2]:
 * (sum, sum of squares) of conv 1 and conv 2 per (item, group) as the kernels themselves accumulated them -- the atomic /
 * launch_gn_stats buffers, or, for a conv with the fused GroupNorm epilogue, the tagged granules of its in-launch exchange read back
 * and summed on the host.  pre (device, NULL: not wanted) [2][B][cout][L] fp32: the outputs of conv 1 and conv 2 as stored, which is
 * what launch_gn_stats and gn_apply read on the unfused route (a conv with the fused epilogue stores none: zeros).  info (int[12], host): [0] [1] conv 1 / conv 2 took the fused epilogue, [2] res_conv folded into conv 1,
 * [3] fused (atomic) statistics rather than launch_gn_stats on the unfused path, [4] the PreNorm output (y_ln) was produced, [5] the
 * row partials for a folded PreNorm were produced, [6] [7] tile rows and wave rows of conv 1, [8] [9] of conv 2, [10] every granule the
 * exchange reads carried both tags, [11] a granule outside those was written.  Synchronous; honours the device-side failure flag
 * ("[gn_wait]").  Allocates and frees its workspace: not for the decode path.  out, mid and stats all NULL: planning only, on the
 * host -- info[0..9] of the run these arguments would make; nothing is launched and the tensors are not read. */
int ldc_debug_resnet_block(ldc_ctx* ctx, const char* name, const float* x1, const float* x2, int B, int L, int t, const int32_t* lens,
                           int shift, const int32_t* t_items, int with_attention, float* out, float* mid, float* stats, float* attn_out,
                           float* pre, int* info, void* stream);

/* Test hook: one SEANet conv on caller-supplied host weights (already weight-norm folded) through the conv path an encode / decode
 * takes (sea_conv: its ConvCall, its split-K workspace under option "sea_splitk").  Plain (transposed = 0; w [Cout, Cin, k], reflect padding
 * as SConv1d.forward) or transposed (w [Cin, Cout, k], k == 2*stride, as SConvTranspose1d.forward); pre_elu applies ELU to the input;
 * residual: NULL or [B, Cout, Lout] fp32 on the device, added in the epilogue (plain only).  Cin == 1 (plain) takes the encoder's first
 * layer's kernels on x [B, 1, L]: causal, stride 1, dilation 1, no ELU, no residual, L > k - 1 (LDC_E_INVALID otherwise).  x / y on the
 * device, [B, Cin, L] / [B, Cout, Lout].  route (int[8], host): [0] = 1 Cin = 1 rows kernel, 2 Cin = 1 generic kernel, 3 pipelined
 * conv kernel, 4 generic conv kernel; for 4, [1..7] = WM, WN, TM, TN of its tile configuration, split-K factor, taps per LDS group,
 * N tile.  Synchronous. */
int ldc_debug_sea_conv(ldc_ctx* ctx, const float* x, int B, int Cin, int L, const float* w_host, const float* b_host, int Cout, int k,
                       int stride, int dilation, int causal, int transposed, int pre_elu, const float* residual, float* y, int* route,
                       void* stream);
/* Test hook: op `index` of the encoder (decoder = 0) or decoder (1) of the loaded codec `which` (LDC_MODEL_MAIN / LDC_MODEL_COND) alone, on
 * x [B, C_in, L] fp32 (device) -> out [B, C_out, L_out].  info (int[4], host) = kind (0 Cin = 1 conv, 1 conv, 2 transposed conv,
 * 3 resblock, 4 LSTM), C_in, C_out, L_out; out == NULL: info only, nothing runs.  Synchronous. */
int ldc_debug_sea_op(ldc_ctx* ctx, int which, int decoder, int index, const float* x, int B, int L, float* out, int64_t capacity_elems,
                     int* info, void* stream);

/* Test hook: raises the context's device-side failure flag exactly as a kernel that gave up would (code 1: the
 * cooperative LSTM's hidden-state exchange, 2: the in-launch GroupNorm exchange of a fused conv, 4: the LinearAttention context
 * fold outside its valid k range).  The next call on the context reports LDC_E_HIP with "device-side failure [coop_lstm]" /
 * "[gn_wait]" / "[ctx_range]" in ldc_last_error and clears the flag. */
int ldc_debug_raise_failure(ldc_ctx* ctx, int code);
/* Test hook: number of device-wide synchronisations (hipDeviceSynchronize) this library has issued in this process.  Steady-state
 * stage calls issue none: the count does not move across warm ldc_decode calls. */
long long ldc_debug_sync_count(void);
/* Test hook: conv_lean_kernel launches of this process by unit kind (0 k = 3, 1 k = 1, 2 k = 1 with the folded LayerNorm, 3 k = 4 stride 2,
 * 4 k = 7; 5 = launches of any kind on the full three-stage ring, option "ring3_tiles"; 6 = k = 3 launches on the window ring -- three window
 * planes, two slab sets --, option "ring3_window"; a launch counts in 5 or in 6, never in both); -1 for an unknown kind.  A test that compares the lean kernel with conv_fast_kernel proves with it that the lean kernel ran. */
long long ldc_debug_lean_launches(int kind);

/* Host-side cost of the step-graph replays since the last reset: milliseconds spent inside hipGraphLaunch, milliseconds spent
 * waiting for the bounded look-ahead window (LDC_FLOW_DEPTH), number of replays. */
int ldc_host_stats(ldc_ctx* ctx, int reset, double* graph_launch_ms, double* lookahead_wait_ms, int64_t* graph_launches);
/* The graph-length rule of the sampler loops; host-only, needs no context or GPU (like ldc_ddim_times).  A loop of n_steps steps over
 * `parts` batch parts replays captured graphs of K steps and, for the remainder, of one step.  strided != 0: a DDIM / DPM loop.
 * graph_steps_option: the value of the "graph_steps" option (0: the default).
 *   want = option, if > 0; else 5 for a strided loop or several parts, 10 for one part of a DDPM loop.
 *   DDPM with option 0: among the lengths that divide n_steps -- 8..25 for one part, 3..7 for several -- the one nearest to want, the
 *   smaller of two equally near, replaces it.  K = want for a strided loop (every step count replays the same graphs), else
 *   min(want, max(1, n_steps - 1)).
 * n_big = n_steps / K replays of the K-step graph and n_single = n_steps - n_big K of the one-step graph: the counts of a loop whose
 * graphs exist (a loop that captures runs its first step eagerly and replays the counts of n_steps - 1, with the same K).  Each output
 * may be NULL.  Refused with LDC_E_INVALID: n_steps < 1, parts outside [1, 4], a negative option. */
int ldc_graph_schedule(int n_steps, int parts, int strided, int graph_steps_option, int* K_out, int* n_big_out, int* n_single_out);
/* Preconditions of the timed mode (round 6): what the part-stream calibration measured -- streams of the context that overlap with the
 * caller's stream and each other / candidates (good = -1: none has run), wall ms of one 150 us spin alone and of all accepted streams
 * spinning together, parts a batch is decoded as. */
int ldc_stream_info(ldc_ctx* ctx, int* good, int* candidates, double* one_spin_ms, double* all_spin_ms, int* parts);
/* One sample of the device clocks behind everything queued on `stream` (synchronises it): out2[0] = 100 MHz wall clock,
 * out2[1] = shader cycles (s_memtime).  Two samples around a region give the shader clock it ran at. */
int ldc_clock_sample(ldc_ctx* ctx, uint64_t* out2, void* stream);

/* Device-side timeline of the timed (graph-replayed, multi-stream) mode: every step of every batch part stamps a 100 MHz
 * clock at its first and last kernel.  ldc_timeline_read: ticks[2j], ticks[2j+1] = begin / end of step j of `part`. */
int ldc_timeline_enable(ldc_ctx* ctx, int on);
int ldc_timeline_read(ldc_ctx* ctx, int part, int n, uint64_t* ticks);
/* Per-kernel durations of the TIMED mode (hipGraph replay, batch parts on their own streams): with stamps enabled every launch of
 * the pipelined conv kernel records its earliest workgroup start and latest workgroup end (100 MHz clock) in a slot of its own per
 * denoise step.  enable / disable rebuilds the plans; reset re-arms the buffers; read returns plan `idx` (creation order = batch
 * part) as ticks[n_steps][n_ops][2] (0 where the op is not a pipelined conv) with the ops' descriptions and LDC_CLASS_* codes.
 * ticks == NULL: only *n_ops is returned. */
int ldc_kstamps_enable(ldc_ctx* ctx, int on);
int ldc_kstamps_reset(ldc_ctx* ctx);
int ldc_kstamps_read(ldc_ctx* ctx, int idx, int n_steps, int* n_ops, uint64_t* ticks, char* infos, int info_cap, int* classes);
/* Tuning aid: times the GroupNorm-apply kernel on [B,L,C] (random data, fixed statistics). */
int ldc_gn_microbench(ldc_ctx* ctx, int dtype, int B, int L, int C, int with_residual, int iters, double* ms_per_launch);
/* Tuning aid: times `iters` launches of one conv-GEMM (random weights/inputs) of the given shape with
 * hipEvents on the context's stream; dtype LDC_F32 | LDC_BF16; ups = 1 folds nearest x2 upsampling. */
int ldc_conv_microbench(ldc_ctx* ctx, int dtype, int B, int L, int cin1, int cin2, int cout, int k, int stride, int ups,
                        int iters, double* ms_per_launch);
/* Self-check: the same layer and pseudo-random operands through the pipelined conv-GEMM with tile shape `tile_cfg` forced
 * (-1: the launcher's choice) and through the generic kernel; largest output difference, largest |output|, largest relative
 * difference of the fused GroupNorm statistics / column maxima.  tile_cfg >= 100 (round 6): both passes on the pipelined path with tile
 * shape tile_cfg - 100 (199: the launcher's choice) -- conv_fast_kernel, then conv_lean_kernel (csrc/conv_lean.inc): the outputs must be bit-identical
 * (max_abs_diff == 0; pass with_gn = 0, the unfused statistics stay on conv_fast_kernel). */
int ldc_conv_compare(ldc_ctx* ctx, int dtype, int B, int L, int cin1, int cin2, int cout, int k, int stride, int ups, int tile_cfg,
                     int with_gn, int with_colmax, int with_residual, double* max_abs_diff, double* max_abs_ref, double* max_rel_stat);
/* Self-check of the LayerNorm folded into a 1x1 conv (the attention blocks' PreNorm in front of to_qkv) on rows x = dc + U(-1, 1):
 * against launch_ln_rows + a plain conv; max_abs_diff2[0]: the folded conv computing the row statistics itself, [1]: from per-row
 * (sum, centred M2) partials per 32-column block as the fused ResnetBlock conv in front leaves them. */
int ldc_ln_fold_compare(ldc_ctx* ctx, int dtype, int rows, int C, int n_out, double dc, double* max_abs_diff2, double* max_abs_ref);
/* Self-check of the fp8 x fp8 conv-GEMM (block-scaled fp8 MFMA): operands drawn on the e4m3 grid through that kernel and through
 * the bf16-activation x fp8-weight kernel, which then computes the same products exactly. */
int ldc_conv_compare_fp8(ldc_ctx* ctx, int B, int L, int cin1, int cin2, int cout, int k, int stride, int ups, int with_gn, int with_colmax,
                         double* max_abs_diff, double* max_abs_ref, double* max_rel_stat);
int ldc_profile_read(ldc_ctx* ctx, double* conv_ms_total, int64_t* conv_launches, double* conv_flops_total);
/* Per kernel class (LDC_CLASS_*) totals of the same profiling pass: event-timed milliseconds, launches, algorithmic
 * flops and algorithmic HBM bytes; arrays of n >= LDC_N_CLASSES entries (any may be NULL). */
enum {
  LDC_CLASS_OTHER = 0,       /* memsets, statistics fallbacks */
  LDC_CLASS_CONV = 1,        /* implicit-GEMM Conv1d (F.conv1d in unet.py) -- MFMA bound */
  LDC_CLASS_GN_APPLY = 2,    /* GroupNorm affine + scale/shift + SiLU (+ residual), unet.py:137-156 -- HBM bound */
  LDC_CLASS_LAYERNORM = 3,   /* channel LayerNorm (+ residual), unet.py:82-101 -- HBM bound */
  LDC_CLASS_LINATTN = 4,     /* LinearAttention core, unet.py:208-222 -- HBM bound */
  LDC_CLASS_ATTN_FULL = 5,   /* bottleneck Attention core, unet.py:234-246 -- latency bound */
  LDC_CLASS_ELEMENTWISE = 6, /* tanh before final_conv, unet.py:467 -- HBM bound */
  LDC_N_CLASSES = 7
};
int ldc_profile_read_classes(ldc_ctx* ctx, int n, double* ms, int64_t* launches, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* LADIFFCODEC_H_ */
