// Internal kernel-launcher interface of libladiffcodec (gfx950 / CDNA4 only).
//
// Internal activation layout is channels-last: a tensor of B items, L positions, C channels is a
// row-major matrix [B*L][C] in the context's compute dtype (float or bf16).  This makes every conv
// an "NT" GEMM whose two MFMA operands are both K(channel)-contiguous, turns channel concatenation
// into a second input pointer, channel LayerNorm / RVQ / LSTM inputs into row operations, and
// nearest-upsampling / striding / causal reflect padding into row-index arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ldc_windows.h"   // WinGroupRec, WinGroupTile: what the window-group kernels read, as the host builder writes it

namespace ldc {

enum { DT_F32 = 0, DT_BF16 = 1, DT_FP8 = 2 };   // DT_FP8: OCP e4m3 conv INPUTS of the fp8 x fp8 MFMA path (conv_fast_fp8.hip); outputs stay bf16
enum { ACT_NONE = 0, ACT_SILU = 1, ACT_ELU = 2, ACT_TANH = 3, ACT_GELU = 4, ACT_SIGMOID = 5, ACT_RELU = 6 };
enum { PAD_ZERO = 0, PAD_REFLECT = 1 };
// GroupNorm statistics accumulators: every (item, group) pair owns a 64-byte line ([0] = sum, [1] = sum of squares).  Packed
// ([B][groups][2] floats) the 4800 fp32 atomics of one conv launch landed on 8 cache lines and were serialised by the L2
// (~10 ns each: +7.7 us per launch, measured on the same conv with and without fused statistics).
static constexpr int kGnPad = 16;

inline size_t dt_size(int dt) { return dt == DT_F32 ? 4 : (dt == DT_FP8 ? 1 : 2); }

// ------------------------------------------------------------------------------------------------
// conv_gemm.hip : implicit-GEMM Conv1d / ConvTranspose1d on MFMA
// ------------------------------------------------------------------------------------------------
// GEMM view: rows m = (item b, output position l), columns n = output channel, K = taps x Cin.
// Input row gathered for (l, tap):  u = l*stride + tap*dil - pad_left ;  row = u >> ups
//   (ups=1 folds nn.Upsample(scale 2, nearest) into the index), zero or reflect outside [0, L_in<<ups).
// Transposed conv (kernel 2s, stride s) is the 2-tap conv over q in [0, L_in] with N = s*Cout
// (phase-major); the epilogue scatters (q, phase) to position q*s + phase - trim_left.
struct ConvLayer {
  int dt = DT_F32;
  int cin1 = 0, cin2 = 0;     // channels of the two (concatenated) inputs; cin2 = 0 for one input
  int n = 0;                  // GEMM N actually stored (Cout, or s*Cout for transposed)
  int n_pad = 0;              // N padded to the tile
  int bn = 128;               // N tile: 32 | 64 | 128
  int taps = 1, stride = 1, dil = 1, pad_left = 0, ups = 0, pad_mode = PAD_ZERO;
  int pre_act = ACT_NONE, post_act = ACT_NONE;
  int tr_stride = 0, tr_cout = 0, tr_trim_left = 0;   // transposed-conv scatter (tr_stride = 0: plain)
  void* w = nullptr;          // packed [chunk][tap][n_pad][64 B of K]  (w8: [chunk][tap][n_pad][32 B], 8-byte slots permuted)
  float* bias = nullptr;      // [n] fp32 or null
  int w8 = 0;                 // weights are OCP fp8 e4m3 (dt must be DT_BF16): value = fp8 * wscale[n]
  float* wscale = nullptr;    // [n] fp32 per-output-channel scale (w8)
  double flops_per_row = 0;   // 2*K*N, for accounting
  // ResnetBlock.res_conv folded into block1's conv (unet.py:171,189-192: both read the same input): the packed image holds
  // wtaps = taps + 1 slabs per channel chunk, the extra one being the 1x1 res_conv weight; the pipelined kernel multiplies it
  // with the centre-tap window it has in LDS anyway into a second accumulator set and writes ConvCall::y2 (+ bias2).
  // PreNorm LayerNorm folded into a 1x1 conv (Residual(PreNorm(attention)).to_qkv, unet.py:82-101,208-246): the weight is packed
  // as W diag(g) and  conv(LN(x))[r][n] = rstd_r * (acc[r][n] - mean_r * ln_s[n]),  ln_s[n] = sum_c (W diag(g))[n][c] of the ROUNDED
  // packed weight; the pipelined kernel computes (mean_r, rstd_r) of its rows in its prologue and applies the identity to the
  // accumulators (one launch and one write + read of the normalised tensor less)
  float* ln_s = nullptr;
  int wtaps = 0;              // 0: no folded second conv
  float* bias2 = nullptr;     // [n] bias of the folded 1x1 conv
};

// tuning knobs of the conv launchers; owned by the context (read from the environment once at ldc_create)
struct ConvTune {
  int force_generic = 0;        // LDC_CONV_V1: every conv on the generic kernel
  int small_max = 100;          // LDC_CONV_SMALL_TILES: 64x64 tiles up to this many 128x128-equivalents (60 through round 5; with the lean kernel 80-150 measure 0.8-1.2 % faster per decode, 200+ slower: tools/sweep_knobs_r06b.sh)
  int splitk = 1;               // LDC_CONV_SPLITK: 0 off | 1 by layer | 2 | 3
  int sk_tiles = 200, sk_u2 = 24, sk_u3 = 60;   // LDC_SK_TILES / LDC_SK_U2 / LDC_SK_U3
  int m_fastest = 1;            // LDC_CONV_MFAST: 0 N-tile fastest | 1 by operand size | 2 M-tile fastest
  int debug = 0;                // LDC_CONV_DEBUG (bits, see conv_fast.inc)
  int gn_nap = 16, gn_nap0 = 0;  // LDC_GN_NAP / LDC_GN_NAP0: 64-clock naps between the polls of the fused GroupNorm exchange / before the first
  int force_tile = -1;          // self-check / tuning: 0 = 64x64, 1 = 128x64 tiles wherever the layer's N allows
  int xcd_order = 1;            // round 6: lean kernel's dispatch order as an xm x xn arrangement of the XCDs chosen by operand bytes (conv_lean.inc: lean_xcd_order); 0 = conv_fast_body's order; 2 / 4 / 8 = xn forced
  int lean = 1;                 // round 6: the instruction-diet kernel (conv_lean.inc) where its shapes allow; 0 = conv_fast_kernel everywhere (LDC_CONV_LEAN)
  int ring3_tiles = 304;        // round 9: conv_lean_kernel's three-stage ring (two units in flight, counted copy waits) for k = 3 / 1x1 launches of at most this many workgroups, split-K slices included; 0 = never (profiles/r09_ring3.md)
  int ring3_wgs = 3;            // ... and only where this many three-stage workgroups still fit a CU's 160 KB of LDS (3: the 64-row tiles; 2: the 128-row tiles too; 1: every tile)
  int ring3_window = 1;         // round 10: where ring3_wgs full rings do not fit a CU but as many window rings do (three window planes, two slab sets, 51.2 KB: conv_lean.inc, LEAN_RING_W) -- the k = 3 128-row tile without the folded second conv -- the window ring; 0 = two stages there (A/B) (profiles/r10_ring_window.md)
  int ring3_window_tiles = 608; // ... for launches of at most this many workgroups, split-K slices included (the window ring costs no co-resident workgroup: the 600-tile launches take it too)
  int ring3_cu_share = 102;    // (not an option: the CUs a batch part's fused GroupNorm launch can count on, set by the planner next to its own residency rule -- unet_plan.cpp: few_tiles)
  int lean_all = 1;             // round 7: also the stride-2 downsamples (k = 4) and init_conv (k = 7) of the bf16 engine on it; 0 = conv_fast_kernel for those (A/B)
};

struct ConvCall {
  const void* x1 = nullptr;
  const void* x2 = nullptr;
  void* y = nullptr;
  void* y2 = nullptr;              // output of the folded 1x1 conv (ConvLayer::wtaps), [rows][n]
  const void* residual = nullptr;  // [rows][n], same dtype, added before post_act (plain conv only)
  int B = 0;
  int L_in = 0;               // positions per item of the input
  int L_rows = 0;             // GEMM rows per item (output positions; L_in+1 for transposed)
  int L_final = 0;            // transposed: final positions per item after trimming
  int y_ld = 0;               // channels per output row
  float* gn_sum = nullptr;    // optional fused GroupNorm statistics: [B][groups][2] (sum, sumsq), pre-zeroed
  int gn_groups = 0;
  unsigned* colmax = nullptr; // optional fused per-item column max, columns [colmax_lo, colmax_hi), pre-zeroed keys
  int colmax_lo = 0, colmax_hi = 0, colmax_stride = 0;
  // LinearAttention context inside to_qkv (round 6, lean kernel, bf16): the layer's output columns are ordered q | (k_h v_h) x heads, the
  // q tiles are stored, a (k_h | v_h) tile accumulates exp(k)^T v and the column sums of exp(k) into the item's workspace
  // (qkv_ctx_ws + item * qkv_ctx_stride floats: kmax keys [HD] (unused) | ksum [HD] | ctx [H][D][D], zeroed every step) and stores nothing.
  // The exponentials are NOT shifted by a column maximum: valid while every column's sum of exp(k) is in [kLinattnKsumMin, kLinattnKsumMax)
  // = [2^-100, 1e26), hence every k < 60; outside that range the tail that consumes the workspace raises the context's failure word to
  // kDevFailCtxRange ("[ctx_range]", fallback fold_ctx 0), never a silently wrong result (see kLinattnKClamp below)
  float* qkv_ctx_ws = nullptr;
  int qkv_ctx_stride = 0;
  float* sk_part = nullptr;   // optional split-K workspace (fp32 partial tiles) and arrival counters (pre-zeroed)
  unsigned* sk_count = nullptr;
  long long sk_part_cap = 0;  // floats
  int sk_count_cap = 0;       // tiles
  int generic_split = 0;      // the generic kernel may split K through sk_part (conv_generic_splitk_floats floats; no counters: a reduce launch follows)
  // Fused GroupNorm apply in the conv epilogue (pipelined kernel only; needs gn_sum): y = SiLU(GN(conv) * (scale + 1) + shift)
  // (+ residual) (tanh).  gn_part: [B][gn_mslots][WM][n / 32] 16-byte granule pairs the waves exchange their partial statistics
  // through, zeroed before every launch (the step's first kernel does it); see ConvKArgs / epilogue_gn_fused in conv_device.h.
  void* gn_part = nullptr;
  int gn_mslots = 0;                // M-tile slots per item (>= (L_rows + BM - 1) / BM + 1 for the tile height the dry run reports)
  const float* gn_gamma = nullptr;
  const float* gn_beta = nullptr;
  const float* gn_ss = nullptr;     // [2 n] scale | shift of the current timestep, or null
  int gn_out = 0;                   // bit 2: tanh after the residual add
  unsigned* fail_flag = nullptr;    // host-mapped word raised when the bounded in-launch wait gives up (2); the LinearAttention tail raises it to 4 when the context fold left its valid range
  float* rowstat_out = nullptr;        // fused apply with residual: per-row (sum, sumsq) partials of the output per 32-column block, [rows][n / 32][2]
  const float* ln_rowstat = nullptr;   // LayerNorm-folded conv (ConvLayer::ln_s): those partials of its input, or null (it reads its rows once more)
  unsigned long long* kst = nullptr;   // timed-mode stamps of this launch (ConvKArgs::kst), pipelined kernel only
  const int* kst_step = nullptr;
  int kst_stride = 0;
  // Stream sessions (generic kernel, one input, SEANet layers): the launch reads a virtual input of L_in rows per item whose first
  // ctx_rows rows are the item's context and whose remaining L_in - ctx_rows rows are x1 (the chunk, [B][L_in - ctx_rows][cin1]).  The layer
  // passed with such a call pads nothing itself (pad_left 0).  ctx_fresh[b] != 0: the item starts a sequence and its context is the
  // reflected start of the chunk, as the whole-sequence call pads (ctx_zero: zero rows -- a transposed conv sees no previous row)
  const void* ctx = nullptr;        // [B][ctx_rows][cin1]
  const int* ctx_fresh = nullptr;   // [B], device
  int ctx_rows = 0, ctx_zero = 0;
  int check_only = 0;               // with ctx: no launch -- hipErrorOutOfMemory when the launch's LDS window would not fit, else hipSuccess
  const ConvTune* tune = nullptr;   // null: defaults
  long long* sk_need = nullptr;     // dry run: no launch, *sk_need = split-K workspace floats this call would use
  int* route_out = nullptr;         // test hook: int[8] = route (CONV_ROUTE_*), then for the generic kernel WM, WN, TM, TN, split-K factor, taps per LDS group tg, N tile
  int* bm_out = nullptr;            // dry run (with sk_need): int[4] = rows per tile of the pipelined kernel (0 when the generic kernel would run), wave rows WM, split-K factor, columns per tile
};

// which kernel a conv call ran on (ConvCall::route_out[0] / launch_conv_cin1's route_out)
enum { CONV_ROUTE_NONE = 0, CONV_ROUTE_CIN1_ROWS = 1, CONV_ROUTE_CIN1_GENERIC = 2, CONV_ROUTE_PIPELINED = 3, CONV_ROUTE_GENERIC = 4 };
hipError_t launch_conv(const ConvLayer& ly, const ConvCall& c, hipStream_t s);
long long conv_generic_splitk_floats(const ConvLayer& ly, const ConvCall& c);   // workspace floats a generic_split call of this shape uses (0: it would not split)
size_t conv_packed_weight_bytes(const ConvLayer& ly);
// host-side packers (fp32 [Cout][Cin][k] or, transposed, [Cin][Cout][k]) -> packed image in ly.dt
void pack_conv_weights(const ConvLayer& ly, const float* w_oik, void* dst_host);
// w8: also fills scales[n] (max |w| of the output channel / 448)
void pack_conv_weights_fp8(const ConvLayer& ly, const float* w_oik, void* dst_host, float* scales);
// ly.dt == DT_FP8 (fp8 inputs): [chunk of 64][tap][n_pad][64 B], fills scales[n]
void pack_conv_weights_fp8act(const ConvLayer& ly, const float* w_oik, void* dst_host, float* scales);
// OCP e4m3fn, round to nearest even, saturating at +-448 (host)
uint8_t host_f32_to_e4m3(float f);
float host_e4m3_to_f32(uint8_t v);
void pack_convtr_weights(const ConvLayer& ly, const float* w_iok, int cin, int cout, int stride, void* dst_host);
int conv_pick_bn(int n);

// ------------------------------------------------------------------------------------------------
// norm_act.hip
// ------------------------------------------------------------------------------------------------
// GroupNorm statistics of x [B][L][C]: stats[b][g] = (sum, sumsq) accumulated with fp32 atomics into a
// pre-zeroed buffer.
// Ragged batches (every launcher below that takes `lens`): a device array of B lengths in rows of level 0; an item's valid rows at this
// tensor's level are lens[b] >> shift, the rows behind them are padding -- left out of every reduction, written as exact zeros, always
// by a select (a NaN in a padding row never reaches a valid one).  lens == null: every row is valid (the equal-length plans).
hipError_t launch_gn_stats(int dt, const void* x, int B, int L, int C, int groups, float* stats, hipStream_t s, const int* lens = nullptr,
                           int shift = 0);
// y = act( GN(x)*(scale+1)+shift ) (+ residual).  scale_shift: fp32 [2*C] (scale then shift) selected
// by *t_ptr from a table with row stride ss_stride, or null.  eps 1e-5.
// out8 bit 0: y is written as OCP fp8 e4m3 ([rows][C] bytes, saturating) instead of dt; bit 1: the same for y_ln; bit 2: y = tanh(y)
// after the residual add (the final ResnetBlock, whose output feeds torch.tanh alone).  (The fp8 x fp8
// conv path: a tensor whose only consumer is a conv is produced in the conv's input type.)
hipError_t launch_gn_apply(int dt, const void* x, void* y, const void* residual, int B, int L, int C, int groups,
                           const float* stats, const float* gamma, const float* beta, const float* ss_table,
                           int ss_stride, const int* t_ptr, int act, hipStream_t s, void* y_ln = nullptr, const float* ln_g = nullptr, int out8 = 0,
                           const int* lens = nullptr, int shift = 0,
                           int t_stride = 0, int t_rows = 0);   // per-item plan: item b's timestep is t_ptr[b * t_stride], clamped to the table's t_rows rows (t_stride 0: one timestep for the launch)
// y_ln != null: also write channel-LayerNorm(y) * ln_g (needs gn_apply_ln_fusable(C) and ACT_SILU)
bool gn_apply_ln_fusable(int C);
// channel LayerNorm (gain only, biased var, eps 1e-5) per row; y = LN(x)*g (+ residual)
hipError_t launch_ln_rows(int dt, const void* x, void* y, const void* residual, const float* g, int rows, int C,
                          hipStream_t s, int out8 = 0, const int* lens = nullptr, int shift = 0, int L = 0);   // lens: rows = B * L
// x [B][L][C]: rows l >= lens[b] >> shift of every item are written as zero (stores only: the padding is never read)
hipError_t launch_mask_rows(int dt, void* x, int B, int L, int C, const int* lens, int shift, hipStream_t s);
// elementwise tanh in place / out of place
hipError_t launch_act(int dt, const void* x, void* y, int64_t n, int act, hipStream_t s, int out8 = 0);

// ------------------------------------------------------------------------------------------------
// attention.hip   (heads x dim_head = 4 x 32 fixed by the reference, unet.py:195,225)
// ------------------------------------------------------------------------------------------------
// qkv [B*L][3*H*D] (q | k | v, head-major).  ctx_ws: fp32 [B][H][D][D].
hipError_t launch_linattn(int dt, const void* qkv, void* out, float* ctx_ws, int B, int L, int heads, int dim_head,
                          bool kmax_fused, hipStream_t s, const int* lens = nullptr, int shift = 0, bool ws_zeroed = false);
// lens: needs !kmax_fused (its own column-max pass).  ws_zeroed: the caller cleared `ws` (no memset here: the column-max pass still runs)
size_t linattn_ws_floats_per_item(int heads, int dim_head);
// LinearAttention in three launches (bf16 engine): qkv conv (+ k column max) -> context -> tail (out + to_out conv + LayerNorm + residual)
bool linattn_tail_supported(int dt, int heads, int dim_head, int C);
hipError_t launch_linattn_ctx(int dt, const void* qkv, float* ctx_ws, int B, int L, int heads, int dim_head, hipStream_t s);
hipError_t launch_linattn_tail(int dt, const void* qkv, const float* ctx_ws, const void* wo_packed, int n_pad, const float* bias, const float* gain,
                               const void* resid, void* out, int B, int L, int heads, int dim_head, int C, unsigned* fail_flag, hipStream_t s);
hipError_t launch_linattn_kmax(int dt, const void* qkv, float* ctx_ws, int B, int L, int heads, int dim_head, hipStream_t s,
                               const int* lens = nullptr, int shift = 0);
// The context fold (ConvCall::qkv_ctx_ws) takes exp(min(k, kLinattnKClamp)) without a shift.  It agrees with the shifted kernels while
// every column's sum of exp(k) lies in [kLinattnKsumMin, kLinattnKsumMax): above the floor every term within 2^-24 of the column's largest
// is a normal number in fp32 and bf16 (a column maximum above about -69 - ln L); below the ceiling no entry was clamped (one clamped entry
// contributes e^60 = 1.14e26, 1.137e26 after its rounding to bf16) and 1 200 positions cannot overflow.  The tail tests the sum it divides by
// and raises the context's failure word to kDevFailCtxRange outside that range (also for Inf / NaN): the call fails with "device-side
// failure [ctx_range]" and option fold_ctx 0 -- column max, then shifted exponentials -- is the fallback.
constexpr float kLinattnKClamp = 60.0f;
constexpr float kLinattnKsumMin = 7.888609052210118e-31f;   // 2^-100
constexpr float kLinattnKsumMax = 1.0e26f;
constexpr unsigned kDevFailCtxRange = 4u;   // (3 is LDC_DEV_BAD_CODE)
hipError_t launch_attn_full(int dt, const void* qkv, void* out, int B, int L, int heads, int dim_head, hipStream_t s, const int* lens = nullptr,
                            int shift = 0);

// ------------------------------------------------------------------------------------------------
// diffusion.hip
// ------------------------------------------------------------------------------------------------
// [B][C][L] fp32 -> [B][L][C] dt  (optionally multiplied by 1/(maxabs[b or 0] + eps))
hipError_t launch_to_cl(int dt, const float* x_bcl, void* y_blc, int B, int C, int L, const float* maxabs,
                        int maxabs_per_item, float eps, hipStream_t s);
// [B][L][C] dt -> [B][C][L] fp32 (same optional scaling)
hipError_t launch_from_cl(int dt, const void* x_blc, float* y_bcl, int B, int C, int L, const float* maxabs,
                          int maxabs_per_item, float eps, hipStream_t s);
// maxabs[b] (or maxabs[0] when !per_item) = max |x| ; buffer must be pre-zeroed.  Works on raw element
// streams: n_per_item elements per item.
hipError_t launch_maxabs(int dt, const void* x, int B, int64_t n_per_item, int per_item, float* maxabs,
                         hipStream_t s);
// Step state on the device: st[0] = current t, st[1] = iteration index j, st[2..3] = the 64-bit Philox key of the
// current sampler call (seed mixed with the context's call counter on the host, written by launch_step_set: a
// captured step graph therefore draws fresh noise on every replayed call).
struct StepTables {            // device pointers, fp32 [T]
  const float* sqrt_recip_alphas_cumprod;
  const float* sqrt_recipm1_alphas_cumprod;
  const float* posterior_mean_coef1;
  const float* posterior_mean_coef2;
  const float* posterior_log_variance_clipped;
};
// x [B][C][L] fp32 in place; eps_cl [B][L][C] dt; noise [.. j ..][B][C][L] fp32 or null (Philox);
// also writes x_cl [B][L][C] dt (the next step's UNet input).  Reads t, j from st.
hipError_t launch_random_fill(float* x, int64_t n, int uniform, uint64_t seed, unsigned step, hipStream_t s);
hipError_t launch_axpby(float* x, const float* y, float a, float b, int64_t n, hipStream_t s);
hipError_t launch_p_sample_update(int dt, float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride,
                                  void* x_cl, int B, int C, int L, StepTables tb, const int* st,
                                  uint64_t elem_base, hipStream_t s, const int* lens = nullptr,   // lens [B] (positions): x and x_cl stay zero behind them
                                  const uint64_t* item_keys = nullptr);
// item_keys [B] (device; launch_p_sample_update and launch_ddim_update): the item-seeded form ("Item seeds") -- item b
// draws under key item_keys[b] at the block index of the item alone, c_first * len_b + l (len_b = lens[b], L without lens): exactly
// launch_p_sample_update_items' draw; elem_base and the step state's key are not read.  Written by launch_item_keys_write, stream-ordered
// (the keys travel as kernel arguments).
hipError_t launch_item_keys_write(uint64_t* dst, const uint64_t* keys_host, int n, hipStream_t s);
// Per-item step state (per-item plans: ldc_unet_forward_items, decode pools): one record per item / pool slot in
// device memory.  Nothing about an item's progress or its sampler is a kernel argument, so one captured step graph replays for any mix
// of states, DDPM, DDIM and DPM-Solver++ items side by side.
union SchedEntry;
enum { ITEM_DDPM = 0, ITEM_DDIM = 1, ITEM_DPM = 2 };   // ItemState::kind (zero: what every record without a schedule is)
struct ItemState {
  int t;                // timestep of the step being executed (unet.py:422-437: one per item)
  int j;                // iteration: which entry of the noise tape / Philox step the update uses
  unsigned key_lo, key_hi;   // Philox key of the item
  int remaining;        // steps not yet begun (0 = idle: finished, evicted or never admitted)
  int len;              // the item's own latent frames (the ragged plan's lens[] holds the same value)
  int active;           // set by the step's first kernel: this step runs for the item (an idle item is computed on and discarded)
  int kind;             // the item's sampler: ITEM_DDPM, ITEM_DDIM or ITEM_DPM; a record with sched == null is DDPM whatever this says
  const float* noise;   // the item's tape [n_steps][C][len] (contiguous for its OWN length) or null: Philox draws; never read for a DPM item
  const SchedEntry* sched;   // the item's schedule, entry j for iteration j (the pool's arena row of its slot), or null: DDPM p_sample
};
constexpr int kItemStateInts = (int)(sizeof(ItemState) / sizeof(int));
static_assert(sizeof(ItemState) == 48, "the record's size is part of the per-item plans (gn_apply's t_stride): the sampler kind took the pad word");
// dst[0..n) = src_host[0..n), stream-ordered (kernel arguments carry the records); lens / flens (optional): lens[i] = len, flens[i] = len / up
hipError_t launch_items_write(ItemState* dst, const ItemState* src_host, int n, int* lens, int* flens, int up, hipStream_t s);
// First kernel of a step of a per-item plan: for every item, active = remaining > 0 and, with `advance`, a running item moves on
// (j + 1, remaining - 1; t - 1 for a DDPM item, t = sched[j].t for an item with a schedule, of either kind); counts the part's epoch word st[4] up once;
// clears the step's accumulator region as launch_step_begin does.
// The timestep's (scale | shift) row is NOT copied: gn_apply selects it from the table by the item's t (launch_gn_apply, t_stride).
hipError_t launch_step_begin_items(ItemState* items, int B, int* st, void* zero, size_t zero_bytes, int advance, hipStream_t s);
// launch_p_sample_update per item: coefficients from the item's t, noise = tape[j] of the item's own tape or a Philox draw with the item's
// key, step j and group index c * len + l (what the item draws alone at B = 1); no noise at t == 0.  x: item b at x + b * x_item_stride,
// [C][len] fp32; eps_cl / x_cl [B][Lmax][C].  An item with active == 0 is not stored (neither x nor x_cl) and neither its tape nor its
// schedule is dereferenced; rows >= len are never touched (x_cl stays zero there from the admission).  T = timesteps (t is clamped to the
// tables).  An item with a schedule (ItemState::sched) takes launch_ddim_update's arithmetic instead, in the same launch (the branch is
// uniform over a workgroup): coefficients of sched[j], noise read or drawn only where !last && sigma > 0, same tape layout and Philox group.
// An item of kind ITEM_DPM takes launch_dpm_update's: coefficients of sched[j].dpm, nothing drawn, neither the tape pointer nor the key
// read.  x0_prev: the items' x0 history, laid out exactly like x (item b's [C][len] block at x0_prev + b * x_item_stride), loaded only
// where the advanced record says j >= 1 && remaining > 0 (what the table's has_prev && !last say), written on every iteration but the
// last, never cleared; rows >= len and idle items never touch it.  Null where no DPM item can exist: a DPM record is then not stored.
hipError_t launch_p_sample_update_items(int dt, float* x, int64_t x_item_stride, const void* eps_cl, void* x_cl, int B, int C, int Lmax,
                                        StepTables tb, const ItemState* items, int T, float* x0_prev, hipStream_t s);
// One iteration of DDIM sampling (reference ddpm_loss.py ddim_sample, clip_denoised): the host fills one entry per
// iteration j (ldc_api.cpp: ddim_schedule) into a device table that the step state indexes.
struct DdimStep {
  int t;           // UNet timestep of iteration j
  int last;        // time_next < 0: x <- x0
  float sqrt_an;   // sqrt(alphas_cumprod[time_next])
  float c;         // sqrt(1 - alpha_next - sigma^2)
  float sigma;     // eta * sqrt((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)); noise is drawn only when > 0
  float pad_[3];
};
// x0 = clamp(sqrt_recip_ac[t] x - sqrt_recipm1_ac[t] eps, -1, 1); x <- last ? x0 : x0 sqrt_an + c eps + sigma z.
// Same layouts as launch_p_sample_update; t, coefficients and the draw of iteration j = st[1] from sched[j]
// (noise tape entry j, or Philox (key, j, global element)).
hipError_t launch_ddim_table_write(DdimStep* dst, const DdimStep* src_host, int n, hipStream_t s);   // dst[0..n) = src_host[0..n), stream-ordered
hipError_t launch_ddim_update(int dt, float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride,
                              void* x_cl, int B, int C, int L, StepTables tb, const DdimStep* sched, const int* st,
                              uint64_t elem_base, hipStream_t s, const int* lens = nullptr, const uint64_t* item_keys = nullptr);
// One iteration of DPM-Solver++(2M) in its data-prediction form: the host fills one entry per iteration j
// (ldc_api.cpp: ldc_dpm_schedule, double arithmetic rounded once to float) into a device table that the step state indexes.
struct DpmStep {
  int t;           // UNet timestep of iteration j
  int last;        // time_next < 0: x <- x0
  int has_prev;    // j >= 1: the update reads x0 of iteration j - 1; 0: the history is NOT loaded (it may hold anything)
  float a;         // sigma_next / sigma_t
  float b0;        // phi (1 + 1 / (2 r)); phi on the first iteration
  float b1;        // -phi / (2 r); 0 on the first iteration
  float pad_[2];
};
// One entry of an item's schedule (a decode pool's arena, ItemState::sched): a DdimStep for an ITEM_DDIM record, a DpmStep for an
// ITEM_DPM one.  Both are 32 bytes with `t` as their first word, so step_begin_items_kernel advances t = sched[j + 1].t without knowing
// the kind; the update kernel reads the member the record's kind names.
union SchedEntry {
  int t;
  DdimStep ddim;
  DpmStep dpm;
};
static_assert(sizeof(DdimStep) == 32 && sizeof(DpmStep) == 32 && sizeof(SchedEntry) == 32, "schedule entries of every kind share one arena row");
static_assert(offsetof(DdimStep, t) == 0 && offsetof(DpmStep, t) == 0, "t is the first word of a schedule entry of every kind");
// x0 = clamp(sqrt_recip_ac[t] x - sqrt_recipm1_ac[t] eps, -1, 1); x <- last ? x0 : a x + b0 x0 + (has_prev ? b1 x0_prev : 0), in fp32;
// then x0_prev <- x0 on every iteration but the last.  Same layouts and `lens` rule as launch_ddim_update (x, x_cl and x0_prev are
// zero behind an item's length); x0_prev [B][C][L] fp32, the layout of x.  No noise: nothing is drawn.
hipError_t launch_dpm_table_write(DpmStep* dst, const DpmStep* src_host, int n, hipStream_t s);   // dst[0..n) = src_host[0..n), stream-ordered
hipError_t launch_dpm_update(int dt, float* x, const void* eps_cl, float* x0_prev, void* x_cl, int B, int C, int L, StepTables tb,
                             const DpmStep* sched, const int* st, hipStream_t s, const int* lens = nullptr);
// Coupled windows: the host-built tables of R recordings whose windows share one batch (ldc_windows.h:
// win_group_build; a single-recording call is R = 1), in device memory.
struct WinGroupTables {
  const WinGroupTile* tile;   // [n_tiles] {recording, l0}: one entry per workgroup column of the update launch
  const WinGroupRec* rec;     // [R] {Ltot_r, w0_r, off_r, cover_off_r, Philox key}
  const int* cover;           // [Lsum] the recordings' cover rows, concatenated; first window counted WITHIN the recording | count << 8
  const float* weight;        // [W_sum][Lw]: the weights of the windows that cover a frame sum to 1, a lone window has 1.0f
  const int* start;           // [W_sum] first frame of each window in its recording's own frames
  const int* wrec;            // [W_sum] window -> recording
  int n_tiles, R, Lw;
};
enum { WIN_BLEND = 0, WIN_DDPM = 1, WIN_DDIM = 2, WIN_DPM = 3 };   // WIN_DPM: launch_windows_group_dpm_update
// The update launch of a coupled-windows step: blends eps_cl [W_sum][Lw][C] dt into the eps of each recording's global frames, applies
// p_sample (WIN_DDPM) or the DDIM entry sched[st[1]] (WIN_DDIM) to the recording's state exactly as the B = 1, L = Ltot_r kernels above
// and stores the new state into every covering window's row of x_cl [W_sum][Lw][C] dt.  x, ebar, x0_prev and every step of the tape are
// packed, recording r's [C][Ltot_r] block at C * off_r floats (noise_step_stride = C * Lsum; noise null: Philox at elem_base 0 under
// the recording table's key).  WIN_BLEND: the blended eps into ebar, nothing else is read or written.  Grid (n_tiles, ceil(C / 32)).
// WIN_DPM is a kernel of its own (it takes the history and a DpmStep table): the same blend, then the update of launch_dpm_update with
// ONE history block per recording (loaded only where sched[st[1]] says has_prev, written on every iteration but the last, never
// cleared).  Nothing is drawn.
hipError_t launch_windows_group_update(int dt, int kind, float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride, void* x_cl,
                                       float* ebar, int C, WinGroupTables gt, StepTables tb, const DdimStep* sched, const int* st, hipStream_t s);
hipError_t launch_windows_group_dpm_update(int dt, float* x, const void* eps_cl, float* x0_prev, void* x_cl, int C, WinGroupTables gt, StepTables tb,
                                           const DpmStep* sched, const int* st, hipStream_t s);
// y [W_sum][Lw][C] dt <- the windows' slices of a packed fp32 sequence whose blocks are [C][Ltot_r / div] at C * off_r / div floats
// (Lw: the frames of a window of this sequence)
hipError_t launch_windows_group_gather(int dt, const float* x, void* y, int W, int C, int Lw, WinGroupTables gt, int div, hipStream_t s);
// rec[r].key = keys_host[r] (null: 0), stream-ordered; the keys travel as kernel arguments
hipError_t launch_windows_group_keys(WinGroupRec* rec, const uint64_t* keys_host, int R, hipStream_t s);
// x /= (maxabs[b or 0] + eps) in place on a raw element stream (n_per_item elements per item)
hipError_t launch_scale_by_maxabs(int dt, void* x, int B, int64_t n_per_item, const float* maxabs, int per_item,
                                  float eps, hipStream_t s);
// torchaudio-style polyphase sinc resampling; bank [nnew][2*width+orig] fp32 (device)
hipError_t launch_resample(const float* wav, int C, int64_t T, const float* bank, int orig, int nnew, int width, int64_t target, float* out,
                           hipStream_t s);
hipError_t launch_scale_copy(int dt, const void* x, void* y, int B, int64_t n_per_item, const float* maxabs, float eps,
                             hipStream_t s);
hipError_t launch_step_advance(int* st, unsigned long long* tl, hipStream_t s);      // t -= 1, j += 1 (tl: timeline slot or null); behind the LAST step of a loop only (launch_step_begin advances)
// cur[0..stride) = table[st[0]][0..stride): the current timestep's scale/shift row, so that consumers need no
// dependent load through the step counter
// also zeroes [zero, zero + zero_bytes) (rounded up to 16 bytes: the caller pads the region): the step's accumulators
// advance = 1: first move the step state on from the previous step (t - 1, iteration + 1), i.e. a loop starts from (t + 1, -1)
// ddim (DDIM loops, else null): then t = ddim[j].t, the timestep of iteration j of the strided schedule
hipError_t launch_step_begin(const float* table, int stride, int* st, float* cur, unsigned long long* tl, hipStream_t s,
                             void* zero = nullptr, size_t zero_bytes = 0, int advance = 0, const DdimStep* ddim = nullptr);
// the same kernel for any schedule table: t = t_words[j * t_stride_ints], the `t` word of entry j of a table whose entries are
// t_stride_ints ints apart (DdimStep, DpmStep); t_words null: no table (DDPM)
hipError_t launch_step_begin_sched(const float* table, int stride, int* st, float* cur, unsigned long long* tl, hipStream_t s, void* zero,
                                   size_t zero_bytes, int advance, const int* t_words, int t_stride_ints);
hipError_t launch_step_set(int* st, int t, int j, uint64_t noise_key, hipStream_t s);
hipError_t launch_clock_sample(unsigned long long* out2, hipStream_t s);   // out2[0] = 100 MHz wall clock, out2[1] = s_memtime (shader cycles)
hipError_t launch_spin_us(unsigned us, hipStream_t s);   // one workgroup busy for `us` microseconds (stream-overlap calibration)
// output normalisation (sample.py:133-134); ws: double [B][2] + float [B] zeroed by the launcher
// lens (needs per_item): item b has lens[b] * lens_unit samples; statistics over those, the tail is written as zero
hipError_t launch_output_normalise(float* x, int B, int64_t n_per_item, int per_item, void* ws, hipStream_t s, const int* lens = nullptr,
                                   int lens_unit = 1);
// dst[0..n) = src_host[0..n), stream-ordered (the values travel as kernel arguments: no host buffer outlives the call)
hipError_t launch_lens_write(int* dst, const int* src_host, int n, hipStream_t s);
// RVQ codes [n_q][B][F] int64 of a ragged batch: frames f >= flens[b] are written as 0
hipError_t launch_mask_codes(int64_t* codes, int n_q, int B, int F, const int* flens, hipStream_t s);
size_t output_normalise_ws_bytes(int B);

// ------------------------------------------------------------------------------------------------
// seanet.hip
// ------------------------------------------------------------------------------------------------
// First SEANet conv: Cin = 1, causal reflect pad.  x [B][L] fp32 -> y [B][L][Cout] dt.  w [Cout][k] fp32.
hipError_t launch_conv_cin1(int dt, const float* x, void* y, const float* w, const float* bias, int B, int L, int Cout,
                            int k, hipStream_t s, int* route_out = nullptr,   // route_out (test hook): *route_out = CONV_ROUTE_CIN1_*
                            const float* ctx = nullptr, const int* fresh = nullptr);   // stream sessions: ctx [B][k - 1] samples before the chunk, used where !fresh[b]
// Stream sessions: the context of the NEXT chunk, nxt[b] = the last P rows of (cur[b] | x[b]) for an item with history, of (left padding |
// x[b]) for a fresh one (zero_pad: zeros, else the reflected start of x).  x [B][L][C] fp32, cur / nxt [B][P][C]; nxt must not alias cur
hipError_t launch_stream_ctx_update(const float* x, const float* cur, float* nxt, const int* fresh, int B, int L, int P, int C, int zero_pad,
                                    hipStream_t s);
// LSTM recurrence over T for one layer.  pre [B][T][4H] dt_pre (input GEMM + both biases), w_hh [4H][H]
// fp32, out [B][T][H]; if skip != null: out = h + skip (SLSTM skip, lstm.py:25-26).
// a stretch of time steps of one LSTM layer on the register kernel: rows are item * bs + t * ts (in rows of 4H / H values), the
// recurrent state [B][2H] (h | c) is read when t0 > 0 and always written
struct LstmSeq {
  int t0 = 0, t1 = 0;
  long long pre_bs = 0, pre_ts = 1, out_bs = 0, out_ts = 1, skip_bs = 0, skip_ts = 1;
  float* state = nullptr;
  const int* fresh = nullptr;   // stream sessions: [B] device flags -- the state is read for the items with fresh[b] == 0 (whatever t0), always written
};
// recurrent state of a stream session for the kernels below: state [B][2H] (h | c) is read for the items with fresh[b] == 0 (the others
// start from zero) and written after the last step; null: every item starts from zero and nothing is kept
struct LstmCarry {
  float* state = nullptr;
  const int* fresh = nullptr;
};
bool lstm_seq_supported(int H);
hipError_t launch_lstm_seq(int dt, const void* pre, const float* w_hh, void* out, const void* skip, int B, int H, const LstmSeq& q,
                           hipStream_t s);
hipError_t launch_lstm_layer(int dt, const void* pre, const float* w_hh, void* out, const void* skip, int B, int T,
                             int H, hipStream_t s, LstmCarry carry = LstmCarry());
// Cooperative weight-stationary variant for H = 256 / 512 (H/4 workgroups exchange h through `ws`); w_rm is the
// row-major [4H][H] matrix.
bool lstm_coop_eligible(int H);
size_t lstm_coop_ws_bytes(int H);
// host_flag: device-visible mapped word set to 1 when the bounded h-exchange spin times out (the output is then NaN).
// Launched cooperatively: returns hipErrorCooperativeLaunchTooLarge when the H/4 workgroups cannot be co-resident
// (the caller falls back to launch_lstm_layer).
bool lstm_coop_resident(int H);
// the XCD-local form (launch_lstm_coop with coop_launch == 2) fits one XCD
int conv_fused_gn_wgs_per_cu(int dt, bool w8);   // occupancy query: workgroups per CU of the kernels a fused-GroupNorm conv lands on
int lstm_xcd_resident(int H);   // teams of sixteen workgroups one XCD holds
// occupancy query x CU count (with a margin) >= the H/4 workgroups that must be co-resident
hipError_t launch_lstm_coop(int dt, const void* pre, const float* w_rm, void* out, const void* skip, int B, int T, int H,
                            void* ws, unsigned* host_flag, int coop_launch, hipStream_t s, LstmCarry carry = LstmCarry());

// ------------------------------------------------------------------------------------------------
// rvq.hip
// ------------------------------------------------------------------------------------------------
// z_cl [B*F][D] fp32 rows; codebooks [n_q][bins][D] fp32 and their squared norms [n_q][bins].
// codes [n_q][B*F] int64 (nullable), quantized_cl [B*F][D] fp32.
hipError_t launch_rvq(const float* z_rows, int rows, int D, const float* codebooks, const float* cb_sqnorm, int bins,
                      int n_q, int64_t* codes, float* quantized_rows, hipStream_t s, int variant = 1);   // variant 0: the round-1 kernel (same codes, bit for bit)
// Dequantisation: rows [Bk*F][D] of items b0 .. b0+Bk-1 from exactly one of codes [n_q][B_total][F] int64 / packed [B][packed_stride]
// (BitPacker payload, `bits` <= 16 per code, compress.py's push order).  A code outside [0, bins) gives a NaN row and raises *flag
// = LDC_DEV_BAD_CODE (flag: the context's host-mapped words; (codebook << 56 | item << 32 | frame) of one bad code in words 2..3).
constexpr unsigned LDC_DEV_BAD_CODE = 3u;
hipError_t launch_rvq_dequant(const int64_t* codes, const uint8_t* packed, int64_t packed_stride, int bits, int n_q, int B_total, int b0,
                              int Bk, int F, const float* codebooks, int bins, int D, float* quantized_rows, unsigned* flag, hipStream_t s,
                              const int* flens = nullptr);
hipError_t launch_sqnorm_rows(const float* x, int rows, int D, float* out, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// train.hip : first slice of the training step (q_sample, L1 objective, Block forward / backward), fp32, [B, C, L]
// ------------------------------------------------------------------------------------------------
// (T = number of timesteps: device-side t is clamped to [0, T) before it indexes a schedule table)
hipError_t launch_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, int B,
                           int64_t n_per_item, float* out, int T, hipStream_t s);
hipError_t launch_predict_x_start(const float* x_t, const float* eps, const int64_t* t, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac,
                                  int B, int64_t n_per_item, float* out, int T, hipStream_t s);
// per item: clamp(-SD-SDR(est, tgt), min clip_min)  (ClippedSDR over asteroid's MultiSrcNegSDR("sdsdr"), one source)
hipError_t launch_neg_sdsdr(const float* est, const float* tgt, int B, int64_t n_per_item, float clip_min, float* per_item, hipStream_t s);
size_t l1_loss_ws_bytes(int B);
hipError_t launch_l1_loss(const float* pred, const float* target, const int64_t* t, const float* p2w, int B, int64_t n_per_item,
                          float* loss, float* grad, void* ws, int T, hipStream_t s);
size_t train_block_ws_floats(int B, int Cin, int Cout, int L, int groups);
hipError_t launch_train_pw_forward(const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int L, int pre_silu, float* y,
                                   hipStream_t s);
hipError_t launch_train_pw_backward(const float* dy, const float* x, const float* w, int B, int Cin, int Cout, int L, int pre_silu, float* dx,
                                    float* dw, float* db, hipStream_t s);
size_t train_linattn_ws_floats(int B, int H, int D, int N);
hipError_t launch_train_linattn_forward(const float* qkv, int B, int H, int D, int N, float* o, float* ws, hipStream_t s);
hipError_t launch_train_linattn_backward(const float* d_o, const float* qkv, int B, int H, int D, int N, float* ws, float* dqkv, hipStream_t s);
hipError_t launch_train_conv_forward(const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int Lin, int K, int S, int P,
                                     float* y, hipStream_t s);
hipError_t launch_train_conv_backward(const float* dy, const float* x, const float* w, int B, int Cin, int Cout, int Lin, int K, int S, int P,
                                      float* dx, float* dw, float* db, hipStream_t s);
hipError_t launch_train_upsample2(const float* in, int64_t rows, int L, int backward, float* out, hipStream_t s);
hipError_t launch_train_act(const float* x, const float* dy, int64_t n, int kind, float* out, hipStream_t s);
size_t train_attn_ws_floats(int B, int H, int N);
hipError_t launch_train_attn_forward(const float* qkv, int B, int H, int D, int N, float* out, float* ws, hipStream_t s);
hipError_t launch_train_attn_backward(const float* d_o, const float* qkv, int B, int H, int D, int N, float* ws, float* dqkv, hipStream_t s);
hipError_t launch_train_convtr_forward(const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int L, int r, float* y,
                                       hipStream_t s);
hipError_t launch_train_convtr_backward(const float* dy, const float* x, const float* w, int B, int Cin, int Cout, int L, int r, float* dx,
                                        float* dw, float* db, hipStream_t s);
hipError_t launch_train_maxscale(const float* x, const float* dy, int B, int64_t n_per_item, float* out, hipStream_t s);
extern int g_train_bf16;        // LDC_TRAIN_BF16 / option train_bf16: the GEMM shapes with the hi terms only (plain bf16 products, fp32 accumulate)
extern int g_train_fp32_mfma;   // LDC_TRAIN_FP32_MFMA: the round-2 exact-fp32 MFMA GEMMs (convmm_kernel) instead of the split-bf16 ones (train_mm3.hip)
// split-bf16 (3 x bf16 MFMA, fp32-class accuracy) GEMM shapes of a Conv1d under training: train_mm3.hip
hipError_t launch_mm3_forward(const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int Lin, int Lout, int K, int S, int P,
                              float* y, hipStream_t s);
// (bias: per output row = input channel; only the transposed-conv forward, which is this GEMM shape, passes one)
hipError_t launch_mm3_dx(const float* dy, const float* w, int B, int Cin, int Cout, int Lin, int Lout, int K, int S, int P, float* dx, hipStream_t s,
                         const float* bias = nullptr);
// (db: optional bias gradient [Cout] = sum over items and positions of dy, accumulated by the workgroups that stage dy anyway)
hipError_t launch_mm3_dw(const float* dy, const float* x, int B, int Cin, int Cout, int Lin, int Lout, int K, int S, int P, float* dw, hipStream_t s,
                         float* db = nullptr);
extern hipStream_t g_train_side_stream;   // the training side stream (train.hip; nullptr until first used): launches on it take their own workspaces
extern int g_train_dw_side;    // option train_dw_side: the weight-gradient GEMMs of the Blocks on a side stream (set by DiffusionTrainer around its backward pass)
hipStream_t train_side_stream();              // the side stream (created on first use; nullptr on failure)
hipError_t launch_train_join(hipStream_t s);   // `s` waits for everything the side stream holds (no-op when it was not used)
extern int g_train_valu;   // LDC_TRAIN_VALU: the training path's GEMM shapes on the VALU reference kernels instead of the fp32 MFMA ones
hipError_t launch_adam(float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float b1, float b2, float eps, hipStream_t s);
hipError_t launch_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, int* step_dev, float lr, float b1, float b2, float eps, hipStream_t s);
hipError_t launch_train_ln_forward(const float* x, const float* g, int B, int C, int L, float* y, float* stats, hipStream_t s);
hipError_t launch_train_ln_backward(const float* dy, const float* x, const float* g, const float* stats, int B, int C, int L, float* dx,
                                    float* dg, hipStream_t s);
hipError_t launch_train_block_forward(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                                      const float* ss, int B, int Cin, int Cout, int L, int groups, float* y, float* ws, hipStream_t s);
hipError_t launch_train_block_backward(const float* dy, const float* x, const float* gamma, const float* beta, const float* ss, int B,
                                       int Cin, int Cout, int L, int groups, float* ws, float* dx, float* dw, float* db, float* dgamma,
                                       float* dbeta, float* dss, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// bitstream.hip : index packing + range coder (bit-exact with srcs/encodec/binary.py, srcs/quantization/ac.py)
// ------------------------------------------------------------------------------------------------
hipError_t launch_pack_codes(const int64_t* codes, int n_q, int B, int F, int bits, uint8_t* out, int64_t out_stride, hipStream_t s);
hipError_t launch_unpack_codes(const uint8_t* in, int64_t in_stride, int n_q, int B, int F, int bits, int64_t* codes, hipStream_t s);
hipError_t launch_build_cdf(const float* pdf, int rows, int card, int total_range_bits, float roundoff, int min_range, int* cdf,
                            hipStream_t s);
// mode 0: cdf table per (stream, step) [B*S][card]; mode 1: `period` static tables, symbol s uses table s % period
hipError_t launch_ac_encode(const int* symbols, const int* cdf, int B, int S, int card, int mode, int period, int total_range_bits,
                            uint8_t* out, int64_t out_stride, int64_t cap, int64_t* nbytes, hipStream_t s, const int* n_sym = nullptr);
hipError_t launch_ac_decode(const uint8_t* in, int64_t in_stride, const int64_t* nbytes, const int* cdf, int B, int S, int card, int mode,
                            int period, int total_range_bits, int* symbols, int* status, hipStream_t s, const int* n_sym = nullptr);

}  // namespace ldc
