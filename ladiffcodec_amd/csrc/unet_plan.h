// unet_plan.h -- the UNet planner: PlanBuilder turns the loaded UNet's blocks into the launches of one step (Plan::step), build_plan
// lays a whole step out on an arena, get_plan is the context's plan cache (LRU) and run_ops issues a plan's launches.  Bodies in
// unet_plan.cpp; the test hooks that build private plans from the same PlanBuilder are in ldc_api_debug.cpp.  Included by ldc_internal.h,
// behind the context.
#pragma once

// fp8 outputs of gn_apply: the channel counts its kernel takes
bool gn_apply_fp8_ok(int C);

struct PlanBuilder {
  ldc_ctx* c;
  Plan* pl;
  Arena* ar;
  int B;
  size_t es;   // element size of the UNet dtype
  float* stats_pool = nullptr;   // [n_gn][B][groups][2]
  int stats_used = 0;
  char* part_pool = nullptr;     // granule regions of the fused GroupNorm applies (inside the region the step's first kernel clears)
  size_t part_used = 0, part_cap = 0;
  float* linattn_ws = nullptr;
  int linattn_used = 0;
  float* sk_part = nullptr;        // split-K workspace shared by the plan's convs (they run one after another)
  unsigned* sk_count = nullptr;    // arrival counters, inside the region the step's memset clears
  long long sk_part_cap = 0;
  int sk_count_cap = 0;

  void* act(int rows, int C);
  // ragged plan: the device lengths and the level of a tensor of L rows per item (a level's lengths are lens[b] >> level)
  // (a planning pass on a measuring arena has no device memory: the lengths' address is a placeholder there, never dereferenced -- a null
  // one made those passes plan the equal-length forms, so that a ragged plan of a model whose ResnetBlocks fuse their GroupNorm apply
  // was measured WITHOUT the conv outputs its unfused forms store, and built past the end of its arena)
  const int* lens() const;
  int level(int L) const;
  // the padding rows of y [B*L][C] written as zero: behind every plain conv whose output another conv reads (its bias and the taps that
  // reach back over the item's edge leave values there)
  void mask(void* y, int L, int C);
  int where = 0;   // stream selector for the ops being added (0 main, 1 side)
  void mark(int kind);   // 2 = fork (side waits for main), 3 = join (main waits for side)
  void add(std::function<hipError_t(hipStream_t)> f, bool is_conv = false, double flops = 0, int cls = LDC_CLASS_OTHER,
           double bytes = 0);
  std::string info;   // description of the next op added
  void* y2_next = nullptr;   // second output of the next conv added (a layer with a folded 1x1 conv)
  float* qkv_ctx_next = nullptr;   // context workspace of the next conv added (to_qkv with the context fold)
  int qkv_ctx_stride_next = 0;
  const float* ln_rowstat_next = nullptr;   // row-statistics partials of the next (LayerNorm-folded) conv's input
  bool want_rowstat = false;                // the next resnet()'s fused block2 conv leaves those partials of its output ...
  float* last_rowstat = nullptr;            // ... here (null when it could not)
  // what the last resnet() built, for ldc_debug_resnet_block (null on every plan of a decode): the route it took and where its
  // intermediate tensors and GroupNorm statistics live
  struct ResnetTrace {
    int epi1 = 0, epi2 = 0, folded = 0, fuse_stats = 0, xn = 0, rowstat = 0;
    int t1[4] = {0, 0, 1, 0}, t2[4] = {0, 0, 1, 0};   // conv_bm of the two launched convs
    void* b = nullptr;                                  // block1's stored output
    void *a = nullptr, *d = nullptr;                    // unfused: the conv outputs as stored (what launch_gn_stats and gn_apply read)
    float *st1 = nullptr, *st2 = nullptr;               // unfused: [B][groups][kGnPad]
    char *part1 = nullptr, *part2 = nullptr;            // fused: the convs' granule regions
    int mslots1 = 0, mslots2 = 0;
  };
  ResnetTrace* trace = nullptr;
  // fused GroupNorm apply of a conv (see ConvCall::gn_cnt)
  struct GnEpi {
    void* part = nullptr;          // granule region of this conv
    int mslots = 0;
    float* rowstat = nullptr;      // with a residual: per-row (sum, sumsq) partials of the output for a LayerNorm folded into the consumer
    const float* gamma = nullptr; const float* beta = nullptr; const float* ss = nullptr;
    int out = 0;
  };
  // rows per tile the pipelined kernel would use for this conv (0: generic kernel) -- the fused apply needs L_out >= that
  // (out[0] = rows per tile, out[1] = wave rows, out[2] = split-K factor)
  void conv_bm(const ConvLayer& ly, int L_in, int L_out, bool with_stats, int* out);   // out: int[4]
  // a granule region for a fused conv with tile height bm and wm wave rows; null when the pool is exhausted (first planning pass: sizes only)
  bool take_part(GnEpi* ge, int L, int bm, int wm, int n);
  void conv(const ConvLayer& ly, const void* x1, const void* x2, void* y, const void* residual, int L_in, int L_out,
            float* gn_sum = nullptr, unsigned* colmax = nullptr, int cm_lo = 0, int cm_hi = 0, int cm_stride = 0,
            const GnEpi* ge = nullptr);
  // zeroed-every-step bytes from the granule pool (nullptr while the pool is being sized)
  void* take_raw(size_t bytes);
  float* next_stats();
  // ResnetBlock.forward (unet.py:176-192)
  // ln_g != null: the block's last kernel also writes LayerNorm(out) * ln_g to *xn_out (the PreNorm of the attention
  // block that consumes `out`)
  // out_mode (final ResnetBlock only): bit 2 = write tanh(out) (unet.py:467), bit 0 = in fp8 (its only consumer is final_conv)
  void* resnet(const ResnetW& r, const void* x1, const void* x2, int L, const float* ln_g = nullptr, void** xn_out = nullptr,
               bool xn_fp8 = false, int out_mode = 0);
  bool qkv_fp8(const LinAttnW& a) const;
  // the attention block's PreNorm can ride inside to_qkv: the folded layer exists, runs on the pipelined kernel, and the ResnetBlock
  // in front fuses its GroupNorm apply (else its gn_apply launch writes the LayerNorm output on the way at no extra launch)
  bool ln_foldable(const LinAttnW& a, int L);
  // Residual(PreNorm(LinearAttention)) (unet.py:208-222) / Residual(PreNorm(Attention)) (:234-246)
  void* attention(const LinAttnW& a, const void* x, int L, bool linear, void* xn_pre = nullptr);
  // a ResnetBlock and the attention block behind it as a step pairs them: the PreNorm either rides inside to_qkv (the block leaves
  // the row statistics) or is written by the block's last kernel.  Returns the attention block's output, *resnet_out the ResnetBlock's
  void* resnet_then_attention(const ResnetW& r, const LinAttnW& a, const void* x1, const void* x2, int L, bool linear, void** resnet_out = nullptr);
  // final ResnetBlock -> tanh: by the block's last kernel where it can (one launch and two passes over the tensor less), else a
  // launch of its own; f8: the result in fp8 (its only consumer is final_conv)
  void* final_block(const ResnetW& r, const void* x1, const void* x2, int L, bool f8);
  // takes the region a step's first kernel clears (plan_passes.h: zero_region_layout) and the split-K workspace from the arena: n_gn
  // GroupNorm sum buffers, the plan's granule pool, n_lin LinearAttention workspaces.  Returns the scale_x maxima
  float* take_zero_region(int n_gn, size_t n_lin, bool lin_cleared, size_t sx_bytes);
};

int build_plan(ldc_ctx* c, Plan* pl, Arena& ar, int B, int L, int F);
// the cached plan of (B, L, F, slot, ...), built on first use behind the LRU eviction
int get_plan(ldc_ctx* c, int B, int L, int F, int slot, hipStream_t s, Plan** out, bool ragged = false, bool items = false, int pool_id = 0,
             const std::vector<int>* win_lens = nullptr, int win_O = 0);
// issues the launches of pl->step (is_step; fork / join markers on the part's side stream, profiling events) or of pl->cond_ops
int run_ops(ldc_ctx* c, Plan* pl, bool is_step, hipStream_t s);
