// ldc_api_pool.cpp -- a timestep per item: ldc_unet_forward_items and the decode pools (include/ladiffcodec.h, "decode pools";
// DESIGN.md section 5d).  Host-side C++ only.  The per-item plan is the ragged plan of unet_plan.cpp (PlanBuilder under Plan::items) whose
// item-state table (ItemState, ldc_kernels.h) replaces the part's step_state {t, j, key} and cur_ss row; the kernels that read the table
// are step_begin_items, gn_apply (t_stride) and p_sample_update_items.  The sampler is part of the record too: a DDIM or DPM-Solver++
// item's record names its kind and points to its schedule, a row of the pool's schedule arena (ldc_pool_admit_ddim, ldc_pool_admit_dpm);
// a DPM item's x0 history is its slot's block of the pool's history buffer.
#include "ldc_internal.h"

namespace {

const char* kNoFp8 = "per-item timesteps are not available on the fp8 engine (its fused forms have no length-aware variant): use dtype bf16 or f32";

// every length of a per-item call, before any GPU work
int check_item_length(int L, int Lmax, int quantum, const char* entry, int item) {
  if (L <= 0 || L > Lmax || L % quantum)
    return fail(LDC_E_INVALID, "%s: length %d of item %d must be a multiple of %d latent frames in (0, %d]", entry, L, item, quantum, Lmax);
  return LDC_OK;
}

int check_pool(ldc_ctx* c, const ldc_pool* p, const char* entry) {
  if (!c) return fail(LDC_E_INVALID, "%s: null pointer: ctx", entry);
  if (!p) return fail(LDC_E_INVALID, "%s: null pointer: pool", entry);
  if (p->ctx != c) return fail(LDC_E_INVALID, "%s: the pool belongs to another context (%p, not %p)", entry, (void*)p->ctx, (void*)c);
  if (p->poisoned)
    return fail(LDC_E_STATE, "%s: an earlier call on this pool failed after its GPU work had started, its state is inconsistent: "
                             "ldc_pool_evict every slot to make it usable again", entry);
  return LDC_OK;
}
int check_slot(const ldc_pool* p, int slot, const char* entry) {
  if (slot < 0 || slot >= p->slots) return fail(LDC_E_INVALID, "%s: slot %d is outside [0, %d)", entry, slot, p->slots);
  return LDC_OK;
}
// a call that failed before its GPU work leaves the pool as it was; one that failed later marks it
int finish_call(ldc_pool* p, int rc) {
  if (rc != LDC_OK && p->touched) p->poisoned = true;
  p->touched = false;
  return rc;
}

// the part of the pool that holds `slot`, and the slot's index inside it
Plan* part_of(const ldc_pool* p, int slot, int* in_part) {
  int k = p->h.n - 1;
  while (k > 0 && p->h.b0[k] > slot) --k;
  *in_part = slot - p->h.b0[k];
  return p->h.p[k];
}

ItemState idle_record(int len) {
  ItemState r{};
  r.len = len;   // (t = 0: a valid row of the timestep table for the discarded computation; no tape, no schedule)
  return r;
}

// the pool's graphs and pinned plans leave the caches (nothing of them may be running)
void drop_pool_plans(ldc_ctx* c, int id) {
  drop_step_graphs(c, [id](const StepGraph& g) { return g.key.pool_id == id; });
  for (size_t i = 0; i < c->plans.size();) {
    if (c->plans[i]->pool_id == id) release_plan(c, i);
    else ++i;
  }
}

// one step of batch part k of the pool on stream sk: the items' states move on, the UNet runs, every running item is updated
int pool_half_step(ldc_ctx* c, ldc_pool* p, int k, hipStream_t sk) {
  Plan* pl = p->h.p[k];
  const int C = c->unet.channels;
  const int64_t item = (int64_t)C * p->Lmax;
  HIPCHK(launch_step_begin_items(pl->item_state, pl->B, pl->step_state, pl->zero_ptr, pl->zero_bytes, 1, sk));
  LDCCHK(run_ops(c, pl, true, sk));
  HIPCHK(launch_p_sample_update_items(c->dt, p->x + (size_t)p->h.b0[k] * item, item, pl->eps_cl, pl->x_cl, pl->B, C, p->Lmax, c->sched,
                                      pl->item_state, c->unet.timesteps, p->x0_prev + (size_t)p->h.b0[k] * item, sk));
  return LDC_OK;
}

int pool_eager_step(ldc_ctx* c, ldc_pool* p, hipStream_t s) {
  const Halves& h = p->h;
  if (parts_parallel(c, h)) {
    LDCCHK(fork_parts(c, h, s));
    int r = LDC_OK;
    for (int k = 0; k < h.n && r == LDC_OK; ++k) r = pool_half_step(c, p, k, k == 0 ? s : c->aux_stream[k]);
    const int jr = join_parts(c, h, s);   // (a failure between fork and join must still join)
    return r != LDC_OK ? r : jr;
  }
  for (int k = 0; k < h.n; ++k) LDCCHK(pool_half_step(c, p, k, s));
  return LDC_OK;
}

constexpr int kPoolGraphSteps = 5;   // steps per replayed graph, as the two-part denoise loop (ldc_api_sample.cpp: denoise_loop); single steps for the remainder

int pool_graph(ldc_ctx* c, const ldc_pool* p, StepGraph** out) {
  StepGraphKey key;
  key.B = p->slots; key.L = p->Lmax; key.F = p->Fmax; key.ragged = 1; key.pool_id = p->id;
  return step_graph_for(c, key, out);
}

// n steps of every running slot.  ONE single-stream graph per batch part (5 steps, and 1 step for the remainder), captured once and
// replayed for every state of the pool: nothing about an item's progress is a kernel argument.  The replays go through replay_parts, the
// interleaved bounded look-ahead of the denoise loop's per-part path.
int pool_steps(ldc_ctx* c, ldc_pool* p, int n, hipStream_t s) {
  const Halves& h = p->h;
  int done = 0;
  const bool eager = c->profile || c->serial_parts;
  if (eager || !p->warm) {   // (the first step of a pool runs eagerly: code objects load outside a capture)
    const int m = eager ? n : 1;
    for (; done < m; ++done) LDCCHK(pool_eager_step(c, p, s));
    p->warm = true;
    if (done == n) return LDC_OK;
  }
  StepGraph* sg = nullptr;
  LDCCHK(pool_graph(c, p, &sg));
  const int K = kPoolGraphSteps;
  if (!sg->built) {
    LDCCHK(build_step_graphs(c, h, sg, K, true, h.n >= 2, s, [&](int k, hipStream_t sk) { return pool_half_step(c, p, k, sk); }));
    sg->bound = StepGraphBinding{p->x, nullptr, s, h.n, K, true};
  }
  const int left = n - done, n_big = left / K, n_rep = n_big + (left - n_big * K);
  if (h.n >= 2) LDCCHK(fork_parts(c, h, s));
  const char* what = "";
  const hipError_t err = replay_parts(c, h, sg, n_big, n_rep, false, s, &what);
  const int jr = h.n >= 2 ? join_parts(c, h, s) : LDC_OK;   // (a failure between fork and join must still join)
  if (err != hipSuccess) return fail(LDC_E_HIP, "%s failed in the pool's graph replay: %s", what, hipGetErrorString(err));
  return jr;
}

}  // namespace

extern "C" int ldc_unet_forward_items(ldc_ctx* c, const float* x, const int32_t* t_host, const float* cond, const int32_t* latent_lens_host, int B,
                                      int Lmax, int Fmax, float* eps_out, void* stream) {
  const char* entry = "ldc_unet_forward_items";
  if (!c || !x || !t_host || !cond || !eps_out)
    return fail(LDC_E_INVALID, "%s: null pointer: %s", entry, !c ? "ctx" : !x ? "x" : !t_host ? "t_host" : !cond ? "cond" : "eps_out");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  LDCCHK(check_unet_args(c, B, Lmax, Fmax));
  for (int b = 0; b < B; ++b)
    if (t_host[b] < 0 || t_host[b] >= c->unet.timesteps)
      return fail(LDC_E_INVALID, "%s: t_host[%d] = %d is outside [0, %d)", entry, b, (int)t_host[b], c->unet.timesteps);
  // (lengths NULL: every item Lmax long.  The quantum is then not asked for: whole condition frames hold through check_unet_args, and a
  // length the UNet's halvings do not survive is refused by the plan builder, as for ldc_unet_forward)
  if (latent_lens_host) {
    const int q = ragged_latent_quantum(c);
    if (Lmax % q) return fail(LDC_E_INVALID, "%s: the padded length %d is not a multiple of %d latent frames", entry, Lmax, q);
    for (int b = 0; b < B; ++b) LDCCHK(check_item_length(latent_lens_host[b], Lmax, q, entry, b));
  }
  if (c->w8) return fail(LDC_E_INVALID, "%s: %s", entry, kNoFp8);
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(get_halves(c, B, Lmax, Fmax, s, &h, true, true, 0));
  const int up = upsample_factor(c), C = c->unet.channels;
  for (int k = 0; k < h.n; ++k) {   // the items' records (and the ragged plan's view of their lengths) in front of everything that reads them
    Plan* pl = h.p[k];
    std::vector<ItemState> recs(pl->B);
    for (int b = 0; b < pl->B; ++b) {
      recs[b] = idle_record(latent_lens_host ? latent_lens_host[h.b0[k] + b] : Lmax);
      recs[b].t = t_host[h.b0[k] + b];
      recs[b].remaining = 1;
    }
    HIPCHK(launch_items_write(pl->item_state, recs.data(), pl->B, pl->lens, pl->flens, up, s));
  }
  LDCCHK(load_cond(c, h, cond, s));
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    HIPCHK(launch_to_cl(c->dt, x + (size_t)h.b0[k] * C * Lmax, pl->x_cl, pl->B, C, Lmax, nullptr, 0, 0.f, s));
    HIPCHK(launch_mask_rows(c->dt, pl->x_cl, pl->B, Lmax, C, pl->lens, 0, s));   // (whatever the caller's padding holds)
    HIPCHK(launch_step_begin_items(pl->item_state, pl->B, pl->step_state, pl->zero_ptr, pl->zero_bytes, 0, s));
    LDCCHK(run_ops(c, pl, true, s));
    HIPCHK(launch_mask_rows(c->dt, pl->eps_cl, pl->B, Lmax, C, pl->lens, 0, s));   // (final_conv's bias)
    HIPCHK(launch_from_cl(c->dt, pl->eps_cl, eps_out + (size_t)h.b0[k] * C * Lmax, pl->B, C, Lmax, nullptr, 0, 0.f, s));
  }
  return finish_stream(c, stream);
}

extern "C" int ldc_pool_create(ldc_ctx* c, int slots, int Lmax, ldc_pool** out) {
  const char* entry = "ldc_pool_create";
  if (!c || !out) return fail(LDC_E_INVALID, "%s: null pointer: %s", entry, !c ? "ctx" : "out");
  *out = nullptr;
  if (slots <= 0) return fail(LDC_E_INVALID, "%s: slots = %d must be positive", entry, slots);
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (c->w8) return fail(LDC_E_INVALID, "%s: %s", entry, kNoFp8);
  const int q = ragged_latent_quantum(c), up = upsample_factor(c);
  if (Lmax <= 0 || Lmax % q) return fail(LDC_E_INVALID, "%s: Lmax = %d is not a positive multiple of %d latent frames", entry, Lmax, q);
  std::unique_ptr<ldc_pool> p(new ldc_pool());
  p->ctx = c; p->id = c->next_pool_id++; p->slots = slots; p->Lmax = Lmax; p->Fmax = Lmax / up;
  p->remaining.assign(slots, -1);
  p->len.assign(slots, q);
  hipStream_t s = c->own_stream;
  const int C = c->unet.channels;
  const size_t es = dt_size(c->dt);
  auto build = [&]() -> int {
    LDCCHK(get_halves(c, slots, Lmax, p->Fmax, s, &p->h, true, true, p->id));
    void* x = nullptr;
    LDCCHK(p->mem.alloc(&x, (size_t)slots * C * Lmax * 4));
    p->x = (float*)x;
    // the DPM items' x0 history, the layout of x: always allocated, so its address is in every captured graph of the pool, also one
    // captured before the first DPM item.  Not cleared: a DPM item's iteration 0 does not load it
    void* hist = nullptr;
    LDCCHK(p->mem.alloc(&hist, (size_t)slots * C * Lmax * 4));
    p->x0_prev = (float*)hist;
    // the schedule arena: a row of `timesteps` entries per slot (a DDIM or DPM item runs at most that many iterations), zero = DDPM-free rows
    void* sc = nullptr;
    const size_t sched_bytes = (size_t)slots * c->unet.timesteps * sizeof(SchedEntry);
    LDCCHK(p->mem.alloc(&sc, sched_bytes));
    p->sched = (SchedEntry*)sc;
    p->sched_host.reserve(c->unet.timesteps);
    p->dpm_host.reserve(c->unet.timesteps);
    HIPCHK(hipMemsetAsync(p->sched, 0, sched_bytes, s));
    // every slot idle on finite state: zero latents and condition, the shortest length, t = 0
    HIPCHK(hipMemsetAsync(p->x, 0, (size_t)slots * C * Lmax * 4, s));
    for (int k = 0; k < p->h.n; ++k) {
      Plan* pl = p->h.p[k];
      const size_t rows = (size_t)pl->B * Lmax;
      HIPCHK(hipMemsetAsync(pl->x_cl, 0, rows * C * es, s));
      HIPCHK(hipMemsetAsync(pl->cond_cl, 0, rows * c->unet.cond_channels * es, s));
      if (pl->init_pc) HIPCHK(hipMemsetAsync(pl->init_pc, 0, rows * c->unet.dim * es, s));
      std::vector<ItemState> recs(pl->B, idle_record(q));
      HIPCHK(launch_items_write(pl->item_state, recs.data(), pl->B, pl->lens, pl->flens, up, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return LDC_OK;
  };
  const int rc = build();
  if (rc != LDC_OK) {
    (void)hipStreamSynchronize(s);
    drop_pool_plans(c, p->id);
    return rc;
  }
  ++c->live_pools;
  *out = p.release();
  return LDC_OK;
}

extern "C" int ldc_pool_destroy(ldc_pool* p) {
  if (!p) return LDC_OK;
  ldc_ctx* c = p->ctx;
  (void)hipSetDevice(c->device);
  if (p->last_stream) (void)hipStreamSynchronize(p->last_stream);   // (the parts' streams were joined into it by the pool's last step call)
  (void)hipStreamSynchronize(c->own_stream);
  drop_pool_plans(c, p->id);
  --c->live_pools;
  delete p;
  return LDC_OK;
}

// ldc_pool_admit (kind ITEM_DDPM: n_steps steps from t = n_steps - 1, t_start not read), ldc_pool_admit_ddim (ITEM_DDIM: n_steps DDIM
// iterations on the schedule (t_start, n_steps, eta), written into the slot's row of the pool's arena) and ldc_pool_admit_dpm (ITEM_DPM:
// n_steps DPM-Solver++ iterations on the schedule (t_start, n_steps) in the same row; no noise, seed or eta)
static int pool_admit(ldc_ctx* c, ldc_pool* p, int slot, const float* img, const float* cond, int L, int kind, int t_start, int n_steps,
                      float eta, const float* noise, uint64_t seed, void* stream, const char* entry) {
  const bool ddim = kind == ITEM_DDIM, dpm = kind == ITEM_DPM;
  LDCCHK(check_pool(c, p, entry));
  if (!img || !cond) return fail(LDC_E_INVALID, "%s: null pointer: %s", entry, !img ? "img" : "cond");
  LDCCHK(check_slot(p, slot, entry));
  if (p->remaining[slot] >= 0)
    return fail(LDC_E_INVALID, "%s: slot %d is not free (%s, %d steps remaining)", entry, slot, p->remaining[slot] ? "running" : "finished", p->remaining[slot]);
  LDCCHK(check_item_length(L, p->Lmax, ragged_latent_quantum(c), entry, slot));
  if (ddim || dpm) {
    if (t_start < 1 || t_start > c->unet.timesteps) return fail(LDC_E_INVALID, "%s: t_start = %d must be in [1, %d]", entry, t_start, c->unet.timesteps);
    if (n_steps < 1 || n_steps > t_start)
      return fail(LDC_E_INVALID, "%s: n_steps = %d must be in [1, t_start = %d] (more would repeat timesteps)", entry, n_steps, t_start);
    if (ddim && !(eta >= 0.0f && eta <= 1.0f)) return fail(LDC_E_INVALID, "%s: eta = %g must be a finite value in [0, 1]", entry, (double)eta);
  } else if (n_steps < 1 || n_steps > c->unet.timesteps) {
    return fail(LDC_E_INVALID, "%s: n_steps = %d must be in [1, %d]", entry, n_steps, c->unet.timesteps);
  }
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (ddim) {   // (host only: nothing of the pool has moved if this fails)
    bool draws = false;
    LDCCHK(ddim_schedule_fill(c, t_start, n_steps, eta, &p->sched_host, &draws));
  } else if (dpm) {
    LDCCHK(dpm_schedule_fill(c, t_start, n_steps, &p->dpm_host));
  }
  hipStream_t s = pick_stream(c, stream);
  const int up = upsample_factor(c), F = L / up, C = c->unet.channels, Cc = c->unet.cond_channels, Lmax = p->Lmax;
  const size_t es = dt_size(c->dt);
  auto body = [&]() -> int {
    // process_cond for the one item on a B = 1 ragged plan of the ordinary cache (nothing of record lives there), then its rows move
    // into the slot: the processed condition and, with the split init_conv, the condition's half of it
    c->call_tick = c->use_tick;
    Plan* p1 = nullptr;
    LDCCHK(get_plan(c, 1, Lmax, p->Fmax, 0, s, &p1, true, false, 0));
    int sb = 0;
    Plan* pk = part_of(p, slot, &sb);
    if ((p1->init_pc != nullptr) != (pk->init_pc != nullptr)) return fail(LDC_E_STATE, "%s: the pool's plan and the admission plan split init_conv differently", entry);
    p->touched = true;
    HIPCHK(launch_lens_write(p1->lens, &L, 1, s));
    HIPCHK(launch_lens_write(p1->flens, &F, 1, s));
    HIPCHK(launch_to_cl(DT_F32, cond, p1->cond_in_cl, 1, Cc, F, nullptr, 0, 0.f, s));   // rows [0, F) of Fmax; cond_ops zero the rest
    LDCCHK(run_ops(c, p1, false, s));
    const size_t crow = (size_t)Lmax * Cc * es, prow = (size_t)Lmax * c->unet.dim * es, xrow = (size_t)Lmax * C * es;
    HIPCHK(hipMemcpyAsync((char*)pk->cond_cl + sb * crow, p1->cond_cl, crow, hipMemcpyDeviceToDevice, s));
    if (pk->init_pc) HIPCHK(hipMemcpyAsync((char*)pk->init_pc + sb * prow, p1->init_pc, prow, hipMemcpyDeviceToDevice, s));
    // the latents: fp32 [C][L] on the item's own length, and the channels-last copy the UNet reads (zero behind the item)
    HIPCHK(hipMemcpyAsync(p->x + (size_t)slot * C * Lmax, img, (size_t)C * L * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemsetAsync((char*)pk->x_cl + sb * xrow, 0, xrow, s));
    HIPCHK(launch_to_cl(c->dt, img, (char*)pk->x_cl + sb * xrow, 1, C, L, nullptr, 0, 0.f, s));
    // a DDIM or DPM item's schedule into the slot's row of the arena, in front of the record that points to it (the slot is free: no
    // step issued before this call reads the row).  The slot's history is NOT cleared: a DPM item's iteration 0 does not load it
    SchedEntry* row = p->sched + (size_t)slot * c->unet.timesteps;
    if (ddim) HIPCHK(launch_ddim_table_write(&row->ddim, p->sched_host.data(), n_steps, s));
    if (dpm) HIPCHK(launch_dpm_table_write(&row->dpm, p->dpm_host.data(), n_steps, s));
    // the record last: the state BEFORE the first step (the step's first kernel advances to iteration 0: t = n_steps - 1, or the
    // first timestep of the schedule)
    ItemState r = idle_record(L);
    r.t = ddim || dpm ? t_start : n_steps; r.j = -1; r.key_lo = (unsigned)seed; r.key_hi = (unsigned)(seed >> 32); r.remaining = n_steps; r.noise = noise;
    r.kind = kind;
    r.sched = ddim || dpm ? row : nullptr;
    HIPCHK(launch_items_write(pk->item_state + sb, &r, 1, pk->lens + sb, pk->flens + sb, up, s));
    p->remaining[slot] = n_steps;
    p->len[slot] = L;
    p->last_stream = s;
    return finish_stream(c, stream);
  };
  return finish_call(p, body());
}

extern "C" int ldc_pool_admit(ldc_ctx* c, ldc_pool* p, int slot, const float* img, const float* cond, int L, int n_steps, const float* noise,
                              uint64_t seed, void* stream) {
  return pool_admit(c, p, slot, img, cond, L, ITEM_DDPM, 0, n_steps, 0.0f, noise, seed, stream, "ldc_pool_admit");
}

extern "C" int ldc_pool_admit_ddim(ldc_ctx* c, ldc_pool* p, int slot, const float* img, const float* cond, int L, int t_start, int n_steps,
                                   float eta, const float* noise, uint64_t seed, void* stream) {
  return pool_admit(c, p, slot, img, cond, L, ITEM_DDIM, t_start, n_steps, eta, noise, seed, stream, "ldc_pool_admit_ddim");
}

extern "C" int ldc_pool_admit_dpm(ldc_ctx* c, ldc_pool* p, int slot, const float* img, const float* cond, int L, int t_start, int n_steps,
                                  void* stream) {
  return pool_admit(c, p, slot, img, cond, L, ITEM_DPM, t_start, n_steps, 0.0f, nullptr, 0, stream, "ldc_pool_admit_dpm");
}

extern "C" int ldc_pool_step(ldc_ctx* c, ldc_pool* p, int n, void* stream) {
  const char* entry = "ldc_pool_step";
  LDCCHK(check_pool(c, p, entry));
  if (n <= 0) return fail(LDC_E_INVALID, "%s: n = %d must be positive", entry, n);
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  hipStream_t s = pick_stream(c, stream);
  auto body = [&]() -> int {
    if (p->h.n >= 2) LDCCHK(calibrate_part_streams(c, s));
    p->touched = true;
    LDCCHK(pool_steps(c, p, n, s));
    for (int& r : p->remaining)
      if (r > 0) r = std::max(0, r - n);
    p->last_stream = s;
    return finish_stream(c, stream);
  };
  return finish_call(p, body());
}

extern "C" int ldc_pool_remaining(const ldc_pool* p, int32_t* remaining_host) {
  if (!p || !remaining_host) return fail(LDC_E_INVALID, "ldc_pool_remaining: null pointer: %s", !p ? "pool" : "remaining_host");
  for (int i = 0; i < p->slots; ++i) remaining_host[i] = p->remaining[i];
  return LDC_OK;
}

// ldc_pool_take (free_slot) / ldc_pool_peek: the latents of a finished slot, copied on the stream
static int pool_read(ldc_ctx* c, ldc_pool* p, int slot, float* latents_out, void* stream, bool free_slot, const char* entry) {
  LDCCHK(check_pool(c, p, entry));
  if (!latents_out) return fail(LDC_E_INVALID, "%s: null pointer: latents_out", entry);
  LDCCHK(check_slot(p, slot, entry));
  if (p->remaining[slot] != 0)
    return fail(LDC_E_STATE, "%s: slot %d is not finished (%s)", entry, slot, p->remaining[slot] < 0 ? "free" : "running");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  hipStream_t s = pick_stream(c, stream);
  auto body = [&]() -> int {
    const int C = c->unet.channels;
    p->touched = true;
    HIPCHK(hipMemcpyAsync(latents_out, p->x + (size_t)slot * C * p->Lmax, (size_t)C * p->len[slot] * 4, hipMemcpyDeviceToDevice, s));
    if (free_slot) p->remaining[slot] = -1;   // (the device record is idle already: the slot stopped behind t = 0)
    p->last_stream = s;
    return finish_stream(c, stream);
  };
  return finish_call(p, body());
}
extern "C" int ldc_pool_take(ldc_ctx* c, ldc_pool* p, int slot, float* latents_out, void* stream) {
  return pool_read(c, p, slot, latents_out, stream, true, "ldc_pool_take");
}
extern "C" int ldc_pool_peek(ldc_ctx* c, ldc_pool* p, int slot, float* latents_out, void* stream) {
  return pool_read(c, p, slot, latents_out, stream, false, "ldc_pool_peek");
}

extern "C" int ldc_pool_evict(ldc_pool* p, int slot) {
  const char* entry = "ldc_pool_evict";
  if (!p) return fail(LDC_E_INVALID, "%s: null pointer: pool", entry);
  LDCCHK(check_slot(p, slot, entry));
  ldc_ctx* c = p->ctx;
  int rc = LDC_OK;
  if (p->remaining[slot] >= 0) {
    // the record goes idle on the stream of the pool's last call (behind every step already issued): no later step stores the item or
    // reads its tape.  Written even on a marked pool, whose host mirror may be behind the device
    hipStream_t s = p->last_stream ? p->last_stream : c->own_stream;
    int sb = 0;
    Plan* pk = part_of(p, slot, &sb);
    const ItemState r = idle_record(p->len[slot]);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = launch_items_write(pk->item_state + sb, &r, 1, pk->lens + sb, pk->flens + sb, upsample_factor(c), s);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      p->poisoned = true;
      rc = fail(LDC_E_HIP, "%s: writing the idle record of slot %d failed: %s", entry, slot, hipGetErrorString(e));
    }
    p->remaining[slot] = -1;
  }
  bool all_free = true;
  for (int r : p->remaining) all_free = all_free && r < 0;
  if (all_free && rc == LDC_OK) p->poisoned = false;
  return rc;
}
