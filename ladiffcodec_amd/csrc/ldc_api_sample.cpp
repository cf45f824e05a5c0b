// ldc_api_sample.cpp -- the sampler loops: one denoise step of a batch part, the step-graph capture and replay of the denoise loop, the
// DDIM / DPM-Solver++ schedules and the sampler entry points over prepared arguments (ldc_p_sample ... ldc_dpm_sample).  Host-side C++
// only.  ldc_decode and the windows front ends (ldc_api.cpp) and the decode pools (ldc_api_pool.cpp) call in through ldc_internal.h.
#include "ldc_internal.h"

// one reverse-diffusion step of batch part k on stream s: select the timestep row, run the UNet, update the state,
// advance this part's step counter.  Parts never interact, so each is a self-contained chain.
// sm (default: DDPM p_sample): the sampler kind and the device schedule table of a DDIM / DPM loop (step_begin takes t from it, the
// update kernel the coefficients)
static int half_step(ldc_ctx* c, const Halves& h, int k, float* x, const float* noise, int64_t noise_stride, hipStream_t s,
                     const StepSampler& sm = StepSampler()) {
  Plan* pl = h.p[k];
  const size_t off = (size_t)h.b0[k] * c->unet.channels * pl->L;
  unsigned long long* tl = c->timeline ? c->tl_buf + (size_t)k * 2048 * 2 : nullptr;
  // (the step state moves on in the step's FIRST kernel: the callers start a loop from (t + 1, iteration - 1), set_steps)
  if (sm.kind == SAMPLER_DPM) {
    if (!sm.dpm || !pl->x0_prev) return fail(LDC_E_STATE, "internal: a DPM step without its schedule table or history buffer");
    HIPCHK(launch_step_begin_sched(c->unet.ss_table, c->unet.ss_stride, pl->step_state, pl->cur_ss, tl, s, pl->zero_ptr, pl->zero_bytes,
                                   c->merge_advance, &sm.dpm->t, (int)(sizeof(DpmStep) / sizeof(int))));
  } else {
    HIPCHK(launch_step_begin(c->unet.ss_table, c->unet.ss_stride, pl->step_state, pl->cur_ss, tl, s, pl->zero_ptr, pl->zero_bytes, c->merge_advance,
                             sm.kind == SAMPLER_DDIM ? sm.ddim : nullptr));
  }
  LDCCHK(run_ops(c, pl, true, s));
  const uint64_t* keys = nullptr;   // the item-seeded update (never a windows plan, never DPM: the entries refuse)
  if (sm.item_seeds) {
    if (!pl->item_keys || pl->win_id || sm.kind == SAMPLER_DPM) return fail(LDC_E_STATE, "internal: an item-seeded step without its key table");
    keys = pl->item_keys;
  }
  if (pl->win_id) {   // coupled windows: x is the recordings' packed state, the blend and the update are one launch (the tape and the DPM history are packed like x, the keys are in the recording table)
    if (h.n != 1) return fail(LDC_E_STATE, "internal: a windows plan steps as one part");
    if (sm.kind == SAMPLER_DPM)
      HIPCHK(launch_windows_group_dpm_update(c->dt, x, pl->eps_cl, pl->x0_prev, pl->x_cl, c->unet.channels, pl->wg, c->sched, sm.dpm, pl->step_state, s));
    else
      HIPCHK(launch_windows_group_update(c->dt, sm.kind == SAMPLER_DDIM ? WIN_DDIM : WIN_DDPM, x, pl->eps_cl, noise, noise_stride, pl->x_cl, nullptr,
                                         c->unet.channels, pl->wg, c->sched, sm.ddim, pl->step_state, s));
  } else if (sm.kind == SAMPLER_DPM)
    HIPCHK(launch_dpm_update(c->dt, x + off, pl->eps_cl, pl->x0_prev, pl->x_cl, pl->B, c->unet.channels, pl->L, c->sched, sm.dpm,
                             pl->step_state, s, pl->ragged ? pl->lens : nullptr));
  else if (sm.kind == SAMPLER_DDIM)
    HIPCHK(launch_ddim_update(c->dt, x + off, pl->eps_cl, noise ? noise + off : nullptr, noise_stride, pl->x_cl, pl->B,
                              c->unet.channels, pl->L, c->sched, sm.ddim, pl->step_state, (uint64_t)off, s, pl->ragged ? pl->lens : nullptr, keys));
  else
    HIPCHK(launch_p_sample_update(c->dt, x + off, pl->eps_cl, noise ? noise + off : nullptr, noise_stride, pl->x_cl, pl->B,
                                  c->unet.channels, pl->L, c->sched, pl->step_state, (uint64_t)off, s, pl->ragged ? pl->lens : nullptr, keys));
  if (!c->merge_advance) HIPCHK(launch_step_advance(pl->step_state, tl, s));   // (LDC_STEP_ADVANCE_LAUNCH: the round-4 structure, for A/B runs)
  return LDC_OK;
}
// timeline runs: the end stamp of a loop's last step (every other step's is taken by the next step's first kernel)
static int stamp_loop_end(ldc_ctx* c, const Halves& h, int k, hipStream_t s) {
  if (!c->timeline || !c->merge_advance) return LDC_OK;
  HIPCHK(launch_step_advance(h.p[k]->step_state, c->tl_buf + (size_t)k * 2048 * 2, s));
  return LDC_OK;
}

bool parts_parallel(ldc_ctx* c, const Halves& h) {
  return h.n >= 2 && !c->profile && !c->serial_parts;   // LDC_SERIAL (diagnostics): parts back to back, eager
}
// the parts' streams pick up after everything queued on s / s waits for every part
int fork_parts(ldc_ctx* c, const Halves& h, hipStream_t s) {
  HIPCHK(hipEventRecord(c->ev_fork, s));
  for (int k = 1; k < h.n; ++k) HIPCHK(hipStreamWaitEvent(c->aux_stream[k], c->ev_fork, 0));
  return LDC_OK;
}
int join_parts(ldc_ctx* c, const Halves& h, hipStream_t s) {
  for (int k = 1; k < h.n; ++k) {
    HIPCHK(hipEventRecord(c->ev_join[k], c->aux_stream[k]));
    HIPCHK(hipStreamWaitEvent(s, c->ev_join[k], 0));
  }
  return LDC_OK;
}
// the state BEFORE the first step of a loop that starts at timestep t, iteration j (half_step's first kernel advances)
static int set_steps(ldc_ctx* c, const Halves& h, int t, int j, hipStream_t s) {
  for (int k = 0; k < h.n; ++k) HIPCHK(launch_step_set(h.p[k]->step_state, t + c->merge_advance, j - c->merge_advance, c->cur_key, s));
  return LDC_OK;
}

// one step of every part, eagerly: part 0 on s, the others on the auxiliary streams, joined at the end
static int one_step(ldc_ctx* c, const Halves& h, float* x, const float* noise, int64_t noise_stride, hipStream_t s,
                    const StepSampler& sm = StepSampler()) {
  if (parts_parallel(c, h)) {
    LDCCHK(fork_parts(c, h, s));
    for (int k = 0; k < h.n; ++k) LDCCHK(half_step(c, h, k, x, noise, noise_stride, k == 0 ? s : c->aux_stream[k], sm));
    LDCCHK(join_parts(c, h, s));
  } else {
    for (int k = 0; k < h.n; ++k) LDCCHK(half_step(c, h, k, x, noise, noise_stride, s, sm));
  }
  return LDC_OK;
}

extern "C" int ldc_p_sample(ldc_ctx* c, float* x, int t, const float* cond, const float* noise, int B, int L, int F,
                            void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!x || !cond) return fail(LDC_E_INVALID, "null tensor");
  if (t < 0 || t >= c->unet.timesteps) return fail(LDC_E_INVALID, "t out of range");
  LDCCHK(check_unet_args(c, B, L, F));
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(load_cond(c, h, cond, s));
  LDCCHK(load_x(c, h, x, s));
  next_noise_key(c, noise == nullptr && t > 0);
  LDCCHK(set_steps(c, h, t, 0, s));
  LDCCHK(one_step(c, h, x, noise, 0, s));
  return finish_stream(c, stream);
}

// the denoise loop on prepared plans (cond already processed, x_cl already set)
// left_forked (optional): the caller continues per part on the parts' streams; the per-part replay path then leaves them un-joined and says so
// sm (optional): SAMPLER_DDIM / SAMPLER_DPM: n_steps iterations on the schedule already written to c->ddim_table / c->dpm_table (DPM:
// the parts' history buffers exist, ensure_history); else DDPM steps from t = n_steps - 1 down to 0
int denoise_loop(ldc_ctx* c, const Halves& h, int B, float* x, const float* noise, int n_steps, hipStream_t s, bool* left_forked, const StepSampler& sm) {
  if (left_forked) *left_forked = false;
  const bool strided = sm.kind != SAMPLER_DDPM;   // a strided schedule, DDIM or DPM: the graph lengths below are theirs alike
  const int L = h.p[0]->L, F = h.p[0]->F;
  const int wl = h.p[0]->win_Ltot, wid = h.p[0]->win_id;   // a coupled-windows plan: graphs of that plan alone, the packed noise tape of wl frames (all its recordings')
  const int64_t stride = wl ? (int64_t)c->unet.channels * wl : (int64_t)B * c->unet.channels * L;
  LDCCHK(set_steps(c, h, n_steps - 1, 0, s));   // (DDIM: t is overwritten from the table in every step's first kernel)
  if (c->profile || c->serial_parts || n_steps < 3) {
    if (left_forked && h.n >= 2) LDCCHK(join_parts(c, h, s));   // (the caller's per-part work is on the auxiliary streams; these steps may all run on s)
    for (int i = 0; i < n_steps; ++i) LDCCHK(one_step(c, h, x, noise, stride, s, sm));
    for (int k = 0; k < h.n; ++k) LDCCHK(stamp_loop_end(c, h, k, s));
    return LDC_OK;
  }
  // the steps of ragged plans and of a coupled-windows plan are graphs of their own; a loop never replays another sampler's graph (DDPM,
  // DDIM, DPM): all stay cached side by side
  StepGraphKey key;
  key.B = B; key.L = L; key.F = F; key.sampler = sm.kind; key.ragged = h.p[0]->ragged ? 1 : 0; key.win_id = wid;
  key.seeded = sm.item_seeds ? 1 : 0;
  StepGraph* sg = nullptr;
  LDCCHK(step_graph_for(c, key, &sg));
  const bool par = parts_parallel(c, h);
  int K = 1;
  LDCCHK(ldc_graph_schedule(n_steps, h.n, strided, c->graph_steps, &K, nullptr, nullptr));
  const StepGraphBinding want{x, noise, s, h.n, K, step_graphs_per_part(c, h)};
  int done = 0;
  if (!sg->built || !(sg->bound == want)) {
    if (sg->built) {
      // replays of the old executable graphs may still be in flight: drain before destroying (a re-capture is one of
      // the documented places where a call waits for the device)
      HIPCHK(counted_device_sync());
      sg->destroy();
    }
    // first step eagerly: loads code objects / sets function attributes outside of the capture
    LDCCHK(one_step(c, h, x, noise, stride, s, sm));
    done = 1;
    LDCCHK(build_step_graphs(c, h, sg, K, want.per_part, par, s, [&](int k, hipStream_t sk) { return half_step(c, h, k, x, noise, stride, sk, sm); }));
    sg->bound = want;
  }
  const int left = n_steps - done, n_big = left / K, n_rep = n_big + (left - n_big * K);   // (ldc_graph_schedule's counts, for the steps that are left)
  if (sg->bound.per_part) {
    LDCCHK(fork_parts(c, h, s));
    // (a failure between fork and join must still join: the auxiliary streams would otherwise be left with work that is unordered
    // against the caller's stream -- ADVICE r4.  Note for asynchronous callers: the look-ahead wait blocks the HOST for up to
    // `depth` replays of a part, on events of this context.)
    const char* what = "";
    hipError_t err = replay_parts(c, h, sg, n_big, n_rep, K == 1, s, &what);
    for (int k = 0; k < h.n && err == hipSuccess; ++k)
      if (stamp_loop_end(c, h, k, k == 0 ? s : c->aux_stream[k]) != LDC_OK) { err = hipErrorUnknown; what = "the loop-end stamp"; }
    if (err == hipSuccess && left_forked) {   // the caller's per-part work follows on the same streams and joins behind it
      *left_forked = true;
      return LDC_OK;
    }
    const int jr = join_parts(c, h, s);
    if (err != hipSuccess) return fail(LDC_E_HIP, "%s failed in the per-part graph replay: %s", what, hipGetErrorString(err));
    return jr;
  }
  // The fork / join graph is launched on s ALONE: its part branches are graph nodes, not aux_stream[k].  A caller that arrives with the parts
  // forked (ldc_decode's per-part front ends, left_forked != null) still has work of parts k >= 1 on the auxiliary streams that nothing
  // orders in front of the replay unless the eager first step above ran (it joins): from the second decode of a shape on it does not
  // (the replayed step kernels raced with part k's front end writing cond / x_cl / x).
  if (left_forked && par) LDCCHK(join_parts(c, h, s));
  LDCCHK(replay_joined(c, sg, n_big, n_rep, K == 1, s));
  for (int k = 0; k < h.n; ++k) LDCCHK(stamp_loop_end(c, h, k, s));
  return LDC_OK;
}

static int ensure_state(ldc_ctx* c, size_t bytes) {
  if (bytes <= c->state_bytes) return LDC_OK;
  HIPCHK(counted_device_sync());
  if (c->state_buf) HIPCHK(hipFree(c->state_buf));
  c->state_buf = nullptr; c->state_bytes = 0;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, bytes));
  c->state_buf = (float*)p; c->state_bytes = bytes;
  return LDC_OK;
}

extern "C" int ldc_denoise(ldc_ctx* c, float* img, const float* cond, const float* noise, int n_steps, int B, int L, int F,
                           void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  if (n_steps < 1 || n_steps > c->unet.timesteps) return fail(LDC_E_INVALID, "n_steps must be in [1,%d]", c->unet.timesteps);
  LDCCHK(check_unet_args(c, B, L, F));
  hipStream_t s = pick_stream(c, stream);
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(load_cond(c, h, cond, s));
  // the loop runs on a context-owned copy of the state: the captured step graphs hold its address, so callers may
  // pass a different tensor every time without forcing a re-capture
  const size_t nbytes = (size_t)B * c->unet.channels * L * 4;
  LDCCHK(ensure_state(c, nbytes));
  HIPCHK(hipMemcpyAsync(c->state_buf, img, nbytes, hipMemcpyDeviceToDevice, s));
  LDCCHK(load_x(c, h, c->state_buf, s));
  next_noise_key(c, noise == nullptr);
  LDCCHK(denoise_loop(c, h, B, c->state_buf, noise, n_steps, s));
  HIPCHK(hipMemcpyAsync(img, c->state_buf, nbytes, hipMemcpyDeviceToDevice, s));
  return finish_stream(c, stream);
}

// GaussianDiffusion1D.p_sample_loop (ddpm_loss.py:253-266): ancestral sampling over ALL timesteps from a standard
// normal start.  img == NULL on entry is not allowed: the caller passes the buffer; fill_start != 0 draws the start
// image on the device (Philox stream 0xffffffff), otherwise the buffer's contents are the start image (parity runs).
extern "C" int ldc_p_sample_loop(ldc_ctx* c, float* img, const float* cond, const float* noise, int fill_start, int B, int L,
                                 int F, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  LDCCHK(check_unet_args(c, B, L, F));
  hipStream_t s = pick_stream(c, stream);
  next_noise_key(c, noise == nullptr || fill_start);
  if (fill_start) HIPCHK(launch_random_fill(img, (int64_t)B * c->unet.channels * L, 0, c->cur_key, 0xffffffffu, s));
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(load_cond(c, h, cond, s));
  const size_t nbytes = (size_t)B * c->unet.channels * L * 4;
  LDCCHK(ensure_state(c, nbytes));
  HIPCHK(hipMemcpyAsync(c->state_buf, img, nbytes, hipMemcpyDeviceToDevice, s));
  LDCCHK(load_x(c, h, c->state_buf, s));
  LDCCHK(denoise_loop(c, h, B, c->state_buf, noise, c->unet.timesteps, s));
  HIPCHK(hipMemcpyAsync(img, c->state_buf, nbytes, hipMemcpyDeviceToDevice, s));
  return finish_stream(c, stream);
}

// GaussianDiffusion1D.infilling (ddpm_loss.py:331-367): for t = midway_t-1 .. 0
//   img <- p_sample(img, t); img <- (1-lam) img + lam infill; infill <- p_sample(infill, t); img <- (1-lam) img + lam infill
// `noise` (optional, parity runs): [2*midway_t][B][C][L], draw 2*i for img and 2*i+1 for infill at iteration i.
// fill_start != 0 draws the uniform [0,1) start image of ddpm_loss.py:336 on the device.
extern "C" int ldc_infilling(ldc_ctx* c, float* img, float* infill_img, const float* cond, int midway_t, const float* noise,
                             float lam, int fill_start, int B, int L, int F, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!img || !infill_img || !cond) return fail(LDC_E_INVALID, "null tensor");
  if (midway_t < 1 || midway_t > c->unet.timesteps) return fail(LDC_E_INVALID, "midway_t must be in [1,%d]", c->unet.timesteps);
  LDCCHK(check_unet_args(c, B, L, F));
  hipStream_t s = pick_stream(c, stream);
  const int64_t n = (int64_t)B * c->unet.channels * L;
  next_noise_key(c, noise == nullptr || fill_start);
  if (fill_start) HIPCHK(launch_random_fill(img, n, 1, c->cur_key, 0xfffffffeu, s));
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(load_cond(c, h, cond, s));
  int draw = 0;
  for (int t = midway_t - 1; t >= 0; --t) {
    LDCCHK(load_x(c, h, img, s));
    LDCCHK(set_steps(c, h, t, draw++, s));
    LDCCHK(one_step(c, h, img, noise, n, s));
    HIPCHK(launch_axpby(img, infill_img, 1.0f - lam, lam, n, s));
    LDCCHK(load_x(c, h, infill_img, s));
    LDCCHK(set_steps(c, h, t, draw++, s));
    LDCCHK(one_step(c, h, infill_img, noise, n, s));
    HIPCHK(launch_axpby(img, infill_img, 1.0f - lam, lam, n, s));
  }
  return finish_stream(c, stream);
}

// ---- DDIM sampling (GaussianDiffusion1D.ddim_sample, ddpm_loss.py:268-303, with clip_denoised) from any t_start <= timesteps ----
// times = reversed(torch.linspace(-1, t_start - 1, n_steps + 1).int()).  ATen's float32 linspace computes the first half forwards
// from the start and the second half backwards from the end (step = (end - start) / (n - 1), all in float32); .int() truncates
// toward zero.  Host-only: needs no context.
extern "C" int ldc_ddim_times(int t_start, int n_steps, int* times_out) {
#pragma clang fp contract(off)
  if (!times_out) return fail(LDC_E_INVALID, "null output");
  if (t_start < 1) return fail(LDC_E_INVALID, "t_start must be >= 1");
  if (n_steps < 1 || n_steps > t_start) return fail(LDC_E_INVALID, "n_steps must be in [1, t_start = %d] (more would repeat timesteps)", t_start);
  const int n = n_steps + 1, half = n / 2;
  const float a = -1.0f, b = (float)(t_start - 1);
  const float step = (b - a) / (float)(n - 1);
  for (int i = 0; i < n; ++i) {
    const float v = i < half ? a + step * (float)i : b - step * (float)(n - 1 - i);
    times_out[n - 1 - i] = (int)v;
  }
  return LDC_OK;
}

// the per-iteration coefficients of a DDIM schedule into `out` (n_steps entries); float32 in the reference's order of operations.
// *draws: some sigma > 0.  The context's samplers fill c->ddim_host (ddim_schedule below), a decode pool the row of one slot.
int ddim_schedule_fill(ldc_ctx* c, int t_start, int n_steps, float eta, std::vector<DdimStep>* out, bool* draws) {
  if (!(eta >= 0.0f && eta <= 1.0f)) return fail(LDC_E_INVALID, "eta must be a finite value in [0, 1]");
  if (t_start < 1 || t_start > c->unet.timesteps) return fail(LDC_E_INVALID, "t_start must be in [1,%d]", c->unet.timesteps);
  if (n_steps < 1 || n_steps > t_start) return fail(LDC_E_INVALID, "n_steps must be in [1, t_start = %d] (more would repeat timesteps)", t_start);
  if ((int)c->alphas_cumprod.size() != c->unet.timesteps) return fail(LDC_E_STATE, "no alphas_cumprod schedule loaded");
  std::vector<int> times(n_steps + 1);
  LDCCHK(ldc_ddim_times(t_start, n_steps, times.data()));
  const std::vector<float>& ac = c->alphas_cumprod;
  out->assign(n_steps, DdimStep{});
  *draws = false;
  for (int j = 0; j < n_steps; ++j) {
    DdimStep& e = (*out)[j];
    const int t = times[j], tn = times[j + 1];
    e.t = t;
    e.last = tn < 0;
    if (e.last) continue;
    const float alpha = ac[t], alpha_next = ac[tn];
    const float sigma = eta * std::sqrt((1.0f - alpha / alpha_next) * (1.0f - alpha_next) / (1.0f - alpha));
    e.sigma = sigma;
    e.c = std::sqrt(std::max(0.0f, 1.0f - alpha_next - sigma * sigma));   // (>= 0 for eta <= 1; the clamp only absorbs rounding)
    e.sqrt_an = std::sqrt(alpha_next);
    *draws = *draws || sigma > 0.0f;
  }
  return LDC_OK;
}
int ddim_schedule(ldc_ctx* c, int t_start, int n_steps, float eta, bool* draws) {
  return ddim_schedule_fill(c, t_start, n_steps, eta, &c->ddim_host, draws);
}

// c->ddim_host -> the context's device table, ordered on s behind everything queued there before (earlier calls' replays read it)
int ddim_upload(ldc_ctx* c, hipStream_t s) {
  if (!c->ddim_table) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, (size_t)(c->unet.timesteps + 1) * sizeof(DdimStep)));
    c->ddim_table = (DdimStep*)p;
  }
  HIPCHK(launch_ddim_table_write(c->ddim_table, c->ddim_host.data(), (int)c->ddim_host.size(), s));
  return LDC_OK;
}

// DDIM over prepared arguments, as ldc_p_sample_loop: fill_start draws the N(0,1) start image on the device (Philox stream
// 0xfffffffd); `noise` (optional, parity runs) [n_steps][B][C][L], entry j for iteration j (the last one is not read)
extern "C" int ldc_ddim_sample(ldc_ctx* c, float* img, const float* cond, const float* noise, int fill_start, int t_start, int n_steps,
                               float eta, int B, int L, int F, void* stream) {
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  LDCCHK(check_unet_args(c, B, L, F));
  bool draws = false;
  LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  hipStream_t s = pick_stream(c, stream);
  LDCCHK(ddim_upload(c, s));
  next_noise_key(c, (noise == nullptr && draws) || fill_start);
  if (fill_start) HIPCHK(launch_random_fill(img, (int64_t)B * c->unet.channels * L, 0, c->cur_key, 0xfffffffdu, s));
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(load_cond(c, h, cond, s));
  const size_t nbytes = (size_t)B * c->unet.channels * L * 4;
  LDCCHK(ensure_state(c, nbytes));
  HIPCHK(hipMemcpyAsync(c->state_buf, img, nbytes, hipMemcpyDeviceToDevice, s));
  LDCCHK(load_x(c, h, c->state_buf, s));
  StepSampler sm;
  sm.kind = SAMPLER_DDIM;
  sm.ddim = c->ddim_table;
  LDCCHK(denoise_loop(c, h, B, c->state_buf, noise, n_steps, s, nullptr, sm));
  HIPCHK(hipMemcpyAsync(img, c->state_buf, nbytes, hipMemcpyDeviceToDevice, s));
  return finish_stream(c, stream);
}

// ---- DPM-Solver++(2M), data-prediction form: second-order multistep on the timestep grid of DDIM -------------
// Per timestep t, from the checkpoint's fp32 tables promoted to double: R = sqrt_recip_alphas_cumprod[t] = 1 / alpha,
// M = sqrt_recipm1_alphas_cumprod[t] = sigma / alpha, lambda = -ln M.  (The x0 formula uses these two tables, so x = alpha x0 + sigma eps
// inverts it exactly; 1 - alphas_cumprod in fp32 loses three digits at small t.)  Row j for (t, tn) = (times[j], times[j + 1]):
// tn < 0: (0, 1, 0), x <- x0.  Else h = lambda_tn - lambda_t, phi = -alpha_tn expm1(-h), a = sigma_tn / sigma_t; j = 0: (a, phi, 0);
// j >= 1: r = (lambda_t - lambda_times[j-1]) / h, (a, phi (1 + 1/(2r)), -phi / (2r)).  Double arithmetic, rounded once to float.
static int dpm_args(int timesteps, int t_start, int n_steps) {
  if (t_start < 1 || t_start > timesteps) return fail(LDC_E_INVALID, "t_start %d: must be in [1,%d]", t_start, timesteps);
  if (n_steps < 1 || n_steps > t_start) return fail(LDC_E_INVALID, "n_steps %d: must be in [1, t_start = %d] (more would repeat timesteps)", n_steps, t_start);
  return LDC_OK;
}
extern "C" int ldc_dpm_schedule(const float* sqrt_recip, const float* sqrt_recipm1, int timesteps, int t_start, int n_steps, int* t_out,
                                float* coef_out) {
  if (!sqrt_recip || !sqrt_recipm1 || !t_out || !coef_out) return fail(LDC_E_INVALID, "null pointer");
  if (timesteps < 1) return fail(LDC_E_INVALID, "timesteps %d: must be >= 1", timesteps);
  LDCCHK(dpm_args(timesteps, t_start, n_steps));
  std::vector<int> times(n_steps + 1);
  LDCCHK(ldc_ddim_times(t_start, n_steps, times.data()));
  auto alpha = [&](int t) { return 1.0 / (double)sqrt_recip[t]; };
  auto sigma = [&](int t) { return (double)sqrt_recipm1[t] / (double)sqrt_recip[t]; };
  auto lambda = [&](int t) { return -std::log((double)sqrt_recipm1[t]); };
  for (int j = 0; j < n_steps; ++j) {
    const int t = times[j], tn = times[j + 1];
    if (t < 0 || t >= timesteps || tn >= t) return fail(LDC_E_INVALID, "internal: timestep list is not strictly decreasing inside [0,%d)", timesteps);
    t_out[j] = t;
    float* row = coef_out + (size_t)j * 3;
    if (tn < 0) { row[0] = 0.f; row[1] = 1.f; row[2] = 0.f; continue; }
    const double h = lambda(tn) - lambda(t);
    const double phi = -alpha(tn) * std::expm1(-h);
    row[0] = (float)(sigma(tn) / sigma(t));
    if (j == 0) {
      row[1] = (float)phi;
      row[2] = 0.f;
    } else {
      const double r = (lambda(t) - lambda(times[j - 1])) / h;
      row[1] = (float)(phi * (1.0 + 0.5 / r));
      row[2] = (float)(-phi * 0.5 / r);
    }
  }
  return LDC_OK;
}

// the schedule of a DPM call into `out` (n_steps entries), from the context's host copies of the two tables.  The context's samplers
// fill c->dpm_host (dpm_schedule below), a decode pool the row of one slot.
int dpm_schedule_fill(ldc_ctx* c, int t_start, int n_steps, std::vector<DpmStep>* out) {
  const int T = c->unet.timesteps;
  LDCCHK(dpm_args(T, t_start, n_steps));
  if ((int)c->sqrt_recip_ac.size() != T || (int)c->sqrt_recipm1_ac.size() != T) return fail(LDC_E_STATE, "no sqrt_recip / sqrt_recipm1 schedule loaded");
  std::vector<int> ts(n_steps);
  std::vector<float> coef((size_t)n_steps * 3);
  LDCCHK(ldc_dpm_schedule(c->sqrt_recip_ac.data(), c->sqrt_recipm1_ac.data(), T, t_start, n_steps, ts.data(), coef.data()));
  out->assign(n_steps, DpmStep{});
  for (int j = 0; j < n_steps; ++j) {
    DpmStep& e = (*out)[j];
    e.t = ts[j];
    e.last = j == n_steps - 1;   // (the timestep list ends in -1: the final iteration, and only it)
    e.has_prev = j >= 1 && !e.last;
    e.a = coef[(size_t)j * 3]; e.b0 = coef[(size_t)j * 3 + 1]; e.b1 = coef[(size_t)j * 3 + 2];
  }
  return LDC_OK;
}
int dpm_schedule(ldc_ctx* c, int t_start, int n_steps) { return dpm_schedule_fill(c, t_start, n_steps, &c->dpm_host); }

// c->dpm_host -> the context's device table, ordered on s behind everything queued there before (as ddim_upload)
int dpm_upload(ldc_ctx* c, hipStream_t s) {
  if (!c->dpm_table) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, (size_t)(c->unet.timesteps + 1) * sizeof(DpmStep)));
    c->dpm_table = (DpmStep*)p;
  }
  HIPCHK(launch_dpm_table_write(c->dpm_table, c->dpm_host.data(), (int)c->dpm_host.size(), s));
  return LDC_OK;
}

// The history buffers of the parts' plans: allocated by the first DPM call on a plan, outside of any capture, and kept until the plan
// goes (evict_plan, ldc_destroy), so every captured DPM graph of the plan keeps a valid address.  Never cleared: the first iteration
// of a loop does not load it.
int ensure_history(ldc_ctx* c, const Halves& h) {
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    if (pl->x0_prev) continue;
    void* p = nullptr;
    const size_t bytes = (size_t)pl->B * c->unet.channels * pl->L * 4;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(LDC_E_NOMEM, "hipMalloc(%zu) for the DPM history failed: %s", bytes, hipGetErrorString(e));
    pl->x0_prev = (float*)p;
  }
  return LDC_OK;
}

// DPM-Solver++(2M) over prepared arguments, as ldc_ddim_sample with fill_start 0: deterministic, nothing is drawn, the Philox epoch
// stays where it is
extern "C" int ldc_dpm_sample(ldc_ctx* c, float* img, const float* cond, int t_start, int n_steps, int B, int L, int F, void* stream) {
  if (t_start < 1) return fail(LDC_E_INVALID, "t_start %d: must be >= 1", t_start);
  if (n_steps < 1 || n_steps > t_start) return fail(LDC_E_INVALID, "n_steps %d: must be in [1, t_start = %d] (more would repeat timesteps)", n_steps, t_start);
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  LDCCHK(check_unet_args(c, B, L, F));
  LDCCHK(dpm_schedule(c, t_start, n_steps));
  hipStream_t s = pick_stream(c, stream);
  LDCCHK(dpm_upload(c, s));
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(ensure_history(c, h));
  LDCCHK(load_cond(c, h, cond, s));
  const size_t nbytes = (size_t)B * c->unet.channels * L * 4;
  LDCCHK(ensure_state(c, nbytes));
  HIPCHK(hipMemcpyAsync(c->state_buf, img, nbytes, hipMemcpyDeviceToDevice, s));
  LDCCHK(load_x(c, h, c->state_buf, s));
  StepSampler sm;
  sm.kind = SAMPLER_DPM;
  sm.dpm = c->dpm_table;
  LDCCHK(denoise_loop(c, h, B, c->state_buf, nullptr, n_steps, s, nullptr, sm));
  HIPCHK(hipMemcpyAsync(img, c->state_buf, nbytes, hipMemcpyDeviceToDevice, s));
  return finish_stream(c, stream);
}

// ---- item seeds ("Item seeds") ----------------------------------------------------------------------------------
// The key tables of the parts' plans: allocated by the first seeded call on a plan, outside of any capture, and kept until the plan goes
// (as ensure_history's buffers), so every captured seeded graph of the plan keeps a valid address.  The keys of THIS call go in on s in
// front of the loop (the parts' streams fork from s behind them): seeds are data, a graph captured under one set serves any other.
int write_item_keys(ldc_ctx* c, const Halves& h, const uint64_t* seeds, hipStream_t s) {
  for (int k = 0; k < h.n; ++k) {
    Plan* pl = h.p[k];
    if (!pl->item_keys) {
      void* p = nullptr;
      const size_t bytes = (size_t)pl->B * sizeof(uint64_t);
      hipError_t e = hipMalloc(&p, bytes);
      if (e != hipSuccess) return fail(LDC_E_NOMEM, "hipMalloc(%zu) for the item keys failed: %s", bytes, hipGetErrorString(e));
      pl->item_keys = (uint64_t*)p;
    }
    HIPCHK(launch_item_keys_write(pl->item_keys, seeds + h.b0[k], pl->B, s));
  }
  return LDC_OK;
}

// ldc_denoise (sampler 0: n_steps DDPM steps from t = n_steps - 1, t_start and eta are not read) / ldc_ddim_sample (sampler 1) on a given
// start image, item b drawing under seeds[b] as if alone; the context's noise epoch is neither read nor advanced
extern "C" int ldc_sample_seeded(ldc_ctx* c, float* img, const float* cond, int sampler, int t_start, int n_steps, float eta, const uint64_t* seeds,
                                 int B, int L, int F, void* stream) {
  LDCCHK(seeded_args(sampler, seeds));
  LDCCHK(check_ready(c, LDC_MODEL_MAIN));
  if (!img || !cond) return fail(LDC_E_INVALID, "null tensor");
  if (sampler == SAMPLER_DDPM && (n_steps < 1 || n_steps > c->unet.timesteps))
    return fail(LDC_E_INVALID, "n_steps %d: must be in [1,%d]", n_steps, c->unet.timesteps);
  LDCCHK(check_unet_args(c, B, L, F));
  bool draws = true;
  if (sampler == SAMPLER_DDIM) LDCCHK(ddim_schedule(c, t_start, n_steps, eta, &draws));
  hipStream_t s = pick_stream(c, stream);
  if (sampler == SAMPLER_DDIM) LDCCHK(ddim_upload(c, s));
  Halves h;
  LDCCHK(get_halves(c, B, L, F, s, &h));
  LDCCHK(write_item_keys(c, h, seeds, s));
  LDCCHK(load_cond(c, h, cond, s));
  const size_t nbytes = (size_t)B * c->unet.channels * L * 4;
  LDCCHK(ensure_state(c, nbytes));
  HIPCHK(hipMemcpyAsync(c->state_buf, img, nbytes, hipMemcpyDeviceToDevice, s));
  LDCCHK(load_x(c, h, c->state_buf, s));
  StepSampler sm;
  sm.kind = sampler;
  sm.ddim = sampler == SAMPLER_DDIM ? c->ddim_table : nullptr;
  sm.item_seeds = true;
  LDCCHK(denoise_loop(c, h, B, c->state_buf, nullptr, n_steps, s, nullptr, sm));
  HIPCHK(hipMemcpyAsync(img, c->state_buf, nbytes, hipMemcpyDeviceToDevice, s));
  return finish_stream(c, stream);
}
