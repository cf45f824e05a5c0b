// step_graphs.h -- the step graphs every sampler loop ends in: denoise steps captured into HIP graphs once per shape and sampler, cached in
// the context, and replayed behind a bounded look-ahead.  Nothing here knows a sampler: the loops (ldc_api_sample.cpp: denoise_loop,
// ldc_api_pool.cpp: pool_steps) pass the one step of a batch part as a callable.  Included by ldc_internal.h, between the batch parts
// (Halves, kMaxParts) and the context that owns the cache.
#pragma once

struct ldc_ctx;

struct StepGraphKey {   // what a cache entry is found by
  int B = 0, L = 0, F = 0;
  int sampler = SAMPLER_DDPM;   // a loop never replays another kind's graph (DDIM, DPM: the schedule table's address is captured, not its contents)
  int ragged = 0;    // the steps of ragged plans
  int pool_id = 0;   // != 0: the step graphs of that decode pool's plans
  int win_id = 0;    // != 0: the steps of that coupled-windows plan (Plan::win_id)
  int seeded = 0;    // the item-seeded update launches (another kernel with another argument list: never replayed for an unseeded loop, nor the reverse)
  bool operator==(const StepGraphKey& o) const {
    return B == o.B && L == o.L && F == o.F && sampler == o.sampler && ragged == o.ragged && pool_id == o.pool_id && win_id == o.win_id &&
           seeded == o.seeded;
  }
};

struct StepGraphBinding {   // what a capture baked into the executables: a loop that arrives with another binding captures again
  float* x = nullptr;
  const float* noise = nullptr;
  hipStream_t stream = nullptr;
  int parts = 0, K = 0;     // batch parts, steps of the long graph
  bool per_part = false;    // one single-stream graph per part (pexec) instead of one fork / join graph (exec)
  bool operator==(const StepGraphBinding& o) const {
    return x == o.x && noise == o.noise && stream == o.stream && parts == o.parts && K == o.K && per_part == o.per_part;
  }
};

struct StepGraph {   // hipGraphs of {step_begin, unet step, p_sample_update | ddim_update | dpm_update, step_advance}; [0] = K steps, [1] = one step (none when K == 1)
  StepGraphKey key;
  StepGraphBinding bound;
  bool built = false;
  hipGraphExec_t exec[2] = {nullptr, nullptr};   // fork / join mode: every part in one graph
  hipGraphExec_t pexec[kMaxParts][2] = {};       // per-part mode: single-stream graphs
  std::vector<hipEvent_t> part_ev;               // per-part mode: look-ahead events [part][depth]
  uint64_t last_use = 0;
  void destroy();   // nothing of the entry may be running
};

// The one begin / end / instantiate sequence of the library: `body` (returns an LDC_* code) is captured on s into *out.  On any failure
// the capture is ended, the graph destroyed and *out left null.
int capture_steps(hipStream_t s, const std::function<int()>& body, hipGraphExec_t* out);
// The whole entry: per part, K steps and one step of part k on its own stream (s, aux_stream[k]); else K steps and one step of every part
// in one graph on s (par: the parts fork and join inside).  half_step(k, stream) is one step of part k.  A failure leaves the entry
// destroyed and unbuilt; the caller records the binding of a success in sg->bound.
int build_step_graphs(ldc_ctx* c, const Halves& h, StepGraph* sg, int K, bool per_part, bool par, hipStream_t s,
                      const std::function<int(int, hipStream_t)>& half_step);
// per-part graphs for this batch?  (two parts; "part_graphs" 2: three / four as well, measured 45 % slower than their fork / join graph)
bool step_graphs_per_part(ldc_ctx* c, const Halves& h);
// the entry of `key`, added if new and marked as used.  At most 16 entries outside of decode pools stay alive: a new one evicts the least
// recently used of them behind a device synchronisation (a pool's graphs leave with the pool)
int step_graph_for(ldc_ctx* c, const StepGraphKey& key, StepGraph** out);
// destroys and erases every entry `pred` selects; the caller has made sure that none of them is running
void drop_step_graphs(ldc_ctx* c, const std::function<bool(const StepGraph&)>& pred);
// n_rep rounds of the per-part graphs, the first n_big of them the K-step graph; the caller forks in front and joins behind (step_graphs.cpp)
hipError_t replay_parts(ldc_ctx* c, const Halves& h, StepGraph* sg, int n_big, int n_rep, bool single_len, hipStream_t s, const char** what);
// n_rep replays of the fork / join graphs on s behind the context's flow-control ring, the first n_big of them the K-step graph
int replay_joined(ldc_ctx* c, StepGraph* sg, int n_big, int n_rep, bool single_len, hipStream_t s);
