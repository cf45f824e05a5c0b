// step_graphs.cpp -- step graphs: the graph-length rule, capture, the context's cache and the two replay paths (step_graphs.h).
// Host-side C++ only.
#include "ldc_internal.h"

// Steps per replayed graph.  The parts fork at the head of a graph and join at its tail, so K > 1 lets them drift apart for K steps
// (concurrent replays of SEPARATE graphs on different streams were measured: the ROCm 7.2 runtime serialises them, 198 vs 188 ms).
// ~1 500 kernel nodes per graph measured best in both arrangements: 5 steps of two chains (3 / 4 / 5 / 7 steps within 0.2 %,
// 10 / 25 steps 2 % / 16 % slower), 10 steps of a single chain (5 steps 2.8 % slower; 8 / 10 / 25 equal).  A remainder of
// single-step replays is slow (13 or 17 steps per graph: 154 instead of 124 ms), so the defaults prefer a graph length that divides the
// step count, within the flat part of the measured range.
// strided (DDIM, DPM): one graph length whatever the step count, so that every S and eta replays the same captured graphs (such a decode
// has a few to a few tens of steps: 5 steps per graph, and single-step replays for the remainder).
extern "C" int ldc_graph_schedule(int n_steps, int parts, int strided, int graph_steps_option, int* K_out, int* n_big_out, int* n_single_out) {
  if (n_steps < 1) return fail(LDC_E_INVALID, "n_steps %d: must be >= 1", n_steps);
  if (parts < 1 || parts > kMaxParts) return fail(LDC_E_INVALID, "parts %d: must be in [1, %d]", parts, kMaxParts);
  if (graph_steps_option < 0) return fail(LDC_E_INVALID, "graph_steps_option %d: must be >= 0 (0: by the number of parts)", graph_steps_option);
  int k_want = graph_steps_option > 0 ? graph_steps_option : (parts == 1 && !strided ? 10 : 5);
  if (!strided && graph_steps_option == 0) {
    const int lo = parts == 1 ? 8 : 3, hi = parts == 1 ? 25 : 7;
    int best = 0;
    for (int k = lo; k <= hi; ++k)
      if (n_steps % k == 0 && (best == 0 || std::abs(k - k_want) < std::abs(best - k_want))) best = k;
    if (best) k_want = best;
  }
  const int K = strided ? k_want : std::min(k_want, std::max(1, n_steps - 1));
  if (K_out) *K_out = K;
  if (n_big_out) *n_big_out = n_steps / K;
  if (n_single_out) *n_single_out = n_steps - n_steps / K * K;
  return LDC_OK;
}

bool step_graphs_per_part(ldc_ctx* c, const Halves& h) {
  return parts_parallel(c, h) && c->part_graphs && (h.n == 2 || c->part_graphs >= 2);
}

void StepGraph::destroy() {
  for (hipEvent_t e : part_ev) (void)hipEventDestroy(e);
  part_ev.clear();
  for (auto& e : exec) { if (e) (void)hipGraphExecDestroy(e); e = nullptr; }
  for (auto& pe : pexec) for (auto& e : pe) { if (e) (void)hipGraphExecDestroy(e); e = nullptr; }
  built = false;
}

int capture_steps(hipStream_t s, const std::function<int()>& body, hipGraphExec_t* out) {
  *out = nullptr;
  HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
  const int r = body();
  hipGraph_t g = nullptr;
  const hipError_t e_end = hipStreamEndCapture(s, &g);
  const hipError_t e_inst = (r == LDC_OK && e_end == hipSuccess) ? hipGraphInstantiate(out, g, nullptr, nullptr, 0) : hipSuccess;
  if (g) (void)hipGraphDestroy(g);
  if (r != LDC_OK) return r;
  if (e_end != hipSuccess) return fail(LDC_E_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e_end));
  if (e_inst != hipSuccess) { *out = nullptr; return fail(LDC_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e_inst)); }
  return LDC_OK;
}

int build_step_graphs(ldc_ctx* c, const Halves& h, StepGraph* sg, int K, bool per_part, bool par, hipStream_t s,
                      const std::function<int(int, hipStream_t)>& half_step) {
  const int n_graphs = K == 1 ? 1 : 2;   // (K == 1: the one-step graph is the long graph)
  int r = LDC_OK;
  if (per_part) {
    // ONE SINGLE-STREAM graph per batch part, captured and replayed on the part's own stream.  ROCm 7.2 replays a
    // single-stream graph from AQL packets recorded at instantiation (~0.4 ms of host time for 1 500 kernel nodes); a graph
    // that forks and joins streams inside takes the node-by-node path (~9 us per node: 140 ms of host time per 50-step decode
    // of two parts, which is then what bounds the decode).  The parts fork once in front of the loop and join once behind it.
    for (int k = 0; k < h.n && r == LDC_OK; ++k) {
      hipStream_t sk = k == 0 ? s : c->aux_stream[k];
      for (int which = 0; which < n_graphs && r == LDC_OK; ++which)
        r = capture_steps(sk, [&]() {
          int rr = LDC_OK;
          for (int i = 0; i < (which == 0 ? K : 1) && rr == LDC_OK; ++i) rr = half_step(k, sk);
          return rr;
        }, &sg->pexec[k][which]);
    }
  } else {
    // K steps (one step) of every part in one graph; the device-side step counters make every replay continue where the last one stopped
    for (int which = 0; which < n_graphs && r == LDC_OK; ++which)
      r = capture_steps(s, [&]() {
        int rr = par ? fork_parts(c, h, s) : LDC_OK;
        for (int k = 0; k < h.n && rr == LDC_OK; ++k)
          for (int i = 0; i < (which == 0 ? K : 1) && rr == LDC_OK; ++i) rr = half_step(k, (k == 0 || !par) ? s : c->aux_stream[k]);
        if (par && rr == LDC_OK) rr = join_parts(c, h, s);
        return rr;
      }, &sg->exec[which]);
  }
  // (a capture that fails midway drops the executables it has made: the entry stays unbuilt and the next call captures afresh)
  if (r != LDC_OK) sg->destroy();
  else sg->built = true;
  return r;
}

void drop_step_graphs(ldc_ctx* c, const std::function<bool(const StepGraph&)>& pred) {
  for (size_t g = 0; g < c->graphs.size();) {
    if (pred(c->graphs[g])) {
      c->graphs[g].destroy();
      c->graphs.erase(c->graphs.begin() + g);
    } else {
      ++g;
    }
  }
}

int step_graph_for(ldc_ctx* c, const StepGraphKey& key, StepGraph** out) {
  StepGraph* sg = nullptr;
  for (auto& g : c->graphs)
    if (g.key == key) sg = &g;
  if (!sg) {
    // graphs of shapes whose plans are gone were dropped with them (evict_plan); additionally keep at most 16 alive
    if (key.pool_id == 0 && c->graphs.size() >= 16) {
      const StepGraph* victim = nullptr;   // (a decode pool's graphs leave with the pool)
      for (const auto& g : c->graphs)
        if (g.key.pool_id == 0 && (!victim || g.last_use < victim->last_use)) victim = &g;
      if (victim) {
        HIPCHK(counted_device_sync());
        const StepGraphKey gone = victim->key;
        drop_step_graphs(c, [&](const StepGraph& g) { return g.key == gone; });
      }
    }
    c->graphs.push_back(StepGraph());
    sg = &c->graphs.back();
    sg->key = key;
  }
  sg->last_use = ++c->use_tick;
  *out = sg;
  return LDC_OK;
}

// The per-part graphs of sg replayed for n_rep rounds: pexec[k][0] (the K-step graph) for the first n_big rounds, pexec[k][1] (one step)
// for the rest (single_len: K == 1, pexec[k][0] throughout).  One single-stream graph per part, replayed from recorded AQL packets.  The
// parts' replays are issued INTERLEAVED (graph j of every part before graph j + 1 of any) behind a bounded look-ahead per part: through
// round 3 all of part 0's replays were issued first, hipGraphLaunch blocked on the full hardware queue for most of the decode (76-105 ms
// "inside hipGraphLaunch") and part 1 started late.  Waiting happens on events of this context, outside hipGraphLaunch.  The caller forks
// the parts in front and joins them behind, whatever this returns (*what names the call that failed).
hipError_t replay_parts(ldc_ctx* c, const Halves& h, StepGraph* sg, int n_big, int n_rep, bool single_len, hipStream_t s, const char** what) {
  const int depth = std::max(1, std::min(c->flow_depth > 0 ? c->flow_depth : 3, 3));
  std::vector<hipEvent_t>& evs = sg->part_ev;
  hipError_t err = hipSuccess;
  while ((int)evs.size() < h.n * depth && err == hipSuccess) {
    hipEvent_t e = nullptr;
    err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (err == hipSuccess) evs.push_back(e);
    else *what = "hipEventCreateWithFlags";
  }
  for (int j = 0; j < n_rep && err == hipSuccess; ++j)
    for (int k = 0; k < h.n && err == hipSuccess; ++k) {
      hipStream_t sk = k == 0 ? s : c->aux_stream[k];
      hipEvent_t ev = evs[(size_t)k * depth + j % depth];
      if (j >= depth) {
        const auto t0 = std::chrono::steady_clock::now();
        err = hipEventSynchronize(ev);   // replay j - depth of this part has finished
        c->host_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (err != hipSuccess) { *what = "hipEventSynchronize"; break; }
      }
      const auto t0 = std::chrono::steady_clock::now();
      err = hipGraphLaunch(sg->pexec[k][(j < n_big || single_len) ? 0 : 1], sk);
      c->host_graph_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      ++c->host_graph_launches;
      if (err != hipSuccess) { *what = "hipGraphLaunch"; break; }
      err = hipEventRecord(ev, sk);
      if (err != hipSuccess) *what = "hipEventRecord";
    }
  return err;
}

// The fork / join graphs of sg replayed n_rep times on s: exec[0] (K steps) for the first n_big, exec[1] (one step) for the rest (single_len:
// K == 1, exec[0] throughout).  Host time inside hipGraphLaunch is accounted (ldc_host_stats): with ~1 500 kernel nodes per replay it is
// what caps one process once the kernels get faster.  Flow control: ldc_ctx::flow_depth.
int replay_joined(ldc_ctx* c, StepGraph* sg, int n_big, int n_rep, bool single_len, hipStream_t s) {
  for (int j = 0; j < n_rep; ++j) {
    if (c->flow_depth > 0 && c->flow_n >= (unsigned long long)c->flow_depth) {
      const auto t0 = std::chrono::steady_clock::now();
      HIPCHK(hipEventSynchronize(c->flow_ev[(c->flow_n - c->flow_depth) % ldc_ctx::kFlowRing]));
      c->host_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipGraphLaunch(sg->exec[(j < n_big || single_len) ? 0 : 1], s);
    c->host_graph_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ++c->host_graph_launches;
    if (e != hipSuccess) return fail(LDC_E_HIP, "hipGraphLaunch failed in the fork / join graph replay: %s", hipGetErrorString(e));
    if (c->flow_depth > 0) {
      HIPCHK(hipEventRecord(c->flow_ev[c->flow_n % ldc_ctx::kFlowRing], s));
      ++c->flow_n;
    }
  }
  return LDC_OK;
}
