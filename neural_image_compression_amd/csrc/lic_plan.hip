// Launch plans: a captured training step replayed on TWO HIP streams without Python in the loop.
//
// The bf16 configurations are host-paced: a step is ~180 launches of 5-100 us, and the Python around each (autograd
// nodes, tensor allocation, ctypes) costs ~18 us -- 3.1 ms of a 3.8 ms step, against 0.7 ms inside this library and
// ~3 ms of GPU work.  HIP graphs remove the host cost, but this ROCm's executor walks a graph with more than one
// branch node by node from the host (measured: 0.09 ms enqueue / 4.47 ms for the single-stream capture of the
// step, 8 ms enqueue / 10 ms for the two-stream capture), and the step needs its two branches: the decoder beside
// the latent side, the weight gradients beside the data gradients.
// So the graph is used only as the RECORD of the step -- torch captures it (private memory pool: every pointer is
// the same on every replay), and lic_plan_create reads the nodes and edges back (hipGraphGetNodes / GetEdges /
// KernelNodeGetParams) into a list of operations with their predecessors.  A SCHEDULE puts the operations in an
// issue order, each on one of two streams, and keeps one event record + wait per cross-stream edge that stream
// order does not already imply.  lic_plan_replay issues a schedule with plain hipLaunchKernel / hipMemsetAsync /
// hipMemcpyAsync calls: ~3 us per operation of host time.
// Two schedules:
//   * capture order (lic_plan_create): topological, ties by creation order = the order the eager step launched in;
//     an operation continues the stream of a predecessor that is still that stream's tail, and one whose
//     predecessors' streams have all moved on starts the other stream -- the eager step's two branches again.
//   * tuned (lic_plan_tune): every operation is timed once (one-stream replay, an event between operations), then
//     list-scheduled by longest remaining path onto the stream where it finishes first, under a model of the GPU as
//     "kernels of >= 192 workgroups take turns, smaller ones run beside anything"; the tuned schedule is kept only
//     if it measures faster end to end than the capture-order one.
// Either way every edge of the capture is honoured (same-stream order or an event), so results are those of the
// eager step bit for bit.  Nothing here knows the model: any capture of kernel, memset, memcpy and empty nodes on
// one device works.
// The schedulers and the builder of the command list a replay walks are host code without HIP: lic_plan_sched.h.  This
// file reads the graph, issues the commands and measures; lic_plan_dag / lic_plan_commands / lic_plan_sched_host hand DAG
// and commands out as data, so that tests/plan_sched_ref.py can check "every edge is honoured" without a race to lose.
#include "lic_common.h"
#include "lic_plan_sched.h"
#include <cstring>

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <queue>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

struct PlanOp {
  hipGraphNodeType type;
  hipKernelNodeParams kp;  // (the argument storage belongs to the graph: the caller keeps the graph alive)
  hipMemsetParams ms;
  hipMemcpy3DParms mc;
};

// the schedules themselves are plain host code over the DAG: lic_plan_sched.h
using lic_sched::Cmd;
using lic_sched::Node;
using lic_sched::NS;
using lic_sched::Schedule;

}  // namespace

struct lic_plan {
  std::vector<PlanOp> ops;  // topological (capture) order
  std::vector<Node> dag;    // the same operations as the schedulers see them
  Schedule sched;
  std::vector<hipEvent_t> events;  // by the event ids of a command list: the fork, the two joins, the schedule's own
  int64_t count[4] = {0, 0, 0, 0};  // kernels, memsets, memcpys, empty
  int tuned = 0;
};

static thread_local std::string g_plan_error;

static int plan_fail(lic_plan* p, int rc, const std::string& why) {
  g_plan_error = why;
  if (p) lic_plan_destroy(p);
  return rc;
}

// events for a schedule with `n` events of its own (and the fork and the joins)
static bool ensure_events(lic_plan* p, int n) {
  while ((int)p->events.size() < lic_sched::EV_FIRST + n) {
    hipEvent_t ev;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return false;
    p->events.push_back(ev);
  }
  return true;
}

LIC_EXPORT const char* lic_plan_last_error(void) { return g_plan_error.c_str(); }

LIC_EXPORT int lic_plan_create(void* hip_graph, lic_plan** out) {
  if (!hip_graph || !out) return LIC_ERR_INVALID;
  *out = nullptr;
  hipGraph_t g = (hipGraph_t)hip_graph;
  size_t n = 0, ne = 0;
  if (hipGraphGetNodes(g, nullptr, &n) != hipSuccess || n == 0) return plan_fail(nullptr, LIC_ERR_INVALID, "hipGraphGetNodes failed or the graph is empty");
  std::vector<hipGraphNode_t> nodes(n);
  if (hipGraphGetNodes(g, nodes.data(), &n) != hipSuccess) return plan_fail(nullptr, LIC_ERR_INVALID, "hipGraphGetNodes failed");
  if (hipGraphGetEdges(g, nullptr, nullptr, &ne) != hipSuccess) return plan_fail(nullptr, LIC_ERR_INVALID, "hipGraphGetEdges failed");
  std::vector<hipGraphNode_t> from(ne), to(ne);
  if (ne && hipGraphGetEdges(g, from.data(), to.data(), &ne) != hipSuccess) return plan_fail(nullptr, LIC_ERR_INVALID, "hipGraphGetEdges failed");
  std::unordered_map<hipGraphNode_t, int> index;
  for (size_t i = 0; i < n; ++i) index[nodes[i]] = (int)i;
  std::vector<std::vector<int>> preds(n), succs(n);
  std::vector<int> indeg(n, 0);
  for (size_t e = 0; e < ne; ++e) {
    auto a = index.find(from[e]), b = index.find(to[e]);
    if (a == index.end() || b == index.end()) return plan_fail(nullptr, LIC_ERR_INVALID, "an edge names a node that is not in the graph");
    preds[b->second].push_back(a->second);
    succs[a->second].push_back(b->second);
    ++indeg[b->second];
  }
  // topological order, ties broken by creation (= capture) order: the order the eager step issued its launches in
  std::priority_queue<int, std::vector<int>, std::greater<int>> ready;
  for (size_t i = 0; i < n; ++i)
    if (indeg[i] == 0) ready.push((int)i);
  std::vector<int> order, rank(n, -1);
  order.reserve(n);
  while (!ready.empty()) {
    const int u = ready.top();
    ready.pop();
    rank[u] = (int)order.size();
    order.push_back(u);
    for (int v : succs[u])
      if (--indeg[v] == 0) ready.push(v);
  }
  if (order.size() != n) return plan_fail(nullptr, LIC_ERR_INVALID, "the graph has a cycle");

  lic_plan* p = new lic_plan();
  p->ops.resize(n);
  p->dag.resize(n);
  for (size_t k = 0; k < n; ++k) {
    const int u = order[k];
    PlanOp& op = p->ops[k];
    Node& nd = p->dag[k];
    for (int q : preds[u]) nd.preds.push_back(rank[q]);
    for (int q : succs[u]) nd.succs.push_back(rank[q]);
    if (hipGraphNodeGetType(nodes[u], &op.type) != hipSuccess) return plan_fail(p, LIC_ERR_INVALID, "hipGraphNodeGetType failed");
    switch (op.type) {
      case hipGraphNodeTypeKernel:
        if (hipGraphKernelNodeGetParams(nodes[u], &op.kp) != hipSuccess) return plan_fail(p, LIC_ERR_INVALID, "hipGraphKernelNodeGetParams failed");
        if (!op.kp.func || (!op.kp.kernelParams && !op.kp.extra)) return plan_fail(p, LIC_ERR_UNSUPPORTED, "a kernel node without a function or arguments");
        nd.wide = (long)op.kp.gridDim.x * op.kp.gridDim.y * op.kp.gridDim.z >= 192;
        if (const char* nm = hipKernelNameRefByPtr(op.kp.func, nullptr)) nd.filler = strstr(nm, "reduce_batch_kernel") != nullptr;
        ++p->count[0];
        break;
      case hipGraphNodeTypeMemset:
        if (hipGraphMemsetNodeGetParams(nodes[u], &op.ms) != hipSuccess) return plan_fail(p, LIC_ERR_INVALID, "hipGraphMemsetNodeGetParams failed");
        if (op.ms.height > 1) return plan_fail(p, LIC_ERR_UNSUPPORTED, "a 2-D memset node");
        ++p->count[1];
        break;
      case hipGraphNodeTypeMemcpy:
        if (hipGraphMemcpyNodeGetParams(nodes[u], &op.mc) != hipSuccess) return plan_fail(p, LIC_ERR_UNSUPPORTED, "a memcpy node whose parameters cannot be read back (1-D copy node)");
        if (getenv("LIC_PLAN_DEBUG"))
          fprintf(stderr, "[lic_plan] memcpy node %zu: src %p pitch %zu dst %p pitch %zu extent %zu x %zu x %zu kind %d\n", k,
                  op.mc.srcPtr.ptr, op.mc.srcPtr.pitch, op.mc.dstPtr.ptr, op.mc.dstPtr.pitch, op.mc.extent.width,
                  op.mc.extent.height, op.mc.extent.depth, (int)op.mc.kind);
        // (this ROCm answers hipSuccess for the 1-D copy node a captured hipMemcpyAsync becomes, with an unfilled struct)
        if (!op.mc.srcPtr.ptr || !op.mc.dstPtr.ptr || !op.mc.extent.width || (unsigned)op.mc.kind > (unsigned)hipMemcpyDefault ||
            op.mc.extent.width > ((size_t)1 << 40) || op.mc.extent.height > ((size_t)1 << 24) || op.mc.extent.depth > ((size_t)1 << 24))
          return plan_fail(p, LIC_ERR_UNSUPPORTED, "a memcpy node whose parameters this ROCm does not hand back (a captured hipMemcpyAsync: "
                                                   "a same-dtype contiguous tensor.copy_ / clone); replace the copy by a kernel");
        ++p->count[2];
        break;
      case hipGraphNodeTypeEmpty:
        ++p->count[3];
        break;
      default:
        return plan_fail(p, LIC_ERR_UNSUPPORTED, "node type " + std::to_string((int)op.type) + " (only kernel, memset, memcpy and empty nodes are replayed)");
    }
  }
  // the capture-order schedule (lic_plan_sched.h)
  p->sched = lic_sched::capture_order_schedule(p->dag);
  if (!ensure_events(p, p->sched.n_events)) return plan_fail(p, LIC_ERR_LAUNCH, "hipEventCreate failed");
  *out = p;
  return LIC_OK;
}

// info[0..6] = operations, kernels, memsets, memcpys, operations on the second stream, cross-stream events,
// 1 if the schedule in use is the tuned one
LIC_EXPORT int lic_plan_info(const lic_plan* p, int64_t* info) {
  if (!p || !info) return LIC_ERR_INVALID;
  info[0] = (int64_t)p->ops.size();
  info[1] = p->count[0];
  info[2] = p->count[1];
  info[3] = p->count[2];
  info[4] = p->sched.on_side;
  info[5] = p->sched.n_events;
  info[6] = p->tuned;
  return LIC_OK;
}

#define PLAN_TRY(expr)                                                                                          \
  do {                                                                                                          \
    const hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) {                                                                                     \
      g_lic_last_hip_error = (int)e_;                                                                           \
      g_plan_error = std::string(#expr) + " at operation " + std::to_string(k_) + ": " + hipGetErrorString(e_); \
      return LIC_ERR_LAUNCH;                                                                                    \
    }                                                                                                           \
  } while (0)

static int issue_op(const PlanOp& op, hipStream_t s, long k_) {
  switch (op.type) {
    case hipGraphNodeTypeKernel:
      if (op.kp.kernelParams) {
        PLAN_TRY(hipLaunchKernel(op.kp.func, op.kp.gridDim, op.kp.blockDim, op.kp.kernelParams, op.kp.sharedMemBytes, s));
      } else {
        PLAN_TRY(hipModuleLaunchKernel((hipFunction_t)op.kp.func, op.kp.gridDim.x, op.kp.gridDim.y, op.kp.gridDim.z,
                                       op.kp.blockDim.x, op.kp.blockDim.y, op.kp.blockDim.z, op.kp.sharedMemBytes, s,
                                       nullptr, op.kp.extra));
      }
      break;
    case hipGraphNodeTypeMemset:
      if (op.ms.elementSize == 4) PLAN_TRY(hipMemsetD32Async((hipDeviceptr_t)op.ms.dst, (int)op.ms.value, op.ms.width, s));
      else if (op.ms.elementSize == 2) PLAN_TRY(hipMemsetD16Async((hipDeviceptr_t)op.ms.dst, (unsigned short)op.ms.value, op.ms.width, s));
      else PLAN_TRY(hipMemsetD8Async((hipDeviceptr_t)op.ms.dst, (unsigned char)op.ms.value, op.ms.width, s));
      break;
    case hipGraphNodeTypeMemcpy:
      // (a one-row extent without pitches is what a 1-D copy looks like; hipMemcpy3DAsync refuses it)
      if (!op.mc.srcArray && !op.mc.dstArray && op.mc.extent.height <= 1 && op.mc.extent.depth <= 1 &&
          !op.mc.srcPos.x && !op.mc.srcPos.y && !op.mc.srcPos.z && !op.mc.dstPos.x && !op.mc.dstPos.y && !op.mc.dstPos.z)
        PLAN_TRY(hipMemcpyAsync(op.mc.dstPtr.ptr, op.mc.srcPtr.ptr, op.mc.extent.width, hipMemcpyDefault, s));
      else
        PLAN_TRY(hipMemcpy3DAsync(&op.mc, s));
      break;
    default:
      break;
  }
  return LIC_OK;
}

static int replay_schedule(lic_plan* p, Schedule& sc, hipStream_t main, const hipStream_t* sides, int n_sides) {
  // streams the caller did not provide fold onto the last one it did (no side stream at all: everything on `main`)
  hipStream_t st[NS];
  st[0] = main;
  for (int i = 1; i < NS; ++i) st[i] = (i <= n_sides && sides && sides[i - 1]) ? sides[i - 1] : st[i - 1];
  int phys[NS] = {0, 0, 0};   // the first stream that is the same HIP stream: side streams that are really others fork and join
  for (int i = 1; i < NS; ++i) {
    phys[i] = i;
    for (int j = i; j-- > 0;)
      if (st[j] == st[i]) phys[i] = j;
  }
  long k_ = -1;
  const hipEvent_t* ev = p->events.data();
  for (const Cmd& c : lic_sched::commands_of(sc, phys)) {   // (built by the first replay of this folding)
    hipStream_t s = st[c.stream];
    if (c.kind == lic_sched::CMD_LAUNCH) {
      k_ = c.arg;
      const int rc = issue_op(p->ops[c.arg], s, c.arg);
      if (rc != LIC_OK) return rc;
    } else if (c.kind == lic_sched::CMD_WAIT) {
      PLAN_TRY(hipStreamWaitEvent(s, ev[c.arg], 0));
    } else {
      PLAN_TRY(hipEventRecord(ev[c.arg], s));
    }
  }
  return LIC_OK;
}

// Issue the plan: `main` is the caller's stream (work queued on it before the call is ordered before the plan, work
// queued after the call is ordered after ALL of the plan); `sides`: up to two more streams of the same device that are
// otherwise idle (fewer than the schedule uses: the missing ones fold onto the last one given; none: one stream).
LIC_EXPORT int lic_plan_replay(lic_plan* p, lic_stream_t main, const lic_stream_t* sides, int32_t n_sides) {
  if (!p || n_sides < 0 || (n_sides > 0 && !sides)) return LIC_ERR_INVALID;
  return replay_schedule(p, p->sched, (hipStream_t)main, (const hipStream_t*)sides, n_sides);
}

// wall time of `reps` back-to-back replays of a schedule, in microseconds per replay (the device is idle before and after)
static int time_schedule(lic_plan* p, Schedule& sc, hipStream_t main, const hipStream_t* sides, int n_sides, int reps, double* us) {
  long k_ = -1;
  hipEvent_t e0, e1;
  PLAN_TRY(hipEventCreate(&e0));
  PLAN_TRY(hipEventCreate(&e1));
  int rc = replay_schedule(p, sc, main, sides, n_sides);  // warm
  PLAN_TRY(hipStreamSynchronize(main));
  if (rc == LIC_OK) {
    PLAN_TRY(hipEventRecord(e0, main));
    for (int r = 0; r < reps && rc == LIC_OK; ++r) rc = replay_schedule(p, sc, main, sides, n_sides);
    PLAN_TRY(hipEventRecord(e1, main));
    PLAN_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    PLAN_TRY(hipEventElapsedTime(&ms, e0, e1));
    *us = (double)ms * 1e3 / reps;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

// Time every operation, list-schedule onto the two streams, keep the fastest of {capture order, tuned candidates}.
// Replays the plan a few dozen times (the step is re-computed from the same inputs: idempotent as long as the
// capture holds no in-place update of its own inputs -- the optimizer stays outside).
// result[0..3] = sum of operation times (us), capture-order step (us), tuned step (us), 1 if the tuned one was kept.
LIC_EXPORT int lic_plan_tune(lic_plan* p, lic_stream_t main_, const lic_stream_t* sides_, int32_t n_sides, double* result) {
  if (!p || !sides_ || n_sides < 1 || !sides_[0] || sides_[0] == main_) return LIC_ERR_INVALID;
  hipStream_t main = (hipStream_t)main_;
  const hipStream_t* sides = (const hipStream_t*)sides_;
  const int ns = std::min(NS, 1 + (int)n_sides);   // streams the tuned schedule may use
  const size_t n = p->ops.size();
  long k_ = -1;
  // ---- 1. operation times: one stream, an event between operations, best of three passes
  std::vector<hipEvent_t> ev(n + 1);
  for (auto& e : ev) PLAN_TRY(hipEventCreate(&e));
  for (Node& nd : p->dag) nd.us = 1e30;
  int rc = LIC_OK;
  for (int pass = 0; pass < 3 && rc == LIC_OK; ++pass) {
    PLAN_TRY(hipEventRecord(ev[0], main));
    for (size_t k = 0; k < n && rc == LIC_OK; ++k) {
      rc = issue_op(p->ops[k], main, (long)k);
      PLAN_TRY(hipEventRecord(ev[k + 1], main));
    }
    PLAN_TRY(hipStreamSynchronize(main));
    for (size_t k = 0; k < n && rc == LIC_OK; ++k) {
      float ms = 0.f;
      PLAN_TRY(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      p->dag[k].us = std::min(p->dag[k].us, std::max((double)ms * 1e3, 0.5));
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  if (rc != LIC_OK) return rc;
  double total = 0.0;
  for (const Node& nd : p->dag) total += nd.us;
  if (const char* dbg = getenv("LIC_PLAN_DEBUG"))
    if (dbg[0] == '2')   // the step as a list of stand-alone operation times (capture order)
      for (size_t k = 0; k < n; ++k) {
        const PlanOp& op = p->ops[k];
        const char* nm = op.type == hipGraphNodeTypeKernel ? hipKernelNameRefByPtr(op.kp.func, main) : "(memset / memcpy / empty)";
        fprintf(stderr, "[lic_plan] op %3zu %8.1f us  grid %6u  %s\n", k, p->dag[k].us,
                op.type == hipGraphNodeTypeKernel ? op.kp.gridDim.x * op.kp.gridDim.y * op.kp.gridDim.z : 0u, nm ? nm : "?");
      }
  // ---- 2. list scheduling (lic_plan_sched.h): long kernels of >= 192 workgroups take turns; candidates differ in what
  //         "long" means
  // ---- 3. measure: the capture-order schedule and the candidates, keep the fastest (a tuned one must win by 2 %)
  double t_cap = 0.0, t_tuned = 1e300, modelled_best = 0.0;
  if ((rc = time_schedule(p, p->sched, main, sides, n_sides, 6, &t_cap)) != LIC_OK) return rc;
  Schedule best_sc;
  const double wide_opts[3] = {25.0, 80.0, 1e30};
  for (double wm : wide_opts) {
    double modelled = 0.0, t = 0.0;
    Schedule cand = lic_sched::list_schedule(p->dag, ns, wm, &modelled);
    if (!ensure_events(p, std::max(cand.n_events, p->sched.n_events))) return LIC_ERR_LAUNCH;
    if ((rc = time_schedule(p, cand, main, sides, n_sides, 6, &t)) != LIC_OK) return rc;
    if (getenv("LIC_PLAN_DEBUG"))
      fprintf(stderr, "[lic_plan] candidate (long >= %.0f us): %.1f us measured, %.1f us modelled, %d on the second stream, %d events\n",
              wm, t, modelled, cand.on_side, cand.n_events);
    if (t < t_tuned) t_tuned = t, best_sc = cand, modelled_best = modelled;
  }
  const bool keep = t_tuned < 0.98 * t_cap;
  if (getenv("LIC_PLAN_DEBUG"))
    fprintf(stderr, "[lic_plan] operations %.1f us in sum; capture order %.1f us (%d on the second stream, %d events); best tuned %.1f us "
                    "(%d on the second stream, %d events, modelled %.1f us): %s\n", total, t_cap, p->sched.on_side, p->sched.n_events,
            t_tuned, best_sc.on_side, best_sc.n_events, modelled_best, keep ? "tuned kept" : "capture order kept");
  if (keep) {
    p->sched = best_sc;
    p->tuned = 1;
  }
  if (result) {
    result[0] = total;
    result[1] = t_cap;
    result[2] = t_tuned;
    result[3] = keep ? 1.0 : 0.0;
  }
  return LIC_OK;
}
#undef PLAN_TRY

// ---- read-back: what the schedulers were given and what a replay issues, as data (tests/plan_sched_ref.py checks it)

static int put_commands(const std::vector<Cmd>& cmds, int64_t cap, int64_t* n_cmds, int32_t* out) {
  *n_cmds = (int64_t)cmds.size();
  if (!out && cap == 0) return LIC_OK;   // (a size query)
  if (!out) return LIC_ERR_INVALID;
  if (cap < (int64_t)cmds.size()) return LIC_ERR_WORKSPACE;
  for (size_t i = 0; i < cmds.size(); ++i) {
    out[3 * i] = cmds[i].kind;
    out[3 * i + 1] = cmds[i].stream;
    out[3 * i + 2] = cmds[i].arg;
  }
  return LIC_OK;
}

LIC_EXPORT int lic_plan_dag(const lic_plan* p, int64_t cap_ops, int64_t cap_edges, int64_t* sizes, int32_t* pred_ptr,
                            int32_t* pred_idx, int32_t* kind, int32_t* flags, double* us) {
  if (!p || !sizes || cap_ops < 0 || cap_edges < 0) return LIC_ERR_INVALID;
  const int64_t n = (int64_t)p->dag.size();
  int64_t ne = 0;
  for (const Node& nd : p->dag) ne += (int64_t)nd.preds.size();
  sizes[0] = n;
  sizes[1] = ne;
  if (!pred_ptr && !pred_idx && !kind && !flags && !us && cap_ops == 0 && cap_edges == 0) return LIC_OK;   // (a size query)
  if (!pred_ptr || (!pred_idx && ne > 0) || !kind || !flags || !us) return LIC_ERR_INVALID;
  if (cap_ops < n || cap_edges < ne) return LIC_ERR_WORKSPACE;
  int64_t e = 0;
  for (int64_t k = 0; k < n; ++k) {
    const Node& nd = p->dag[k];
    pred_ptr[k] = (int32_t)e;
    for (int q : nd.preds) pred_idx[e++] = q;
    const hipGraphNodeType t = p->ops[k].type;
    kind[k] = t == hipGraphNodeTypeKernel ? 0 : t == hipGraphNodeTypeMemset ? 1 : t == hipGraphNodeTypeMemcpy ? 2 : 3;
    flags[k] = (nd.wide ? 1 : 0) | (nd.filler ? 2 : 0);
    us[k] = nd.us;
  }
  pred_ptr[n] = (int32_t)e;
  return LIC_OK;
}

LIC_EXPORT int lic_plan_commands(lic_plan* p, int32_t n_sides, int64_t cap, int64_t* n_cmds, int32_t* cmds) {
  if (!p || !n_cmds || n_sides < 0 || n_sides > NS - 1 || cap < 0) return LIC_ERR_INVALID;
  int phys[NS];
  lic_sched::fold_of_sides(n_sides, phys);
  return put_commands(lic_sched::commands_of(p->sched, phys), cap, n_cmds, cmds);
}

// the schedulers and the command-list builder on a caller's DAG: no HIP call, runs without a GPU
LIC_EXPORT int lic_plan_sched_host(int64_t n_ops, const int32_t* pred_ptr, const int32_t* pred_idx, const double* us,
                                   const int32_t* flags, int32_t mode, int32_t ns, double wide_min_us, int32_t n_sides,
                                   int64_t cap, int64_t* n_cmds, int32_t* cmds, int64_t* info) {
  if (n_ops < 1 || n_ops > (1 << 24) || !pred_ptr || !us || !flags || !n_cmds || cap < 0) return LIC_ERR_INVALID;
  if ((mode != 0 && mode != 1) || (mode == 1 && (ns < 1 || ns > NS)) || n_sides < 0 || n_sides > NS - 1) return LIC_ERR_INVALID;
  if (pred_ptr[0] != 0) return LIC_ERR_INVALID;
  std::vector<Node> dag((size_t)n_ops);
  for (int64_t k = 0; k < n_ops; ++k) {
    if (pred_ptr[k + 1] < pred_ptr[k] || (pred_ptr[k + 1] > pred_ptr[k] && !pred_idx)) return LIC_ERR_INVALID;
    if (!(us[k] >= 0.0) || !(us[k] < 1e30)) return LIC_ERR_INVALID;
    Node& nd = dag[k];
    for (int32_t e = pred_ptr[k]; e < pred_ptr[k + 1]; ++e) {
      const int32_t q = pred_idx[e];
      if (q < 0 || q >= k) return LIC_ERR_INVALID;   // capture order: predecessors first
      nd.preds.push_back(q);
      dag[q].succs.push_back((int)k);
    }
    nd.us = us[k];
    nd.wide = (flags[k] & 1) != 0;
    nd.filler = (flags[k] & 2) != 0;
  }
  Schedule sc = mode == 0 ? lic_sched::capture_order_schedule(dag) : lic_sched::list_schedule(dag, ns, wide_min_us, nullptr);
  if (info) {
    info[0] = sc.on_side;
    info[1] = sc.n_events;
  }
  int phys[NS];
  lic_sched::fold_of_sides(n_sides, phys);
  return put_commands(lic_sched::command_list(sc, phys), cap, n_cmds, cmds);
}

LIC_EXPORT void lic_plan_destroy(lic_plan* p) {
  if (!p) return;
  for (hipEvent_t e : p->events) (void)hipEventDestroy(e);
  delete p;
}
