// The host side of a launch plan (lic_plan.hip): which stream every operation of a captured step goes to, in which
// order, which cross-stream edges get an event -- and the flat list of commands a replay issues for a schedule.
// Plain C++ over a DAG of indices: no HIP header, so the same code runs in lic_plan.hip, in the host-only entry
// lic_plan_sched_host and in tests/sanitize_plan_sched.cpp, and tests/plan_sched_ref.py can hold every list it produces
// to HIP's ordering rules without a GPU.
#ifndef LIC_PLAN_SCHED_H
#define LIC_PLAN_SCHED_H

#include <algorithm>
#include <vector>

namespace lic_sched {

constexpr int NS = 3;  // streams a schedule may use: the caller's and up to two more

// what a schedule needs to know of an operation (capture order: preds < own index < succs)
struct Node {
  std::vector<int> preds, succs;
  double us = 0.0;      // measured duration (lic_plan_tune)
  bool wide = false;    // fills the chip: does not overlap with another wide operation
  bool filler = false;  // the batched reduction forked off beside a chain (reduce_batch_kernel): goes to the last stream
};

struct Slot {
  int op;
  int stream;
  int record = -1;         // event recorded right after this operation (a successor on the other stream waits for it)
  std::vector<int> waits;  // events the operation's stream waits for first
};

// what a replay issues, one command per HIP call
enum { CMD_WAIT = 0, CMD_LAUNCH = 1, CMD_RECORD = 2 };
// event ids of a command list: the fork, the two joins, then the schedule's own events
enum { EV_FORK = 0, EV_JOIN = 1, EV_FIRST = 3 };
struct Cmd {
  int kind;    // CMD_*
  int stream;  // physical stream: 0 = the caller's, i = its i-th side stream
  int arg;     // CMD_LAUNCH: the operation; CMD_WAIT / CMD_RECORD: the event id
};

struct Schedule {
  std::vector<Slot> slots;  // issue order
  int n_events = 0;
  int on_side = 0;
  // the command list per folding (fold_key), built by the first replay that uses the folding and kept
  std::vector<Cmd> cmds[2 * NS];
};

// events for every cross-stream edge that earlier waits do not cover
inline void add_events(const std::vector<Node>& ops, Schedule& sc) {
  const size_t n = sc.slots.size();
  std::vector<int> slot_of(n, -1), pos(n, -1);
  int len[NS] = {0, 0, 0};
  int waited[NS][NS];  // waited[s][o]: position on stream o that stream s has already waited for
  for (auto& row : waited)
    for (int& w : row) w = -1;
  sc.n_events = 0;
  sc.on_side = 0;
  for (auto& c : sc.cmds) c.clear();
  for (size_t k = 0; k < n; ++k) {
    Slot& sl = sc.slots[k];
    sl.record = -1;
    sl.waits.clear();
    slot_of[sl.op] = (int)k;
  }
  for (size_t k = 0; k < n; ++k) {
    Slot& sl = sc.slots[k];
    const int s = sl.stream;
    for (int q : ops[sl.op].preds) {
      Slot& pq = sc.slots[slot_of[q]];
      if (pq.stream == s || pos[slot_of[q]] <= waited[s][pq.stream]) continue;
      if (pq.record < 0) pq.record = sc.n_events++;
      sl.waits.push_back(pq.record);
      waited[s][pq.stream] = pos[slot_of[q]];
    }
    pos[k] = len[s]++;
    if (s != 0) ++sc.on_side;
  }
}

// Capture-order schedule.  The capture's streams are chains of the graph (consecutive launches of a stream depend on
// each other); where a chain forks, the successor with the longest way to go continues the stream and the others
// start (or resume) another one: a stream that was never used, else the one that has been quiet longest.
inline Schedule capture_order_schedule(const std::vector<Node>& ops) {
  const size_t n = ops.size();
  Schedule sc;
  sc.slots.resize(n);
  std::vector<int> stream(n, 0), depth(n, 1);
  for (size_t k = n; k-- > 0;)
    for (int v : ops[k].succs) depth[k] = std::max(depth[k], depth[v] + 1);
  int tail[NS] = {-1, -1, -1};
  for (size_t k = 0; k < n; ++k) {
    int s = -1;
    for (int q : ops[k].preds) {
      if (tail[stream[q]] != q) continue;
      bool continues = true;  // k continues q's stream unless a sibling has the longer way to go
      for (int v : ops[q].succs)
        if (v != (int)k && (depth[v] > depth[k] || (depth[v] == depth[k] && v < (int)k))) continues = false;
      if (continues && (s < 0 || stream[q] < s)) s = stream[q];
    }
    if (s < 0) {
      if (ops[k].preds.empty()) {
        s = 0;
      } else {
        int latest = -1;
        for (int q : ops[k].preds) latest = std::max(latest, q);
        const int avoid = stream[latest];
        int pick = -1;
        for (int c = 0; c < NS; ++c)
          if (c != avoid && (pick < 0 || tail[c] < tail[pick])) pick = c;  // (-1 = never used sorts first)
        // the batched reduction forked off beside a chain (functional.flush_point) is a filler: it goes to the LAST stream --
        // the callers give the first extra stream a high priority for the chain it carries, and a high-priority launch
        // of ~6000 blocks takes the chip from the other chain's small launches (a 4 MB cast measured 69 us beside it)
        if (avoid != NS - 1 && ops[k].filler) pick = NS - 1;
        s = pick;
      }
    }
    stream[k] = s;
    tail[s] = (int)k;
    sc.slots[k].op = (int)k;
    sc.slots[k].stream = s;
  }
  add_events(ops, sc);
  return sc;
}

constexpr double SYNC_US = 6.0;  // what the list scheduler charges a cross-stream dependency

// List scheduling onto `ns` streams.  Priority = longest path to the end (own time included).  Repeatedly the (ready
// operation, stream) pair that can START earliest is placed (ties: the more critical operation; a cross-stream
// dependency costs SYNC_US, so a chain stays on its stream unless the other one is clearly free earlier) --
// weight-gradient and reduction launches, which nothing but the optimizer waits for, fill whichever stream is idle
// instead of sitting in the data-gradient chain's queue.  Wide kernels of >= wide_min_us take turns (two of them side
// by side gain nothing).  *modelled = the step time under that model.
inline Schedule list_schedule(const std::vector<Node>& ops, int ns, double wide_min_us, double* modelled) {
  const size_t n = ops.size();
  std::vector<double> up(n, 0.0);
  for (size_t k = n; k-- > 0;) {
    double m = 0.0;
    for (int v : ops[k].succs) m = std::max(m, up[v]);
    up[k] = ops[k].us + m;
  }
  Schedule sc;
  sc.slots.reserve(n);
  std::vector<double> finish(n, 0.0);
  std::vector<int> stream(n, -1), missing(n, 0);
  std::vector<int> ready;
  for (size_t k = 0; k < n; ++k) {
    missing[k] = (int)ops[k].preds.size();
    if (!missing[k]) ready.push_back((int)k);
  }
  double avail[NS] = {0.0, 0.0, 0.0}, wide_until = 0.0;
  while (!ready.empty()) {
    // earliest possible start over all (ready operation, stream) pairs; among the pairs within 1 us of it the most
    // critical operation, then the earlier start, then stream 0
    auto start_of = [&](int k, int s2) {
      const Node& op = ops[k];
      double start = avail[s2];
      for (int q : op.preds) start = std::max(start, finish[q] + (stream[q] != s2 ? SYNC_US : 0.0));
      if (op.wide && op.us >= wide_min_us) start = std::max(start, wide_until);
      return start;
    };
    double min_start = 1e300;
    for (int k : ready)
      for (int s2 = 0; s2 < ns; ++s2) min_start = std::min(min_start, start_of(k, s2));
    int bi = -1, bs = 0;
    double b_start = 1e300;
    for (size_t i = 0; i < ready.size(); ++i)
      for (int s2 = 0; s2 < ns; ++s2) {
        const double st = start_of(ready[i], s2);
        if (st > min_start + 1.0) continue;
        const bool better = bi < 0 || up[ready[i]] > up[ready[bi]] + 1e-9 ||
                            (ready[i] == ready[bi] && st < b_start - 1e-9);
        if (better) bi = (int)i, bs = s2, b_start = st;
      }
    const int k = ready[bi];
    const Node& op = ops[k];
    const double start = start_of(k, bs);
    stream[k] = bs;
    finish[k] = start + op.us;
    avail[bs] = finish[k];
    if (op.wide && op.us >= wide_min_us) wide_until = finish[k];
    Slot sl;
    sl.op = k;
    sl.stream = bs;
    sc.slots.push_back(sl);
    ready.erase(ready.begin() + bi);
    for (int v : op.succs)
      if (--missing[v] == 0) ready.push_back(v);
  }
  add_events(ops, sc);
  if (modelled) *modelled = std::max(avail[0], std::max(avail[1], avail[2]));
  return sc;
}

// A folding says which physical stream each of the schedule's streams is issued on: phys[0] = 0 and phys[i] <= i is
// the first stream of the replay that is the same HIP stream as stream i (a side stream the caller did not give folds
// onto the last one it did; none at all: everything on the caller's stream).
inline int fold_key(const int phys[NS]) { return phys[1] * NS + phys[2]; }

// the folding of a replay with `n_sides` side streams that are all different from the caller's and from each other
inline void fold_of_sides(int n_sides, int phys[NS]) {
  for (int i = 0; i < NS; ++i) phys[i] = std::min(i, std::max(n_sides, 0));
}

// The commands of one replay: the fork record and the side streams' waits for it; per slot its waits, its launch and
// its record; the side streams' join records, each followed by the caller's stream's wait for it.  Only side streams
// that are really other streams (phys[i] == i) fork and join.
inline std::vector<Cmd> command_list(const Schedule& sc, const int phys[NS]) {
  std::vector<Cmd> out;
  size_t total = 2 * NS + sc.slots.size();
  for (const Slot& sl : sc.slots) total += sl.waits.size() + (sl.record >= 0 ? 1 : 0);
  out.reserve(total);
  bool distinct[NS] = {false, false, false};  // side streams that are really other streams (each once)
  for (int i = 1; i < NS; ++i) distinct[i] = phys[i] == i;
  if (distinct[1] || distinct[2]) out.push_back({CMD_RECORD, 0, EV_FORK});
  for (int i = 1; i < NS; ++i)
    if (distinct[i]) out.push_back({CMD_WAIT, i, EV_FORK});
  for (const Slot& sl : sc.slots) {
    const int s = phys[sl.stream];
    for (int w : sl.waits) out.push_back({CMD_WAIT, s, EV_FIRST + w});  // (same stream after folding: a no-op for the GPU)
    out.push_back({CMD_LAUNCH, s, sl.op});
    if (sl.record >= 0) out.push_back({CMD_RECORD, s, EV_FIRST + sl.record});
  }
  for (int i = 1; i < NS; ++i)
    if (distinct[i]) {
      out.push_back({CMD_RECORD, i, EV_JOIN + i - 1});
      out.push_back({CMD_WAIT, 0, EV_JOIN + i - 1});
    }
  return out;
}

// the kept command list of a schedule for a folding
inline const std::vector<Cmd>& commands_of(Schedule& sc, const int phys[NS]) {
  std::vector<Cmd>& c = sc.cmds[fold_key(phys)];
  if (c.empty()) c = command_list(sc, phys);
  return c;
}

}  // namespace lic_sched
#endif  // LIC_PLAN_SCHED_H
