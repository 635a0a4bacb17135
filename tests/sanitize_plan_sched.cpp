// Stand-alone check of the launch plan's host code (neural_image_compression_amd/csrc/lic_plan_sched.h) for memory and
// undefined-behaviour errors: random DAGs through the capture-order assignment, the list scheduler (1, 2 and 3 streams,
// the three bounds lic_plan_tune tries) and the command-list builder for every folding.  Not a pytest; build and run it
// by hand, from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ineural_image_compression_amd/csrc tests/sanitize_plan_sched.cpp -o /tmp/sanitize_plan_sched
//   /tmp/sanitize_plan_sched
// It prints "ok" and exits 0 when every list had the shape it should and the sanitizers saw nothing.  (Whether a list
// honours every edge is tests/test_plan_sched_host.py's question, not this program's.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lic_plan_sched.h"

#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using namespace lic_sched;

static uint32_t rng_state = 12345u;
static uint32_t rng() { return (rng_state = rng_state * 1664525u + 1013904223u) >> 8; }

// every operation launched once, on a stream of the folding; every wait for an event that an earlier command recorded
static int check_list(const std::vector<Cmd>& cmds, const Schedule& sc, size_t n, const int phys[NS]) {
  std::vector<int> launched(n, 0), recorded(EV_FIRST + sc.n_events, 0);
  for (const Cmd& c : cmds) {
    EXPECT(c.stream >= 0 && c.stream < NS && phys[c.stream] == c.stream);
    if (c.kind == CMD_LAUNCH) {
      EXPECT(c.arg >= 0 && (size_t)c.arg < n);
      EXPECT(++launched[c.arg] == 1);
    } else {
      EXPECT(c.kind == CMD_WAIT || c.kind == CMD_RECORD);
      EXPECT(c.arg >= 0 && c.arg < EV_FIRST + sc.n_events);
      if (c.kind == CMD_RECORD) EXPECT(++recorded[c.arg] == 1);
      else EXPECT(recorded[c.arg] == 1);
    }
  }
  for (size_t k = 0; k < n; ++k) EXPECT(launched[k] == 1);
  return 0;
}

int main() {
  long lists = 0;
  for (int trial = 0; trial < 3000; ++trial) {
    const size_t n = 1 + rng() % (trial % 50 == 0 ? 300 : 40);
    std::vector<Node> ops(n);
    const uint32_t reach = 1 + rng() % 12;
    for (size_t k = 0; k < n; ++k) {
      ops[k].us = 0.5 + (rng() % 3000) / 10.0;
      ops[k].wide = rng() % 3 == 0;
      ops[k].filler = rng() % 16 == 0;
      const uint32_t m = k ? rng() % 4 : 0;
      for (uint32_t j = 0; j < m; ++j) {
        const int q = (int)(k - 1 - rng() % (k < reach ? k : reach));
        if (std::find(ops[k].preds.begin(), ops[k].preds.end(), q) != ops[k].preds.end()) continue;
        ops[k].preds.push_back(q);
        ops[q].succs.push_back((int)k);
      }
    }
    std::vector<Schedule> scheds;
    scheds.push_back(capture_order_schedule(ops));
    const double wide_opts[3] = {25.0, 80.0, 1e30};
    for (int ns = 1; ns <= NS; ++ns)
      for (double wm : wide_opts) {
        double modelled = -1.0;
        scheds.push_back(list_schedule(ops, ns, wm, &modelled));
        EXPECT(modelled > 0.0);
        for (const Slot& sl : scheds.back().slots) EXPECT(sl.stream >= 0 && sl.stream < ns);
      }
    for (Schedule& sc : scheds) {
      EXPECT(sc.slots.size() == n);
      for (int p1 = 0; p1 <= 1; ++p1)
        for (int p2 = 0; p2 <= 2; ++p2) {
          const int phys[NS] = {0, p1, p2};
          if (p2 == 1 && p1 == 0) continue;   // (stream 2 cannot be stream 1 when stream 1 is stream 0: it is stream 0 then)
          const std::vector<Cmd>& kept = commands_of(sc, phys);
          if (check_list(kept, sc, n, phys)) return 1;
          EXPECT(&commands_of(sc, phys) == &kept && kept.size() == command_list(sc, phys).size());
          ++lists;
        }
      int phys[NS];
      for (int n_sides = 0; n_sides < NS; ++n_sides) {
        fold_of_sides(n_sides, phys);
        EXPECT(phys[0] == 0 && phys[1] == (n_sides ? 1 : 0) && phys[2] == n_sides);
        EXPECT(fold_key(phys) >= 0 && fold_key(phys) < 2 * NS);
      }
    }
  }
  std::printf("ok (%ld command lists)\n", lists);
  return 0;
}
