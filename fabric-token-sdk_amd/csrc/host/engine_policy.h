// Where the job engine (engine.hip) puts a device pass: which of the context's
// stream triples it is enqueued on, and whether it may be enqueued behind a
// pass that is still running there.  Host-only and free of HIP, so the rules
// are tested on the CPU (tests/native/engine_policy_main.cpp).
//
// The engine owns `triples` stream triples (ftz_options.slots of them, at most
// four) and triples * (base + lookahead) buffer sets.  A pass takes its triple
// when it is dispatched: the one with the fewest passes enqueued, the oldest
// first on ties -- among idle triples the one idle longest, among busy ones the
// one whose running pass was dispatched first, i.e. is due to end first.
//   * Any pass may go to a triple that holds fewer than `base` passes;
//     base = ceil(slots / triples) is 1 for up to four slots, so this is "a
//     triple with nothing on it" (more than four slots share the four triples
//     and count as the next multiple of four).
//   * A full pass -- one that closed at its item or pair budget, the mark of a
//     big call -- may also be enqueued up to `lookahead` passes deeper: planned,
//     uploaded and launched while the pass ahead of it runs, so that its first
//     kernel starts when that pass ends and the host's plan and enqueue time
//     are off the device's critical path.  A partial pass never is: it carries
//     small callers, who would wait out the pass ahead on top of their own.
// lookahead = 0 is the engine before lookahead existed: passes cycle through
// the triples in the order they fall idle.
#pragma once
#include <stdint.h>

#include <vector>

namespace ftsh {

struct EnginePolicy {
  uint32_t lookahead = 0, base = 1;
  std::vector<uint32_t> count;  // passes enqueued per triple
  std::vector<uint64_t> stamp;  // idle triple: when it fell idle; busy: when its oldest pass was dispatched
  std::vector<std::vector<uint64_t>> seqs;  // dispatch stamps of a triple's passes, oldest first
  uint64_t clock = 0;
  uint32_t total = 0;

  EnginePolicy() {}
  EnginePolicy(uint32_t triples, uint32_t slots, uint32_t lookahead_)
      : lookahead(lookahead_), count(triples, 0), stamp(triples, 0), seqs(triples) {
    base = slots > triples ? (slots + triples - 1) / triples : 1;
    for (uint32_t t = 0; t < triples; t++) stamp[t] = clock++;  // idle in index order
  }

  uint32_t triples() const { return (uint32_t)count.size(); }
  // buffer sets the engine needs so that a pass this policy admits always finds one
  uint32_t buffer_sets() const { return triples() * (base + lookahead); }

  // The triple the next pass goes to, or -1 when it has to wait for a
  // completion.  full: the pass closed at its item or pair budget.
  int pick(bool full) const {
    int best = -1;
    for (uint32_t t = 0; t < triples(); t++)
      if (best < 0 || count[t] < count[best] || (count[t] == count[best] && stamp[t] < stamp[best])) best = (int)t;
    if (best < 0) return -1;
    if (count[best] < base || (full && count[best] < base + lookahead)) return best;
    return -1;
  }

  // A pass was enqueued on triple t; returns how many passes were ahead of it there.
  uint32_t enqueue(int t) {
    uint32_t ahead = count[t]++;
    total++;
    seqs[t].push_back(clock);
    if (ahead == 0) stamp[t] = clock;
    clock++;
    return ahead;
  }

  // The oldest pass of triple t completed (in-stream order: always the oldest).
  void release(int t) {
    count[t]--;
    total--;
    seqs[t].erase(seqs[t].begin());
    stamp[t] = seqs[t].empty() ? clock++ : seqs[t].front();
  }
};

}  // namespace ftsh
