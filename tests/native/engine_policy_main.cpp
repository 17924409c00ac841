// TEST-ONLY stand-alone driver of the job engine's placement rules
// (fabric-token-sdk_amd/csrc/host/engine_policy.h): random arrival and
// completion sequences, checked against the rules the engine relies on.
// Prints "ok <checks>" and exits 0, or the first violation and exits 1.
//   engine_policy_main [seed]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <deque>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/host/engine_policy.h"

using ftsh::EnginePolicy;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static uint64_t checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    checks++;                                             \
    if (!(cond)) {                                        \
      printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
      exit(1);                                            \
    }                                                     \
  } while (0)

static uint32_t spread(const EnginePolicy& p) {
  uint32_t lo = p.count[0], hi = p.count[0];
  for (uint32_t c : p.count) {
    lo = c < lo ? c : lo;
    hi = c > hi ? c : hi;
  }
  return hi - lo;
}

// Mixed full and partial passes, completions of any triple's oldest pass.
static void random_mix(uint32_t triples, uint32_t lookahead, int steps) {
  EnginePolicy p(triples, triples, lookahead);
  CHECK(p.buffer_sets() == triples * (1 + lookahead), "%u", p.buffer_sets());
  for (int s = 0; s < steps; s++) {
    if (rnd(3) != 0) {
      bool full = rnd(2) != 0;
      int t = p.pick(full);
      if (t < 0) {
        // refused: a partial pass finds no idle triple, a full one no triple with room
        for (uint32_t k = 0; k < triples; k++)
          CHECK(full ? p.count[k] == 1 + lookahead : p.count[k] >= 1, "triple %u holds %u", k, p.count[k]);
        continue;
      }
      for (uint32_t k = 0; k < triples; k++) CHECK(p.count[t] <= p.count[k], "not the least loaded triple");
      if (!full) CHECK(p.count[t] == 0, "partial pass behind %u running", p.count[t]);
      uint32_t ahead = p.enqueue(t);
      CHECK(ahead + 1 == p.count[t], "ahead %u", ahead);
      CHECK(p.count[t] <= 1 + lookahead, "triple %d holds %u > 1 + %u", t, p.count[t], lookahead);
      CHECK(p.total <= p.buffer_sets(), "total %u", p.total);
    } else {
      uint32_t t = rnd(triples);
      if (p.count[t]) p.release((int)t);
    }
    uint32_t sum = 0;
    for (uint32_t c : p.count) sum += c;
    CHECK(sum == p.total, "total %u != %u", p.total, sum);
  }
}

// A big call: a full pass is always pending, the completer frees passes in
// dispatch order, a random number of them between two dispatches.
static void saturated(uint32_t triples, uint32_t lookahead, int steps) {
  EnginePolicy p(triples, triples, lookahead);
  std::deque<int> inflight;
  std::vector<std::deque<uint64_t>> order(triples);  // per triple: pass numbers in enqueue order
  uint64_t pass = 0;
  for (int s = 0; s < steps; s++) {
    int t;
    while ((t = p.pick(true)) >= 0) {  // the dispatcher keeps up: every admitted pass goes at once
      p.enqueue(t);
      inflight.push_back(t);
      order[t].push_back(pass++);
      CHECK(p.count[t] <= 1 + lookahead, "triple %d holds %u", t, p.count[t]);
      CHECK(spread(p) <= 1, "counts differ by %u", spread(p));
      if (rnd(4) == 0) break;  // ... or is still planning when the next completion comes
    }
    uint32_t done = 1 + rnd(triples * (1 + lookahead));
    while (done-- && !inflight.empty()) {
      int c = inflight.front();
      inflight.pop_front();
      // the oldest pass in flight is the oldest of its triple: in-stream order
      for (uint32_t k = 0; k < triples; k++)
        if (!order[k].empty()) CHECK(order[c].front() <= order[k].front(), "completion out of stream order");
      order[c].pop_front();
      p.release(c);
      CHECK(spread(p) <= 1, "counts differ by %u after a completion", spread(p));
    }
  }
  CHECK(pass >= (uint64_t)steps, "only %llu passes", (unsigned long long)pass);
}

// lookahead = 0 against the engine before lookahead: slot k owned triple k and
// free slots were taken first in, first out.
static void parent_order(uint32_t slots, int steps) {
  EnginePolicy p(slots, slots, 0);
  std::deque<int> free_slots;
  std::vector<int> busy;
  for (uint32_t k = 0; k < slots; k++) free_slots.push_back((int)k);
  for (int s = 0; s < steps; s++) {
    if (rnd(2)) {
      bool full = rnd(2) != 0;
      int t = p.pick(full);
      if (free_slots.empty()) {
        CHECK(t < 0, "picked %d with every slot busy", t);
        continue;
      }
      CHECK(t == free_slots.front(), "picked %d, the parent takes slot %d", t, free_slots.front());
      CHECK(p.enqueue(t) == 0, "queued behind a pass with lookahead 0");
      busy.push_back(t);
      free_slots.pop_front();
    } else if (!busy.empty()) {
      uint32_t k = rnd(4) ? 0 : rnd((uint32_t)busy.size());  // mostly the oldest, sometimes a failed submission
      int t = busy[k];
      busy.erase(busy.begin() + k);
      p.release(t);
      free_slots.push_back(t);
    }
  }
}

// More slots than triples: the shared triples take ceil(slots / triples) passes
// of any kind, lookahead adds full passes on top, and the buffer sets suffice.
static void many_slots(uint32_t triples, uint32_t slots, uint32_t lookahead, int steps) {
  EnginePolicy p(triples, slots, lookahead);
  const uint32_t base = (slots + triples - 1) / triples;
  for (int s = 0; s < steps; s++) {
    if (rnd(3) != 0) {
      bool full = rnd(2) != 0;
      int t = p.pick(full);
      if (t < 0) continue;
      if (!full) CHECK(p.count[t] < base, "partial pass at depth %u", p.count[t]);
      p.enqueue(t);
      CHECK(p.count[t] <= base + lookahead, "triple %d holds %u", t, p.count[t]);
      CHECK(p.total <= p.buffer_sets(), "%u passes, %u buffer sets", p.total, p.buffer_sets());
    } else {
      uint32_t t = rnd(triples);
      if (p.count[t]) p.release((int)t);
    }
  }
}

int main(int argc, char** argv) {
  if (argc > 1) rng_state ^= strtoull(argv[1], nullptr, 0) * 0xD1342543DE82EF95ull + 1;
  for (uint32_t triples = 1; triples <= 4; triples++)
    for (uint32_t la = 0; la <= 3; la++) {
      random_mix(triples, la, 20000);
      saturated(triples, la, 5000);
    }
  for (uint32_t slots = 1; slots <= 4; slots++) parent_order(slots, 20000);
  for (uint32_t slots = 5; slots <= 9; slots++)
    for (uint32_t la = 0; la <= 2; la++) many_slots(4, slots, la, 10000);
  printf("ok %llu\n", (unsigned long long)checks);
  return 0;
}
