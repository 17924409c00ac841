// TEST-ONLY stand-alone driver of the signature pipelines' shared host side
// (fabric-token-sdk_amd/csrc/host/sigpipe.h): the chunk splitter against the
// loop the four runtimes used to carry inline, the two-slot driver through
// recorded submit / collect events with injected errors, and the message
// layout through random items over a small pool of buffers.
// Prints "ok <checks>" and exits 0, or the first violation and exits 1.
//   sigpipe_main [seed]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/host/sigpipe.h"

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

// The chunk boundaries as ftz_verify_ecdsa_signatures, ftz_sign_ecdsa,
// ftz_verify_owner_signatures and ftz_sign_owner_signatures computed them
// inline: msg_len[b] + ITEM_BYTES is cost[b] here.
static std::vector<size_t> inline_bounds(const std::vector<size_t>& cost, size_t CHUNK_SIGS, size_t CHUNK_BYTES) {
  std::vector<size_t> ends;
  const size_t n = cost.size();
  size_t a = 0;
  while (a < n) {
    size_t b = a, bytes = 0;
    while (b < n && b - a < CHUNK_SIGS && (b == a || bytes + cost[b] < CHUNK_BYTES)) {
      bytes += cost[b];
      b++;
    }
    ends.push_back(b);
    a = b;
  }
  return ends;
}

static std::vector<size_t> random_costs(size_t n, size_t max_bytes) {
  std::vector<size_t> cost(n);
  for (size_t& c : cost) {
    uint32_t kind = rnd(8);
    c = kind == 0 ? max_bytes + rnd(50)                         // alone beyond the byte limit
        : kind == 1 ? max_bytes - 1 - rnd(2)                    // at the limit
                    : 1 + rnd((uint32_t)(max_bytes / 2 + 1));
  }
  return cost;
}

static void splitter() {
  const size_t n = rnd(41), max_items = 1 + rnd(8), max_bytes = 2 + rnd(rnd(2) ? 40 : 400);
  const std::vector<size_t> cost = random_costs(n, max_bytes);
  const std::vector<size_t> want = inline_bounds(cost, max_items, max_bytes);
  size_t a = 0, c = 0;
  while (a < n) {
    const size_t b = ftsh::sig_chunk_end(a, n, max_items, max_bytes, [&](size_t i) { return cost[i]; });
    CHECK(c < want.size() && b == want[c], "chunk %zu ends at %zu", c, b);
    CHECK(b > a && b <= n, "empty or overlong chunk [%zu, %zu)", a, b);
    CHECK(b - a <= max_items, "%zu items > %zu", b - a, max_items);
    size_t sum = 0;
    for (size_t i = a; i < b; i++) sum += cost[i];
    CHECK(b - a == 1 || sum < max_bytes, "%zu bytes in %zu items, limit %zu", sum, b - a, max_bytes);
    a = b;
    c++;
  }
  CHECK(a == n && c == want.size(), "%zu chunks end at %zu of %zu", c, a, n);
  CHECK(ftsh::sig_chunk_end(n, n, max_items, max_bytes, [&](size_t i) { return cost[i]; }) == n, "past the end");
}

// n items through fake slots; fail_at >= 0 makes the event of that number
// (submits and collects of a pass in flight, counted together) return an error.
static void driver(size_t n, size_t max_items, int fail_at) {
  const size_t max_bytes = 1000;
  std::vector<size_t> cost(n);
  for (size_t& c : cost) c = 1 + rnd(600);
  const std::vector<size_t> want = inline_bounds(cost, max_items, max_bytes);
  bool busy[2] = {false, false};
  size_t held[2] = {0, 0};                      // the chunk in flight in a slot
  std::vector<int> collected(want.size(), 0);   // per chunk
  size_t submits = 0, next_a = 0;
  int events = 0, injected = 0, calls_after_loop[2] = {0, 0};
  size_t failed_submit = (size_t)-1;
  bool failed = false;
  auto collect = [&](int slot) -> int {
    CHECK(slot == 0 || slot == 1, "slot %d", slot);
    calls_after_loop[slot]++;
    if (!busy[slot]) return 0;
    busy[slot] = false;  // a collect ends the pass, also when it reports an error
    collected[held[slot]]++;
    if (events++ == fail_at && !failed) {
      failed = true;
      return injected = 100 + events;
    }
    return failed && rnd(2) ? 7 : 0;  // later errors must not replace the first
  };
  auto submit = [&](int slot, size_t a, size_t b) -> int {
    CHECK(!failed, "submit of [%zu, %zu) after an error", a, b);
    CHECK(slot == (int)(submits & 1), "chunk %zu in slot %d", submits, slot);
    CHECK(!busy[slot], "chunk %zu submitted into slot %d with its pass uncollected", submits, slot);
    CHECK(submits < want.size() && a == next_a && b == want[submits], "chunk %zu is [%zu, %zu)", submits, a, b);
    calls_after_loop[0] = calls_after_loop[1] = 0;
    next_a = b;
    if (events++ == fail_at) {  // nothing was enqueued: the slot stays idle
      failed = true;
      failed_submit = submits++;
      return injected = 100 + events;
    }
    busy[slot] = true;
    held[slot] = submits++;
    return 0;
  };
  const int rc = ftsh::sig_run(n, max_items, max_bytes, [&](size_t i) { return cost[i]; }, collect, submit);
  CHECK(!busy[0] && !busy[1], "a pass is still in flight");
  CHECK(calls_after_loop[0] >= 1 && calls_after_loop[1] >= 1, "a slot was not collected after the last submit");
  if (failed) {
    CHECK(rc == injected, "returned %d, the first error was %d", rc, injected);
  } else {
    CHECK(rc == 0, "returned %d", rc);
    CHECK(submits == want.size() && next_a == n, "%zu of %zu chunks", submits, want.size());
  }
  for (size_t c = 0; c < submits; c++)  // the submit that failed left no pass to collect
    CHECK(collected[c] == (c == failed_submit ? 0 : 1), "chunk %zu collected %d times", c, collected[c]);
}

static void drivers() {
  const size_t sizes[] = {0, 1, 2, 3, 4, 5, 9, 1 + rnd(40)};
  for (size_t n : sizes)
    for (size_t max_items = 1; max_items <= 3; max_items++) {
      driver(n, max_items, -1);
      for (int k = 0; k < 4; k++) driver(n, max_items, (int)rnd(2 * (uint32_t)n + 2));
    }
  // exactly two chunks, and three: the first reuse of a slot
  driver(2, 1, -1);
  driver(3, 1, -1);
  for (int at = 0; at < 6; at++) driver(3, 1, at);
}

static void layout(size_t rem) {
  static uint8_t pool[6][80];
  for (auto& p : pool)
    for (uint8_t& x : p) x = (uint8_t)rnd(256);
  const size_t m = rnd(30), start = rnd(200);
  std::vector<std::pair<const uint8_t*, size_t>> items(m);
  for (auto& it : items) {
    uint32_t p = rnd(6);
    // lengths from few values, so that one pointer comes with two lengths and pairs repeat; 0 among them
    const size_t lens[] = {0, 1, 15, 16, 17, 33, 64, 80};
    it = {rnd(12) == 0 ? nullptr : pool[p], lens[rnd(8)]};
    if (!it.first) it.second = 0;
  }
  ftsh::MsgLayout L;
  L.msg_off.assign(3, 77);  // a reused layout starts over
  L.distinct.assign(2, {5, 5});
  ftsh::sig_layout_messages(m, start, rem, [&](size_t k) { return items[k]; }, L);
  CHECK(L.msg_off.size() == m && L.distinct.size() <= m, "%zu offsets, %zu distinct", L.msg_off.size(), L.distinct.size());
  CHECK(L.end >= start, "end %zu before start %zu", L.end, start);
  for (size_t k = 0; k < m; k++) {
    CHECK(L.msg_off[k] % 16 == rem, "offset %u, remainder %zu", L.msg_off[k], rem);
    CHECK(L.msg_off[k] >= start && L.msg_off[k] + items[k].second <= L.end, "item %zu outside [start, end)", k);
    for (size_t j = 0; j < k; j++) {
      if (items[j] == items[k]) {
        CHECK(L.msg_off[j] == L.msg_off[k], "equal messages at %u and %u", L.msg_off[j], L.msg_off[k]);
      } else {
        const size_t a0 = L.msg_off[j], a1 = a0 + items[j].second, b0 = L.msg_off[k], b1 = b0 + items[k].second;
        CHECK(a1 <= b0 || b1 <= a0, "items %zu and %zu overlap", j, k);
      }
    }
  }
  // every distinct message is listed once, under its first item
  for (size_t d = 0; d < L.distinct.size(); d++) {
    const size_t k = L.distinct[d].second;
    CHECK(k < m && L.distinct[d].first == L.msg_off[k], "distinct %zu", d);
    for (size_t j = 0; j < k; j++) CHECK(!(items[j] == items[k]), "distinct %zu names item %zu, not the first", d, k);
    for (size_t e = 0; e < d; e++) CHECK(!(items[L.distinct[e].second] == items[k]), "message listed twice");
  }
  // fill as the runtimes do and read every item's message back
  std::vector<uint8_t> blob(L.end + 64, 0xEE);
  for (size_t d = 0; d < L.distinct.size(); d++)
    ftsh::sig_copy_message(L, d, blob.data(), [&](size_t k) { return items[k]; });
  for (size_t i = L.end; i < blob.size(); i++) CHECK(blob[i] == 0xEE, "byte %zu past the end written", i);
  for (size_t k = 0; k < m; k++)
    CHECK(items[k].second == 0 || memcmp(blob.data() + L.msg_off[k], items[k].first, items[k].second) == 0,
          "item %zu reads another message", k);
}

int main(int argc, char** argv) {
  if (argc > 1) rng_state ^= strtoull(argv[1], nullptr, 0) * 0xD1342543DE82EF95ull + 1;
  for (int r = 0; r < 4000; r++) splitter();
  for (int r = 0; r < 150; r++) drivers();
  for (int r = 0; r < 1500; r++) {
    layout(0);  // the ECDSA paths
    layout(4);  // NymCurve<fp>::PRE % 16, BN254
    layout(6);  // NymCurve<fq>::PRE % 16, FP256BN
  }
  // the library's own limits: a call of 2 * SIG_CHUNK_ITEMS + 1 small items is three chunks
  size_t a = 0, chunks = 0;
  while (a < 2 * ftsh::SIG_CHUNK_ITEMS + 1) {
    a = ftsh::sig_chunk_end(a, 2 * ftsh::SIG_CHUNK_ITEMS + 1, ftsh::SIG_CHUNK_ITEMS, ftsh::SIG_CHUNK_BYTES,
                            [](size_t) { return (size_t)512; });
    chunks++;
  }
  CHECK(chunks == 3, "%zu chunks", chunks);
  printf("ok %llu\n", (unsigned long long)checks);
  return 0;
}
