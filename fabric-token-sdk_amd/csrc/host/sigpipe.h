// What the four batched signature calls share on the host (ecdsa_rt.hip,
// idemix_rt.hip; DESIGN.md "Signature pipelines"): how a call is cut into
// device passes, the order in which two pipeline slots take them, and where a
// pass's messages lie in its blob.  Host-only and free of HIP, so the rules are
// tested on the CPU (tests/native/sigpipe_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <unordered_map>
#include <utility>
#include <vector>

namespace ftsh {

constexpr size_t SIG_CHUNK_ITEMS = 4096;             // items per pipelined device pass
constexpr size_t SIG_CHUNK_BYTES = (size_t)1 << 30;  // keeps every blob offset in 32 bits

// End b of the chunk [a, b) of n items: never empty for a < n, at most
// max_items items, and the sum of cost(i) below max_bytes unless it is one item.
template <class Cost>
size_t sig_chunk_end(size_t a, size_t n, size_t max_items, size_t max_bytes, Cost cost) {
  size_t b = a, bytes = 0;
  while (b < n && b - a < max_items && (b == a || bytes + cost(b) < max_bytes)) {
    bytes += cost(b);
    b++;
  }
  return b;
}

// Run n items through two slots: chunk c goes to slot c & 1, so chunk c + 1 is
// prepared on the host while chunk c runs.  collect(slot) waits for the pass in
// a slot, if there is one, and delivers its results; submit(slot, a, b) starts
// the pass of items [a, b) in a collected slot.  Both return 0 or an error
// code.  The loop stops at the first error; both slots are collected
// afterwards whatever happened, and the first error is returned.
template <class Cost, class Collect, class Submit>
int sig_run(size_t n, size_t max_items, size_t max_bytes, Cost cost, Collect collect, Submit submit) {
  int rc = 0;
  for (size_t a = 0, c = 0; a < n && rc == 0; c++) {
    const size_t b = sig_chunk_end(a, n, max_items, max_bytes, cost);
    rc = collect((int)(c & 1));
    if (rc == 0) rc = submit((int)(c & 1), a, b);
    a = b;
  }
  for (int slot = 0; slot < 2; slot++) {
    const int r2 = collect(slot);
    if (rc == 0) rc = r2;
  }
  return rc;
}

// Where the messages of a pass lie in its blob: every distinct message (same
// pointer and same length) once.
struct MsgLayout {
  std::vector<uint32_t> msg_off;                        // per item
  std::vector<std::pair<uint32_t, uint32_t>> distinct;  // (blob offset, first item with that message)
  size_t end = 0;                                       // one past the last message byte
};

// Lay m messages out from offset `start` on, each at an offset = rem mod 16
// (rem < 16); msg(k) gives item k's (pointer, length).
template <class Msg>
void sig_layout_messages(size_t m, size_t start, size_t rem, Msg msg, MsgLayout& L) {
  struct Hash {
    size_t operator()(const std::pair<const uint8_t*, size_t>& k) const {
      return std::hash<const uint8_t*>()(k.first) ^ (k.second * 0x9E3779B97F4A7C15ull);
    }
  };
  std::unordered_map<std::pair<const uint8_t*, size_t>, uint32_t, Hash> at;
  at.reserve(m);  // no rehash while it fills
  L.msg_off.resize(m);
  L.distinct.clear();
  L.end = start;
  for (size_t k = 0; k < m; k++) {
    const std::pair<const uint8_t*, size_t> key = msg(k);
    auto it = at.find(key);
    if (it == at.end()) {
      const size_t off = ((L.end + 15) & ~(size_t)15) + rem;
      it = at.emplace(key, (uint32_t)off).first;
      L.distinct.push_back({(uint32_t)off, (uint32_t)k});
      L.end = off + key.second;
    }
    L.msg_off[k] = it->second;
  }
}

// copy the d-th distinct message of a layout into the blob; msg as above
template <class Msg>
void sig_copy_message(const MsgLayout& L, size_t d, uint8_t* blob, Msg msg) {
  const std::pair<const uint8_t*, size_t> m = msg(L.distinct[d].second);
  if (m.second) memcpy(blob + L.distinct[d].first, m.first, m.second);
}

}  // namespace ftsh
