// TEST-ONLY stand-alone host run of tools/devcheck_ops.h (tests/test_devcheck.py
// builds it plainly and with -fsanitize=address,undefined).  `--table` prints
// the op table (index name nin nout).  Otherwise stdin is a stream of records
// of 32-bit little-endian words and stdout gets each record's result words:
//   [op][n] n * nin words                       -> n * nout words
//   [0xFFFFFFFF][n][arena_len][nseg] first[n + 1] segs[2 nseg] arena (padded
//     to whole words)                            -> n * 16 words (dc_sha)
// Every result buffer is filled with 0xA5A5A5A5 before the op runs, as the
// device harness fills its own, and every buffer is a heap block of exactly the
// record's size, so a read or write past a vector is the sanitizer's to report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../fabric-token-sdk_amd/csrc/tools/devcheck_ops.h"

using namespace fts;

static bool rd(void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, stdin) == bytes; }

template <int OP>
static void run(uint32_t n, const uint32_t* in, uint32_t* out) {
  const DcInfo& e = dc_table()[OP];
  for (uint32_t j = 0; j < n; j++) dc_apply<OP>(in + (size_t)j * e.nin, out + (size_t)j * e.nout);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--table")) {
    for (int i = 0; i < DC_OP_COUNT; i++)
      printf("%d %s %u %u\n", i, dc_table()[i].name, dc_table()[i].nin, dc_table()[i].nout);
    return 0;
  }
  uint32_t hdr[2];
  while (fread(hdr, 4, 2, stdin) == 2) {
    const uint32_t op = hdr[0], n = hdr[1];
    if (op == 0xFFFFFFFFu) {
      uint32_t h2[2];
      if (!rd(h2, 8)) return 2;
      const uint32_t arena_len = h2[0], nseg = h2[1];
      std::vector<uint32_t> first((size_t)n + 1), segs((size_t)nseg * 2), out((size_t)n * 16, 0xA5A5A5A5u);
      if (!rd(first.data(), first.size() * 4) || !rd(segs.data(), segs.size() * 4)) return 2;
      void* arena = nullptr;
      if (posix_memalign(&arena, 16, arena_len ? arena_len : 1)) return 3;
      uint32_t pad = 0;
      if (!rd(arena, arena_len) || !rd(&pad, (4 - arena_len % 4) % 4)) return 2;
      for (uint32_t j = 0; j < n; j++)
        dc_sha((const uint8_t*)arena, segs.data() + 2 * (size_t)first[j], first[j + 1] - first[j],
               out.data() + (size_t)j * 16);
      free(arena);
      fwrite(out.data(), 4, out.size(), stdout);
      continue;
    }
    if (op >= (uint32_t)DC_OP_COUNT) return 4;
    const DcInfo& e = dc_table()[op];
    std::vector<uint32_t> in((size_t)n * e.nin), out((size_t)n * e.nout, 0xA5A5A5A5u);
    if (!rd(in.data(), in.size() * 4)) return 2;
    switch (op) {
#define DC_X(name, nin, nout)                    \
  case DC_##name:                                \
    run<DC_##name>(n, in.data(), out.data());    \
    break;
      DC_OPS(DC_X)
#undef DC_X
    }
    fwrite(out.data(), 4, out.size(), stdout);
  }
  return 0;
}
