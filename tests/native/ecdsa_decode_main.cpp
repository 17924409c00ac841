// TEST-ONLY stand-alone driver of the x509 decoders (host/x509id.cpp), built
// with -fsanitize=address,undefined by tests/test_ecdsa.py and run as a
// subprocess.  Input file: one item per line, "I <hex>" (an identity) or
// "S <hex>" (a signature).  Every item is decoded as it is, at every prefix
// length, and under `mutations` single-byte mutations, each time from a heap
// buffer of exactly the input's size so that any read past it is reported.
// Exit 0 when everything ran; the sanitizers abort otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/host/x509id.h"

static unsigned long long decoded = 0, accepted = 0;

static void decode(char kind, const std::vector<uint8_t>& v, size_t len) {
  uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(buf, v.data(), len);
  uint8_t a[64], b[32];
  int code;
  if (kind == 'I') {
    std::string why;
    code = ftsh::decode_x509_identity(len ? buf : nullptr, len, a, &why);
  } else {
    code = ftsh::decode_ecdsa_signature(len ? buf : nullptr, len, a, b);
  }
  decoded++;
  accepted += code == 0;
  free(buf);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <items file> <mutations>\n", argv[0]);
    return 2;
  }
  const int mutations = atoi(argv[2]);
  std::ifstream in(argv[1]);
  std::string line;
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  size_t items = 0;
  while (std::getline(in, line)) {
    if (line.size() < 2 || (line[0] != 'I' && line[0] != 'S') || line[1] != ' ' || (line.size() - 2) % 2) return 2;
    std::vector<uint8_t> v;
    for (size_t i = 2; i < line.size(); i += 2) v.push_back((uint8_t)strtoul(line.substr(i, 2).c_str(), nullptr, 16));
    items++;
    decode(line[0], v, v.size());
    for (size_t k = 0; k < v.size(); k++) decode(line[0], v, k);
    if (v.empty()) continue;
    for (int m = 0; m < mutations; m++) {
      std::vector<uint8_t> w = v;
      size_t pos = next() % w.size();
      uint8_t x = (uint8_t)(next() >> 32);
      w[pos] = w[pos] == x ? (uint8_t)~x : x;
      decode(line[0], w, w.size());
    }
  }
  printf("%zu items, %llu decodes, %llu accepted\n", items, decoded, accepted);
  return items ? 0 : 2;
}
