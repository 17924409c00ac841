// TEST-ONLY stand-alone driver of the emulated signing job and the DER encoder
// (ecsign_emu.cpp), built with -fsanitize=address,undefined by
// tests/test_ecsign.py and run as a subprocess.  Input file: one case per line,
// "<d hex> <msg hex or -> <entropy hex or -> <expected DER hex>".  Every case is
// signed from heap buffers of exactly the inputs' sizes into a heap buffer of
// exactly 72 bytes, compared with the expected bytes, and read back by the
// decoder.  Exit 0 when everything ran and matched; the sanitizers abort otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
int ecsign_emu_sign(const uint8_t* d, const uint8_t* msg, size_t msg_len, const uint8_t* entropy, uint8_t* sig,
                    size_t* sig_len);
size_t ecsign_emu_encode(const uint8_t* r, const uint8_t* s, uint8_t* out);
int ecsign_emu_decode(const uint8_t* sig, size_t len, uint8_t* r, uint8_t* s);
}

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
static uint8_t* heap_copy(const std::vector<uint8_t>& v) {
  uint8_t* p = (uint8_t*)malloc(v.size() ? v.size() : 1);
  if (!v.empty()) memcpy(p, v.data(), v.size());
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line;
  size_t cases = 0, bad = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string ds, ms, es, ss;
    if (!(ls >> ds >> ms >> es >> ss)) return 2;
    std::vector<uint8_t> d = unhex(ds), msg = unhex(ms), ent = unhex(es), want = unhex(ss);
    if (d.size() != 32 || (!ent.empty() && ent.size() != 32)) return 2;
    uint8_t *dp = heap_copy(d), *mp = heap_copy(msg), *ep = ent.empty() ? nullptr : heap_copy(ent);
    uint8_t* sig = (uint8_t*)malloc(72);
    size_t len = 0;
    int code = ecsign_emu_sign(dp, mp, msg.size(), ep, sig, &len);
    bool ok = code == 0 && len == want.size() && memcmp(sig, want.data(), len) == 0;
    // the decoder reads back what the encoder wrote, and the encoder writes it again
    uint8_t r[32], s[32];
    uint8_t* again = (uint8_t*)malloc(72);
    ok = ok && ecsign_emu_decode(sig, len, r, s) == 0 && ecsign_emu_encode(r, s, again) == len &&
         memcmp(again, sig, len) == 0;
    cases++;
    bad += !ok;
    free(again);
    free(sig);
    free(ep);
    free(mp);
    free(dp);
  }
  printf("%zu cases, %zu mismatches\n", cases, bad);
  return cases && !bad ? 0 : 1;
}
