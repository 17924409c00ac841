// TEST-ONLY stand-alone driver of the emulated Pointcheval-Sanders pass
// (ps_emu.cpp), built with -fsanitize=address,undefined by tests/test_ps.py and
// run as a subprocess.  Input file: the public parameters on the first line
// ("<pp hex>"), then one case per line, "<m hex> <h hex> <r hex> <s hex> <code>".
// All cases run as ONE batch from a heap buffer of exactly n x 192 bytes into a
// heap buffer of exactly n codes, under the exact final exponentiation planned
// in one piece and under the Fuentes-Castaneda one planned in several; then the audit of the parameters' own
// signed values, which must all pass.  Exit 0 when everything ran and matched;
// the sanitizers abort otherwise.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
void* ps_emu_create(const uint8_t* pp, size_t len);
void ps_emu_destroy(void* h);
void ps_emu_set_fexp(void* h, int variant);
int ps_emu_verify(void* h, size_t n, const uint8_t* sigs, int32_t* codes, int threads);
int ps_emu_audit(void* h, int32_t* codes, size_t cap, size_t* count);
}

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line;
  if (!std::getline(in, line)) return 2;
  std::vector<uint8_t> pp = unhex(line);
  uint8_t* ppb = (uint8_t*)malloc(pp.size() ? pp.size() : 1);
  memcpy(ppb, pp.data(), pp.size());
  void* h = ps_emu_create(ppb, pp.size());
  free(ppb);
  if (!h) return 2;
  std::vector<uint8_t> recs;
  std::vector<int32_t> want;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string ms, hs, rs, ss;
    int code;
    if (!(ls >> ms >> hs >> rs >> ss >> code)) return 2;
    std::vector<uint8_t> m = unhex(ms), hh = unhex(hs), r = unhex(rs), s = unhex(ss);
    if (m.size() != 32 || hh.size() != 32 || r.size() != 64 || s.size() != 64) return 2;
    recs.insert(recs.end(), m.begin(), m.end());
    recs.insert(recs.end(), hh.begin(), hh.end());
    recs.insert(recs.end(), r.begin(), r.end());
    recs.insert(recs.end(), s.begin(), s.end());
    want.push_back(code);
  }
  const size_t n = want.size();
  size_t bad = 0, runs = 0;
  for (int variant = 0; variant < 2; variant++) {
    const int threads = variant ? 3 : 1;
    ps_emu_set_fexp(h, variant);
    uint8_t* buf = (uint8_t*)malloc(recs.size() ? recs.size() : 1);
    memcpy(buf, recs.data(), recs.size());
    int32_t* codes = (int32_t*)malloc(n ? n * sizeof(int32_t) : 1);
    if (ps_emu_verify(h, n, buf, codes, threads) != 0) return 2;
    for (size_t i = 0; i < n; i++) bad += codes[i] != want[i];
    runs++;
    free(codes);
    free(buf);
  }
  size_t count = 0;
  if (ps_emu_audit(h, nullptr, 0, &count) == 0 && count) return 2;  // a short buffer is refused
  int32_t* ac = (int32_t*)malloc(count ? count * sizeof(int32_t) : 1);
  if (ps_emu_audit(h, ac, count, &count) != 0) return 2;
  for (size_t i = 0; i < count; i++) bad += ac[i] != 0;
  free(ac);
  ps_emu_destroy(h);
  printf("%zu cases x %zu runs, %zu audited, %zu mismatches\n", n, runs, count, bad);
  return n && !bad ? 0 : 1;
}
