// TEST-ONLY stand-alone driver of the emulated pseudonym signing job and the
// proto encoder (nymsign_emu.cpp), built with -fsanitize=address,undefined by
// tests/test_nymsign.py and run as a subprocess.  Input file: the issuer key on
// the first line ("<ipk hex>"), then one case per line,
// "<sk hex> <r_nym hex> <nym hex> <msg hex or -> <entropy hex or -> <expected signature hex>".
// Every case is signed from heap buffers of exactly the inputs' sizes into a
// heap buffer of exactly 136 bytes and compared with the expected bytes; the
// pseudonym is derived again and compared with the case's; the encoder runs on
// the signature's own four integers.  Exit 0 when everything ran and matched;
// the sanitizers abort otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
void* nymsign_emu_create(const uint8_t* ipk, size_t len);
void nymsign_emu_destroy(void* h);
int nymsign_emu_sign(void* h, const uint8_t* sk, const uint8_t* rnym, const uint8_t* nym, const uint8_t* msg,
                     size_t msg_len, const uint8_t* entropy, uint8_t* sig);
void nymsign_emu_make_nym(void* h, const uint8_t* sk, const uint8_t* rnym, uint8_t* out);
void nymsign_emu_encode(const uint8_t* raw, uint8_t* out);
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
  if (!std::getline(in, line)) return 2;
  std::vector<uint8_t> ipk = unhex(line);
  void* h = nymsign_emu_create(ipk.data(), ipk.size());
  if (!h) return 2;
  size_t cases = 0, bad = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string ks, rs, ns, ms, es, ss;
    if (!(ls >> ks >> rs >> ns >> ms >> es >> ss)) return 2;
    std::vector<uint8_t> sk = unhex(ks), rn = unhex(rs), nym = unhex(ns), msg = unhex(ms), ent = unhex(es),
                         want = unhex(ss);
    if (sk.size() != 32 || rn.size() != 32 || nym.size() != 64 || want.size() != 136 ||
        (!ent.empty() && ent.size() != 32))
      return 2;
    uint8_t *kp = heap_copy(sk), *rp = heap_copy(rn), *np = heap_copy(nym), *mp = heap_copy(msg),
            *ep = ent.empty() ? nullptr : heap_copy(ent);
    uint8_t* sig = (uint8_t*)malloc(136);
    uint8_t* made = (uint8_t*)malloc(64);
    uint8_t* again = (uint8_t*)malloc(136);
    uint8_t* raw = (uint8_t*)malloc(128);
    int code = nymsign_emu_sign(h, kp, rp, np, mp, msg.size(), ep, sig);
    bool ok = code == 0 && memcmp(sig, want.data(), 136) == 0;
    nymsign_emu_make_nym(h, kp, rp, made);
    ok = ok && memcmp(made, nym.data(), 64) == 0;
    for (int k = 0; k < 4; k++) memcpy(raw + 32 * k, sig + 34 * k + 2, 32);
    nymsign_emu_encode(raw, again);
    ok = ok && memcmp(again, sig, 136) == 0;
    cases++;
    bad += !ok;
    free(raw);
    free(again);
    free(made);
    free(sig);
    free(ep);
    free(mp);
    free(np);
    free(rp);
    free(kp);
  }
  nymsign_emu_destroy(h);
  printf("%zu cases, %zu mismatches\n", cases, bad);
  return cases && !bad ? 0 : 1;
}
