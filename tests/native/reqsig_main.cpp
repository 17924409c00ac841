// TEST-ONLY stand-alone driver of the signed request path's host side
// (fabric-token-sdk_amd/csrc/host/request.cpp): the message assembly, the
// signature stage's item building and the verdict merge, with every device
// check answered from a table the test wrote (keyed by an FNV-1a hash of the
// bytes the check is about), so that it runs under AddressSanitizer + UBSan
// without the curve arithmetic.  A check the table does not know answers 99: it
// shows in the verdict unless an earlier check already failed.
//   reqsig_main <job file> [chunk] [inflight]
// Job file, one record per line (x<hex> = bytes, x alone = empty):
//   config <ix 0/1> <ec 0/1> <nil | x<auditor>> <auditor code> {x<issuer> <code>}
//   ledger x<key> x<value>
//   elem <hash> 0                      a 64-byte element gnark SetBytes refuses
//   zk <hash> <code>                   a proof: kind, counts, commitments, proof bytes
//   own <hash> <code>  /  osig <hash> <code>   an owner's verifier / its signature check
//   eid <hash> <code>  /  esig <hash> <code>   an x509 identity / its signature check
//   request x<raw> x<binding> <code> <failed_action>
//   run                                verify the requests so far, compare, forget them
// Prints "ok <requests>" and exits 0, or the first difference and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/host/request.h"

typedef std::vector<uint8_t> Bytes;

static uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) {
  uint8_t len[8];
  for (int k = 0; k < 8; k++) len[k] = (uint8_t)((uint64_t)n >> (8 * k));
  for (int k = 0; k < 8; k++) h = (h ^ len[k]) * 0x100000001B3ull;
  for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
  return h;
}
static const uint64_t FNV0 = 0xCBF29CE484222325ull;

static Bytes unhex(const std::string& s) {
  Bytes out;
  if (s.empty() || s[0] != 'x' || (s.size() & 1) == 0) {
    printf("FAIL bad hex field\n");
    exit(1);
  }
  for (size_t i = 1; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

struct Job {
  bool ix = false, ec = false, has_auditor = false;
  Bytes auditor;
  int32_t auditor_code = 0;
  std::vector<Bytes> issuers;
  std::vector<int32_t> issuer_codes;
  std::map<std::string, Bytes> ledger;
  std::map<std::string, std::map<uint64_t, int32_t>> tab;
  std::vector<Bytes> raw, binding;
  std::vector<int32_t> code, failed;
  std::vector<Bytes> keys;  // registered x509 identities by key index
  std::vector<Bytes> held;  // the values of the last get_states call
  int32_t look(const char* t, uint64_t h, int32_t miss = 99) const {
    auto f = tab.find(t);
    if (f == tab.end()) return miss;
    auto g = f->second.find(h);
    return g == f->second.end() ? miss : g->second;
  }
};

static int get_states(void* user, size_t n, const ftz_bytes* keys, ftz_bytes* vals) {
  Job* j = (Job*)user;
  j->held.clear();
  j->held.reserve(n);
  for (size_t i = 0; i < n; i++) {
    auto f = j->ledger.find(std::string((const char*)keys[i].p, keys[i].len));
    if (f == j->ledger.end() || f->second.empty()) {
      vals[i] = ftz_bytes{nullptr, 0};
      continue;
    }
    j->held.push_back(f->second);  // a copy that lives until the next call, as the contract says
    vals[i] = ftz_bytes{j->held.back().data(), j->held.back().size()};
  }
  return 0;
}

static uint64_t zk_hash(uint8_t kind, const uint8_t* in, uint32_t n_in, const uint8_t* out, uint32_t n_out,
                        const uint8_t* proof, size_t plen, uint8_t anon) {
  uint8_t head[2] = {kind, anon};
  uint64_t h = fnv(FNV0, head, 2);
  h = fnv(h, in, 64 * (size_t)n_in);
  h = fnv(h, out, 64 * (size_t)n_out);
  return fnv(h, proof, plen);
}

static size_t run(Job& j, size_t chunk, size_t inflight) {
  ftsh::RequestHooks h;
  h.check = [&j](size_t m, const uint8_t* slots, uint8_t* ok) {
    for (size_t i = 0; i < m; i++) ok[i] = (uint8_t)j.look("elem", fnv(FNV0, slots + 64 * i, 64), 1);
    return 0;
  };
  h.verify_transfers = [&j](size_t m, const ftz_transfer* t, int32_t* c) {
    for (size_t i = 0; i < m; i++)
      c[i] = j.look("zk", zk_hash(1, t[i].inputs, t[i].n_in, t[i].outputs, t[i].n_out, t[i].proof, t[i].proof_len, 0));
    return 0;
  };
  h.verify_issues = [&j](size_t m, const ftz_issue* t, int32_t* c) {
    for (size_t i = 0; i < m; i++)
      c[i] = j.look("zk", zk_hash(0, nullptr, 0, t[i].outputs, t[i].n_out, t[i].proof, t[i].proof_len,
                                  t[i].anonymous ? 1 : 0));
    return 0;
  };
  h.get_states = get_states;
  h.user = &j;
  if (chunk) h.chunk = chunk;
  if (inflight) h.inflight = inflight;
  ftsh::RequestSigners sg;
  if (j.ix)
    sg.verify_owners = [&j](size_t m, const ftz_owner_sig* s, int32_t* c) {
      for (size_t i = 0; i < m; i++) {
        c[i] = j.look("own", fnv(FNV0, s[i].owner, s[i].owner_len));
        if (c[i]) continue;
        if (s[i].sig_len == 0) {
          c[i] = FTZ_ERR_SIGNATURE;
          continue;
        }
        uint64_t k = fnv(fnv(fnv(FNV0, s[i].owner, s[i].owner_len), s[i].msg, s[i].msg_len), s[i].sig, s[i].sig_len);
        c[i] = j.look("osig", k);
      }
      return 0;
    };
  if (j.ec)
    sg.verify_ecdsa = [&j](size_t m, const ftz_ecdsa_sig* s, int32_t* c) {
      for (size_t i = 0; i < m; i++) {
        const uint8_t* id = s[i].identity;
        size_t idl = s[i].identity_len;
        if (s[i].key >= 0) {
          if ((size_t)s[i].key >= j.keys.size()) return (int)FTZ_E_INVALID;
          id = j.keys[s[i].key].data(), idl = j.keys[s[i].key].size();
          c[i] = 0;
        } else {
          c[i] = j.look("eid", fnv(FNV0, id, idl));
        }
        if (c[i]) continue;
        if (s[i].sig_len == 0) {
          c[i] = FTZ_ERR_SIGNATURE;
          continue;
        }
        c[i] = j.look("esig", fnv(fnv(fnv(FNV0, id, idl), s[i].msg, s[i].msg_len), s[i].sig, s[i].sig_len));
      }
      return 0;
    };
  auto key_of = [&j](const Bytes& id, int32_t code) {
    ftsh::SignerKey k;
    k.code = code;
    if (code) return k;
    k.key = (int32_t)j.keys.size();
    j.keys.push_back(id);
    return k;
  };
  j.keys.clear();
  sg.has_auditor = j.has_auditor;
  sg.auditor = ftsh::Slice{j.auditor.data(), j.auditor.size()};
  if (j.ec && !j.auditor.empty()) sg.auditor_key = key_of(j.auditor, j.auditor_code);
  sg.issuers.resize(j.issuers.size());
  sg.issuer_keys.resize(j.issuers.size());
  for (size_t i = 0; i < j.issuers.size(); i++) {
    sg.issuers[i] = ftsh::Slice{j.issuers[i].data(), j.issuers[i].size()};
    if (j.ec) sg.issuer_keys[i] = key_of(j.issuers[i], j.issuer_codes[i]);
  }
  const size_t n = j.raw.size();
  std::vector<ftz_bytes> raw(n), bind(n);
  for (size_t i = 0; i < n; i++) {
    raw[i] = ftz_bytes{j.raw[i].data(), j.raw[i].size()};
    bind[i] = ftz_bytes{j.binding[i].data(), j.binding[i].size()};
  }
  sg.bindings = bind.data();
  std::vector<int32_t> codes(n + 1, -7), failed(n + 1, -7);
  std::string err;
  int rc = ftsh::verify_signed_token_requests(n, raw.data(), h, sg, codes.data(), failed.data(), err);
  if (rc != 0) {
    printf("FAIL verify_signed_token_requests returned %d: %s\n", rc, err.c_str());
    exit(1);
  }
  for (size_t i = 0; i < n; i++)
    if (codes[i] != j.code[i] || failed[i] != j.failed[i]) {
      printf("FAIL request %zu: got (%d, %d), want (%d, %d)\n", i, codes[i], failed[i], j.code[i], j.failed[i]);
      exit(1);
    }
  if (codes[n] != -7 || failed[n] != -7) {
    printf("FAIL wrote past the verdict arrays\n");
    exit(1);
  }
  return n;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: reqsig_main <job file> [chunk] [inflight]\n");
    return 2;
  }
  const size_t chunk = argc > 2 ? strtoul(argv[2], nullptr, 10) : 0, inflight = argc > 3 ? strtoul(argv[3], nullptr, 10) : 0;
  std::ifstream f(argv[1]);
  if (!f) {
    printf("FAIL cannot read %s\n", argv[1]);
    return 1;
  }
  Job j;
  std::string line;
  size_t done = 0;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string kind, a, b;
    in >> kind;
    if (kind == "config") {
      int ix, ec;
      int32_t ac;
      in >> ix >> ec >> a >> ac;
      std::map<std::string, std::map<uint64_t, int32_t>> keep;
      keep.swap(j.tab);
      j = Job();
      j.tab.swap(keep);
      j.ix = ix != 0, j.ec = ec != 0;
      j.has_auditor = a != "nil";
      if (j.has_auditor) j.auditor = unhex(a);
      j.auditor_code = ac;
      int32_t code;
      while (in >> a >> code) {
        j.issuers.push_back(unhex(a));
        j.issuer_codes.push_back(code);
      }
    } else if (kind == "ledger") {
      in >> a >> b;
      Bytes k = unhex(a);
      j.ledger[std::string(k.begin(), k.end())] = unhex(b);
    } else if (kind == "request") {
      int32_t code, failed;
      in >> a >> b >> code >> failed;
      j.raw.push_back(unhex(a));
      j.binding.push_back(unhex(b));
      j.code.push_back(code);
      j.failed.push_back(failed);
    } else if (kind == "run") {
      done += run(j, chunk, inflight);
      j.raw.clear(), j.binding.clear(), j.code.clear(), j.failed.clear();
    } else if (!kind.empty()) {
      uint64_t hash;
      int32_t code;
      in >> a >> code;
      hash = strtoull(a.c_str(), nullptr, 16);
      j.tab[kind][hash] = code;
    }
  }
  printf("ok %zu\n", done);
  return 0;
}
