// TEST-ONLY host build of the signed request path: the product's orchestration
// (host/request.cpp verify_signed_token_requests) over the host builds of the
// proof jobs (emu_exec.cpp), the idemix owner signatures (idemix_emu.cpp) and
// the x509 ECDSA signatures (ecdsa_emu.cpp), so the CPU tier checks every
// verdict of the signed path without a GPU.  Built by tests/test_signed_requests.py
// into a library of its own, beside the sources of libftsemu.so.  Never loaded
// by the product.
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/dev/jobs.h"
#include "../../fabric-token-sdk_amd/csrc/host/planner.h"
#include "../../fabric-token-sdk_amd/csrc/host/request.h"
#include "../../include/ftsamd.h"

extern "C" {
int emu_verify_transfers(void* ctx, size_t n, const ftz_transfer* tx, int32_t* codes);
int emu_verify_issues(void* ctx, size_t n, const ftz_issue* is, int32_t* codes);
int emu_verify_owner_signatures(void* ix, size_t n, const ftz_owner_sig* s, int32_t* codes);
int ecdsa_emu_identity(const uint8_t* id, size_t len, uint8_t* xy);
int ecdsa_emu_verify(const uint8_t* id, size_t id_len, const uint8_t* registered_xy, const uint8_t* msg,
                     size_t msg_len, const uint8_t* sig, size_t sig_len);
}

namespace {
// the registered keys of the emulated x509 handle: index -> X || Y
struct EmuKeys {
  std::vector<std::vector<uint8_t>> xy;
  std::map<std::string, int32_t> ids;
  ftsh::SignerKey add(const uint8_t* id, size_t len) {
    ftsh::SignerKey k;
    std::string b((const char*)id, len);
    auto f = ids.find(b);
    if (f != ids.end()) {
      k.key = f->second;
      return k;
    }
    uint8_t p[64];
    k.code = ecdsa_emu_identity(id, len, p);
    if (k.code) return k;
    k.key = (int32_t)xy.size();
    xy.emplace_back(p, p + 64);
    ids[b] = k.key;
    return k;
  }
};
}  // namespace

extern "C" {

// the signed message of a request that decodes: 0 and *out_len (bytes written
// when cap is large enough), or -1 when der_token_request refuses `raw`
int emu_signed_message(const uint8_t* raw, size_t len, const uint8_t* binding, size_t blen, uint8_t* out, size_t cap,
                       size_t* out_len) {
  std::vector<ftsh::Slice> f[4];
  if (!ftsh::der_token_request(raw, len, f).empty()) return -1;
  std::vector<uint8_t> m;
  ftsh::signed_message(raw, len, binding, blen, m);
  *out_len = m.size();
  if (m.size() <= cap && !m.empty()) memcpy(out, m.data(), m.size());
  return 0;
}

// ftz_verify_signed_token_requests on the host: ctx from emu_ctx_create, ix from
// emu_idemix_create_curve (or NULL), use_ec 0 = no x509 handle.  chunk /
// inflight 0 = the product's defaults.
int emu_verify_signed_token_requests(void* ctx, void* ix, int use_ec, const uint8_t* auditor, size_t auditor_len,
                                     const ftz_bytes* issuers, size_t n_issuers, size_t n,
                                     const ftz_signed_request* reqs, ftz_get_states_fn get_states, void* user,
                                     size_t chunk, size_t inflight, int par_threads, int32_t* codes,
                                     int32_t* failed) {
  using namespace fts;
  ftsh::RequestHooks h;
  h.check = [](size_t m, const uint8_t* slots, uint8_t* ok) {
    for (size_t i = 0; i < m; i++) {
      g1a a;
      ok[i] = g1_setbytes(slots + 64 * i, 64, a) ? 1 : 0;
    }
    return 0;
  };
  h.verify_transfers = [ctx](size_t m, const ftz_transfer* tx, int32_t* c) { return emu_verify_transfers(ctx, m, tx, c); };
  h.verify_issues = [ctx](size_t m, const ftz_issue* is, int32_t* c) { return emu_verify_issues(ctx, m, is, c); };
  h.get_states = get_states;
  h.user = user;
  if (chunk) h.chunk = chunk;
  if (inflight) h.inflight = inflight;
  std::unique_ptr<ftsh::WorkPool> pool;
  if (par_threads > 0) {
    pool.reset(new ftsh::WorkPool(par_threads));
    ftsh::WorkPool* pp = pool.get();
    h.par = [pp](size_t k, const std::function<void(size_t)>& f) { pp->run(k, f); };
  }
  EmuKeys keys;
  ftsh::RequestSigners sg;
  if (ix) sg.verify_owners = [ix](size_t m, const ftz_owner_sig* s, int32_t* c) { return emu_verify_owner_signatures(ix, m, s, c); };
  if (use_ec)
    sg.verify_ecdsa = [&keys](size_t m, const ftz_ecdsa_sig* s, int32_t* c) {
      static std::mutex mu;  // ecdsa_emu_verify caches its key tables without a lock
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < m; i++) {
        if (s[i].key >= (int32_t)keys.xy.size()) return (int)FTZ_E_INVALID;
        c[i] = ecdsa_emu_verify(s[i].identity, s[i].identity_len, s[i].key >= 0 ? keys.xy[s[i].key].data() : nullptr,
                                s[i].msg, s[i].msg_len, s[i].sig, s[i].sig_len);
      }
      return (int)FTZ_SUCCESS;
    };
  sg.has_auditor = auditor != nullptr;
  sg.auditor = ftsh::Slice{auditor, auditor ? auditor_len : 0};
  if (use_ec && sg.auditor.len) sg.auditor_key = keys.add(auditor, auditor_len);
  sg.issuers.resize(n_issuers);
  sg.issuer_keys.resize(n_issuers);
  for (size_t i = 0; i < n_issuers; i++) {
    sg.issuers[i] = ftsh::Slice{issuers[i].p, issuers[i].len};
    if (use_ec) sg.issuer_keys[i] = keys.add(issuers[i].p, issuers[i].len);
  }
  std::vector<ftz_bytes> raw(n), bind(n);
  for (size_t i = 0; i < n; i++) raw[i] = reqs[i].raw, bind[i] = reqs[i].binding;
  sg.bindings = bind.data();
  std::string err;
  return ftsh::verify_signed_token_requests(n, raw.data(), h, sg, codes, failed, err);
}

}  // extern "C"
