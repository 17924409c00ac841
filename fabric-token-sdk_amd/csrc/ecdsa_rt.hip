// C ABI of batched x509 ECDSA P-256 signature verification (include/ftsamd.h):
// the auditor's and the issuers' signatures of a token request, and fabtoken
// owners.  Identities and DER signatures are decoded on the host pool
// (host/x509id.cpp); SHA-256 of the message, s^-1 and the curve arithmetic run
// on the GPU (k_ecdsa_pre / _part / _fin, dev/p256.h).  Mirrors idemix_rt.hip.
#include <hip/hip_runtime.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "ecdsa_k.h"
#include "host/x509id.h"
#include "rt_internal.h"

// One pipeline slot: pinned staging, device blob / scalars / partials / verdicts, its stream.
struct EcdsaSlot {
  PinnedMem h_blob, h_ok;
  DevMem d_blob, d_ok, d_u, d_part, d_vt;
  hipStream_t st = nullptr;
  std::vector<uint32_t> idx;  // call-relative indices of the slot's signatures
  bool busy = false;
};

struct ftz_ecdsa {
  ftz_ctx* ctx = nullptr;
  DBuf<P256Aff> tabs;                  // table 0: G; table 1 + k: registered key k (all allocated at creation)
  std::map<std::string, int32_t> ids;  // identity bytes -> key index
  int32_t n_keys = 0;
  std::mutex mu;                       // one call on the device at a time
  WorkPool* pool = nullptr;            // host decoding threads
  EcdsaSlot slot[2];                   // chunk k+1 is decoded and laid out while chunk k runs
  ~ftz_ecdsa() {
    for (EcdsaSlot& q : slot)
      if (q.st) {
        (void)hipStreamSynchronize(q.st);
        (void)hipStreamDestroy(q.st);
      }
    delete pool;
  }
};

namespace {
constexpr size_t ECDSA_CHUNK_BYTES = (size_t)1 << 30;  // keeps every blob offset in 32 bits
constexpr size_t ECDSA_CHUNK_SIGS = 4096;              // signatures per pipelined device pass
constexpr size_t ECDSA_ITEM_BYTES = 16 + ECDSA_SC_BYTES + 16;  // job, scalars / key, message alignment

void table_of(const uint8_t xy[64], std::vector<P256Aff>& tab) {
  uint32_t x[8], y[8];
  be32_to_limbs(x, xy);
  be32_to_limbs(y, xy + 32);
  tab.resize(P256_TAB_ENTRIES);
  p256_build_table(pf_from_int(x), pf_from_int(y), tab.data());
}

struct EcdsaDecoded {
  int code = 0;  // 0 = goes to the device
  uint8_t r[32], s[32], xy[64];
};

// collect the verdicts of a slot's pass
int ecdsa_collect(EcdsaSlot& q, int32_t* codes) {
  if (!q.busy) return FTZ_SUCCESS;
  q.busy = false;
  HC(hipStreamSynchronize(q.st));
  for (size_t k = 0; k < q.idx.size(); k++) codes[q.idx[k]] = q.h_ok.p[k] ? FTZ_OK : FTZ_ERR_SIGNATURE;
  return FTZ_SUCCESS;
}

// decode s[a..b) on the pool; queue the device pass of the ones that reach the curve arithmetic
int ecdsa_chunk(ftz_ecdsa* e, EcdsaSlot& q, const ftz_ecdsa_sig* s, size_t a, size_t b, int32_t* codes) {
  size_t n = b - a;
  std::vector<EcdsaDecoded> dec(n);
  e->pool->run((n + 63) / 64, [&](size_t p) {
    for (size_t i = p * 64; i < n && i < (p + 1) * 64; i++) {
      const ftz_ecdsa_sig& it = s[a + i];
      EcdsaDecoded& d = dec[i];
      // the verifier is deserialized first (identity errors), then Verify unmarshals the signature
      if (it.key < 0) d.code = ftsh::decode_x509_identity(it.identity, it.identity_len, d.xy);
      if (d.code == 0) d.code = ftsh::decode_ecdsa_signature(it.sig, it.sig_len, d.r, d.s);
    }
  });
  // registered-key jobs first, then the ad-hoc ones (k_ecdsa_part's lane ranges)
  std::vector<uint32_t> idx;  // chunk-relative
  for (size_t i = 0; i < n; i++) {
    codes[a + i] = dec[i].code;
    if (dec[i].code == 0 && s[a + i].key >= 0) idx.push_back((uint32_t)i);
  }
  size_t n_reg = idx.size();
  for (size_t i = 0; i < n; i++)
    if (dec[i].code == 0 && s[a + i].key < 0) idx.push_back((uint32_t)i);
  if (idx.empty()) return FTZ_SUCCESS;
  size_t m = idx.size();
  // blob: jobs | r, s, Qx, Qy per job | every distinct message (same pointer and length) once, 16-aligned
  std::vector<EcdsaJob> jobs(m);
  std::vector<uint8_t> copies(m, 0);
  std::unordered_map<const uint8_t*, std::pair<uint32_t, uint32_t>> seen;  // pointer -> (offset, length)
  size_t off = (m * sizeof(EcdsaJob) + 15) & ~(size_t)15;
  for (size_t k = 0; k < m; k++) {
    jobs[k].sc = (uint32_t)off;
    off += ECDSA_SC_BYTES;
  }
  for (size_t k = 0; k < m; k++) {
    const ftz_ecdsa_sig& it = s[a + idx[k]];
    jobs[k].msg_len = (uint32_t)it.msg_len;
    jobs[k].key = it.key >= 0 ? it.key + 1 : -1;
    auto f = it.msg_len ? seen.find(it.msg) : seen.end();
    if (f != seen.end() && f->second.second == it.msg_len) {
      jobs[k].msg = f->second.first;
      continue;
    }
    jobs[k].msg = (uint32_t)off;
    copies[k] = 1;
    if (it.msg_len) seen[it.msg] = {(uint32_t)off, (uint32_t)it.msg_len};
    off += (it.msg_len + 15) & ~(size_t)15;
  }
  size_t total = off + 64;  // slack: the SHA-256 block loads never leave the buffer
  HC(q.h_blob.reserve(total));
  HC(q.d_blob.reserve(total));
  HC(q.h_ok.reserve(m));
  HC(q.d_ok.reserve(m));
  HC(q.d_u.reserve(2 * m * 32));
  HC(q.d_part.reserve(2 * m * sizeof(P256Jac)));
  HC(q.d_vt.reserve((m - n_reg + 1) * P256_VT_WORDS * sizeof(uint32_t)));
  uint8_t* blob = q.h_blob.p;
  memcpy(blob, jobs.data(), m * sizeof(EcdsaJob));
  e->pool->run((m + 63) / 64, [&](size_t p) {
    for (size_t k = p * 64; k < m && k < (p + 1) * 64; k++) {
      const EcdsaDecoded& d = dec[idx[k]];
      const ftz_ecdsa_sig& it = s[a + idx[k]];
      uint8_t* sc = blob + jobs[k].sc;
      memcpy(sc, d.r, 32);
      memcpy(sc + 32, d.s, 32);
      if (it.key < 0)
        memcpy(sc + 64, d.xy, 64);
      else
        memset(sc + 64, 0, 64);
      if (copies[k] && it.msg_len) memcpy(blob + jobs[k].msg, it.msg, it.msg_len);
    }
  });
  const EcdsaJob* djobs = reinterpret_cast<const EcdsaJob*>(q.d_blob.p);
  uint32_t(*du)[8] = reinterpret_cast<uint32_t(*)[8]>(q.d_u.p);
  P256Jac* part = reinterpret_cast<P256Jac*>(q.d_part.p);
  HC(hipMemcpyAsync(q.d_blob.p, q.h_blob.p, off, hipMemcpyHostToDevice, q.st));
  const uint32_t g1 = (uint32_t)((m + 63) / 64), g2 = (uint32_t)((2 * m + 63) / 64);
  k_ecdsa_pre<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, q.d_blob.p, du, q.d_ok.p);
  k_ecdsa_part<<<g2, 64, 0, q.st>>>(djobs, (uint32_t)m, (uint32_t)n_reg, q.d_blob.p, du, e->tabs.p,
                                    reinterpret_cast<uint32_t*>(q.d_vt.p), part);
  k_ecdsa_fin<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, q.d_blob.p, part, q.d_ok.p);
  HC(hipGetLastError());
  HC(hipMemcpyAsync(q.h_ok.p, q.d_ok.p, m, hipMemcpyDeviceToHost, q.st));
  q.idx.resize(m);
  for (size_t k = 0; k < m; k++) q.idx[k] = (uint32_t)(a + idx[k]);
  q.busy = true;
  return FTZ_SUCCESS;
}
}  // namespace

extern "C" int ftz_ecdsa_create(ftz_ctx* ctx, ftz_ecdsa** out) {
  if (!ctx || !out) return set_err(FTZ_E_INVALID, "null argument");
  HC(hipSetDevice(ctx->device));
  std::vector<P256Aff> g;
  uint8_t gxy[64];
  uint32_t t[8];
  pf_to_int(t, pf_const(P256_GX));
  limbs_to_be32(gxy, t);
  pf_to_int(t, pf_const(P256_GY));
  limbs_to_be32(gxy + 32, t);
  table_of(gxy, g);
  ftz_ecdsa* e = new ftz_ecdsa();
  e->ctx = ctx;
  e->pool = new WorkPool(ctx->opt.threads ? (int)ctx->opt.threads : 8);
  for (EcdsaSlot& q : e->slot) {
    hipError_t se = hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking);
    if (se != hipSuccess) {
      delete e;
      return set_err(FTZ_E_DEVICE, std::string("hipStreamCreate failed: ") + hipGetErrorString(se));
    }
  }
  hipError_t he = e->tabs.alloc((size_t)(P256_MAX_KEYS + 1) * P256_TAB_ENTRIES);
  if (he == hipSuccess)
    he = hipMemcpy(e->tabs.p, g.data(), g.size() * sizeof(P256Aff), hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    delete e;
    return set_err(FTZ_E_DEVICE, std::string("ECDSA table upload failed: ") + hipGetErrorString(he));
  }
  *out = e;
  return FTZ_SUCCESS;
}

extern "C" void ftz_ecdsa_destroy(ftz_ecdsa* e) { delete e; }

extern "C" int ftz_x509_public_key(const uint8_t* id, size_t id_len, uint8_t xy[64]) {
  if ((!id && id_len) || !xy) return set_err(FTZ_E_INVALID, "null argument");
  std::string why;
  int code = ftsh::decode_x509_identity(id, id_len, xy, &why);
  if (code != FTZ_OK) g_err = why;
  return code;
}

extern "C" int ftz_ecdsa_add_identity(ftz_ecdsa* e, const uint8_t* id, size_t id_len, int32_t* key) {
  if (!e || !key || (!id && id_len)) return set_err(FTZ_E_INVALID, "null argument");
  std::string bytes((const char*)id, id_len);
  std::lock_guard<std::mutex> lk(e->mu);
  auto f = e->ids.find(bytes);
  if (f != e->ids.end()) {
    *key = f->second;
    return FTZ_SUCCESS;
  }
  uint8_t xy[64];
  std::string why;
  int code = ftsh::decode_x509_identity(id, id_len, xy, &why);
  if (code != FTZ_OK) return set_err(FTZ_E_INVALID, "identity not registered: " + why);
  if (e->n_keys >= P256_MAX_KEYS)
    return set_err(FTZ_E_INVALID, "too many registered keys (at most " + std::to_string(P256_MAX_KEYS) + ")");
  std::vector<P256Aff> tab;
  table_of(xy, tab);
  HC(hipSetDevice(e->ctx->device));
  // no pass is in flight (the verification call holds the mutex until it has collected its slots)
  HC(hipMemcpy(e->tabs.p + (size_t)(e->n_keys + 1) * P256_TAB_ENTRIES, tab.data(), tab.size() * sizeof(P256Aff),
               hipMemcpyHostToDevice));
  *key = e->n_keys++;
  e->ids[bytes] = *key;
  return FTZ_SUCCESS;
}

extern "C" int ftz_verify_ecdsa_signatures(ftz_ecdsa* e, size_t n, const ftz_ecdsa_sig* s, int32_t* codes) {
  if (!e || (n && (!s || !codes))) return set_err(FTZ_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  for (size_t i = 0; i < n; i++) {
    if ((s[i].key < 0 && !s[i].identity && s[i].identity_len) || (!s[i].msg && s[i].msg_len) ||
        (!s[i].sig && s[i].sig_len))
      return set_err(FTZ_E_INVALID, "null buffer with non-zero length");
    if (s[i].msg_len > ECDSA_CHUNK_BYTES / 2) return set_err(FTZ_E_INVALID, "message larger than 512 MiB");
    if (s[i].key < -1 || s[i].key >= e->n_keys)
      return set_err(FTZ_E_INVALID, "key " + std::to_string(s[i].key) + " is not a registered key");
  }
  HC(hipSetDevice(e->ctx->device));
  // chunks of <= ECDSA_CHUNK_SIGS signatures and < ECDSA_CHUNK_BYTES of blob, alternating
  // between the two slots: chunk k+1 is decoded and laid out while chunk k runs
  size_t a = 0, c = 0;
  int rc = FTZ_SUCCESS;
  while (a < n && rc == FTZ_SUCCESS) {
    size_t b = a, bytes = 0;
    while (b < n && b - a < ECDSA_CHUNK_SIGS &&
           (b == a || bytes + s[b].msg_len + ECDSA_ITEM_BYTES < ECDSA_CHUNK_BYTES)) {
      bytes += s[b].msg_len + ECDSA_ITEM_BYTES;
      b++;
    }
    EcdsaSlot& q = e->slot[c & 1];
    rc = ecdsa_collect(q, codes);
    if (rc == FTZ_SUCCESS) rc = ecdsa_chunk(e, q, s, a, b, codes);
    a = b;
    c++;
  }
  for (EcdsaSlot& q : e->slot) {
    int r2 = ecdsa_collect(q, codes);
    if (rc == FTZ_SUCCESS) rc = r2;
  }
  return rc;
}
