// C ABI of batched x509 ECDSA P-256 signature verification (include/ftsamd.h):
// the auditor's and the issuers' signatures of a token request, and fabtoken
// owners.  Identities and DER signatures are decoded on the host pool
// (host/x509id.cpp); SHA-256 of the message, s^-1 and the curve arithmetic run
// on the GPU (k_ecdsa_pre / _part / _fin, dev/p256.h).  The second half signs.
// Both calls run their chunks through the two-slot driver of host/sigpipe.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "ecdsa_k.h"
#include "ecsign_k.h"
#include "host/x509id.h"
#include "sigpipe_rt.h"

// One pipeline slot: pinned staging, device blob / scalars / partials / verdicts.
struct EcdsaSlot : SigSlot {
  PinnedMem h_blob, h_ok;
  DevMem d_blob, d_ok, d_u, d_part, d_vt;
};

// One pipeline slot of the signer: pinned staging, device blob / nonces / digests / partials / r || s.
struct EcsignSlot : SigSlot {
  PinnedMem h_blob, h_out;
  DevMem d_blob, d_out, d_k, d_e, d_part;
};

struct ftz_ecdsa {
  ftz_ctx* ctx = nullptr;
  DBuf<P256Aff> tabs;                  // table 0: G; table 1 + k: registered key k (all allocated at creation)
  std::map<std::string, int32_t> ids;  // identity bytes -> key index
  int32_t n_keys = 0;
  std::mutex mu;                       // one call on the device at a time
  WorkPool* pool = nullptr;            // host decoding threads
  EcdsaSlot slot[2];
  // signing (ftz_ecdsa_add_signer / ftz_sign_ecdsa): the private scalars live on the device only
  std::vector<P256Aff> gtab;           // host copy of table 0 (public keys of new signers)
  SignerKeys signers;                  // ECSIGN_MAX_SIGNERS of them
  EcsignSlot sslot[2];                 // streams created by the first signing call
  ~ftz_ecdsa() {
    for (EcsignSlot& q : sslot) q.close();  // no signing pass reads the keys any more
    signers.wipe();
    for (EcdsaSlot& q : slot) q.close();
    delete pool;
  }
};

namespace {
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

// decode s[a..b) on the pool; queue the device pass of the ones that reach the curve arithmetic
int ecdsa_chunk(ftz_ecdsa* e, EcdsaSlot& q, const ftz_ecdsa_sig* s, size_t a, size_t b, int32_t* codes) {
  size_t n = b - a;
  std::vector<EcdsaDecoded> dec(n);
  par_for(e->pool, n, [&](size_t i) {
    const ftz_ecdsa_sig& it = s[a + i];
    EcdsaDecoded& d = dec[i];
    // the verifier is deserialized first (identity errors), then Verify unmarshals the signature
    if (it.key < 0) d.code = ftsh::decode_x509_identity(it.identity, it.identity_len, d.xy);
    if (d.code == 0) d.code = ftsh::decode_ecdsa_signature(it.sig, it.sig_len, d.r, d.s);
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
  // blob: jobs | r, s, Qx, Qy per job | every distinct message once, 16-aligned
  const size_t sc_at = (m * sizeof(EcdsaJob) + 15) & ~(size_t)15;
  auto msg = [&](size_t k) { return std::make_pair(s[a + idx[k]].msg, s[a + idx[k]].msg_len); };
  MsgLayout L;
  sig_layout_messages(m, sc_at + m * ECDSA_SC_BYTES, 0, msg, L);
  size_t total = L.end + 64;  // slack: the SHA-256 block loads never leave the buffer
  HC(q.h_blob.reserve(total));
  HC(q.d_blob.reserve(total));
  HC(q.h_ok.reserve(m));
  HC(q.d_ok.reserve(m));
  HC(q.d_u.reserve(2 * m * 32));
  HC(q.d_part.reserve(2 * m * sizeof(P256Jac)));
  HC(q.d_vt.reserve((m - n_reg + 1) * P256_VT_WORDS * sizeof(uint32_t)));
  uint8_t* blob = q.h_blob.p;
  par_for(e->pool, m + L.distinct.size(), [&](size_t k) {  // the jobs, then the messages
    if (k >= m) return sig_copy_message(L, k - m, blob, msg);
    const EcdsaDecoded& d = dec[idx[k]];
    const ftz_ecdsa_sig& it = s[a + idx[k]];
    EcdsaJob j;
    j.sc = (uint32_t)(sc_at + k * ECDSA_SC_BYTES);
    j.msg = L.msg_off[k];
    j.msg_len = (uint32_t)it.msg_len;
    j.key = it.key >= 0 ? it.key + 1 : -1;
    memcpy(blob + k * sizeof(EcdsaJob), &j, sizeof j);
    uint8_t* sc = blob + j.sc;
    memcpy(sc, d.r, 32);
    memcpy(sc + 32, d.s, 32);
    if (it.key < 0)
      memcpy(sc + 64, d.xy, 64);
    else
      memset(sc + 64, 0, 64);
  });
  const EcdsaJob* djobs = reinterpret_cast<const EcdsaJob*>(q.d_blob.p);
  uint32_t(*du)[8] = reinterpret_cast<uint32_t(*)[8]>(q.d_u.p);
  P256Jac* part = reinterpret_cast<P256Jac*>(q.d_part.p);
  sig_pass_begin(q, a, idx.data(), m);
  HC(hipMemcpyAsync(q.d_blob.p, q.h_blob.p, L.end, hipMemcpyHostToDevice, q.st));
  const uint32_t g1 = (uint32_t)((m + 63) / 64), g2 = (uint32_t)((2 * m + 63) / 64);
  k_ecdsa_pre<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, q.d_blob.p, du, q.d_ok.p);
  k_ecdsa_part<<<g2, 64, 0, q.st>>>(djobs, (uint32_t)m, (uint32_t)n_reg, q.d_blob.p, du, e->tabs.p,
                                    reinterpret_cast<uint32_t*>(q.d_vt.p), part);
  k_ecdsa_fin<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, q.d_blob.p, part, q.d_ok.p);
  HC(hipGetLastError());
  HC(hipMemcpyAsync(q.h_ok.p, q.d_ok.p, m, hipMemcpyDeviceToHost, q.st));
  q.enqueued = true;
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
    hipError_t se = q.open();
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
  e->gtab = std::move(g);
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
    if (s[i].msg_len > ftsh::SIG_CHUNK_BYTES / 2) return set_err(FTZ_E_INVALID, "message larger than 512 MiB");
    if (s[i].key < -1 || s[i].key >= e->n_keys)
      return set_err(FTZ_E_INVALID, "key " + std::to_string(s[i].key) + " is not a registered key");
  }
  HC(hipSetDevice(e->ctx->device));
  return ftsh::sig_run(
      n, ftsh::SIG_CHUNK_ITEMS, ftsh::SIG_CHUNK_BYTES, [&](size_t i) { return s[i].msg_len + ECDSA_ITEM_BYTES; },
      [&](int k) { return sig_collect_verdicts(e->slot[k], e->slot[k].h_ok.p, codes); },
      [&](int k, size_t a, size_t b) { return ecdsa_chunk(e, e->slot[k], s, a, b, codes); });
}

// ------------------------------------------------------------------ signing
// edsaSigner.Sign (identity/msp/x509/ecdsa.go:50-64) in batches: SHA-256, the
// RFC 6979 nonce, k G, r, s and ToLowS on the GPU (k_ecsign_pre / _part /
// _fin, dev/ecsign.h), DER on the host pool.  The nonces never leave the device.
namespace {
constexpr size_t ECSIGN_ITEM_BYTES = sizeof(EcsignJob) + 32 + 16;  // job, entropy, message alignment
static_assert(ECSIGN_MAX_SIGNERS == FTZ_ECDSA_MAX_SIGNERS, "the device array holds what the header promises");

// wait for a slot's pass and write its DER signatures
int ecsign_collect(ftz_ecdsa* e, EcsignSlot& q, uint8_t* sigs, uint32_t* sig_lens, int32_t* codes) {
  if (!q.busy) return FTZ_SUCCESS;
  int rc = sig_pass_end(q);
  const size_t m = q.idx.size();
  if (rc != FTZ_SUCCESS) {  // the wipes the pass ends with may not have run
    (void)hipMemset(q.d_k.p, 0, m * 32);
    (void)hipMemset(q.d_e.p, 0, m * 32);
    (void)hipMemset(q.d_part.p, 0, ECSIGN_PARTS * m * sizeof(P256Jac));
    return rc;
  }
  const uint8_t* rs = q.h_out.p;
  const uint8_t* ok = q.h_out.p + m * 64;
  par_for(e->pool, m, [&](size_t k) {
    const size_t i = q.idx[k];
    uint8_t* out = sigs + i * FTZ_ECDSA_SIG_MAX;
    memset(out, 0, FTZ_ECDSA_SIG_MAX);
    if (!ok[k]) {
      sig_lens[i] = 0;
      codes[i] = FTZ_ERR_SIGNATURE;
      return;
    }
    sig_lens[i] = (uint32_t)ftsh::encode_ecdsa_signature(rs + k * 64, rs + k * 64 + 32, out);
    codes[i] = FTZ_OK;
  });
  return FTZ_SUCCESS;
}

// lay out it[a..b) and queue its device pass
int ecsign_chunk(ftz_ecdsa* e, EcsignSlot& q, const ftz_ecdsa_sign_item* it, size_t a, size_t b) {
  const size_t m = b - a;
  // blob: jobs | 32 entropy bytes per hedged job | every distinct message once, 16-aligned
  std::vector<EcsignJob> jobs(m);
  size_t off = (m * sizeof(EcsignJob) + 15) & ~(size_t)15;
  for (size_t k = 0; k < m; k++) {
    jobs[k].entropy = 0;
    if (it[a + k].entropy) {
      jobs[k].entropy = (uint32_t)off;
      off += 32;
    }
  }
  auto msg = [&](size_t k) { return std::make_pair(it[a + k].msg, it[a + k].msg_len); };
  MsgLayout L;
  sig_layout_messages(m, off, 0, msg, L);
  const size_t total = L.end + 64;  // slack: the SHA-256 block loads never leave the buffer
  HC(q.h_blob.reserve(total));
  HC(q.d_blob.reserve(total));
  HC(q.h_out.reserve(m * 65));
  HC(q.d_out.reserve(m * 65));
  HC(q.d_k.reserve(m * 32));
  HC(q.d_e.reserve(m * 32));
  HC(q.d_part.reserve(ECSIGN_PARTS * m * sizeof(P256Jac)));
  uint8_t* blob = q.h_blob.p;
  par_for(e->pool, m + L.distinct.size(), [&](size_t k) {  // the jobs, then the messages
    if (k >= m) return sig_copy_message(L, k - m, blob, msg);
    const ftz_ecdsa_sign_item& s = it[a + k];
    jobs[k].msg = L.msg_off[k];
    jobs[k].msg_len = (uint32_t)s.msg_len;
    jobs[k].signer = s.signer;
    memcpy(blob + k * sizeof(EcsignJob), &jobs[k], sizeof(EcsignJob));
    if (s.entropy) memcpy(blob + jobs[k].entropy, s.entropy, 32);
  });
  const EcsignJob* djobs = reinterpret_cast<const EcsignJob*>(q.d_blob.p);
  uint32_t(*dk)[8] = reinterpret_cast<uint32_t(*)[8]>(q.d_k.p);
  uint32_t(*de)[8] = reinterpret_cast<uint32_t(*)[8]>(q.d_e.p);
  P256Jac* part = reinterpret_cast<P256Jac*>(q.d_part.p);
  uint8_t* d_rs = q.d_out.p;
  uint8_t* d_ok = q.d_out.p + m * 64;
  sig_pass_begin(q, a, nullptr, m);
  HC(hipMemcpyAsync(q.d_blob.p, q.h_blob.p, L.end, hipMemcpyHostToDevice, q.st));
  const uint32_t g1 = (uint32_t)((m + 63) / 64), g4 = (uint32_t)((ECSIGN_PARTS * m + 63) / 64);
  k_ecsign_pre<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, q.d_blob.p, e->signers.keys(), dk, de);
  k_ecsign_part<<<g4, 64, 0, q.st>>>((uint32_t)m, dk, e->tabs.p, part);
  k_ecsign_fin<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, e->signers.keys(), part, dk, de, d_rs, d_ok);
  HC(hipGetLastError());
  HC(hipMemcpyAsync(q.h_out.p, q.d_out.p, m * 65, hipMemcpyDeviceToHost, q.st));
  // nothing secret stays behind the pass: the nonces (k_ecsign_fin has zeroed its own), the digests
  // and the partial sums of k G, from which the windows of k could be read back
  HC(hipMemsetAsync(q.d_k.p, 0, m * 32, q.st));
  HC(hipMemsetAsync(q.d_e.p, 0, m * 32, q.st));
  HC(hipMemsetAsync(q.d_part.p, 0, ECSIGN_PARTS * m * sizeof(P256Jac), q.st));
  q.enqueued = true;
  return FTZ_SUCCESS;
}
}  // namespace

extern "C" int ftz_ecdsa_add_signer(ftz_ecdsa* e, const uint8_t d[32], int32_t* signer, uint8_t public_xy[64]) {
  if (!e || !d || !signer) return set_err(FTZ_E_INVALID, "null argument");
  uint32_t dl[8];
  be32_to_limbs(dl, d);
  if (u256_is_zero(dl) || u256_geq(dl, P256_N)) {
    explicit_bzero(dl, sizeof dl);
    return set_err(FTZ_E_INVALID, "private scalar not in [1, n)");
  }
  std::lock_guard<std::mutex> lk(e->mu);
  int rc = FTZ_SUCCESS;
  hipError_t he = hipSuccess;
  if (e->signers.n >= ECSIGN_MAX_SIGNERS) {
    rc = set_err(FTZ_E_INVALID, "too many signers (at most " + std::to_string(ECSIGN_MAX_SIGNERS) + ")");
  } else {
    if (public_xy) {  // d G on the host; d < n is no multiple of n: never infinity
      p256j q = p256_fixed_mul(e->gtab.data(), dl);
      pf zi = pf_inv(q.z);
      pf zi2 = pf_sqr(zi);
      uint32_t t[8];
      pf_to_int(t, q.x * zi2);
      limbs_to_be32(public_xy, t);
      pf_to_int(t, q.y * zi2 * zi);
      limbs_to_be32(public_xy + 32, t);
    }
    he = e->signers.add(e->ctx->device, ECSIGN_MAX_SIGNERS, dl, signer);
  }
  explicit_bzero(dl, sizeof dl);
  if (he != hipSuccess) return set_err(FTZ_E_DEVICE, std::string("signer upload failed: ") + hipGetErrorString(he));
  return rc;
}

extern "C" int ftz_sign_ecdsa(ftz_ecdsa* e, size_t n, const ftz_ecdsa_sign_item* it, uint8_t* sigs,
                              uint32_t* sig_lens, int32_t* codes) {
  if (!e || (n && (!it || !sigs || !sig_lens || !codes))) return set_err(FTZ_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  for (size_t i = 0; i < n; i++) {
    if (!it[i].msg && it[i].msg_len) return set_err(FTZ_E_INVALID, "null buffer with non-zero length");
    if (it[i].msg_len > ftsh::SIG_CHUNK_BYTES / 2) return set_err(FTZ_E_INVALID, "message larger than 512 MiB");
    if (it[i].signer < 0 || it[i].signer >= e->signers.n)
      return set_err(FTZ_E_INVALID, "signer " + std::to_string(it[i].signer) + " is not a registered signer");
  }
  if (n == 0) return FTZ_SUCCESS;
  HC(hipSetDevice(e->ctx->device));
  for (EcsignSlot& q : e->sslot) HC(q.open());
  return ftsh::sig_run(
      n, ftsh::SIG_CHUNK_ITEMS, ftsh::SIG_CHUNK_BYTES, [&](size_t i) { return it[i].msg_len + ECSIGN_ITEM_BYTES; },
      [&](int k) { return ecsign_collect(e, e->sslot[k], sigs, sig_lens, codes); },
      [&](int k, size_t a, size_t b) { return ecsign_chunk(e, e->sslot[k], it, a, b); });
}
