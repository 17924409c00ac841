// C ABI of idemix owner-signature verification (include/ftsamd.h, SURVEY 8(f)
// row 3) on BN254 or FP256BN_AMCL: owner identity and signature protos decoded
// on the host pool (host/idemix.cpp), NymSignature.Ver's curve arithmetic and
// hashes on the GPU (k_nym_part/_fin, _bn for BN254; dev/idemix.h).  On BN254
// the same handle signs: NewNymSignature and MakeNym in batches (k_nymsign_*,
// dev/nymsign.h), the second half of this file.  Both calls run their chunks
// through the two-slot driver of host/sigpipe.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "host/idemix.h"
#include "launch.h"
#include "nymsign_k.h"
#include "sigpipe_rt.h"

// One pipeline slot: pinned staging, device blob / partials / verdicts.  A call holds the handle's mutex
// until it has collected its passes, so verifying and signing passes share the slots.
struct NymSlot : SigSlot {
  PinnedMem h_blob, h_ok;
  DevMem d_blob, d_ok, d_part;
  // signing passes
  PinnedMem h_sig;
  DevMem d_sig, d_rand;      // 128 bytes + ok byte per signature; r_sk, r_rnym, nonce
  size_t rnym_at = 0;        // the blob's section of RNym values, 32 bytes per item of the pass
};

struct ftz_idemix {
  ftz_ctx* ctx = nullptr;
  int curve = FTZ_CURVE_FP256BN_AMCL;
  std::vector<uint8_t> ipk_hash;  // IssuerPublicKey.Hash (copy(proofData[index:], ipk.Hash))
  DBuf<QDev> tab;              // HSk, HRand (and HAttrs[2]) fixed-base tables
  size_t n_hattrs = 0;         // len(IssuerPublicKey.HAttrs)
  bool heid_ok = false;        // HAttrs[2] decoded on the curve (its table exists)
  bool strict_nym = false;     // ftz_idemix_set_strict_nym: reject off-curve nyms on the host
  PinnedMem h_eid, h_eid_ok;   // auditor owner match (ftz_audit_owners)
  DevMem d_eid, d_eid_ok;
  std::mutex mu;               // one call on the device at a time
  WorkPool* pool = nullptr;    // host decoding / layout threads
  NymSlot slot[2];             // chunk k+1 is decoded and laid out while chunk k runs
  // signing (ftz_idemix_add_signer / ftz_sign_owner_signatures / ftz_idemix_make_nyms): the user
  // secrets live on the device only
  SignerKeys signers;          // NYMSIGN_MAX_SIGNERS of them
  PinnedMem h_mk;              // ftz_idemix_make_nyms staging: RNym values in, nyms out
  DevMem d_mk;
  ~ftz_idemix() {
    for (NymSlot& q : slot) q.close();
    signers.wipe();
    delete pool;
  }
};

extern "C" int ftz_idemix_create(ftz_ctx* ctx, const uint8_t* ipk, size_t ipk_len, int curve_id, ftz_idemix** out) {
  if (!ctx || !out || (!ipk && ipk_len)) return set_err(FTZ_E_INVALID, "null argument");
  if (curve_id != FTZ_CURVE_FP256BN_AMCL && curve_id != FTZ_CURVE_BN254)
    return set_err(FTZ_E_INVALID, "unsupported idemix curve id " + std::to_string(curve_id) +
                                      " (BN254 = 1 or FP256BN_AMCL = 0)");
  if (ipk_len == 0) return set_err(FTZ_E_PP, "empty idemix issuer public key");
  ftsh::IdemixIpk k;
  std::string e = ftsh::parse_ipk(ipk, ipk_len, k);
  if (!e.empty()) return set_err(FTZ_E_PP, e);
  bool heid = false;
  std::vector<QDev> tab;
  if (curve_id == FTZ_CURVE_BN254) {
    // gurvy G1FromProto: exactly 32-byte coordinates, gnark SetBytes
    g1a bases[3];
    auto dec = [](const std::vector<uint8_t>& x, const std::vector<uint8_t>& y, g1a& a) {
      return x.size() == 32 && y.size() == 32 && bn_point_from_xy(x.data(), y.data(), a) && !a.inf;
    };
    if (!dec(k.hsk_x, k.hsk_y, bases[0]) || !dec(k.hrand_x, k.hrand_y, bases[1]))
      return set_err(FTZ_E_PP, "issuer public key: HSk / HRand not a finite BN254 point");
    heid = k.hattrs_x.size() > 2 && dec(k.hattrs_x[2], k.hattrs_y[2], bases[2]);
    tab.resize((heid ? 3 : 2) * NYM_TAB_PER_BASE);
    nym_build_tables(bases, heid ? 3 : 2, tab.data());
  } else {
    q1a bases[3];
    if (!nym_point_from_be(k.hsk_x.data(), k.hsk_y.data(), bases[0]) ||
        !nym_point_from_be(k.hrand_x.data(), k.hrand_y.data(), bases[1]))
      return set_err(FTZ_E_PP, "issuer public key: HSk / HRand not on FP256BN");
    // HAttrs[2] (the enrollment-id base of the auditor's EidNym check)
    heid = k.hattrs_x.size() > 2 && k.hattrs_x[2].size() >= 32 && k.hattrs_y[2].size() >= 32 &&
           nym_point_from_be(k.hattrs_x[2].data(), k.hattrs_y[2].data(), bases[2]);
    tab.resize((heid ? 3 : 2) * NYM_TAB_PER_BASE);
    nym_build_tables(bases, heid ? 3 : 2, tab.data());
  }
  HC(hipSetDevice(ctx->device));
  ftz_idemix* ix = new ftz_idemix();
  ix->ctx = ctx;
  ix->pool = new WorkPool(ctx->opt.threads ? (int)ctx->opt.threads : 8);
  for (NymSlot& q : ix->slot) {
    hipError_t se = q.open();
    if (se != hipSuccess) {
      delete ix;
      return set_err(FTZ_E_DEVICE, std::string("hipStreamCreate failed: ") + hipGetErrorString(se));
    }
  }
  ix->curve = curve_id;
  ix->ipk_hash = k.hash;
  ix->n_hattrs = k.hattrs_x.size();
  ix->heid_ok = heid;
  hipError_t he = ix->tab.upload(tab, ctx->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
  if (he != hipSuccess) {
    delete ix;
    return set_err(FTZ_E_DEVICE, std::string("idemix table upload failed: ") + hipGetErrorString(he));
  }
  *out = ix;
  return FTZ_SUCCESS;
}

void ftz_idemix_destroy(ftz_idemix* ix) { delete ix; }

extern "C" int ftz_idemix_set_strict_nym(ftz_idemix* ix, int on) {
  if (!ix) return set_err(FTZ_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->strict_nym = on != 0;
  return FTZ_SUCCESS;
}

namespace {
constexpr size_t NYM_ITEM_BYTES = 512;  // per signature beside its message: job, integers, prefix slot, alignment

// decode s[a..b) on the pool; queue the device pass of the ones that reach the curve arithmetic
int nym_chunk(ftz_idemix* ix, NymSlot& q, const ftz_owner_sig* s, size_t a, size_t b, int32_t* codes) {
  size_t n = b - a;
  std::vector<ftsh::NymDecoded> dec(n);
  par_for(ix->pool, n, [&](size_t i) {
    ftsh::decode_owner_signature(s[a + i].owner, s[a + i].owner_len, s[a + i].sig, s[a + i].sig_len, dec[i],
                                 ix->curve);
  });
  std::vector<uint32_t> idx;  // chunk-relative
  for (size_t i = 0; i < n; i++) {
    if (ix->strict_nym && ix->curve == FTZ_CURVE_FP256BN_AMCL && dec[i].code == 0) {
      q1a nym;
      if (!nym_point_from_be(dec[i].ints[0], dec[i].ints[1], nym)) {
        dec[i].code = FTZ_ERR_OWNER;
        dec[i].why = "pseudonym is not on FP256BN (strict nym import)";
      }
    }
    codes[a + i] = dec[i].code;
    if (dec[i].code == 0) idx.push_back((uint32_t)i);
  }
  if (idx.empty()) return FTZ_SUCCESS;
  size_t m = idx.size();
  ftsh::NymLayout L;
  ftsh::nym_plan_layout(s + a, idx.data(), m, L, ix->curve);
  HC(q.h_blob.reserve(L.total));
  HC(q.d_blob.reserve(L.total));
  HC(q.h_ok.reserve(m));
  HC(q.d_ok.reserve(m));
  HC(q.d_part.reserve(4 * m * sizeof(QJDev)));
  WorkPool* pool = ix->pool;
  ftsh::nym_fill(s + a, idx.data(), m, dec.data(), ix->ipk_hash, L, q.h_blob.p,
                 [pool](size_t k, const std::function<void(size_t)>& f) { pool->run(k, f); }, ix->curve);
  const NymJob* jobs = reinterpret_cast<const NymJob*>(q.d_blob.p);
  QJDev* part = reinterpret_cast<QJDev*>(q.d_part.p);
  sig_pass_begin(q, a, idx.data(), m);
  HC(hipMemcpyAsync(q.d_blob.p, q.h_blob.p, L.total, hipMemcpyHostToDevice, q.st));
  const uint32_t gp = (uint32_t)((4 * m + 63) / 64), gf = (uint32_t)((m + 63) / 64);
  if (ix->curve == FTZ_CURVE_BN254) {
    k_nym_part_bn<<<gp, 64, 0, q.st>>>(jobs, (uint32_t)m, q.d_blob.p, ix->tab.p, part);
    k_nym_fin_bn<<<gf, 64, 0, q.st>>>(jobs, (uint32_t)m, q.d_blob.p, part, q.d_ok.p);
  } else {
    k_nym_part<<<gp, 64, 0, q.st>>>(jobs, (uint32_t)m, q.d_blob.p, ix->tab.p, part);
    k_nym_fin<<<gf, 64, 0, q.st>>>(jobs, (uint32_t)m, q.d_blob.p, part, q.d_ok.p);
  }
  HC(hipGetLastError());
  HC(hipMemcpyAsync(q.h_ok.p, q.d_ok.p, m, hipMemcpyDeviceToHost, q.st));
  q.enqueued = true;
  return FTZ_SUCCESS;
}
}  // namespace

extern "C" int ftz_verify_owner_signatures(ftz_idemix* ix, size_t n, const ftz_owner_sig* s, int32_t* codes) {
  if (!ix || (n && (!s || !codes))) return set_err(FTZ_E_INVALID, "null argument");
  for (size_t i = 0; i < n; i++) {
    if ((!s[i].owner && s[i].owner_len) || (!s[i].msg && s[i].msg_len) || (!s[i].sig && s[i].sig_len))
      return set_err(FTZ_E_INVALID, "null buffer with non-zero length");
    if (s[i].msg_len > ftsh::SIG_CHUNK_BYTES / 2) return set_err(FTZ_E_INVALID, "message larger than 512 MiB");
  }
  std::lock_guard<std::mutex> lk(ix->mu);
  HC(hipSetDevice(ix->ctx->device));
  return ftsh::sig_run(
      n, ftsh::SIG_CHUNK_ITEMS, ftsh::SIG_CHUNK_BYTES, [&](size_t i) { return s[i].msg_len + NYM_ITEM_BYTES; },
      [&](int k) { return sig_collect_verdicts(ix->slot[k], ix->slot[k].h_ok.p, codes); },
      [&](int k, size_t a, size_t b) { return nym_chunk(ix, ix->slot[k], s, a, b, codes); });
}

// Auditor owner match: decode on the pool, one device pass over the tokens
// whose check reaches the curve arithmetic
extern "C" int ftz_audit_owners(ftz_idemix* ix, size_t n, const ftz_owner_audit* it, int32_t* codes) {
  if (!ix || (n && (!it || !codes))) return set_err(FTZ_E_INVALID, "null argument");
  for (size_t i = 0; i < n; i++)
    if ((!it[i].owner && it[i].owner_len) || (!it[i].audit_info && it[i].audit_info_len))
      return set_err(FTZ_E_INVALID, "null buffer with non-zero length");
  if (n > (1u << 26)) return set_err(FTZ_E_INVALID, "too many tokens in one call");
  if (ix->n_hattrs > 2 && !ix->heid_ok) return set_err(FTZ_E_PP, "issuer public key: HAttrs[2] not on the idemix curve");
  std::vector<ftsh::EidDecoded> dec(n);
  par_for(ix->pool, n, [&](size_t i) {
    ftsh::decode_owner_audit(it[i].owner, it[i].owner_len, it[i].audit_info, it[i].audit_info_len, ix->n_hattrs,
                             dec[i], ix->curve);
  });
  std::vector<uint32_t> idx;
  for (size_t i = 0; i < n; i++) {
    codes[i] = dec[i].code;
    if (dec[i].code == 0) idx.push_back((uint32_t)i);
  }
  if (idx.empty()) return FTZ_SUCCESS;
  std::lock_guard<std::mutex> lk(ix->mu);
  HC(hipSetDevice(ix->ctx->device));
  size_t m = idx.size();
  HC(ix->h_eid.reserve(m * EID_JOB_BYTES));
  HC(ix->d_eid.reserve(m * EID_JOB_BYTES));
  HC(ix->h_eid_ok.reserve(m));
  HC(ix->d_eid_ok.reserve(m));
  for (size_t k = 0; k < m; k++) {
    const ftsh::EidDecoded& d = dec[idx[k]];
    uint8_t* o = ix->h_eid.p + k * EID_JOB_BYTES;
    memcpy(o, d.eid_digest, 32);
    memcpy(o + 32, d.rnym, 32);
    memcpy(o + 64, d.nym_x, 32);
    memcpy(o + 96, d.nym_y, 32);
  }
  hipStream_t st = ix->slot[0].st;
  HC(hipMemcpyAsync(ix->d_eid.p, ix->h_eid.p, m * EID_JOB_BYTES, hipMemcpyHostToDevice, st));
  if (ix->curve == FTZ_CURVE_BN254)
    k_eid_bn<<<(uint32_t)((m + 63) / 64), 64, 0, st>>>(ix->d_eid.p, (uint32_t)m, ix->tab.p, ix->d_eid_ok.p);
  else
    k_eid<<<(uint32_t)((m + 63) / 64), 64, 0, st>>>(ix->d_eid.p, (uint32_t)m, ix->tab.p, ix->d_eid_ok.p);
  HC(hipGetLastError());
  HC(hipMemcpyAsync(ix->h_eid_ok.p, ix->d_eid_ok.p, m, hipMemcpyDeviceToHost, st));
  HC(hipStreamSynchronize(st));
  for (size_t k = 0; k < m; k++) codes[idx[k]] = ix->h_eid_ok.p[k] ? FTZ_OK : FTZ_ERR_AUDIT;
  return FTZ_SUCCESS;
}

// ------------------------------------------------------------------ signing (BN254)
// SigningIdentity.Sign (identity/msp/idemix/id.go:195-210 -> IBM/idemix
// NewNymSignature) in batches: SHA-256 of the message, the DRBG, the two
// fixed-base products, the transcript hash and the responses on the GPU
// (k_nymsign_pre / _part / _fin, dev/nymsign.h), the proto on the host pool.
// r_sk, r_rnym and the partial sums never leave the device; the RNym values
// cross the pinned staging buffer, which is wiped after each pass.
namespace {
static_assert(NYMSIGN_MAX_SIGNERS == FTZ_IDEMIX_MAX_SIGNERS, "the device array holds what the header promises");
static_assert(4 * 34 == FTZ_NYMSIG_LEN, "four fields of tag, length and 32 bytes");
// per item beside its message: job, RNym, entropy, prefix slot, message alignment
constexpr size_t NYMSIGN_ITEM_BYTES = sizeof(NymSignJob) + 32 + 32 + NYM_PRE_SLOT + 20;

int nymsign_check_handle(ftz_idemix* ix) {
  if (ix->curve != FTZ_CURVE_BN254)
    return set_err(FTZ_E_INVALID, "idemix signing is implemented on BN254 only (this handle is FP256BN_AMCL: "
                                  "the device has no scalar field mod n for that curve)");
  return FTZ_SUCCESS;
}

// wait for a slot's signing pass, write its protos and wipe the staged RNym values
int nymsign_collect(ftz_idemix* ix, NymSlot& q, uint8_t* sigs, int32_t* codes) {
  if (!q.busy) return FTZ_SUCCESS;
  int rc = sig_pass_end(q);
  const size_t m = q.idx.size();
  explicit_bzero(q.h_blob.p + q.rnym_at, m * 32);
  if (rc != FTZ_SUCCESS) {  // the wipes the pass ends with may not have run
    (void)hipMemset(q.d_blob.p + q.rnym_at, 0, m * 32);
    (void)hipMemset(q.d_rand.p, 0, 3 * m * 32);
    (void)hipMemset(q.d_part.p, 0, NYMSIGN_PARTS * m * sizeof(QJDev));
    return rc;
  }
  const uint8_t* raw = q.h_sig.p;
  const uint8_t* ok = q.h_sig.p + m * NYMSIGN_RAW_BYTES;
  par_for(ix->pool, m, [&](size_t k) {
    uint8_t* out = sigs + (size_t)q.idx[k] * FTZ_NYMSIG_LEN;
    if (!ok[k]) {
      memset(out, 0, FTZ_NYMSIG_LEN);
      codes[q.idx[k]] = FTZ_ERR_SIGNATURE;
      return;
    }
    ftsh::encode_nym_signature(raw + k * NYMSIGN_RAW_BYTES, out);
    codes[q.idx[k]] = FTZ_OK;
  });
  return FTZ_SUCCESS;
}

// check the nyms of it[a..b) on the pool, lay out the rest and queue their device pass
int nymsign_chunk(ftz_idemix* ix, NymSlot& q, const ftz_nym_sign_item* it, size_t a, size_t b, uint8_t* sigs,
                  int32_t* codes) {
  const size_t n = b - a;
  std::vector<uint8_t> good(n, 0);
  par_for(ix->pool, n, [&](size_t i) { good[i] = ftsh::nymsign_nym_ok(it[a + i].nym) ? 1 : 0; });
  std::vector<uint32_t> idx;  // chunk-relative
  for (size_t i = 0; i < n; i++) {
    if (good[i]) {
      idx.push_back((uint32_t)i);
    } else {
      codes[a + i] = FTZ_ERR_OWNER;
      memset(sigs + (a + i) * FTZ_NYMSIG_LEN, 0, FTZ_NYMSIG_LEN);
    }
  }
  const size_t m = idx.size();
  if (m == 0) return FTZ_SUCCESS;
  // blob: jobs | the RNym values, contiguous | 32 entropy bytes per hedged job | the prefix slots | every distinct
  // message (same pointer and length) once, aligned as nym_plan_layout aligns them
  std::vector<NymSignJob> jobs(m);
  size_t off = (m * sizeof(NymSignJob) + 15) & ~(size_t)15;
  const size_t rnym_at = off;
  off += m * 32;
  for (size_t k = 0; k < m; k++) {
    jobs[k].entropy = 0;
    if (it[a + idx[k]].entropy) {
      jobs[k].entropy = (uint32_t)off;
      off += 32;
    }
  }
  const size_t pre_at = off;
  off += m * NYM_PRE_SLOT;
  auto msg = [&](size_t k) { return std::make_pair(it[a + idx[k]].msg, it[a + idx[k]].msg_len); };
  MsgLayout L;
  sig_layout_messages(m, off, NymCurve<fp>::PRE % 16, msg, L);
  const size_t total = L.end + 64;  // slack: the hash reads whole 16-byte words
  HC(q.h_blob.reserve(total));
  HC(q.d_blob.reserve(total));
  HC(q.h_sig.reserve(m * (NYMSIGN_RAW_BYTES + 1)));
  HC(q.d_sig.reserve(m * (NYMSIGN_RAW_BYTES + 1)));
  HC(q.d_rand.reserve(3 * m * 32));
  HC(q.d_part.reserve(NYMSIGN_PARTS * m * sizeof(QJDev)));
  uint8_t* blob = q.h_blob.p;
  // from here on the staging buffer holds RNym values: nymsign_collect wipes them, also after an error below
  q.rnym_at = rnym_at;
  sig_pass_begin(q, a, idx.data(), m);
  par_for(ix->pool, m + L.distinct.size(), [&](size_t k) {  // the jobs, then the messages
    if (k >= m) return sig_copy_message(L, k - m, blob, msg);
    const ftz_nym_sign_item& s = it[a + idx[k]];
    NymSignJob& j = jobs[k];
    j.msg = L.msg_off[k];
    j.msg_len = (uint32_t)s.msg_len;
    j.signer = s.signer;
    j.rnym = (uint32_t)(rnym_at + k * 32);
    j.pre = (uint32_t)(pre_at + k * NYM_PRE_SLOT);
    memcpy(blob + k * sizeof(NymSignJob), &j, sizeof j);
    memcpy(blob + j.rnym, s.r_nym, 32);
    if (s.entropy) memcpy(blob + j.entropy, s.entropy, 32);
    ftsh::nymsign_fill_prefix(blob + j.pre, s.nym, ix->ipk_hash, s.msg_len);
  });
  const NymSignJob* djobs = reinterpret_cast<const NymSignJob*>(q.d_blob.p);
  const uint32_t(*keys)[8] = ix->signers.keys();
  uint32_t(*d_rsk)[8] = reinterpret_cast<uint32_t(*)[8]>(q.d_rand.p);
  uint32_t(*d_rrn)[8] = d_rsk + m;
  uint32_t(*d_non)[8] = d_rrn + m;
  QJDev* part = reinterpret_cast<QJDev*>(q.d_part.p);
  uint8_t* d_raw = q.d_sig.p;
  uint8_t* d_ok = q.d_sig.p + m * NYMSIGN_RAW_BYTES;
  HC(hipMemcpyAsync(q.d_blob.p, q.h_blob.p, L.end, hipMemcpyHostToDevice, q.st));
  HC(hipMemsetAsync(d_ok, 0, m, q.st));
  const uint32_t g1 = (uint32_t)((m + 63) / 64), gp = (uint32_t)((NYMSIGN_PARTS * m + 63) / 64);
  k_nymsign_pre<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, q.d_blob.p, keys, d_rsk, d_rrn, d_non);
  k_nymsign_part<<<gp, 64, 0, q.st>>>((uint32_t)m, d_rsk, d_rrn, ix->tab.p, part);
  k_nymsign_fin<<<g1, 64, 0, q.st>>>(djobs, (uint32_t)m, q.d_blob.p, keys, part, d_rsk, d_rrn, d_non, d_raw, d_ok);
  HC(hipGetLastError());
  HC(hipMemcpyAsync(q.h_sig.p, q.d_sig.p, m * (NYMSIGN_RAW_BYTES + 1), hipMemcpyDeviceToHost, q.st));
  // nothing secret stays behind the pass: the RNym values, the randomness (k_nymsign_fin has zeroed its own) and
  // the partial sums, from which the windows of r_sk and r_rnym could be read back
  HC(hipMemsetAsync(q.d_blob.p + rnym_at, 0, m * 32, q.st));
  HC(hipMemsetAsync(q.d_rand.p, 0, 3 * m * 32, q.st));
  HC(hipMemsetAsync(q.d_part.p, 0, NYMSIGN_PARTS * m * sizeof(QJDev), q.st));
  q.enqueued = true;
  return FTZ_SUCCESS;
}
}  // namespace

extern "C" int ftz_idemix_add_signer(ftz_idemix* ix, const uint8_t sk[32], int32_t* signer) {
  if (!ix || !sk || !signer) return set_err(FTZ_E_INVALID, "null argument");
  int rc = nymsign_check_handle(ix);
  if (rc != FTZ_SUCCESS) return rc;
  if (!ftsh::nymsign_scalar_ok(sk, true)) return set_err(FTZ_E_INVALID, "user secret not in [1, r)");
  uint32_t l[8];
  be32_to_limbs(l, sk);
  std::lock_guard<std::mutex> lk(ix->mu);
  hipError_t he = hipSuccess;
  if (ix->signers.n >= NYMSIGN_MAX_SIGNERS)
    rc = set_err(FTZ_E_INVALID, "too many signers (at most " + std::to_string(NYMSIGN_MAX_SIGNERS) + ")");
  else
    he = ix->signers.add(ix->ctx->device, NYMSIGN_MAX_SIGNERS, l, signer);
  explicit_bzero(l, sizeof l);
  if (he != hipSuccess) return set_err(FTZ_E_DEVICE, std::string("signer upload failed: ") + hipGetErrorString(he));
  return rc;
}

extern "C" int ftz_sign_owner_signatures(ftz_idemix* ix, size_t n, const ftz_nym_sign_item* it, uint8_t* sigs,
                                         int32_t* codes) {
  if (!ix || (n && (!it || !sigs || !codes))) return set_err(FTZ_E_INVALID, "null argument");
  int rc = nymsign_check_handle(ix);
  if (rc != FTZ_SUCCESS) return rc;
  std::lock_guard<std::mutex> lk(ix->mu);
  for (size_t i = 0; i < n; i++) {
    if (!it[i].msg && it[i].msg_len) return set_err(FTZ_E_INVALID, "null buffer with non-zero length");
    if (!it[i].r_nym || !it[i].nym) return set_err(FTZ_E_INVALID, "null r_nym or nym");
    if (it[i].msg_len > ftsh::SIG_CHUNK_BYTES / 2) return set_err(FTZ_E_INVALID, "message larger than 512 MiB");
    if (it[i].signer < 0 || it[i].signer >= ix->signers.n)
      return set_err(FTZ_E_INVALID, "signer " + std::to_string(it[i].signer) + " is not a registered signer");
    if (!ftsh::nymsign_scalar_ok(it[i].r_nym, false))
      return set_err(FTZ_E_INVALID, "r_nym of item " + std::to_string(i) + " is not below the group order");
  }
  if (n == 0) return FTZ_SUCCESS;
  HC(hipSetDevice(ix->ctx->device));
  return ftsh::sig_run(
      n, ftsh::SIG_CHUNK_ITEMS, ftsh::SIG_CHUNK_BYTES, [&](size_t i) { return it[i].msg_len + NYMSIGN_ITEM_BYTES; },
      [&](int k) { return nymsign_collect(ix, ix->slot[k], sigs, codes); },
      [&](int k, size_t a, size_t b) { return nymsign_chunk(ix, ix->slot[k], it, a, b, sigs, codes); });
}

// MakeNym in batches: Nym_i = sk HSk + RNym_i HRand through the signing pass's parts kernel
extern "C" int ftz_idemix_make_nyms(ftz_idemix* ix, int32_t signer, size_t n, const uint8_t* r_nyms, uint8_t* nyms) {
  if (!ix || (n && (!r_nyms || !nyms))) return set_err(FTZ_E_INVALID, "null argument");
  int rc = nymsign_check_handle(ix);
  if (rc != FTZ_SUCCESS) return rc;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (signer < 0 || signer >= ix->signers.n)
    return set_err(FTZ_E_INVALID, "signer " + std::to_string(signer) + " is not a registered signer");
  for (size_t i = 0; i < n; i++)
    if (!ftsh::nymsign_scalar_ok(r_nyms + i * 32, false))
      return set_err(FTZ_E_INVALID, "r_nym " + std::to_string(i) + " is not below the group order");
  if (n == 0) return FTZ_SUCCESS;
  HC(hipSetDevice(ix->ctx->device));
  NymSlot& q = ix->slot[0];
  const uint32_t(*keys)[8] = ix->signers.keys();
  const size_t cap = ftsh::SIG_CHUNK_ITEMS;
  HC(ix->h_mk.reserve(cap * 64));
  HC(ix->d_mk.reserve(cap * (32 + 64)));
  HC(q.d_rand.reserve(3 * cap * 32));
  HC(q.d_part.reserve(NYMSIGN_PARTS * cap * sizeof(QJDev)));
  for (size_t a = 0; a < n && rc == FTZ_SUCCESS; a += cap) {
    const size_t m = n - a < cap ? n - a : cap;
    uint8_t* d_in = ix->d_mk.p;
    uint8_t* d_out = ix->d_mk.p + cap * 32;
    uint32_t(*s0)[8] = reinterpret_cast<uint32_t(*)[8]>(q.d_rand.p);
    uint32_t(*s1)[8] = s0 + m;
    QJDev* part = reinterpret_cast<QJDev*>(q.d_part.p);
    memcpy(ix->h_mk.p, r_nyms + a * 32, m * 32);
    hipError_t he = hipMemcpyAsync(d_in, ix->h_mk.p, m * 32, hipMemcpyHostToDevice, q.st);
    if (he == hipSuccess) {
      const uint32_t g1 = (uint32_t)((m + 63) / 64), gp = (uint32_t)((NYMSIGN_PARTS * m + 63) / 64);
      k_nym_make_pre<<<g1, 64, 0, q.st>>>((uint32_t)m, keys, signer, d_in, s0, s1);
      k_nymsign_part<<<gp, 64, 0, q.st>>>((uint32_t)m, s0, s1, ix->tab.p, part);
      k_nym_make_fin<<<g1, 64, 0, q.st>>>((uint32_t)m, part, s0, s1, d_out);
      he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(ix->h_mk.p, d_out, m * 64, hipMemcpyDeviceToHost, q.st);
    if (he == hipSuccess) he = hipMemsetAsync(d_in, 0, m * 32, q.st);
    if (he == hipSuccess) he = hipMemsetAsync(q.d_rand.p, 0, 2 * m * 32, q.st);
    if (he == hipSuccess) he = hipMemsetAsync(q.d_part.p, 0, NYMSIGN_PARTS * m * sizeof(QJDev), q.st);
    hipError_t hs = hipStreamSynchronize(q.st);
    if (he == hipSuccess) he = hs;
    if (he == hipSuccess)
      memcpy(nyms + a * 64, ix->h_mk.p, m * 64);
    else
      rc = set_err(FTZ_E_DEVICE, std::string("make_nyms pass failed: ") + hipGetErrorString(he));
    explicit_bzero(ix->h_mk.p, m * 64);  // the staged RNym values (overwritten by the nyms on success)
  }
  return rc;
}
