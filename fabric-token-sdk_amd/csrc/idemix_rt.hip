// C ABI of idemix owner-signature verification (include/ftsamd.h, SURVEY 8(f)
// row 3) on BN254 or FP256BN_AMCL: owner identity and signature protos decoded
// on the host pool (host/idemix.cpp), NymSignature.Ver's curve arithmetic and
// hashes on the GPU (k_nym_part/_fin, _bn for BN254; dev/idemix.h).  On BN254
// the same handle signs: NewNymSignature and MakeNym in batches (k_nymsign_*,
// dev/nymsign.h), the second half of this file.
#include <hip/hip_runtime.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "host/idemix.h"
#include "launch.h"
#include "nymsign_k.h"
#include "rt_internal.h"

// One pipeline slot: pinned staging, device blob / partials / verdicts, its stream.
struct NymSlot {
  PinnedMem h_blob, h_ok;
  DevMem d_blob, d_ok, d_part;
  hipStream_t st = nullptr;
  std::vector<uint32_t> idx;  // call-relative indices of the slot's signatures
  bool busy = false;
  // signing passes on the same slot (a call collects its passes before it returns the mutex)
  PinnedMem h_sig;
  DevMem d_sig, d_rand;      // 128 bytes + ok byte per signature; r_sk, r_rnym, nonce
  size_t sec_at = 0, sec_len = 0;  // the blob's section of RNym values
  bool sbusy = false;
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
  DBuf<uint32_t> skeys;        // NYMSIGN_MAX_SIGNERS x 8 limbs (256 bytes), allocated with the first signer
  int32_t n_signers = 0;
  PinnedMem h_mk;              // ftz_idemix_make_nyms staging: RNym values in, nyms out
  DevMem d_mk;
  ~ftz_idemix() {
    for (NymSlot& q : slot)
      if (q.st) {
        (void)hipStreamSynchronize(q.st);
        (void)hipStreamDestroy(q.st);
      }
    if (skeys.p) (void)hipMemset(skeys.p, 0, skeys.n * sizeof(uint32_t));
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
    hipError_t se = hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking);
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
constexpr size_t NYM_CHUNK_BYTES = (size_t)1 << 30;  // keeps every blob offset in 32 bits
constexpr size_t NYM_CHUNK_SIGS = 4096;              // signatures per pipelined device pass

// collect the verdicts of a slot's pass
int nym_collect(NymSlot& q, int32_t* codes) {
  if (!q.busy) return FTZ_SUCCESS;
  q.busy = false;
  HC(hipStreamSynchronize(q.st));
  for (size_t k = 0; k < q.idx.size(); k++) codes[q.idx[k]] = q.h_ok.p[k] ? FTZ_OK : FTZ_ERR_SIGNATURE;
  return FTZ_SUCCESS;
}

// decode s[a..b) on the pool; queue the device pass of the ones that reach the curve arithmetic
int nym_chunk(ftz_idemix* ix, NymSlot& q, const ftz_owner_sig* s, size_t a, size_t b, int32_t* codes) {
  size_t n = b - a;
  std::vector<ftsh::NymDecoded> dec(n);
  ix->pool->run((n + 63) / 64, [&](size_t p) {
    for (size_t i = p * 64; i < n && i < (p + 1) * 64; i++)
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
  q.idx.resize(m);
  for (size_t k = 0; k < m; k++) q.idx[k] = (uint32_t)(a + idx[k]);
  q.busy = true;
  return FTZ_SUCCESS;
}
}  // namespace

extern "C" int ftz_verify_owner_signatures(ftz_idemix* ix, size_t n, const ftz_owner_sig* s, int32_t* codes) {
  if (!ix || (n && (!s || !codes))) return set_err(FTZ_E_INVALID, "null argument");
  for (size_t i = 0; i < n; i++) {
    if ((!s[i].owner && s[i].owner_len) || (!s[i].msg && s[i].msg_len) || (!s[i].sig && s[i].sig_len))
      return set_err(FTZ_E_INVALID, "null buffer with non-zero length");
    if (s[i].msg_len > NYM_CHUNK_BYTES / 2) return set_err(FTZ_E_INVALID, "message larger than 512 MiB");
  }
  std::lock_guard<std::mutex> lk(ix->mu);
  HC(hipSetDevice(ix->ctx->device));
  // chunks of <= NYM_CHUNK_SIGS signatures and < NYM_CHUNK_BYTES of blob, alternating
  // between the two slots: chunk k+1 is decoded and laid out while chunk k runs
  size_t a = 0, c = 0;
  int rc = FTZ_SUCCESS;
  while (a < n && rc == FTZ_SUCCESS) {
    size_t b = a, bytes = 0;
    while (b < n && b - a < NYM_CHUNK_SIGS && (b == a || bytes + s[b].msg_len + 512 < NYM_CHUNK_BYTES)) {
      bytes += s[b].msg_len + 512;
      b++;
    }
    NymSlot& q = ix->slot[c & 1];
    rc = nym_collect(q, codes);
    if (rc == FTZ_SUCCESS) rc = nym_chunk(ix, q, s, a, b, codes);
    a = b;
    c++;
  }
  for (NymSlot& q : ix->slot) {
    int r2 = nym_collect(q, codes);
    if (rc == FTZ_SUCCESS) rc = r2;
  }
  return rc;
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
  ix->pool->run((n + 63) / 64, [&](size_t p) {
    for (size_t i = p * 64; i < n && i < (p + 1) * 64; i++)
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
  if (!q.sbusy) return FTZ_SUCCESS;
  q.sbusy = false;
  hipError_t he = hipStreamSynchronize(q.st);
  explicit_bzero(q.h_blob.p + q.sec_at, q.sec_len);
  if (he != hipSuccess)
    return set_err(FTZ_E_DEVICE, std::string("hipStreamSynchronize failed: ") + hipGetErrorString(he));
  const size_t m = q.idx.size();
  const uint8_t* raw = q.h_sig.p;
  const uint8_t* ok = q.h_sig.p + m * NYMSIGN_RAW_BYTES;
  ix->pool->run((m + 63) / 64, [&](size_t p) {
    for (size_t k = p * 64; k < m && k < (p + 1) * 64; k++) {
      uint8_t* out = sigs + (size_t)q.idx[k] * FTZ_NYMSIG_LEN;
      if (!ok[k]) {
        memset(out, 0, FTZ_NYMSIG_LEN);
        codes[q.idx[k]] = FTZ_ERR_SIGNATURE;
        continue;
      }
      ftsh::encode_nym_signature(raw + k * NYMSIGN_RAW_BYTES, out);
      codes[q.idx[k]] = FTZ_OK;
    }
  });
  return FTZ_SUCCESS;
}

// check the nyms of it[a..b) on the pool, lay out the rest and queue their device pass
int nymsign_chunk(ftz_idemix* ix, NymSlot& q, const ftz_nym_sign_item* it, size_t a, size_t b, uint8_t* sigs,
                  int32_t* codes) {
  const size_t n = b - a;
  std::vector<uint8_t> good(n, 0);
  ix->pool->run((n + 63) / 64, [&](size_t p) {
    for (size_t i = p * 64; i < n && i < (p + 1) * 64; i++) good[i] = ftsh::nymsign_nym_ok(it[a + i].nym) ? 1 : 0;
  });
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
  std::vector<uint8_t> copies(m, 0);
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
  std::map<std::pair<const uint8_t*, size_t>, uint32_t> at;
  for (size_t k = 0; k < m; k++) {
    const ftz_nym_sign_item& s = it[a + idx[k]];
    jobs[k].msg_len = (uint32_t)s.msg_len;
    jobs[k].signer = s.signer;
    jobs[k].rnym = (uint32_t)(rnym_at + k * 32);
    jobs[k].pre = (uint32_t)(pre_at + k * NYM_PRE_SLOT);
    auto key = std::make_pair(s.msg, s.msg_len);
    auto f = at.find(key);
    if (f == at.end()) {
      off = ((off + 15) & ~(size_t)15) + NymCurve<fp>::PRE % 16;
      f = at.emplace(key, (uint32_t)off).first;
      copies[k] = 1;
      off += s.msg_len;
    }
    jobs[k].msg = f->second;
  }
  const size_t total = off + 64;  // slack: the hash reads whole 16-byte words
  HC(q.h_blob.reserve(total));
  HC(q.d_blob.reserve(total));
  HC(q.h_sig.reserve(m * (NYMSIGN_RAW_BYTES + 1)));
  HC(q.d_sig.reserve(m * (NYMSIGN_RAW_BYTES + 1)));
  HC(q.d_rand.reserve(3 * m * 32));
  HC(q.d_part.reserve(NYMSIGN_PARTS * m * sizeof(QJDev)));
  uint8_t* blob = q.h_blob.p;
  memcpy(blob, jobs.data(), m * sizeof(NymSignJob));
  ix->pool->run((m + 63) / 64, [&](size_t p) {
    for (size_t k = p * 64; k < m && k < (p + 1) * 64; k++) {
      const ftz_nym_sign_item& s = it[a + idx[k]];
      memcpy(blob + jobs[k].rnym, s.r_nym, 32);
      if (s.entropy) memcpy(blob + jobs[k].entropy, s.entropy, 32);
      ftsh::nymsign_fill_prefix(blob + jobs[k].pre, s.nym, ix->ipk_hash, s.msg_len);
      if (copies[k] && s.msg_len) memcpy(blob + jobs[k].msg, s.msg, s.msg_len);
    }
  });
  // from here on the staging buffer holds RNym values: nymsign_collect wipes them, also after an error below
  q.sec_at = rnym_at;
  q.sec_len = m * 32;
  q.idx.resize(m);
  for (size_t k = 0; k < m; k++) q.idx[k] = (uint32_t)(a + idx[k]);
  q.sbusy = true;
  const NymSignJob* djobs = reinterpret_cast<const NymSignJob*>(q.d_blob.p);
  const uint32_t(*keys)[8] = reinterpret_cast<const uint32_t(*)[8]>(ix->skeys.p);
  uint32_t(*d_rsk)[8] = reinterpret_cast<uint32_t(*)[8]>(q.d_rand.p);
  uint32_t(*d_rrn)[8] = d_rsk + m;
  uint32_t(*d_non)[8] = d_rrn + m;
  QJDev* part = reinterpret_cast<QJDev*>(q.d_part.p);
  uint8_t* d_raw = q.d_sig.p;
  uint8_t* d_ok = q.d_sig.p + m * NYMSIGN_RAW_BYTES;
  HC(hipMemcpyAsync(q.d_blob.p, q.h_blob.p, off, hipMemcpyHostToDevice, q.st));
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
  if (ix->n_signers >= NYMSIGN_MAX_SIGNERS) {
    rc = set_err(FTZ_E_INVALID, "too many signers (at most " + std::to_string(NYMSIGN_MAX_SIGNERS) + ")");
  } else {
    he = hipSetDevice(ix->ctx->device);
    if (he == hipSuccess && !ix->skeys.p) {
      he = ix->skeys.alloc((size_t)NYMSIGN_MAX_SIGNERS * 8);
      if (he == hipSuccess) he = hipMemset(ix->skeys.p, 0, ix->skeys.n * sizeof(uint32_t));
    }
    // no pass is in flight (a call holds the mutex until it has collected its slots)
    if (he == hipSuccess) he = hipMemcpy(ix->skeys.p + (size_t)ix->n_signers * 8, l, sizeof l, hipMemcpyHostToDevice);
    if (he == hipSuccess) *signer = ix->n_signers++;
  }
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
    if (it[i].msg_len > NYM_CHUNK_BYTES / 2) return set_err(FTZ_E_INVALID, "message larger than 512 MiB");
    if (it[i].signer < 0 || it[i].signer >= ix->n_signers)
      return set_err(FTZ_E_INVALID, "signer " + std::to_string(it[i].signer) + " is not a registered signer");
    if (!ftsh::nymsign_scalar_ok(it[i].r_nym, false))
      return set_err(FTZ_E_INVALID, "r_nym of item " + std::to_string(i) + " is not below the group order");
  }
  if (n == 0) return FTZ_SUCCESS;
  HC(hipSetDevice(ix->ctx->device));
  // chunks of <= NYM_CHUNK_SIGS signatures and < NYM_CHUNK_BYTES of blob, alternating
  // between the two slots: chunk k+1 is laid out while chunk k runs
  size_t a = 0, c = 0;
  while (a < n && rc == FTZ_SUCCESS) {
    size_t b = a, bytes = 0;
    while (b < n && b - a < NYM_CHUNK_SIGS &&
           (b == a || bytes + it[b].msg_len + NYMSIGN_ITEM_BYTES < NYM_CHUNK_BYTES)) {
      bytes += it[b].msg_len + NYMSIGN_ITEM_BYTES;
      b++;
    }
    NymSlot& q = ix->slot[c & 1];
    rc = nymsign_collect(ix, q, sigs, codes);
    if (rc == FTZ_SUCCESS) rc = nymsign_chunk(ix, q, it, a, b, sigs, codes);
    a = b;
    c++;
  }
  for (NymSlot& q : ix->slot) {
    int r2 = nymsign_collect(ix, q, sigs, codes);
    if (rc == FTZ_SUCCESS) rc = r2;
  }
  return rc;
}

// MakeNym in batches: Nym_i = sk HSk + RNym_i HRand through the signing pass's parts kernel
extern "C" int ftz_idemix_make_nyms(ftz_idemix* ix, int32_t signer, size_t n, const uint8_t* r_nyms, uint8_t* nyms) {
  if (!ix || (n && (!r_nyms || !nyms))) return set_err(FTZ_E_INVALID, "null argument");
  int rc = nymsign_check_handle(ix);
  if (rc != FTZ_SUCCESS) return rc;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (signer < 0 || signer >= ix->n_signers)
    return set_err(FTZ_E_INVALID, "signer " + std::to_string(signer) + " is not a registered signer");
  for (size_t i = 0; i < n; i++)
    if (!ftsh::nymsign_scalar_ok(r_nyms + i * 32, false))
      return set_err(FTZ_E_INVALID, "r_nym " + std::to_string(i) + " is not below the group order");
  if (n == 0) return FTZ_SUCCESS;
  HC(hipSetDevice(ix->ctx->device));
  NymSlot& q = ix->slot[0];
  const uint32_t(*keys)[8] = reinterpret_cast<const uint32_t(*)[8]>(ix->skeys.p);
  const size_t cap = NYM_CHUNK_SIGS;
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
