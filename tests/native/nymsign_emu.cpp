// TEST-ONLY host build of the pseudonym signing job (dev/nymsign.h,
// dev/hmac256.h) and its host pieces (host/idemix.cpp: the nym check, the
// prefix slot, the proto encoder), for tests/test_nymsign.py and the sanitizer
// program nymsign_main.cpp.  Integers cross the boundary as 32 bytes big-endian.
#include <string.h>

#include <string>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/dev/nymsign.h"
#include "../../fabric-token-sdk_amd/csrc/host/idemix.h"

using namespace fts;

struct EmuNymSign {
  std::vector<uint8_t> ipk_hash;
  std::vector<QDev> tab;  // HSk, HRand
};

namespace {
void words_in(uint32_t w[8], const uint8_t* b) {
  uint32_t l[8];
  be32_to_limbs(l, b);
  nymsign_words(w, l);
}
void words_out(uint8_t* b, const uint32_t w[8]) {
  uint32_t l[8];
  nymsign_words(l, w);
  limbs_to_be32(b, l);
}
// affine X || Y through the variable-time inverse; returns 1 for the point at infinity
int aff_out(uint8_t* o, const Jac<fp>& p) {
  Aff<fp> a = jac_to_aff(p);
  g1_to_bytes(o, a);
  return a.inf ? 1 : 0;
}
// the pass's blob for one signature: the prefix slot at 0, the message at 176 + 4 (= 4 mod 16), RNym after it
struct OneBlob {
  std::vector<uint8_t> b;
  NymSignJob j;
  OneBlob(const EmuNymSign* ix, const uint8_t* rnym, const uint8_t* nym, const uint8_t* msg, size_t msg_len) {
    size_t rn_at = (NYM_PRE_SLOT + 4 + msg_len + 15) & ~(size_t)15;
    b.assign(rn_at + 32, 0);  // exactly what the job may touch: the sanitizer build sees any access past it
    j.pre = 0;
    j.msg = NYM_PRE_SLOT + 4;
    j.msg_len = (uint32_t)msg_len;
    j.signer = 0;
    j.entropy = 0;
    j.rnym = (uint32_t)rn_at;
    ftsh::nymsign_fill_prefix(b.data(), nym, ix->ipk_hash, msg_len);
    if (msg_len) memcpy(b.data() + j.msg, msg, msg_len);
    memcpy(b.data() + rn_at, rnym, 32);
  }
};
Jac<fp> sum_parts(const EmuNymSign* ix, const uint32_t s0[8], const uint32_t s1[8]) {
  // as k_nymsign_part lays them out for n = 1, then nymsign_sum_parts
  QJDev part[NYMSIGN_PARTS];
  for (int p = 0; p < NYMSIGN_PARTS; p++) {
    int base = p / NYMSIGN_SLICES, slice = p % NYMSIGN_SLICES;
    qj_store(part[p], q1_fixed_mul_uniform<fp>(ix->tab.data() + (size_t)base * NYM_TAB_PER_BASE, base ? s1 : s0,
                                               slice * NYMSIGN_PART_WINDOWS, NYMSIGN_PART_WINDOWS));
  }
  return nymsign_sum_parts(part, 1, 0);
}
}  // namespace

extern "C" {

void* nymsign_emu_create(const uint8_t* ipk, size_t len) {
  ftsh::IdemixIpk k;
  if (!ftsh::parse_ipk(ipk, len, k).empty()) return nullptr;
  g1a bases[2];
  if (k.hsk_x.size() != 32 || k.hsk_y.size() != 32 || k.hrand_x.size() != 32 || k.hrand_y.size() != 32) return nullptr;
  if (!bn_point_from_xy(k.hsk_x.data(), k.hsk_y.data(), bases[0]) || bases[0].inf) return nullptr;
  if (!bn_point_from_xy(k.hrand_x.data(), k.hrand_y.data(), bases[1]) || bases[1].inf) return nullptr;
  EmuNymSign* ix = new EmuNymSign();
  ix->ipk_hash = k.hash;
  ix->tab.resize(2 * NYM_TAB_PER_BASE);
  nym_build_tables(bases, 2, ix->tab.data());
  return ix;
}
void nymsign_emu_destroy(void* h) { delete (EmuNymSign*)h; }
int nymsign_emu_parts() { return NYMSIGN_PARTS; }

// Rfc6979::init(x, z, extra) and `count` outputs, 32 bytes each
void nymsign_emu_drbg(const uint8_t* x, const uint8_t* z, const uint8_t* extra, int count, uint8_t* out) {
  uint32_t xw[8], zw[8], ew[8];
  words_in(xw, x);
  words_in(zw, z);
  words_in(ew, extra);
  Rfc6979 g;
  g.init(xw, zw, ew, true);
  for (int k = 0; k < count; k++) {
    g.next();
    words_out(out + 32 * k, g.V);
  }
}
void nymsign_emu_wide(const uint8_t* hi, const uint8_t* lo, uint8_t* out) {
  uint32_t h[8], l[8], r[8];
  be32_to_limbs(h, hi);
  be32_to_limbs(l, lo);
  fr_wide_reduce(r, h, l);
  limbs_to_be32(out, r);
}
// r_sk || r_rnym || nonce as k_nymsign_pre computes them
void nymsign_emu_randomness(const uint8_t* sk, const uint8_t* rnym, const uint8_t* msg, size_t msg_len,
                            const uint8_t* entropy, uint8_t* out) {
  uint32_t dg[8], s[8], r[8], ent[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a[8], b[8], c[8];
  nymsign_msg_digest(dg, msg, (uint32_t)msg_len);
  be32_to_limbs(s, sk);
  be32_to_limbs(r, rnym);
  if (entropy) words_in(ent, entropy);
  nymsign_randomness(a, b, c, s, r, dg, ent, entropy != nullptr);
  limbs_to_be32(out, a);
  limbs_to_be32(out + 32, b);
  limbs_to_be32(out + 64, c);
}
// windows [first, first + count) of k H_base by the uniform routine
int nymsign_emu_fixed(void* h, int base, const uint8_t* k, int first, int count, uint8_t* out) {
  EmuNymSign* ix = (EmuNymSign*)h;
  uint32_t t[8];
  be32_to_limbs(t, k);
  return aff_out(out, q1_fixed_mul_uniform<fp>(ix->tab.data() + (size_t)base * NYM_TAB_PER_BASE, t, first, count));
}
// k H_base by dev/idemix.h's q1_fixed_mul (the verifier's routine)
int nymsign_emu_fixed_plain(void* h, int base, const uint8_t* k, uint8_t* out) {
  EmuNymSign* ix = (EmuNymSign*)h;
  uint32_t t[8];
  be32_to_limbs(t, k);
  return aff_out(out, q1_fixed_mul<fp>(ix->tab.data() + (size_t)base * NYM_TAB_PER_BASE, t));
}
// a point through the fixed-exponent conversion the kernels use
int nymsign_emu_fixed_to_aff(void* h, int base, const uint8_t* k, uint8_t* out) {
  EmuNymSign* ix = (EmuNymSign*)h;
  uint32_t t[8];
  be32_to_limbs(t, k);
  g1_to_bytes(out, nymsign_to_aff(q1_fixed_mul_uniform<fp>(ix->tab.data() + (size_t)base * NYM_TAB_PER_BASE, t, 0,
                                                            NYM_WINDOWS)));
  return 0;
}
// MakeNym as k_nym_make_pre / k_nymsign_part / k_nym_make_fin split it
void nymsign_emu_make_nym(void* h, const uint8_t* sk, const uint8_t* rnym, uint8_t* out) {
  uint32_t s0[8], s1[8];
  be32_to_limbs(s0, sk);
  be32_to_limbs(s1, rnym);
  g1_to_bytes(out, nymsign_to_aff(sum_parts((EmuNymSign*)h, s0, s1)));
}
int nymsign_emu_nym_ok(const uint8_t* nym) { return ftsh::nymsign_nym_ok(nym) ? 1 : 0; }
int nymsign_emu_scalar_ok(const uint8_t* k, int nonzero) { return ftsh::nymsign_scalar_ok(k, nonzero != 0) ? 1 : 0; }
void nymsign_emu_encode(const uint8_t* raw, uint8_t* out) { ftsh::encode_nym_signature(raw, out); }
// The whole job as the kernels and the runtime split it: the nym check, pre, the parts, fin, the
// encoder.  FTZ_OK with 136 bytes in sig, or FTZ_ERR_OWNER with sig zeroed.
int nymsign_emu_sign(void* h, const uint8_t* sk, const uint8_t* rnym, const uint8_t* nym, const uint8_t* msg,
                     size_t msg_len, const uint8_t* entropy, uint8_t* sig) {
  EmuNymSign* ix = (EmuNymSign*)h;
  if (!ftsh::nymsign_nym_ok(nym)) {
    memset(sig, 0, FTZ_NYMSIG_LEN);
    return FTZ_ERR_OWNER;
  }
  OneBlob ob(ix, rnym, nym, msg, msg_len);
  uint32_t dg[8], s[8], r[8], ent[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a[8], b[8], c[8];
  nymsign_msg_digest(dg, ob.b.data() + ob.j.msg, ob.j.msg_len);
  be32_to_limbs(s, sk);
  be32_to_limbs(r, ob.b.data() + ob.j.rnym);
  if (entropy) words_in(ent, entropy);
  nymsign_randomness(a, b, c, s, r, dg, ent, entropy != nullptr);
  uint8_t raw[NYMSIGN_RAW_BYTES];
  job_nymsign_fin(ob.j, ob.b.data(), sum_parts(ix, a, b), s, a, b, c, raw);
  ftsh::encode_nym_signature(raw, sig);
  return FTZ_OK;
}
}
