// The idemix pseudonym signing job of token owners on BN254: IBM/idemix
// NewNymSignature (identity/msp/idemix/id.go:195-210 SigningIdentity.Sign ->
// CSP.Sign(UserKey, msg, IdemixNymSignerOpts)) and the pseudonym derivation
// MakeNym, restated (oracle idemix.py bn_nym_sign / bn_make_nym):
//   t = r_sk HSk + r_rnym HRand
//   c = HashToZr("sign" || t || Nym || ipk.Hash || msg || 00 00)
//   ProofC = HashToZr(c || nonce)
//   ProofSSk = r_sk + ProofC sk,  ProofSRNym = r_rnym + ProofC RNym   (mod r)
// The reference draws r_sk, r_rnym and nonce from crypto/rand.  Here they are
// the output of the HMAC-SHA-256 DRBG of dev/hmac256.h, keyed with the user
// secret, the message digest and RNym (nymsign_randomness): signatures are a
// function of their inputs, optionally hedged with 32 bytes of caller entropy.
// Only the generator is RFC 6979's: each value is 512 DRBG bits reduced mod r
// (bias below 2^-250), without that RFC's retry loop.
//
// Everything is FTS_HD like dev/idemix.h: device (k_nymsign.hip), host emulation
// (tests).  Secrets here are sk, RNym, r_sk and r_rnym (the nonce is
// published).  No branch and no trip count depends on them in the table walk,
// the DRBG or the responses: digits pick table entries by address (an accepted
// limit: the process owns the device), every other choice is a select on
// values.  The sum of the partial points uses curve.h's full addition, whose
// exceptional branches need an all-zero window slice or two equal partials
// (probability below 2^-120 each).
#pragma once
#include "hmac256.h"
#include "idemix.h"

namespace fts {

#ifndef FTS_NYMSIGN_PARTS
#define FTS_NYMSIGN_PARTS 4  // 2, 4 or 8 (build.py --variant; the sweep is in profiles/nymsign_parts_sweep.json)
#endif
static constexpr int NYMSIGN_PARTS = FTS_NYMSIGN_PARTS;                     // lanes per signature in k_nymsign_part
static constexpr int NYMSIGN_SLICES = NYMSIGN_PARTS / 2;                    // window ranges per base
static constexpr int NYMSIGN_PART_WINDOWS = NYM_WINDOWS / NYMSIGN_SLICES;  // windows per lane
static_assert(NYMSIGN_SLICES >= 1 && 2 * NYMSIGN_SLICES == NYMSIGN_PARTS, "two bases, the same slices of each");
static_assert(NYMSIGN_SLICES * NYMSIGN_PART_WINDOWS == NYM_WINDOWS, "the slices cover the windows exactly");
static constexpr int NYMSIGN_MAX_SIGNERS = 8;
static constexpr uint32_t NYMSIGN_RAW_BYTES = 128;  // ProofC, ProofSSk, ProofSRNym, Nonce: 32 bytes BE each

// One signature on the device: offsets into the pass's blob.
struct NymSignJob {
  uint32_t msg;  // blob offset of the message, = NymCurve<fp>::PRE mod 16 (4-aligned; stream byte 192 is 16-aligned)
  uint32_t msg_len;
  int32_t signer;    // index into the handle's user secrets
  uint32_t entropy;  // blob offset (16-aligned) of 32 bytes of entropy; 0: none (offset 0 holds the jobs)
  uint32_t rnym;     // blob offset (16-aligned) of RNym, 32 bytes big-endian, < r
  uint32_t pre;      // blob offset (16-aligned) of the 176-byte transcript prefix slot: "sign", room for t,
                     // Nym, the IPK hash and the 2 tail bytes in place (host/idemix.cpp nymsign_fill_prefix)
};

// limbs (little-endian) <-> big-endian words
FTS_HD void nymsign_words(uint32_t w[8], const uint32_t l[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = l[7 - i];
}

// a mod r for any a < 2^256 (2^256 < 6 r), by selects
FTS_HD void u256_mod_r_uniform(uint32_t out[8], const uint32_t a[8]) {
  uint32_t x[8], mm[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x[i] = a[i];
    mm[i] = R_MOD[i];
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    uint32_t t[8];
    const uint32_t br = sub8(t, x, mm);
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = br ? x[i] : t[i];
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = x[i];
}

// (hi 2^256 + lo) mod r for any two 256-bit halves (limbs).  With R = 2^256
// the Montgomery form of hi, (hi mod r) R mod r, read as an integer is the
// high half's contribution; lo mod r is added to it.
FTS_HD void fr_wide_reduce(uint32_t out[8], const uint32_t hi[8], const uint32_t lo[8]) {
  fr h, l;
  u256_mod_r_uniform(h.v, hi);
  u256_mod_r_uniform(l.v, lo);
  fr s = h * fe_const<ModR>(R_R2) + l;
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = s.v[i];
}

// One compression of the 64 bytes a || b (big-endian words) and the padding
// block: SHA-256(a || b) as big-endian words, with constant indices only.
FTS_HD void sha256_two_words8(uint32_t out[8], const uint32_t a[8], const uint32_t b[8]) {
  uint32_t blk[16];
  Sha256 h;
  h.init();
#pragma unroll
  for (int i = 0; i < 8; i++) {
    blk[i] = a[i];
    blk[8 + i] = b[i];
  }
  h.compress_words(blk);
#pragma unroll
  for (int i = 0; i < 16; i++) blk[i] = 0;
  blk[0] = 0x80000000u;
  blk[15] = 512;
  h.compress_words(blk);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = h.h[i];
}

// SHA-256 of a public message as big-endian words.  On the device a 4-aligned
// message (the blob's are: NymSignJob.msg) is read in whole blocks of dword
// loads; the rest goes through Sha256's block buffer.
FTS_HD void nymsign_msg_digest(uint32_t out[8], const uint8_t* p, uint32_t n) {
  Sha256 h;
  h.init();
  uint32_t i = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  if ((((uintptr_t)p) & 3) == 0) {
#pragma nounroll
    while (n - i >= 64) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p + i);
      uint32_t W[16];
#pragma unroll
      for (int k = 0; k < 16; k++) W[k] = __builtin_bswap32(q[k]);
      h.compress_words(W);
      h.total += 64;
      i += 64;
    }
  }
#endif
  h.update(p + i, n - i);
  uint8_t dg[32];
  h.final(dg);
#pragma unroll
  for (int k = 0; k < 8; k++)
    out[k] = ((uint32_t)dg[4 * k] << 24) | ((uint32_t)dg[4 * k + 1] << 16) | ((uint32_t)dg[4 * k + 2] << 8) | dg[4 * k + 3];
}

// r_sk, r_rnym and nonce (limbs, < r) of one signature.  sk, rnym: limbs;
// digest: SHA-256(msg) as big-endian words; entropy: 32 bytes as big-endian
// words, read when has_entropy.
//   z = digest, or SHA-256(digest || entropy) when hedged
//   DRBG init(x = sk, z, extra = RNym), outputs V1..V6
//   r_sk = (V1 || V2) mod r, r_rnym = (V3 || V4) mod r, nonce = (V5 || V6) mod r
FTS_HD void nymsign_randomness(uint32_t r_sk[8], uint32_t r_rnym[8], uint32_t nonce[8], const uint32_t sk[8],
                               const uint32_t rnym[8], const uint32_t digest[8], const uint32_t entropy[8],
                               bool has_entropy) {
  uint32_t x[8], e[8], z[8], zh[8];
  nymsign_words(x, sk);
  nymsign_words(e, rnym);
  sha256_two_words8(zh, digest, entropy);
#pragma unroll
  for (int i = 0; i < 8; i++) z[i] = has_entropy ? zh[i] : digest[i];
  Rfc6979 g;
  g.init(x, z, e, true);
  // three draws in a rolled loop (one copy of the DRBG step in the code); the
  // outputs are picked by selects on the trip number, not by an indexed array
#pragma unroll
  for (int i = 0; i < 8; i++) r_sk[i] = r_rnym[i] = nonce[i] = 0;
#pragma nounroll
  for (int k = 0; k < 3; k++) {
    uint32_t hi[8], lo[8], v[8];
    g.next();
    nymsign_words(hi, g.V);
    g.next();
    nymsign_words(lo, g.V);
    fr_wide_reduce(v, hi, lo);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      r_sk[i] = k == 0 ? v[i] : r_sk[i];
      r_rnym[i] = k == 1 ? v[i] : r_rnym[i];
      nonce[i] = k == 2 ? v[i] : nonce[i];
    }
  }
}

// select on values: c ? a : b
FTS_HD fp fp_sel(bool c, const fp& a, const fp& b) {
  fp r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// madd-2007-bl (curve.h jac_add_aff) for a secret accumulator: the formulas run
// whatever the operands are; `p_inf` (the accumulator is still empty) selects
// the entry itself.  The caller rules out H = 0 (q1_fixed_mul_uniform).
FTS_HD Jac<fp> jac_add_aff_uniform(const Jac<fp>& p, bool p_inf, const fp& qx, const fp& qy) {
  fp Z1Z1 = sqr(p.z);
  fp U2 = qx * Z1Z1;
  fp S2 = qy * p.z * Z1Z1;
  fp H = U2 - p.x;
  fp rr = S2 - p.y;
  fp HH = sqr(H);
  fp I = HH + HH;
  I = I + I;
  fp J = H * I;
  rr = rr + rr;
  fp V = p.x * I;
  fp X3 = sqr(rr) - J - V - V;
  fp Y1J = p.y * J;
  fp Y3 = rr * (V - X3) - Y1J - Y1J;
  fp t = p.z + H;
  fp Z3 = sqr(t) - Z1Z1 - HH;
  return {fp_sel(p_inf, qx, X3), fp_sel(p_inf, qy, Y3), fp_sel(p_inf, fe_one<ModP>(), Z3)};
}

// The sum of `count` windows of k H from window `first` on, from H's table
// (dev/idemix.h: tab[w * 255 + d - 1] = d 2^(8w) H), for a secret k < r: every
// window costs one table load and one mixed addition.  A zero digit loads
// entry 1 of its window and keeps the old accumulator by selects
// (q1_fixed_mul skips it, which is right for public scalars only).  H = 0
// cannot happen in the addition: the accumulator holds a multiple below
// 2^(8w) and the entry a multiple d 2^(8w), d >= 1, both below r, so they are
// neither equal nor opposite.  The scalar is consumed by shifting (a
// runtime-indexed limb array would live in scratch memory).
template <class F>
FTS_HD Jac<F> q1_fixed_mul_uniform(const QDev* tab, const uint32_t k[8], int first, int count);
template <>
FTS_HD Jac<fp> q1_fixed_mul_uniform<fp>(const QDev* tab, const uint32_t k[8], int first, int count) {
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kk[i] = k[i];
#pragma nounroll
  for (int w = 0; w < first; w++) {
#pragma unroll
    for (int i = 0; i < 7; i++) kk[i] = (kk[i] >> 8) | (kk[i + 1] << 24);
    kk[7] >>= 8;
  }
  Jac<fp> acc = jac_inf<fp>();
  bool empty = true;
#pragma nounroll
  for (int w = first; w < first + count; w++) {
    const uint32_t d = kk[0] & 0xffu;
#pragma unroll
    for (int i = 0; i < 7; i++) kk[i] = (kk[i] >> 8) | (kk[i + 1] << 24);
    kk[7] >>= 8;
    const bool nz = d != 0;
    const QDev& e = tab[w * 255 + (nz ? d - 1 : 0)];
    fp x, y;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      x.v[i] = e.x[i];
      y.v[i] = e.y[i];
    }
    const Jac<fp> s = jac_add_aff_uniform(acc, empty, x, y);
    acc.x = fp_sel(nz, s.x, acc.x);
    acc.y = fp_sel(nz, s.y, acc.y);
    acc.z = fp_sel(nz, s.z, acc.z);
    empty = empty && !nz;
  }
  return acc;
}

// a^(p-2) with the loop of fe_pow written inline: fe_pow is an out-of-line
// function, and a call passes its operand through the lane's scratch memory,
// which nothing clears after the kernel.  The operand here is Z(t): the
// projective coordinate of r_sk HSk + r_rnym HRand leaks bits of the scalars.
// fp_inv_var's divsteps take a data-dependent number of steps.  0 -> 0.
FTS_HD fp nymsign_fp_inv(const fp& a) {
  fp a2 = fe_sqr(a);
  fp a3 = a2 * a;
  fp r = fe_one<ModP>();
#pragma nounroll
  for (int w = 127; w >= 0; w--) {
    r = fe_sqr(r);
    r = fe_sqr(r);
    const uint32_t d = (P_MINUS_2[w >> 4] >> ((w & 15) * 2)) & 3;
    if (d) {  // the exponent is the same in every lane
      fp s;
#pragma unroll
      for (int i = 0; i < 8; i++) s.v[i] = d == 1 ? a.v[i] : (d == 2 ? a2.v[i] : a3.v[i]);
      r = r * s;
    }
  }
  return r;
}

// Jacobian -> affine with the fixed-exponent inverse; the point at infinity
// (Z = 0) comes out as (0, 0), which is its RawBytes encoding
FTS_HD Aff<fp> nymsign_to_aff(const Jac<fp>& p) {
  fp zi = nymsign_fp_inv(p.z);
  fp zi2 = sqr(zi);
  Aff<fp> r;
  r.x = p.x * zi2;
  r.y = p.y * zi2 * zi;
  r.inf = false;
  return r;
}

// the sum of a signature's (or a pseudonym's) partial points, stride n apart
FTS_HD Jac<fp> nymsign_sum_parts(const QJDev* part, size_t n, size_t i) {
  Jac<fp> t = qj_load<fp>(part[i]);
#pragma nounroll
  for (int p = 1; p < NYMSIGN_PARTS; p++) t = jac_add_inl(t, qj_load<fp>(part[(size_t)p * n + i]));
  return t;
}

// The rest of NewNymSignature for one signature given t in Jacobian form: the
// prefix slot at blob + j.pre receives t; out receives ProofC, ProofSSk,
// ProofSRNym and Nonce, 32 bytes big-endian each.
FTS_HD void job_nymsign_fin(const NymSignJob& j, uint8_t* blob, const Jac<fp>& tj, const uint32_t sk[8],
                            const uint32_t r_sk[8], const uint32_t r_rnym[8], const uint32_t nonce[8], uint8_t* out) {
  typedef NymCurve<fp> C;
  uint8_t* pre = blob + j.pre;
  g1_to_bytes(pre + 4, nymsign_to_aff(tj));
  Sha256 s;
  s.init();
  s.update(pre, C::PRE);
  const uint32_t head = j.msg_len < 192 - C::PRE ? j.msg_len : 192 - C::PRE;  // completes the third block
  s.update(blob + j.msg, head);
  s.update(blob + j.msg + head, j.msg_len - head);
  s.update(pre + C::PRE, C::TAIL);
  uint8_t d[32];
  s.final(d);
  uint32_t c[8], cw[8], nw[8], pw[8], pc[8];
  digest_mod_r(c, d);
  // ProofC = HashToZr(c || nonce)
  nymsign_words(cw, c);
  nymsign_words(nw, nonce);
  sha256_two_words8(pw, cw, nw);
  nymsign_words(pc, pw);
  u256_mod_r_uniform(pc, pc);
  // responses: the Montgomery product of the integer ProofC and x R is ProofC x mod r
  uint32_t rn[8];
  be32_to_limbs_g(rn, blob + j.rnym);
  fr pcf, skf, rnf, a, b;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    pcf.v[i] = pc[i];
    skf.v[i] = sk[i];
    rnf.v[i] = rn[i];
    a.v[i] = r_sk[i];
    b.v[i] = r_rnym[i];
  }
  const fr r2 = fe_const<ModR>(R_R2);
  a = a + pcf * (skf * r2);
  b = b + pcf * (rnf * r2);
  limbs_to_be32_g(out, pc);
  limbs_to_be32_g(out + 32, a.v);
  limbs_to_be32_g(out + 64, b.v);
  limbs_to_be32_g(out + 96, nonce);
}

}  // namespace fts
