// The ECDSA P-256 signing job of the x509 identities (auditor and issuer
// endorsements): token/core/identity/msp/x509/ecdsa.go:50-64 edsaSigner.Sign =
// SHA-256, ecdsa.Sign, ToLowS, DER.  The nonce is the deterministic one of
// RFC 6979 (HMAC_DRBG over the private key and the digest, dev/hmac256.h),
// optionally hedged with 32 bytes of caller entropy as the additional data k'
// of RFC 6979 3.6; Go draws its nonce at random, so the bytes differ from the
// reference's while every signature passes edsaVerifier.Verify.
//
// Everything is FTS_HD like dev/p256.h: device (k_ecsign.hip), host emulation
// (tests).  Secrets here are the private scalar d and the nonce k.  No branch
// and no trip count depends on either: digits pick table entries by address
// (an accepted limit: the process owns the device), every other choice is a
// select on values.  The one loop that looks at a secret is RFC 6979's own
// retry on a candidate outside [1, n), taken with probability 2^-32.
#pragma once
#include "hmac256.h"
#include "p256.h"

namespace fts {

#ifndef FTS_ECSIGN_PARTS
#define FTS_ECSIGN_PARTS 4  // 1, 2, 4 or 8 (build.py --variant; the sweep is in profiles/ecsign_parts_sweep.json)
#endif
static constexpr int ECSIGN_PARTS = FTS_ECSIGN_PARTS;                    // lanes per signature in k_ecsign_part
static constexpr int ECSIGN_PART_WINDOWS = P256_WINDOWS / ECSIGN_PARTS;  // 8 windows of k each
static_assert(ECSIGN_PARTS * ECSIGN_PART_WINDOWS == P256_WINDOWS, "the parts cover the windows exactly");
static constexpr int ECSIGN_MAX_SIGNERS = 8;

// One signature on the device: offsets into the pass's blob.
struct EcsignJob {
  uint32_t msg;  // blob offset (16-aligned) of the message
  uint32_t msg_len;
  int32_t signer;    // index into the handle's private scalars
  uint32_t entropy;  // blob offset (16-aligned) of 32 bytes of entropy; 0: none (offset 0 holds the jobs)
};

// limbs (little-endian) <-> big-endian words
FTS_HD void limbs_to_words(uint32_t w[8], const uint32_t l[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = l[7 - i];
}

// a mod n for a < 2^256 < 2n
FTS_HD void u256_mod_n(uint32_t r[8], const uint32_t a[8]) {
  uint32_t t[8], nn[8];
#pragma unroll
  for (int i = 0; i < 8; i++) nn[i] = P256_N[i];
  uint32_t br = sub8(t, a, nn);
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = br ? a[i] : t[i];
}

// r = x mod n for an affine coordinate x < p < 2n: one conditional subtraction
FTS_HD void ecsign_x_mod_n(uint32_t r[8], const uint32_t x[8]) { u256_mod_n(r, x); }

// ToLowS: s > (n-1)/2 becomes n - s (0 < s < n)
FTS_HD void ecsign_low_s(uint32_t s[8]) {
  uint32_t t[8], h[8], nn[8], f[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    h[i] = P256_N_HALF[i];
    nn[i] = P256_N[i];
  }
  uint32_t high = sub8(t, h, s);  // (n-1)/2 - s borrows
  sub8(f, nn, s);
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = high ? f[i] : s[i];
}

// the RFC 6979 nonce.  d: the private scalar; e: the digest as an integer
// (limbs, not reduced); extra: the 32 entropy bytes as big-endian words, read when has_extra
FTS_HD void ecsign_nonce(uint32_t k[8], const uint32_t d[8], const uint32_t e[8], const uint32_t extra[8],
                         bool has_extra) {
  uint32_t x[8], z[8], zr[8];
  limbs_to_words(x, d);
  u256_mod_n(zr, e);  // bits2octets(h1) = int2octets(h1 mod n)
  limbs_to_words(z, zr);
  Rfc6979 g;
  g.init(x, z, extra, has_extra);
  for (;;) {
    g.next();
    limbs_to_words(k, g.V);  // bits2int: qlen = hlen
    if (!u256_is_zero(k) && !u256_geq(k, P256_N)) return;
    g.retry();
  }
}

// The sum of `count` windows of k B from window `first` on, from B's table,
// for a secret k: every window costs one table load and one mixed addition.  A
// zero digit loads entry 1 of its window and keeps the old accumulator by
// selects (p256_fixed_mul skips it, which is right for public scalars only).
// p256_add_aff's exceptional branch is never taken: the accumulator holds a
// multiple below 2^(8w) and the entry a multiple d 2^(8w), d >= 1, both below
// n, so they are neither equal nor opposite (opposite would need k = n).
FTS_HD p256j p256_fixed_mul_uniform(const P256Aff* tab, const uint32_t k[8], int first, int count) {
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kk[i] = k[i];
#pragma nounroll
  for (int w = 0; w < first; w++) {
#pragma unroll
    for (int i = 0; i < 7; i++) kk[i] = (kk[i] >> 8) | (kk[i + 1] << 24);
    kk[7] >>= 8;
  }
  p256j acc = p256_inf();
#pragma nounroll
  for (int w = first; w < first + count; w++) {
    const uint32_t d = kk[0] & 0xffu;
#pragma unroll
    for (int i = 0; i < 7; i++) kk[i] = (kk[i] >> 8) | (kk[i + 1] << 24);
    kk[7] >>= 8;
    const bool nz = d != 0;
    const P256Aff& e = tab[w * 255 + (nz ? d - 1 : 0)];
    pf x, y;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      x.v[i] = e.x[i];
      y.v[i] = e.y[i];
    }
    acc = p256_sel(nz, p256_add_aff(acc, x, y), acc);
  }
  return acc;
}

// (a + b) mod n on Montgomery (or any reduced) values
FTS_HD pn pn_add(const pn& a, const pn& b) {
  pn s, t;
  uint32_t nn[8];
#pragma unroll
  for (int i = 0; i < 8; i++) nn[i] = P256_N[i];
  uint32_t c = add8(s.v, a.v, b.v);
  uint32_t br = sub8(t.v, s.v, nn);
  const bool over = (c | (br ^ 1u)) != 0;
#pragma unroll
  for (int i = 0; i < 8; i++) s.v[i] = over ? t.v[i] : s.v[i];
  return s;
}

// pf_inv and pn_inv (dev/p256.h) inlined: those two are out-of-line functions,
// and a call passes its operand and result through the lane's scratch memory,
// which nothing clears after the kernel.  Here the operands are Z(R)^2 (the
// projective coordinate of k G leaks bits of k) and the nonce itself.
FTS_HD pf ecsign_pf_inv(const pf& a) {
  pf r = pf_one();
#pragma nounroll
  for (int i = 255; i >= 0; i--) {
    r = pf_sqr(r);
    if ((P256_P_MINUS_2[i >> 5] >> (i & 31)) & 1) r = r * a;  // the exponent is the same in every lane
  }
  return r;
}
FTS_HD pn ecsign_pn_inv(const pn& a) {
  pn a2 = a * a;
  pn a3 = a2 * a;
  pn r = pn_const(P256_N_ONE);
#pragma nounroll
  for (int w = 127; w >= 0; w--) {
    r = r * r;
    r = r * r;
    const uint32_t d = (P256_N_MINUS_2[w >> 4] >> ((w & 15) * 2)) & 3;
    if (d) {  // the exponent is the same in every lane
      pn s;
#pragma unroll
      for (int i = 0; i < 8; i++) s.v[i] = d == 1 ? a.v[i] : (d == 2 ? a2.v[i] : a3.v[i]);
      r = r * s;
    }
  }
  return r;
}

// R = k G (Jacobian, the sum of the parts) -> r = x(R) mod n,
// s = k^-1 (e + r d) mod n made low; false when r = 0 or s = 0 (probability
// about 2^-256; R at infinity gives x = 0 through pf_inv(0) = 0)
FTS_HD bool ecsign_finish(const p256j& R, const uint32_t k[8], const uint32_t e[8], const uint32_t d[8],
                          uint32_t r[8], uint32_t s[8]) {
  uint32_t x[8];
  pf_to_int(x, R.x * ecsign_pf_inv(pf_sqr(R.z)));
  ecsign_x_mod_n(r, x);
  pn kinv = ecsign_pn_inv(pn_from_int(k));
  pn t = pn_add(pn_from_int(e), pn_from_int(r) * pn_from_int(d));
  pn_to_int(s, kinv * t);
  const bool ok = !u256_is_zero(r) && !u256_is_zero(s);
  ecsign_low_s(s);
  return ok;
}

}  // namespace fts
