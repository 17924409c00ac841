// NIST P-256 and the ECDSA verification job of the x509 identities (auditor,
// issuers, fabtoken owners): token/core/identity/msp/x509/ecdsa.go:70-101
// edsaVerifier.Verify = SHA-256, the low-S rule, go1.18 crypto/ecdsa.Verify.
// Everything is FTS_HD: the same code runs on the device (k_ecdsa.hip), on the
// host (table building, ecdsa_rt.hip) and in the CPU test tier.
//
// Base field: p = 2^256 - 2^224 + 2^192 + 2^96 - 1, one element per lane, 8 x
// 32-bit limbs, Montgomery form with R = 2^256, always fully reduced.  Because
// p = -1 mod 2^32 the Montgomery quotient word of a CIOS round is t[0] itself,
// and m p is m added at limbs 3, 6, 8 and subtracted at limbs 0, 7: a round's
// reduction is one add-with-carry chain and one short subtract chain, no
// multiplications.  One product costs 64 32x32 MADs (the 8 x 8 limb products;
// the generic CIOS of dev/fp256bn.h spends 136).  p > 2^255, so sums and the
// pre-subtraction value carry out of 8 limbs; the carry is kept as fp256bn.h does.
//
// Scalar field (mod the group order n): generic CIOS, used for two products,
// the conversions around them and one inversion per signature.
//
// Group law on y^2 = x^3 - 3x + b, Jacobian coordinates, infinity as Z = 0.
// All three additions are complete: crafted signatures reach P = Q (u1 G =
// u2 Q) and P = -Q in the final addition.
//
// Fixed-base tables (G, and every registered key): P256_WINDOWS = 32 windows of
// 8 bits, entries d 2^(8w) B for d = 1..255 as Montgomery affine points:
// 32 * 255 * 64 = 522,240 bytes per key; a scalar multiplication is at most 32
// mixed additions and no doubling.  ecdsa_rt.hip keeps at most
// P256_MAX_KEYS = 64 registered keys (plus G: 65 tables, 32.4 MiB).
#pragma once
#include "fp.h"
#include "p256_const.h"
#include "sha256.h"

namespace fts {

// ------------------------------------------------------------------ base field
struct pf {
  uint32_t v[8];
};

FTS_HD pf pf_const(const uint32_t* c) {
  pf r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c[i];
  return r;
}
FTS_HD pf pf_zero() {
  pf r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = 0;
  return r;
}
FTS_HD pf pf_one() { return pf_const(P256_P_ONE); }

// r = a - p; returns the borrow (1: a < p)
FTS_HD uint32_t pf_sub_p(uint32_t r[8], const uint32_t a[8]) {
  uint32_t mm[8];
#pragma unroll
  for (int i = 0; i < 8; i++) mm[i] = P256_P[i];
  return sub8(r, a, mm);
}

FTS_HD pf operator+(const pf& a, const pf& b) {
  pf s, t;
  uint32_t c = add8(s.v, a.v, b.v);
  uint32_t br = pf_sub_p(t.v, s.v);
  // s + c 2^256 >= p  <=>  carry out, or no borrow from s - p
  return (c | (br ^ 1u)) ? t : s;
}

FTS_HD pf operator-(const pf& a, const pf& b) {
  pf d, t;
  uint32_t br = sub8(d.v, a.v, b.v);
  uint32_t mm[8];
#pragma unroll
  for (int i = 0; i < 8; i++) mm[i] = P256_P[i];
  add8(t.v, d.v, mm);  // d + p - 2^256 when a < b
  return br ? t : d;
}

// Montgomery product; a, b < p, result < p.  Round i adds a b[i] to the running
// value t (< 2p, ten words with the carries), then (t + t[0] p) / 2^32: limb 0
// cancels exactly, and the shifted value gains t[0] at limbs 2, 5, 7 and loses
// it at limb 6.
FTS_HD pf operator*(const pf& a, const pf& b) {
  FTS_COUNT_MAD(64);
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c = (uint64_t)a.v[j] * b.v[i] + t[j] + (c >> 32);
      t[j] = (uint32_t)c;
    }
    uint64_t s = (uint64_t)t[8] + (c >> 32);
    t[8] = (uint32_t)s;
    t[9] = (uint32_t)(s >> 32);
    const uint32_t m = t[0];
    uint32_t cy, bw;
    t[0] = t[1];
    t[1] = t[2];
    t[2] = addc32(t[3], m, 0, &cy);
    t[3] = addc32(t[4], 0, cy, &cy);
    t[4] = addc32(t[5], 0, cy, &cy);
    t[5] = addc32(t[6], m, cy, &cy);
    t[6] = addc32(t[7], 0, cy, &cy);
    t[7] = addc32(t[8], m, cy, &cy);
    t[8] = t[9] + cy;
    t[6] = subb32(t[6], m, 0, &bw);
    t[7] = subb32(t[7], 0, bw, &bw);
    t[8] -= bw;
  }
  pf r, u;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
  uint32_t br = pf_sub_p(u.v, r.v);
  return (t[8] | (br ^ 1u)) ? u : r;
}

FTS_HD pf pf_sqr(const pf& a) { return a * a; }
FTS_HD pf pf_dbl(const pf& a) { return a + a; }
FTS_HD pf pf_neg(const pf& a) { return pf_zero() - a; }
FTS_HD bool pf_is_zero(const pf& a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i];
  return o == 0;
}
FTS_HD bool pf_eq(const pf& a, const pf& b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
  return o == 0;
}
// canonical integer a < p -> Montgomery form
FTS_HD pf pf_from_int(const uint32_t a[8]) {
  pf x;
#pragma unroll
  for (int i = 0; i < 8; i++) x.v[i] = a[i];
  return x * pf_const(P256_P_R2);
}
FTS_HD void pf_to_int(uint32_t out[8], const pf& a) {
  pf one;
#pragma unroll
  for (int i = 0; i < 8; i++) one.v[i] = (i == 0);
  pf r = a * one;
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = r.v[i];
}
// a^(p-2) (a != 0); host table building only
FTS_HDN pf pf_inv(const pf& a) {
  pf r = pf_one();
#pragma nounroll
  for (int i = 255; i >= 0; i--) {
    r = pf_sqr(r);
    if ((P256_P_MINUS_2[i >> 5] >> (i & 31)) & 1) r = r * a;
  }
  return r;
}

// ------------------------------------------------------------------ scalar field
struct pn {
  uint32_t v[8];
};

FTS_HD pn pn_const(const uint32_t* c) {
  pn r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c[i];
  return r;
}

// a >= b as 256-bit integers (b a constant)
FTS_HD bool u256_geq(const uint32_t a[8], const uint32_t* b) {
  uint32_t t[8], bb[8];
#pragma unroll
  for (int i = 0; i < 8; i++) bb[i] = b[i];
  return sub8(t, a, bb) == 0;
}
FTS_HD bool u256_is_zero(const uint32_t a[8]) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a[i];
  return o == 0;
}

// Montgomery product mod n (CIOS with a ninth word: n > 2^255)
FTS_HD pn operator*(const pn& a, const pn& b) {
  FTS_COUNT_MUL();
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c = (uint64_t)a.v[j] * b.v[i] + t[j] + (c >> 32);
      t[j] = (uint32_t)c;
    }
    uint64_t s = (uint64_t)t[8] + (c >> 32);
    t[8] = (uint32_t)s;
    t[9] = (uint32_t)(s >> 32);
    uint32_t m = t[0] * P256_N_INV;
    c = (uint64_t)m * P256_N[0] + t[0];
#pragma unroll
    for (int j = 1; j < 8; j++) {
      c = (uint64_t)m * P256_N[j] + t[j] + (c >> 32);
      t[j - 1] = (uint32_t)c;
    }
    s = (uint64_t)t[8] + (c >> 32);
    t[7] = (uint32_t)s;
    t[8] = t[9] + (uint32_t)(s >> 32);
  }
  pn r, u;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
  uint32_t mm[8];
#pragma unroll
  for (int i = 0; i < 8; i++) mm[i] = P256_N[i];
  uint32_t br = sub8(u.v, r.v, mm);
  return (t[8] | (br ^ 1u)) ? u : r;
}

// any 256-bit integer -> Montgomery form of (a mod n); a < 2^256 < 2n: one subtraction
FTS_HD pn pn_from_int(const uint32_t a[8]) {
  pn x, t;
#pragma unroll
  for (int i = 0; i < 8; i++) x.v[i] = a[i];
  uint32_t mm[8];
#pragma unroll
  for (int i = 0; i < 8; i++) mm[i] = P256_N[i];
  uint32_t br = sub8(t.v, x.v, mm);
  return (br ? x : t) * pn_const(P256_N_R2);
}
FTS_HD void pn_to_int(uint32_t out[8], const pn& a) {
  pn one;
#pragma unroll
  for (int i = 0; i < 8; i++) one.v[i] = (i == 0);
  pn r = a * one;
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = r.v[i];
}

// a^(n-2) = a^-1 (a != 0 mod n), per-lane Fermat over the fixed exponent:
// left-to-right 2-bit windows with a, a^2, a^3 chosen by selects (a runtime-
// indexed table would live in scratch): 256 squarings + 2 + 100 products.  The
// exponent is the same in every lane, so no lane diverges.
FTS_HDN pn pn_inv(const pn& a) {
  pn a2 = a * a;
  pn a3 = a2 * a;
  pn r = pn_const(P256_N_ONE);
#pragma nounroll
  for (int w = 127; w >= 0; w--) {
    r = r * r;
    r = r * r;
    uint32_t d = (P256_N_MINUS_2[w >> 4] >> ((w & 15) * 2)) & 3;
    if (d) {
      pn s;
#pragma unroll
      for (int i = 0; i < 8; i++) s.v[i] = d == 1 ? a.v[i] : (d == 2 ? a2.v[i] : a3.v[i]);
      r = r * s;
    }
  }
  return r;
}

// ------------------------------------------------------------------ group law
struct P256Aff {  // Montgomery affine (table entries, keys); never infinity
  uint32_t x[8], y[8];
};
struct P256Jac {  // device memory form of p256j
  uint32_t x[8], y[8], z[8];
};
struct p256j {
  pf x, y, z;  // infinity: z = 0
};

FTS_HD p256j p256_inf() {
  p256j r;
  r.x = pf_one();
  r.y = pf_one();
  r.z = pf_zero();
  return r;
}
FTS_HD bool p256_is_inf(const p256j& a) { return pf_is_zero(a.z); }
FTS_HD p256j p256_from_aff(const pf& x, const pf& y) {
  p256j r;
  r.x = x;
  r.y = y;
  r.z = pf_one();
  return r;
}
FTS_HD void p256_store(P256Jac& d, const p256j& p) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    d.x[i] = p.x.v[i];
    d.y[i] = p.y.v[i];
    d.z[i] = p.z.v[i];
  }
}
FTS_HD p256j p256_load(const P256Jac& d) {
  p256j p;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    p.x.v[i] = d.x[i];
    p.y.v[i] = d.y[i];
    p.z.v[i] = d.z[i];
  }
  return p;
}

// y^2 == x^3 - 3x + b
FTS_HD bool p256_on_curve(const pf& x, const pf& y) {
  pf rhs = pf_sqr(x) * x - (x + x + x) + pf_const(P256_B);
  return pf_eq(pf_sqr(y), rhs);
}

// 2P for a = -3 (3M + 5S); infinity stays infinity (Z3 = 2 Y1 Z1), and no
// point has Y = 0 (the group order is odd)
FTS_HD p256j p256_dbl(const p256j& p) {
  pf delta = pf_sqr(p.z), gamma = pf_sqr(p.y);
  pf beta = p.x * gamma;
  pf t = (p.x - delta) * (p.x + delta);
  pf alpha = t + t + t;
  pf b2 = pf_dbl(beta), b4 = pf_dbl(b2), b8 = pf_dbl(b4);
  p256j r;
  r.x = pf_sqr(alpha) - b8;
  r.z = pf_sqr(p.y + p.z) - gamma - delta;
  pf g2 = pf_sqr(gamma);
  pf g8 = pf_dbl(pf_dbl(pf_dbl(g2)));
  r.y = alpha * (b4 - r.x) - g8;
  return r;
}

// c ? a : b, limb by limb: selects on values (returning one of two structs
// from different paths made the compiler pick between their scratch copies)
FTS_HD p256j p256_sel(bool c, const p256j& a, const p256j& b) {
  p256j r;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    r.x.v[i] = c ? a.x.v[i] : b.x.v[i];
    r.y.v[i] = c ? a.y.v[i] : b.y.v[i];
    r.z.v[i] = c ? a.z.v[i] : b.z.v[i];
  }
  return r;
}

// P + (x2, y2), the second operand affine and finite (8M + 3S); complete:
// P at infinity, P = (x2, y2) (falls through to the doubling) and
// P = -(x2, y2) (infinity) are handled.  The general formula always runs (with
// P at infinity it works on defined values and its result is dropped).
FTS_HD p256j p256_add_aff(const p256j& p, const pf& x2, const pf& y2) {
  const bool pinf = p256_is_inf(p);
  pf z1z1 = pf_sqr(p.z);
  pf u2 = x2 * z1z1, s2 = y2 * p.z * z1z1;
  pf h = u2 - p.x, rr = s2 - p.y;
  pf hh = pf_sqr(h);
  pf hhh = h * hh, v = p.x * hh;
  p256j r;
  r.x = pf_sqr(rr) - hhh - pf_dbl(v);
  r.y = rr * (v - r.x) - p.y * hhh;
  r.z = p.z * h;
  if (pf_is_zero(h) && !pinf) r = p256_sel(pf_is_zero(rr), p256_dbl(p), p256_inf());
  return p256_sel(pinf, p256_from_aff(x2, y2), r);
}

// P + Q, complete (12M + 4S): either operand at infinity, P = Q (falls
// through to the doubling), P = -Q (infinity)
FTS_HD p256j p256_add(const p256j& p, const p256j& q) {
  const bool pinf = p256_is_inf(p), qinf = p256_is_inf(q);
  pf z1z1 = pf_sqr(p.z), z2z2 = pf_sqr(q.z);
  pf u1 = p.x * z2z2, u2 = q.x * z1z1;
  pf s1 = p.y * q.z * z2z2, s2 = q.y * p.z * z1z1;
  pf h = u2 - u1, rr = s2 - s1;
  pf hh = pf_sqr(h);
  pf hhh = h * hh, v = u1 * hh;
  p256j r;
  r.x = pf_sqr(rr) - hhh - pf_dbl(v);
  r.y = rr * (v - r.x) - s1 * hhh;
  r.z = p.z * q.z * h;
  if (pf_is_zero(h) && !pinf && !qinf) r = p256_sel(pf_is_zero(rr), p256_dbl(p), p256_inf());
  return p256_sel(pinf, q, p256_sel(qinf, p, r));
}

// ------------------------------------------------------------------ scalar multiplications
static constexpr int P256_WBITS = 8;
static constexpr int P256_WINDOWS = 32;
static constexpr int P256_TAB_ENTRIES = P256_WINDOWS * 255;  // per base: 522,240 bytes
static constexpr int P256_MAX_KEYS = 64;                     // registered keys of one ftz_ecdsa handle

// k B from B's table: sum over the byte windows of k of tab[w][byte_w - 1].
// The scalar is consumed from the bottom by shifting (a runtime-indexed limb
// would put the array in scratch).
FTS_HD p256j p256_fixed_mul(const P256Aff* tab, const uint32_t k[8]) {
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kk[i] = k[i];
  p256j acc = p256_inf();
#pragma nounroll
  for (int w = 0; w < P256_WINDOWS; w++) {
    uint32_t d = kk[0] & 0xffu;
#pragma unroll
    for (int i = 0; i < 7; i++) kk[i] = (kk[i] >> 8) | (kk[i + 1] << 24);
    kk[7] >>= 8;
    if (d) {
      const P256Aff& e = tab[w * 255 + d - 1];
      pf x, y;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        x.v[i] = e.x[i];
        y.v[i] = e.y[i];
      }
      acc = p256_add_aff(acc, x, y);
    }
  }
  return acc;
}

// k Q for a key seen once: 4-bit windows from the top, 1Q .. 15Q in Jacobian
// form.  The multiples live in global memory, lane-interleaved: word j of
// multiple d of lane `lane` (of `lanes`) is vt[((d - 1) * 24 + j) * lanes + lane]
// -- 360 * lanes words in all.  (x, y) is a finite affine point.
static constexpr uint32_t P256_VT_WORDS = 15 * 24;
FTS_HD void p256_vt_store(uint32_t* vt, uint32_t lanes, uint32_t lane, uint32_t d, const p256j& p) {
  uint32_t* o = vt + (size_t)(d - 1) * 24 * lanes + lane;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    o[(size_t)i * lanes] = p.x.v[i];
    o[(size_t)(8 + i) * lanes] = p.y.v[i];
    o[(size_t)(16 + i) * lanes] = p.z.v[i];
  }
}
FTS_HD p256j p256_vt_load(const uint32_t* vt, uint32_t lanes, uint32_t lane, uint32_t d) {
  const uint32_t* o = vt + (size_t)(d - 1) * 24 * lanes + lane;
  p256j p;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    p.x.v[i] = o[(size_t)i * lanes];
    p.y.v[i] = o[(size_t)(8 + i) * lanes];
    p.z.v[i] = o[(size_t)(16 + i) * lanes];
  }
  return p;
}
FTS_HD p256j p256_var_mul(const pf& x, const pf& y, const uint32_t k[8], uint32_t* vt, uint32_t lanes,
                          uint32_t lane) {
  p256j m = p256_from_aff(x, y);
  p256_vt_store(vt, lanes, lane, 1, m);
#pragma nounroll
  for (uint32_t d = 2; d < 16; d++) {
    m = p256_add_aff(m, x, y);  // reaches the doubling at d = 2
    p256_vt_store(vt, lanes, lane, d, m);
  }
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kk[i] = k[i];
  p256j acc = p256_inf();
#pragma nounroll
  for (int w = 0; w < 64; w++) {
    acc = p256_dbl(p256_dbl(p256_dbl(p256_dbl(acc))));
    uint32_t d = kk[7] >> 28;
#pragma unroll
    for (int i = 7; i > 0; i--) kk[i] = (kk[i] << 4) | (kk[i - 1] >> 28);
    kk[0] <<= 4;
    if (d) acc = p256_add(acc, p256_vt_load(vt, lanes, lane, d));
  }
  return acc;
}

// ------------------------------------------------------------------ the verification job
// go1.18 ecdsa.Verify behind edsaVerifier.Verify, for one signature:
//   e = the SHA-256 digest as a 256-bit integer (hashToInt: no truncation on a
//       256-bit order; the arithmetic mod n reduces it);
//   reject unless 1 <= r < n and 1 <= s <= (n-1)/2 (IsLowS; it subsumes s < n);
//   w = s^-1 mod n, u1 = e w, u2 = r w, R = u1 G + u2 Q; reject R = infinity;
//   accept iff x(R) mod n == r.
// The kernels split it: ecdsa_scalars (one lane), the two scalar
// multiplications (one lane each), ecdsa_accept (one lane).

// 1 <= r < n and 1 <= s <= (n-1)/2, canonical little-endian limbs
FTS_HD bool ecdsa_rs_in_range(const uint32_t r[8], const uint32_t s[8]) {
  if (u256_is_zero(r) || u256_geq(r, P256_N)) return false;
  if (u256_is_zero(s)) return false;
  uint32_t t[8], h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = P256_N_HALF[i];
  return sub8(t, h, s) == 0;  // (n-1)/2 - s does not borrow
}

// u1 = e s^-1, u2 = r s^-1 mod n (canonical); r, s in range
FTS_HD void ecdsa_scalars(const uint8_t digest[32], const uint32_t r[8], const uint32_t s[8], uint32_t u1[8],
                          uint32_t u2[8]) {
  uint32_t e[8];
  be32_to_limbs(e, digest);
  pn w = pn_inv(pn_from_int(s));
  pn_to_int(u1, pn_from_int(e) * w);
  pn_to_int(u2, pn_from_int(r) * w);
}

// x(X / Z^2) mod n == r without the inversion, for Z != 0 and 1 <= r < n:
// x < p < 2n, so x mod n == r  <=>  x == r, or x == r + n when r + n < p;
// each as X == c Z^2.  (p - n is about 2^128: no honest signature takes the
// second branch.)
FTS_HD bool p256_x_matches(const pf& X, const pf& Z, const uint32_t r[8]) {
  pf z2 = pf_sqr(Z);
  if (pf_eq(X, pf_from_int(r) * z2)) return true;
  if (u256_geq(r, P256_P_MINUS_N)) return false;
  uint32_t rn[8], nn[8];
#pragma unroll
  for (int i = 0; i < 8; i++) nn[i] = P256_N[i];
  add8(rn, r, nn);  // < p: no carry
  return pf_eq(X, pf_from_int(rn) * z2);
}

// R = A + B (the two scalar multiplications); accept iff R is finite and x(R) mod n == r
FTS_HD bool ecdsa_accept(const p256j& a, const p256j& b, const uint32_t r[8]) {
  p256j R = p256_add(a, b);
  if (p256_is_inf(R)) return false;
  return p256_x_matches(R.x, R.z, r);
}

// One signature on the device: offsets into the pass's blob.
struct EcdsaJob {
  uint32_t sc;       // blob offset (16-aligned) of ECDSA_SC_BYTES: r, s, Qx, Qy (32 bytes big-endian each;
                     // Qx, Qy canonical and on the curve, read when key < 0)
  uint32_t msg;      // blob offset (16-aligned) of the message
  uint32_t msg_len;
  int32_t key;       // >= 0: table index of the registered key (table 0 is G's); -1: ad-hoc
};
static constexpr uint32_t ECDSA_SC_BYTES = 128;

// Host: the fixed-base table of (x, y) (finite, on the curve):
// tab[w * 255 + d - 1] = d 2^(8w) B.  Window bases by doublings, entries by
// mixed additions, one batch inversion per window.  No entry is infinity:
// d 2^(8w) < 2^256 is no multiple of the prime order n (255 * 2^248 < n).
inline void p256_build_table(const pf& x, const pf& y, P256Aff* tab) {
  pf bx = x, by = y;
  for (int w = 0; w < P256_WINDOWS; w++) {
    p256j e[255];
    e[0] = p256_from_aff(bx, by);
    for (int d = 1; d < 255; d++) e[d] = p256_add_aff(e[d - 1], bx, by);
    pf pre[255];
    pre[0] = e[0].z;
    for (int d = 1; d < 255; d++) pre[d] = pre[d - 1] * e[d].z;
    pf inv_all = pf_inv(pre[254]);
    for (int d = 254; d >= 0; d--) {
      pf zi = d ? inv_all * pre[d - 1] : inv_all;
      if (d) inv_all = inv_all * e[d].z;
      pf zi2 = pf_sqr(zi);
      pf ax = e[d].x * zi2, ay = e[d].y * zi2 * zi;
      P256Aff& o = tab[w * 255 + d];
      for (int i = 0; i < 8; i++) {
        o.x[i] = ax.v[i];
        o.y[i] = ay.v[i];
      }
    }
    // next window base: 2^8 (bx, by) = 255 (bx, by) + (bx, by)
    p256j nb = p256_add_aff(e[254], bx, by);
    pf zi = pf_inv(nb.z);
    pf zi2 = pf_sqr(zi);
    bx = nb.x * zi2;
    by = nb.y * zi2 * zi;
  }
}

}  // namespace fts
