// TEST-ONLY stand-alone driver (own main) for the fused G1 formulas of
// dev/fp29.h -- the scanned balanced products (s29_*), f29_half3, j29_dbl,
// j29_madd, x29_madd -- and g1_mul_glv16 (dev/jobs.h) built on them, against
// the 32-bit code of dev/curve.h: jac_dbl, jac_add_aff and jac_add as
// projective points (cross-multiplied), g1_mul_glv as affine points.
//
// Every section prints one line "name checked bad [hits]"; tests/test_g1_fused.py
// asserts on them.  Built a second time with
// -fsanitize=signed-integer-overflow,undefined, a column that passes 2^63 (or
// any other undefined operation) aborts the run instead of giving a wrong digit.
#include <stdio.h>
#include <stdlib.h>

#include "../../fabric-token-sdk_amd/csrc/dev/jobs.h"

using namespace fts;

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
fp rnd_fp() {
  uint32_t v[8];
  for (int i = 0; i < 8; i++) v[i] = (uint32_t)rnd();
  v[7] &= 0x1fffffffu;  // < 2^253 < p
  return fe_from_int<ModP>(v);
}
void rnd_scalar(uint32_t s[8]) {
  for (int i = 0; i < 8; i++) s[i] = (uint32_t)rnd();
  s[7] &= 0x0fffffffu;  // < 2^252 < r
}

const int32_t B28 = 1 << 28, B29 = 1 << 29;
// limb 8 of the largest values the contracts allow (p / 2^232 = 3171406.45):
// 2.5 p for a coordinate, 32 p for an affine operand, less the two units the
// limbs below can add
const int32_t TOP_COORD = 7928513, TOP_AFF = 101485003;
// and of the results: 2.1 p and 0.57 p, plus one
const int32_t OUT_X = 6659955, OUT_YZ = 1807703;

// the same element in one of the representations the formulas accept: the
// balanced reduction, that plus or minus p (limbs within 2^29), f29_reduce's
// unsigned limbs, or the unreduced entry form (affine operands only)
f29 rep(const fp& x, int kind) {
  const f29 e = f29_from_fp(x);
  if (kind == 3) return f29_reduce(e);
  if (kind == 4) return e;
  f29 b = f29_breduce(e);
  for (int i = 0; i < 9; i++) b.l[i] += kind == 1 ? P29B[i] : (kind == 2 ? -P29B[i] : 0);
  return b;
}
// every limb 0..7 = +-lim by the bits of signs, limb 8 = top
f29 corner(int32_t lim, uint32_t signs, int32_t top) {
  f29 r;
  for (int i = 0; i < 8; i++) r.l[i] = ((signs >> i) & 1) ? -lim : lim;
  r.l[8] = top;
  return r;
}

bool balanced(const f29& a, int32_t top) {
  for (int i = 0; i < 8; i++)
    if (a.l[i] < -B28 || a.l[i] >= B28) return false;
  return a.l[8] >= -top && a.l[8] <= top;
}
bool out_ok(const j29& a) { return a.inf || (balanced(a.x, OUT_X) && balanced(a.y, OUT_YZ) && balanced(a.z, OUT_YZ)); }
bool out_ok(const x29& a) {
  return a.inf || (balanced(a.x, OUT_X) && balanced(a.y, OUT_YZ) && balanced(a.zz, OUT_YZ) && balanced(a.zzz, OUT_YZ));
}

// the same projective point: both infinity, or X1 Z2^2 = X2 Z1^2 and Y1 Z2^3 = Y2 Z1^3
bool proj_same(const g1j& a, const g1j& b) {
  if (is_zero(a.z) || is_zero(b.z)) return is_zero(a.z) && is_zero(b.z);
  const fp za = sqr(a.z), zb = sqr(b.z);
  return fe_eq(a.x * zb, b.x * za) && fe_eq(a.y * (zb * b.z), b.y * (za * a.z));
}
bool aff_same(const g1a& a, const g1a& b) {
  if (a.inf || b.inf) return a.inf == b.inf;
  return fe_eq(a.x, b.x) && fe_eq(a.y, b.y);
}
g1j to_g1j(const j29& a) { return j29_to(a); }
g1j to_g1j(const x29& a) { return j29_to(x29_to_j29(a)); }
g1a aff_of(const f29& x, const f29& y) { return {f29_to_fp(x), f29_to_fp(y), false}; }

g1a gen() { return {fe_one<ModP>(), fe_one<ModP>() + fe_one<ModP>(), false}; }
// random multiples of the generator: a pool built once (a scalar multiplication
// and an inversion each), from which the sections draw
const int POOL = 192;
g1a pool[POOL];
void fill_pool() {
  for (int i = 0; i < POOL; i++) {
    uint32_t s[8];
    rnd_scalar(s);
    pool[i] = jac_to_aff(aff_mul(gen(), s));
  }
}
g1a rnd_point() { return pool[rnd() % POOL]; }
// (x z^2, y z^3, z) for a random z
g1j rnd_jac(const g1a& a) {
  const fp z = rnd_fp(), z2 = sqr(z);
  return {a.x * z2, a.y * (z2 * z), z};
}
j29 j29_rep(const g1j& p, int kind) { return {rep(p.x, kind), rep(p.y, kind), rep(p.z, kind), is_zero(p.z)}; }
x29 x29_rep(const g1j& p, int kind) {
  const fp zz = sqr(p.z);
  return {rep(p.x, kind), rep(p.y, kind), rep(zz, kind), rep(zz * p.z, kind), is_zero(p.z)};
}

void report(const char* name, long checked, long bad, long hits = -1) {
  if (hits >= 0)
    printf("%s %ld %ld %ld\n", name, checked, bad, hits);
  else
    printf("%s %ld %ld\n", name, checked, bad);
}

// ---- the field helpers: congruence (through f29_to_fp) and balanced results
void check_field(const f29& a, const f29& b, const f29& c, const f29& d, const f29& f, long& n, long& bad) {
  const fp A = f29_to_fp(a), Bv = f29_to_fp(b), C = f29_to_fp(c), D = f29_to_fp(d), F = f29_to_fp(f);
  const f29 r1 = s29_mul(a, b), r2 = s29_sqr(a), r3 = s29_sqr_add(a, f), r4 = s29_mul2(a, b, c, d);
  const f29 r5 = s29_mul_sub_sqr(a, b, c);
  if (!fe_eq(f29_to_fp(r1), A * Bv) || !fe_eq(f29_to_fp(r2), sqr(A)) || !fe_eq(f29_to_fp(r3), sqr(A) + F) ||
      !fe_eq(f29_to_fp(r4), A * Bv + C * D) || !fe_eq(f29_to_fp(r5), A * Bv - sqr(C)))
    bad++;
  if (!balanced(r1, B28) || !balanced(r2, B28) || !balanced(r3, B29) || !balanced(r4, B28) || !balanced(r5, B28)) bad++;
  n += 5;
}
void field_section() {
  long n = 0, bad = 0;
  for (int it = 0; it < 10000; it++) {
    const f29 a = rep(rnd_fp(), it % 4), b = rep(rnd_fp(), (it / 4) % 5), c = rep(rnd_fp(), (it / 20) % 4);
    const f29 d = rep(rnd_fp(), (it / 80) % 4), f = rep(rnd_fp(), it % 3);
    check_field(a, b, c, d, f, n, bad);
    const f29 h = f29_half3(f29_breduce(a));  // twice the result is 3 a
    const fp H = f29_to_fp(h), A = f29_to_fp(a);
    if (!fe_eq(H + H, A + A + A)) bad++;
    for (int i = 0; i < 9; i++)
      if (h.l[i] < -3 * B28 || h.l[i] > 3 * B28) bad++;
    n++;
  }
  report("field_random", n, bad);
  // the column budget: L_a L_b + L_c L_d <= 13 with every limb product of a
  // column of one sign -- (3 x 2) + (2 x 2) + the digits, (3 x 3) alone for the
  // squares, (2 x 2) + (3 x 3) -- and with alternating signs
  n = bad = 0;
  const uint32_t pats[6] = {0x00, 0xff, 0x55, 0xaa, 0x0f, 0x33};
  for (int pa = 0; pa < 6; pa++)
    for (int pb = 0; pb < 6; pb++) {
      const f29 a3 = corner(3 * B28, pats[pa], TOP_COORD), b2 = corner(B29, pats[pb], TOP_COORD);
      const f29 c2 = corner(B29, pats[pb], -TOP_COORD), d2 = corner(B29, pats[pa], TOP_COORD);
      const f29 f3 = corner(3 * B28, pats[pa] ^ pats[pb], TOP_COORD);
      check_field(a3, b2, c2, d2, f3, n, bad);
      check_field(a3, a3, f29_neg(c2), d2, f29_neg(f3), n, bad);
      check_field(b2, d2, a3, a3, f3, n, bad);
      const f29 h = f29_half3(corner(B28, pats[pa], pb & 1 ? -1585704 : 1585704));
      const fp H = f29_to_fp(h), A = f29_to_fp(corner(B28, pats[pa], pb & 1 ? -1585704 : 1585704));
      if (!fe_eq(H + H, A + A + A)) bad++;
      n++;
    }
  report("field_corners", n, bad);
}

// ---- one doubling / mixed addition of each kind against the 32-bit code
void check_ops(const j29& pj, const x29& px, const f29& x2, const f29& y2, long& n, long& bad) {
  const g1j P = to_g1j(pj);
  const g1a Q = aff_of(x2, y2);
  const j29 d = j29_dbl(pj), s = j29_madd(pj, x2, y2);
  if (!proj_same(to_g1j(d), jac_dbl(P)) || !out_ok(d)) bad++;
  if (!proj_same(to_g1j(s), jac_add_aff(P, Q)) || !out_ok(s)) bad++;
  const x29 t = x29_madd(px, x2, y2);
  // x29_dbl_aff (the sum was a doubling) is the first form's: not balanced
  const bool dbl = !px.inf && proj_same(to_g1j(px), jac_from_aff(Q));
  if (!proj_same(to_g1j(t), jac_add_aff(to_g1j(px), Q)) || (!dbl && !out_ok(t))) bad++;
  n += 3;
}
void point_section() {
  long n = 0, bad = 0;
  for (int it = 0; it < 10000; it++) {
    const g1j P = rnd_jac(rnd_point());
    const g1a Q = rnd_point();
    const int kp = it % 4, kq = (it / 4) % 5;
    const f29 y2 = rep(Q.y, kq);
    check_ops(j29_rep(P, kp), x29_rep(P, kp), rep(Q.x, kq), (it & 16) ? f29_neg(y2) : y2, n, bad);
  }
  report("points_random", n, bad);

  // infinity, P + P through the additions (the doubling branch), P + (-P)
  n = bad = 0;
  for (int it = 0; it < 400; it++) {
    const g1a A = rnd_point();
    const g1j P = rnd_jac(A);
    const int kp = it % 4, kq = (it / 4) % 5;
    j29 inf = j29_rep(P, kp);
    inf.inf = true;
    x29 xinf = x29_rep(P, kp);
    xinf.inf = true;
    const f29 x2 = rep(A.x, kq), y2 = rep(A.y, kq);
    check_ops(inf, xinf, x2, y2, n, bad);                          // infinity + A (and 2 infinity)
    check_ops(j29_rep(P, kp), x29_rep(P, kp), x2, y2, n, bad);     // P + P
    check_ops(j29_rep(P, kp), x29_rep(P, kp), x2, f29_neg(y2), n, bad);  // P + (-P)
    const j29 z = j29_madd(j29_rep(P, kp), x2, f29_neg(y2));
    const x29 xz = x29_madd(x29_rep(P, kp), x2, f29_neg(y2));
    if (!z.inf || !xz.inf) bad++;
    const j29 two = j29_madd(j29_rep(P, kp), x2, y2);
    if (two.inf || !aff_same(jac_to_aff(to_g1j(two)), jac_to_aff(jac_dbl(jac_from_aff(A))))) bad++;
    // the full addition of the first form takes the new routines' outputs and feeds them
    const g1j Q = rnd_jac(rnd_point());
    const j29 dq = j29_dbl(j29_rep(Q, kp));
    const j29 sum = j29_add(two, dq);
    if (!proj_same(to_g1j(sum), jac_add(jac_dbl(P), jac_dbl(Q)))) bad++;
    if (!proj_same(to_g1j(j29_dbl(sum)), jac_dbl(jac_add(jac_dbl(P), jac_dbl(Q))))) bad++;
    if (!proj_same(to_g1j(j29_madd(sum, x2, y2)), jac_add_aff(jac_add(jac_dbl(P), jac_dbl(Q)), A))) bad++;
    n += 5;
  }
  report("points_exceptional", n, bad);

  // coordinates at the extremes of the contract: every limb +-2^29 (the
  // accumulator) and +-(2^29 - 1) (the affine operand), limb 8 at its maximum.
  // The formulas are polynomial identities, so the operands need not lie on
  // the curve.
  n = bad = 0;
  const uint32_t pats[6] = {0x00, 0xff, 0x55, 0xaa, 0x0f, 0xc3};
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++)
      for (int c = 0; c < 6; c++)
        for (int lim = 0; lim < 2; lim++) {
          const int32_t L = lim ? B29 : B28, top = (a + b + c) & 1 ? -TOP_COORD : TOP_COORD;
          const j29 pj = {corner(L, pats[a], top), corner(L, pats[b], -top), corner(L, pats[c], top), false};
          const f29 x2 = corner(B29 - 1, pats[b], c & 1 ? -TOP_AFF : TOP_AFF), y2 = corner(B29 - 1, pats[a], TOP_AFF);
          // ZZ^3 = ZZZ^2 is what makes an XYZZ accumulator a point: take ZZ = z^2, ZZZ = z^3 of an extreme z
          // through the products (balanced), and the extreme X, Y
          const f29 zz = s29_sqr(pj.z), zzz = s29_mul(zz, pj.z);
          const x29 px = {pj.x, pj.y, zz, zzz, false};
          check_ops(pj, px, x2, y2, n, bad);
        }
  report("points_extremes", n, bad);
}

// ---- outputs fed back in: a bound that does not close shows up
void chain_section() {
  long n = 0, bad = 0;
  for (int chain = 0; chain < 4; chain++) {
    g1j acc = rnd_jac(rnd_point());
    j29 a = j29_rep(acc, chain);
    x29 x = x29_rep(acc, chain);
    g1j xacc = acc;
    for (int step = 0; step < 1000; step++) {
      const g1a Q = rnd_point();
      const int kq = step % 5;
      f29 x2 = rep(Q.x, kq), y2 = rep(Q.y, kq);
      g1a Qs = Q;
      if (step % 3 == 0) {
        y2 = f29_neg(y2);
        Qs = aff_neg(Q);
      }
      if (step % 7 < 5) {
        a = j29_dbl(a);
        acc = jac_dbl(acc);
      } else {
        a = j29_madd(a, x2, y2);
        acc = jac_add_aff(acc, Qs);
      }
      x = x29_madd(x, x2, y2);
      xacc = jac_add_aff(xacc, Qs);
      if (!out_ok(a) || !out_ok(x)) bad++;
      if (!proj_same(to_g1j(a), acc) || !proj_same(to_g1j(x), xacc)) bad++;
      n += 2;
    }
  }
  report("chains", n, bad);
}

// ---- g1_mul_glv16 against g1_mul_glv, and its window loop on chosen halves
g1j mul128(const g1a& p, const uint32_t h[4], bool neg) {
  const uint32_t k[8] = {h[0], h[1], h[2], h[3], 0, 0, 0, 0};
  const g1j r = aff_mul(p, k);
  return neg ? jac_neg(r) : r;
}
void glv_section() {
  long n = 0, bad = 0;
  // scalars: 0, 1, r - 1, 2^127, 2^127 lambda, random ones
  uint32_t ks[48][8] = {{0}, {1}, {0}, {0, 0, 0, 0x80000000u}, {0}};
  fe_to_int(ks[2], fe_zero<ModR>() - fe_one<ModR>());
  fe_to_int(ks[4], fe_from_int<ModR>(ks[3]) * fe_const<ModR>(GLV_LAMBDA));
  for (int t = 5; t < 48; t++) rnd_scalar(ks[t]);
  for (int t = 0; t < 48; t++) {
    const g1a P = rnd_point();
    G1Dev loc[16];
    const g1a got = jac_to_aff(g1_mul_glv16(P, ks[t], loc, 1)), want = jac_to_aff(g1_mul_glv(P, ks[t]));
    if (!aff_same(got, want) || !aff_same(got, jac_to_aff(aff_mul(P, ks[t])))) bad++;
    n++;
  }
  report("glv16", n, bad);
  // halves: 0, 1, 2^127 (the top window's digit 1), 2^128 - 1, every window
  // digit -8 or 8 (nibbles 8, 7, 8, 7, ... from the bottom), with both signs
  n = bad = 0;
  long top = 0, eights = 0;
  const uint32_t hs[6][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0x80000000u}, {~0u, ~0u, ~0u, ~0u},
                             {0x78787878u, 0x78787878u, 0x78787878u, 0x78787878u},
                             {0x87878788u, 0x78787878u, 0x78787878u, 0xf8787878u}};
  for (int a = 0; a < 6; a++) {
    int all8 = 1;
    for (int i = 0; i < 32; i++) all8 &= abs(booth16(hs[a], i)) == 8;
    eights += all8;
    top += booth16(hs[a], 32) != 0;
    for (int b = 0; b < 6; b++)
      for (int sg = 0; sg < 4; sg++) {
        const g1a P = rnd_point();
        const g1a phi = {P.x * fe_const<ModP>(GLV_BETA), P.y, false};
        G1Dev loc[16];
        const g1j got = g1_mul_glv16_halves(P, fe_one<ModP>(), hs[a], sg & 1, hs[b], sg & 2, loc, 1);
        const g1j want = jac_add(mul128(P, hs[a], sg & 1), mul128(phi, hs[b], sg & 2));
        if (!aff_same(jac_to_aff(got), jac_to_aff(want))) bad++;
        n++;
      }
  }
  report("glv16_halves", n, bad);
  report("glv16_shapes", top, 0, eights);
}

}  // namespace

int main() {
  fill_pool();
  field_section();
  point_section();
  chain_section();
  glv_section();
  return 0;
}
