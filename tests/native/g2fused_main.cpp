// TEST-ONLY stand-alone driver (own main) for the fused G2 formulas: the
// two-row scanned sums of dev/g2x29.h (q2_scan and its q2s_* forms), x2q_madd
// built on them, and the line steps g2l_dbl / g2l_add of dev/g2lines29.h with
// the whole 88-step chain -- against the 32-bit code: fp2 arithmetic
// (dev/tower.h), jac_add_aff on Fp2 (dev/curve.h), dbl_step_inl / add_step_inl
// (dev/pairing.h) and job_g2lines_parts (dev/jobs.h).
//
// Points are compared projectively (cross-multiplied).  A line is compared up
// to one factor in Fp: the ratio lambda of one non-zero coefficient to the
// reference's must have a zero u-component, and the other two coefficients
// must be lambda times the reference's.
//
// Every section prints one line "name checked bad"; tests/test_g2_fused.py
// asserts on them.  Built a second time with
// -fsanitize=signed-integer-overflow,undefined, a column that passes 2^63 (or
// any other undefined operation) aborts the run instead of giving a wrong digit.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../fabric-token-sdk_amd/csrc/dev/g2lines29.h"

using namespace fts;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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
fp2 rnd_fp2() { return {rnd_fp(), rnd_fp()}; }
void rnd_scalar(uint32_t s[8]) {
  for (int i = 0; i < 8; i++) s[i] = (uint32_t)rnd();
  s[7] &= 0x0fffffffu;  // < 2^252 < r
}

const int32_t B28 = 1 << 28;
// limb 8 of the largest operand the contract of q2_scan allows, and of the
// values: 0.7 p for a coordinate of T going in and 0.55 p coming out, 0.52 p
// for a line coefficient, 2.2 p and 0.6 p for the accumulator of x2q_madd
// (p / 2^232 = 3171406.45), plus one
const int32_t TOP8 = 1 << 24, IN_T = 2219985, OUT_T = 1744275, OUT_LINE = 1649132, OUT_AX = 6977095, OUT_A = 1902844;

// the same element in one of the representations the contracts accept: the
// balanced reduction (L = 1), or that plus or minus p (limbs within 2^29,
// L = 2: a multiplicand only)
f29 rep(const fp& x, int kind) {
  f29 b = f29_breduce(f29_from_fp(x));
  for (int i = 0; i < 9; i++) b.l[i] += kind == 1 ? P29B[i] : (kind == 2 ? -P29B[i] : 0);
  return b;
}
q2 rep2(const fp2& x, int kind) { return {rep(x.c0, kind % 3), rep(x.c1, (kind / 3 + kind) % 3)}; }
// the element with balanced limbs and the value moved by +-p (kind 1, 2): what
// an accumulator's X (|X| <= 2.2 p) may look like
f29 repb(const fp& x, int kind) {
  f29 pb;
  for (int i = 0; i < 9; i++) pb.l[i] = P29B[i];
  return f29_lin2_ns(f29_breduce(f29_from_fp(x)), 1, pb, kind == 1 ? 1 : (kind == 2 ? -1 : 0));
}
// every limb 0..7 = +-lim by the bits of signs, limb 8 = top
f29 corner(int32_t lim, uint32_t signs, int32_t top) {
  f29 r;
  for (int i = 0; i < 8; i++) r.l[i] = ((signs >> i) & 1) ? -lim : lim;
  r.l[8] = top;
  return r;
}
// the element of any limb vector: peeled into parts f29_to_fp accepts
fp val(const f29& a) {
  f29 rest = a;
  fp acc = fe_zero<ModP>();
  for (int it = 0; it < 16; it++) {
    f29 part;
    bool any = false;
    for (int i = 0; i < 9; i++) {
      const int32_t v = rest.l[i];
      part.l[i] = v > B28 ? B28 : (v < -B28 ? -B28 : v);
      rest.l[i] = v - part.l[i];
      any |= part.l[i] != 0;
    }
    if (!any) break;
    acc = acc + f29_to_fp(part);
  }
  return acc;
}
fp2 val(const q2& a) { return {val(a.c0), val(a.c1)}; }

bool balanced(const f29& a, int32_t top) {
  for (int i = 0; i < 8; i++)
    if (a.l[i] < -B28 || a.l[i] >= B28) return false;
  return a.l[8] >= -top && a.l[8] <= top;
}
bool balanced(const q2& a, int32_t top) { return balanced(a.c0, top) && balanced(a.c1, top); }

void report(const char* name, long checked, long bad) { printf("%s %ld %ld\n", name, checked, bad); }

// ---- the scanned sums in every term combination the formulas use
// a b + f, a b + c d, c a^2 + f (c = 1, -1, -3), a s
void check_scan(const q2& a, const q2& b, const q2& c, const q2& d, const q2& f, const q2& sq, int32_t top, long& n,
                long& bad) {
  const fp2 A = val(a), Bv = val(b), C = val(c), D = val(d), F = val(f), S = val(sq);
  const q2 r1 = q2s_mul_add(a, b, f), r2 = q2s_mul2(a, b, c, d);
  const q2 r3 = q2s_sqr_add(sq, sq, f), r4 = q2s_sqr_add(sq, q2_neg(sq), f);
  const q2 s3 = q2_neg(q2_add(sq, q2_add(sq, sq)));
  const q2 r5 = q2s_sqr_add(sq, s3, f), r6 = q2s_mulf(a, b.c0);
  const q2 r7 = q2_scan<Q2S_MUL, Q2S_NONE, false>(a, b, a, a, a);
  const fp2 S2 = f2_sqr(S);
  if (!f2_eq(val(r1), A * Bv + F) || !f2_eq(val(r2), A * Bv + C * D) || !f2_eq(val(r3), S2 + F) ||
      !f2_eq(val(r4), F - S2) || !f2_eq(val(r5), F - (S2 + S2 + S2)) || !f2_eq(val(r6), f2_mul_fp(A, Bv.c0)) ||
      !f2_eq(val(r7), A * Bv))
    bad++;
  if (!balanced(r1, top) || !balanced(r2, top) || !balanced(r3, top) || !balanced(r4, top) || !balanced(r5, top) ||
      !balanced(r6, top) || !balanced(r7, top))
    bad++;
  n += 7;
}
void scan_section() {
  long n = 0, bad = 0;
  for (int it = 0; it < 10000; it++) {
    // (2 x 1) + (2 x 1): column 64; the square of a balanced value; f a sum of up to three values
    const q2 a = rep2(rnd_fp2(), it % 6), b = rep2(rnd_fp2(), 0), c = rep2(rnd_fp2(), (it / 6) % 6);
    const q2 d = rep2(rnd_fp2(), 0), sq = rep2(rnd_fp2(), 0);
    q2 f = rep2(rnd_fp2(), (it / 36) % 6);
    if (it & 1) f = q2_add(f, q2_add(d, d));
    check_scan(a, b, c, d, f, sq, 4 * OUT_AX, n, bad);
    // q2_scan's single product is q2_mulb's, limb for limb
    const q2 x = q2_scan<Q2S_MUL, Q2S_NONE, false>(a, c, a, a, a), y = q2_mulb(a, c);
    if (memcmp(&x, &y, sizeof(q2))) bad++;
    n++;
  }
  report("scan_random", n, bad);
  // the column budget: sum of (16 | 32 | 8) L_a L_b <= 118 with every limb
  // product of a column of one sign, limb 8 at 2^24, no operand of a product
  // above L = 3: (2 x 2) + (3 x 1) (the doubling's Y3), (3 x 2) + (1 x 1),
  // (3 x 1) + (3 x 1), -3 a^2 of a balanced a (96), a (1 x 7) Fp2 x Fp product
  n = bad = 0;
  const uint32_t pats[6] = {0x00, 0xff, 0x55, 0xaa, 0x0f, 0x33};
  for (int p0 = 0; p0 < 6; p0++)
    for (int p1 = 0; p1 < 6; p1++)
      for (int p2 = 0; p2 < 6; p2++)
        for (int p3 = 0; p3 < 6; p3++) {
          const int32_t t = (p0 + p3) & 1 ? -TOP8 : TOP8;
          const q2 d1 = {corner(B28, pats[p3], -t), corner(B28, pats[p2] ^ 0xff, t)};
          const q2 sq = {corner(B28, pats[p0], t), corner(B28, pats[p1], t)};
          const q2 f = {corner(4 * B28, pats[p1], 4 * TOP8), corner(4 * B28, pats[p0], -4 * TOP8)};
          const int32_t la[3] = {2, 3, 3}, lb[3] = {2, 2, 1}, lc[3] = {3, 1, 3};
          for (int v = 0; v < 3; v++) {
            const q2 a = {corner(la[v] * B28, pats[p0], t), corner(la[v] * B28, pats[p1], -t)};
            const q2 b = {corner(lb[v] * B28, pats[p2], t), corner(lb[v] * B28, pats[p3], -t)};
            const q2 c = {corner(lc[v] * B28, pats[p1], t), corner(lc[v] * B28, pats[p0], t)};
            check_scan(a, b, c, d1, f, sq, 8 * TOP8, n, bad);
          }
          const q2 a1 = {corner(B28, pats[p0], t), corner(B28, pats[p1], -t)};
          const f29 s7 = corner(7 * B28, pats[p2], t);
          const q2 r = q2s_mulf(a1, s7);
          if (!f2_eq(val(r), f2_mul_fp(val(a1), val(s7))) || !balanced(r, 8 * TOP8)) bad++;
          n++;
        }
  report("scan_corners", n, bad);
}

// ---- G2: points of the twist from multiples of its generator
g2a g2gen() {
  return {{fe_const<ModP>(G2_GEN_X0), fe_const<ModP>(G2_GEN_X1)}, {fe_const<ModP>(G2_GEN_Y0), fe_const<ModP>(G2_GEN_Y1)}, false};
}
const int POOL = 96;
g2a pool[POOL];
g1a pool1[POOL];
void fill_pool() {
  const g1a g1 = {fe_one<ModP>(), fe_one<ModP>() + fe_one<ModP>(), false};
  for (int i = 0; i < POOL; i++) {
    uint32_t s[8];
    rnd_scalar(s);
    pool[i] = jac_to_aff(aff_mul(g2gen(), s));
    rnd_scalar(s);
    pool1[i] = jac_to_aff(aff_mul(g1, s));
  }
}
g2a rnd_point() { return pool[rnd() % POOL]; }
g1a rnd_point1() { return pool1[rnd() % POOL]; }

bool proj_same(const g2j& a, const g2j& b) {
  if (is_zero(a.z) || is_zero(b.z)) return is_zero(a.z) && is_zero(b.z);
  const fp2 za = sqr(a.z), zb = sqr(b.z);
  return f2_eq(a.x * zb, b.x * za) && f2_eq(a.y * (zb * b.z), b.y * (za * a.z));
}
// homogeneous projective: (X : Y : Z) the same up to one factor
bool hom_same(const g2p& a, const g2p& b) {
  if ((is_zero(a.x) && is_zero(a.y) && is_zero(a.z)) || (is_zero(b.x) && is_zero(b.y) && is_zero(b.z))) return false;
  return f2_eq(a.x * b.z, b.x * a.z) && f2_eq(a.y * b.z, b.y * a.z) && f2_eq(a.x * b.y, b.x * a.y);
}
// got = lambda want with lambda in Fp
bool line_same(const fp2 got[3], const fp2 want[3]) {
  int k = -1;
  for (int i = 0; i < 3; i++)
    if (!is_zero(want[i])) k = i;
  if (k < 0) return is_zero(got[0]) && is_zero(got[1]) && is_zero(got[2]);
  const fp2 lam = got[k] * f2_inv(want[k]);
  if (!fe_is_zero(lam.c1) || fe_is_zero(lam.c0)) return false;
  for (int i = 0; i < 3; i++)
    if (!f2_eq(got[i], f2_mul_fp(want[i], lam.c0))) return false;
  return true;
}

// x2q of a Jacobian point scaled by a random z, in representation kind
x2q x2q_rep(const g2a& a, int kind) {
  const fp2 z = rnd_fp2(), zz = sqr(z), zzz = zz * z;
  const fp2 X = a.x * zz;
  return {{repb(X.c0, kind % 3), repb(X.c1, kind / 3)}, rep2(a.y * zzz, 0), rep2(zz, 0), rep2(zzz, 0), a.inf};
}
bool acc_ok(const x2q& a) {
  return a.inf || (balanced(a.x, OUT_AX) && balanced(a.y, OUT_A) && balanced(a.zz, OUT_A) && balanced(a.zzz, OUT_A));
}
g2j to_g2j(const x2q& a) { return x2q_to_g2j(a); }

void madd_section() {
  long n = 0, bad = 0;
  for (int it = 0; it < 10000; it++) {
    const g2a A = rnd_point(), Q = rnd_point();
    const x2q p = x2q_rep(A, it % 9);
    q2 y2 = q2_from_fp2(Q.y);
    g2a Qs = Q;
    if (it & 1) {
      y2 = q2_neg(y2);
      Qs = aff_neg(Q);
    }
    bool dbl = false;
    const x2q s = x2q_madd(p, q2_from_fp2(Q.x), y2, &dbl);
    const bool same = f2_eq(A.x, Qs.x) && f2_eq(A.y, Qs.y);
    if (dbl != same) bad++;
    if (!dbl && (!proj_same(to_g2j(s), jac_add_aff(to_g2j(p), Qs)) || !acc_ok(s))) bad++;
    n++;
  }
  report("madd_random", n, bad);

  // the accumulator at infinity, P + P (the doubling flag, and the doubling
  // itself without the flag), P + (-P)
  n = bad = 0;
  for (int it = 0; it < 400; it++) {
    const g2a A = rnd_point();
    const q2 x2 = q2_from_fp2(A.x), y2 = q2_from_fp2(A.y);
    x2q inf = x2q_rep(A, 0);
    inf.inf = true;
    bool dbl = false;
    const x2q a = x2q_madd(inf, x2, y2, &dbl);
    if (dbl || a.inf || !proj_same(to_g2j(a), jac_from_aff(A))) bad++;
    const x2q p = x2q_rep(A, 0);
    const x2q b = x2q_madd(p, x2, y2, &dbl);
    if (!dbl || b.inf) bad++;
    const x2q c = x2q_madd(p, x2, y2);
    if (c.inf || !proj_same(to_g2j(c), jac_dbl(jac_from_aff(A))) || !acc_ok(c)) bad++;
    dbl = false;
    const x2q d = x2q_madd(p, x2, q2_neg(y2), &dbl);
    if (dbl || !d.inf || !is_zero(to_g2j(d).z)) bad++;
    // the doubled point feeds the next addition
    const g2a Q = rnd_point();
    const x2q e = x2q_madd(c, q2_from_fp2(Q.x), q2_from_fp2(Q.y));
    if (!proj_same(to_g2j(e), jac_add_aff(jac_dbl(jac_from_aff(A)), Q)) || !acc_ok(e)) bad++;
    n += 5;
  }
  report("madd_exceptional", n, bad);

  // coordinates at the extremes of the contract: every limb +-2^28, limb 8 at
  // the value bounds; the formulas are polynomial identities, so the operands
  // need not lie on the curve (ZZ^3 = ZZZ^2 is not used by the addition)
  n = bad = 0;
  const uint32_t pats[6] = {0x00, 0xff, 0x55, 0xaa, 0x0f, 0xc3};
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++)
      for (int c = 0; c < 6; c++)
        for (int d = 0; d < 6; d++) {
          const int32_t s = (a + d) & 1 ? -1 : 1;
          const x2q p = {{corner(B28, pats[a], s * (OUT_AX - 1)), corner(B28, pats[b], -s * (OUT_AX - 1))},
                         {corner(B28, pats[c], s * (OUT_A - 1)), corner(B28, pats[d], s * (OUT_A - 1))},
                         {corner(B28, pats[b], -s * (OUT_A - 1)), corner(B28, pats[a], s * (OUT_A - 1))},
                         {corner(B28, pats[d], s * (OUT_A - 1)), corner(B28, pats[c], -s * (OUT_A - 1))},
                         false};
          const q2 x2 = {corner(B28, pats[c], s * (OUT_LINE - 1)), corner(B28, pats[a], -s * (OUT_LINE - 1))};
          const q2 y2 = {corner(B28, pats[b], -s * (OUT_LINE - 1)), corner(B28, pats[d], s * (OUT_LINE - 1))};
          const x2q r = x2q_madd(p, x2, y2);
          // madd-2008-s on the values
          const fp2 X = val(p.x), Y = val(p.y), ZZ = val(p.zz), ZZZ = val(p.zzz);
          const fp2 P = val(x2) * ZZ - X, R = val(y2) * ZZZ - Y, PP = sqr(P), PPP = P * PP, Q = X * PP;
          const fp2 X3 = sqr(R) - PPP - (Q + Q), Y3 = R * (Q - X3) - Y * PPP;
          if (r.inf || !f2_eq(val(r.x), X3) || !f2_eq(val(r.y), Y3) || !f2_eq(val(r.zz), ZZ * PP) ||
              !f2_eq(val(r.zzz), ZZZ * PPP) || !acc_ok(r))
            bad++;
          n++;
        }
  report("madd_extremes", n, bad);

  // chains of 1,000 additions that feed the outputs back in
  n = bad = 0;
  for (int chain = 0; chain < 4; chain++) {
    const g2a A = rnd_point();
    x2q x = x2q_rep(A, chain * 2);
    g2j acc = to_g2j(x);
    for (int step = 0; step < 1000; step++) {
      g2a Q = rnd_point();
      if (step % 3 == 0) Q = aff_neg(Q);
      x = x2q_madd(x, q2_from_fp2(Q.x), q2_from_fp2(Q.y));
      acc = jac_add_aff(acc, Q);
      if (!acc_ok(x) || !proj_same(to_g2j(x), acc)) bad++;
      n++;
    }
  }
  report("madd_chains", n, bad);
}

// ---- one line step of each kind against dbl_step_inl / add_step_inl
struct Lines {
  q2 c[3];
};
bool step_ok(const q2& X, const q2& Y, const q2& Z, const Lines& l) {
  return balanced(X, OUT_T) && balanced(Y, OUT_T) && balanced(Z, OUT_T) && balanced(l.c[0], OUT_LINE) &&
         balanced(l.c[1], OUT_LINE) && balanced(l.c[2], OUT_LINE);
}
// T and the operands as values; one doubling and one addition of the new form
// against the 32-bit steps
void check_steps(const q2& X, const q2& Y, const q2& Z, const q2& Qx, const q2& Qy, const f29& yP, const f29& xP,
                 long& n, long& bad) {
  const G2LP pm = g2l_pmults(yP, xP);
  const fp yp = val(yP), xp = val(xP);
  for (int add = 0; add < 2; add++) {
    q2 x = X, y = Y, z = Z;
    Lines l;
    auto emit = [&](int c, const q2& v) { l.c[c] = v; };
    g2p T = {val(X), val(Y), val(Z)};
    LineCoef ref;
    if (add) {
      g2l_add(x, y, z, Qx, Qy, pm, emit);
      ref = add_step_inl(T, g2a{val(Qx), val(Qy), false});
    } else {
      g2l_dbl(x, y, z, pm, emit);
      ref = dbl_step_inl(T);
    }
    const fp2 got[3] = {val(l.c[0]), val(l.c[1]), val(l.c[2])};
    const fp2 want[3] = {f2_mul_fp(ref.r0, yp), f2_mul_fp(ref.r1, xp), ref.r2};
    if (!hom_same(g2p{val(x), val(y), val(z)}, T) || !line_same(got, want) || !step_ok(x, y, z, l)) bad++;
    n++;
  }
}
void steps_section() {
  long n = 0, bad = 0;
  for (int it = 0; it < 10000; it++) {
    // T = a random point in a random homogeneous scaling
    const g2a A = rnd_point();
    g2a Q = rnd_point();
    while (f2_eq(Q.x, A.x)) Q = rnd_point();  // T = +-Q has no chord: both forms return the zero triple
    const g1a P = rnd_point1();
    const fp2 z = rnd_fp2();
    check_steps(q2_from_fp2(A.x * z), q2_from_fp2(A.y * z), q2_from_fp2(z), q2_from_fp2(Q.x),
                it & 1 ? q2_neg(q2_from_fp2(Q.y)) : q2_from_fp2(Q.y), f29_breduce(f29_from_fp(P.y)),
                f29_breduce(f29_from_fp(P.x)), n, bad);
  }
  report("steps_random", n, bad);

  // every limb +-2^28 and limb 8 at the bound of T (0.7 p) and of the affine
  // operands (0.52 p): polynomial identities, the operands need not be points
  n = bad = 0;
  const uint32_t pats[6] = {0x00, 0xff, 0x55, 0xaa, 0x0f, 0xc3};
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++)
      for (int c = 0; c < 6; c++)
        for (int d = 0; d < 6; d++) {
          const int32_t s = (a + c) & 1 ? -1 : 1, t = s * (IN_T - 1), u = s * (OUT_LINE - 1);
          const q2 X = {corner(B28, pats[a], t), corner(B28, pats[b], -t)};
          const q2 Y = {corner(B28, pats[c], -t), corner(B28, pats[d], -t)};
          const q2 Z = {corner(B28, pats[b], t), corner(B28, pats[c], t)};
          const q2 Qx = {corner(B28, pats[d], u), corner(B28, pats[a], -u)};
          const q2 Qy = {corner(B28, pats[a] ^ 0xff, -u), corner(B28, pats[b], u)};
          check_steps(X, Y, Z, Qx, Qy, corner(B28, pats[c], u), corner(B28, pats[d], -u), n, bad);
        }
  report("steps_extremes", n, bad);

  // 1,000 steps that feed T back in (five doublings, two additions, ...)
  n = bad = 0;
  for (int chain = 0; chain < 4; chain++) {
    const g2a A = rnd_point();
    const g1a P = rnd_point1();
    const f29 yP = f29_breduce(f29_from_fp(P.y)), xP = f29_breduce(f29_from_fp(P.x));
    const G2LP pm = g2l_pmults(yP, xP);
    q2 X = q2_from_fp2(A.x), Y = q2_from_fp2(A.y), Z = q2_one29();
    g2p T = {A.x, A.y, f2_one()};
    for (int step = 0; step < 1000; step++) {
      Lines l;
      auto emit = [&](int c, const q2& v) { l.c[c] = v; };
      LineCoef ref;
      if (step % 7 < 5) {
        g2l_dbl(X, Y, Z, pm, emit);
        ref = dbl_step_inl(T);
      } else {
        g2a Q = rnd_point();
        if (step & 1) Q = aff_neg(Q);
        g2l_add(X, Y, Z, q2_from_fp2(Q.x), q2_from_fp2(Q.y), pm, emit);
        ref = add_step_inl(T, Q);
      }
      const fp2 got[3] = {val(l.c[0]), val(l.c[1]), val(l.c[2])};
      const fp2 want[3] = {f2_mul_fp(ref.r0, P.y), f2_mul_fp(ref.r1, P.x), ref.r2};
      if (!hom_same(g2p{val(X), val(Y), val(Z)}, T) || !line_same(got, want) || !step_ok(X, Y, Z, l)) bad++;
      n++;
    }
  }
  report("steps_chains", n, bad);
}

// ---- the full 88-step chain through the job routines, against the 32-bit one
fp2 line_coef(const EvLineDev* lines, int s, int c) {
  q2 v;
  const int32_t* b0 = (const int32_t*)lines + evl_off((uint32_t)s, 2 * c, 0, 1);
  const int32_t* b1 = (const int32_t*)lines + evl_off((uint32_t)s, 2 * c + 1, 0, 1);
  for (int i = 0; i < 9; i++) {
    v.c0.l[i] = b0[i];
    v.c1.l[i] = b1[i];
  }
  return val(v);
}
void chain88_section() {
  long n = 0, bad = 0, inf_lines = 0;
  for (int it = 0; it < 64 + 3; it++) {
    // the part sums of t': four random Jacobian points (or, past the 64 random
    // pairs: t' at infinity, R at infinity, both)
    const bool tinf = it == 64 || it == 66, rinf = it >= 65;
    std::vector<G2PartDev> part(4);
    const g2a A = rnd_point();
    for (int q = 0; q < 4; q++) {
      g2a Bq = q == 3 && tinf ? aff_neg(A) : (q == 2 && tinf ? A : rnd_point());
      if (tinf && q < 2) Bq.inf = true;
      const fp2 z = rnd_fp2(), zz = sqr(z);
      g2part_store(part[q], Bq.inf ? jac_inf<fp2>() : g2j{Bq.x * zz, Bq.y * (zz * z), z});
    }
    g1a P = rnd_point1();
    P.inf = rinf;
    G1Dev pt;
    g1_store(pt, P);
    G2Job g;
    memset(&g, 0, sizeof(g));
    PairJob j = {0, 0, 0, 0};
    std::vector<G2Dev> o1(1), o2(1);
    std::vector<EvLineDev> l1(MILLER_LINES), l2(MILLER_LINES);
    job_g2lines_parts(g, j, part.data(), o1.data(), &pt, l1.data(), 0, 1);
    job_g2lines_parts_x29(g, j, part.data(), o2.data(), &pt, l2.data(), 0, 1);
    if (memcmp(o1.data(), o2.data(), sizeof(G2Dev))) bad++;
    if (g2_load(o2[0]).inf != tinf) bad++;
    for (int s = 0; s < MILLER_LINES; s++) {
      const fp2 got[3] = {line_coef(l2.data(), s, 0), line_coef(l2.data(), s, 1), line_coef(l2.data(), s, 2)};
      const fp2 want[3] = {line_coef(l1.data(), s, 0), line_coef(l1.data(), s, 1), line_coef(l1.data(), s, 2)};
      if (!line_same(got, want)) bad++;
      if (tinf || rinf) {  // the line is 1
        if (!f2_eq(got[0], f2_one()) || !is_zero(got[1]) || !is_zero(got[2])) bad++;
        inf_lines++;
      }
      n++;
    }
  }
  report("chain88", n, bad);
  report("chain88_infinity_lines", inf_lines, 0);
}

}  // namespace

int main() {
  fill_pool();
  scan_section();
  madd_section();
  steps_section();
  chain88_section();
  return 0;
}
