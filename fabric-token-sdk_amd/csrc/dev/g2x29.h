// Fixed-base G2 partial sums (k_g2_part) on the carry-free balanced form of the
// sextet kernels (dev/fp29.h q2, dev/sx29.h w29_redc): the XYZZ mixed addition
// (madd-2008-s, 8M + 2S; x2q_madd) over balanced Fp2 values instead of the
// 32-bit Jacobian one of curve.h (a Jacobian q2 form, madd-2007-bl, took more
// VALU instructions: profiles/r05/g2_part_xyzz2_ab.txt).  The rare doubling
// case (a running sum equal to its next table point) redoes the lane in the
// 32-bit code, so that its registers stay out of the loop (two waves per SIMD).
//
// One Fp2 product is q2_mulb: three 81-MAD limb-product rows (Karatsuba) folded
// by columns into the two rows the balanced reductions need, reduced while they
// are scanned -- against three 32-bit Montgomery products with a carry add per
// MAD.  The partial leaves in 32-bit Jacobian form, so job_g2lines_parts (the
// one-lane line kernel) reads it unchanged; t' = the sum of the four partials
// in affine form does not depend on their representatives, so g2out and every
// line byte are identical to job_g2_part's.
//
// Bounds: the accumulator's coordinates are x2q_madd's outputs (balanced limbs,
// |X| <= 2.2 p, the rest <= 0.6 p: q2_scan's contract below); table points
// enter balanced (q2_from_fp2).  q2_mulb takes operands with limbs within 2^29
// (a difference of two balanced values), q2_sqrb balanced ones.
#pragma once
#include "jobs.h"
#include "sx29.h"

namespace fts {

// Product scanning: column k of both result rows is formed, the reduction's
// multiples m_i p_j (i + j = k) of the digits already chosen are added, and
// the column either yields the next balanced digit m_k (k < 9: the running sum
// then divides exactly by 2^29) or the next output digit -- w29_redc's digits
// and output, with two running sums and the 18 digits live instead of the
// 34 columns of each row (a lone product here sits next to four coordinates).
struct Scan2 {
  int64_t ar, ai;
  int32_t mr[9], mi[9];
};
// the reduction's share of column k on the running sums; with ADD, f's limb
// k - 9 joins before the output digit is taken (R f, as w29_redc_t<true>)
template <bool ADD>
FTS_HD void scan2_reduce(Scan2& s, int k, const q2& f, q2& r) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int j = k - i;
    if (i >= k || j < 0 || j > 8) continue;
    s.ar += (int64_t)s.mr[i] * P29B[j];
    s.ai += (int64_t)s.mi[i] * P29B[j];
  }
  if (k < 9) {
    const uint32_t m0 = ((uint32_t)s.ar * P29_INV) & (uint32_t)F29_MASK;
    const uint32_t m1 = ((uint32_t)s.ai * P29_INV) & (uint32_t)F29_MASK;
    s.mr[k] = (int32_t)((m0 + (uint32_t)F29_HALF) & (uint32_t)F29_MASK) - F29_HALF;
    s.mi[k] = (int32_t)((m1 + (uint32_t)F29_HALF) & (uint32_t)F29_MASK) - F29_HALF;
    s.ar = (s.ar + (int64_t)s.mr[k] * P29B[0]) >> 29;  // a multiple of 2^29 now
    s.ai = (s.ai + (int64_t)s.mi[k] * P29B[0]) >> 29;
  } else {
    if (ADD) {
      s.ar += f.c0.l[k - 9];
      s.ai += f.c1.l[k - 9];
    }
    r.c0.l[k - 9] = f29_bdigit(s.ar);
    r.c1.l[k - 9] = f29_bdigit(s.ai);
    s.ar = (s.ar + F29_HALF) >> 29;
    s.ai = (s.ai + F29_HALF) >> 29;
  }
}
FTS_HD void scan2_step(Scan2& s, int k, int64_t re, int64_t im, q2& r) {
  s.ar += re;
  s.ai += im;
  scan2_reduce<false>(s, k, r, r);
}
// a b (limbs within 2^29): the Karatsuba columns of sx29.h w29_prod1, scanned
FTS_HD q2 q2_mulb(const q2& a, const q2& b) {
  FTS_COUNT_MAD(192);
  FTS_SCHED_FENCE();
  const f29 sa = f29_add(a.c0, a.c1), sb = f29_add(b.c0, b.c1);
  Scan2 s;
  s.ar = s.ai = 0;
  q2 r;
#pragma unroll
  for (int k = 0; k < 17; k++) {
    uint64_t u = 0, v = 0, w = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int j = k - i;
      if (j < 0 || j > 8) continue;
      u += w29_p(a.c0.l[i], b.c0.l[j]);
      v += w29_p(a.c1.l[i], b.c1.l[j]);
      w += w29_p(sa.l[i], sb.l[j]);
    }
    scan2_step(s, k, (int64_t)(u - v), (int64_t)(w - (u + v)), r);
  }
  r.c0.l[8] = (int32_t)s.ar;
  r.c1.l[8] = (int32_t)s.ai;
  return r;
}
// a^2 = (a0 + a1)(a0 - a1) + 2 a0 a1 u (a balanced): two limb-product rows
FTS_HD q2 q2_sqrb(const q2& a) {
  FTS_COUNT_MAD(128);
  FTS_SCHED_FENCE();
  const f29 s0 = f29_add(a.c0, a.c1), d = f29_sub(a.c0, a.c1), t = f29_add(a.c0, a.c0);
  Scan2 s;
  s.ar = s.ai = 0;
  q2 r;
#pragma unroll
  for (int k = 0; k < 17; k++) {
    int64_t re = 0, im = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int j = k - i;
      if (j < 0 || j > 8) continue;
      re += (int64_t)s0.l[i] * d.l[j];
      im += (int64_t)t.l[i] * a.c1.l[j];
    }
    scan2_step(s, k, re, im, r);
  }
  r.c0.l[8] = (int32_t)s.ar;
  r.c1.l[8] = (int32_t)s.ai;
  return r;
}
// ------------------------------------------- sums of Fp2 terms, one reduction
// The two-row counterpart of fp29.h s29_scan: (term1 [+ term2]) / R [+ f] with
// ONE Montgomery reduction per row.  A term is
//   Q2S_MUL   a b, Fp2 x Fp2: the Karatsuba rows U = a0 b0, V = a1 b1,
//             W = (a0 + a1)(b0 + b1); re = U - V, im = W - (U + V)  (q2_mulb);
//   Q2S_SQR   a b with b = c a for an integer c (1: a^2, -1: -a^2, -3: -3 a^2;
//             the caller forms b): re = (a0 + a1)(b0 - b1), im = (2 a0) b1
//             (q2_sqrb's two rows);
//   Q2S_MULF  a s, Fp2 x Fp with s = b.c0 (b.c1 is not read): re = a0 s,
//             im = a1 s.
// A term is negated by negating one operand (b = -a for a square); f is an Fp2
// value whose limb k - 9 joins column k of its row before the output digit is
// taken, so f may be any sum of balanced values (its limbs far below 2^56).
//
// Contract (L = max |limb 0..7| in units of 2^28; every operand's |limb 8| is
// at most 2^24, which any value up to 5 p has; B = max |component value| in
// units of p; R = 2^261 > 169 p):
//   columns: a product of two limbs below 8 is at most L_a L_b 2^56, one with
//     a limb 8 at most 2^-4 of that.  Column 7 holds the most full-size
//     products, eight per limb-product row (column 8: seven, and two with a
//     limb 8).  Row re of a column takes 16 L_a L_b 2^56 from a Q2S_MUL term
//     (rows U and V), 32 L_a L_b from a Q2S_SQR term (one row of two doubled
//     limbs) and 8 L_a L_s from a Q2S_MULF term; row im takes the same or less
//     (a0 b1 + a1 b0: 16 L_a L_b; 2 a0 b1: 16 L_a L_b; 8 L_a L_s).  With the
//     multiples m_i p_j (at most eight of 2^56: p's limb 8 is below 2^22) and
//     the carry of the column before (< 2^36), |re|, |im| < 2^63 needs
//         sum over terms of (16 | 32 | 8) L_a L_b  <=  118.
//     So: a product or a sum of two products up to L_a L_b + L_c L_d = 7, a
//     square only of L <= 1.9 (-3 a^2 of a balanced a takes 96).  The rows'
//     own operands a0 + a1, b0 + b1, b0 - b1 and 2 a0 are 32-bit limbs: every
//     operand of a product or a square has L <= 3 (an Fp factor s: L <= 7).
//     U and V are signed sums inside that budget.  The row W alone may wrap modulo 2^64
//     (its limbs are doubled twice: up to 32 L_a L_b 2^56 per term); it is
//     summed unsigned and only W - (U + V), which fits, is read as signed --
//     re and im must not wrap.
//   value: |m p / R| <= (1/2 + 2^-29) p, |re|, |im| of a product <= 2 B_a B_b p^2
//     (a square: 2 |c| B_a^2, Fp2 x Fp: B_a B_s), so
//         B_out <= (sum over terms) / 169 + 0.5001 + B_f;
//   limbs 0..7 of the result are balanced digits in [-2^28, 2^28) whatever f
//     is; limb 8 is the signed rest, |limb 8| < B_out 2^21.7 + 1.
// A result with B_out < 1 that is a multiple of p is 0, and 0 has one balanced
// representation (q2_rzero).
enum { Q2S_NONE = 0, Q2S_MUL = 1, Q2S_SQR = 2, Q2S_MULF = 3 };

// the limb-product rows of one term: (x0, y0) and (x1, y1) are U and V of a
// Q2S_MUL term and the re and im rows of the others; (x2, y2) is W
struct Q2Rows {
  f29 x0, y0, x1, y1, x2, y2;
};
template <int KIND>
FTS_HD Q2Rows q2s_rows(const q2& a, const q2& b) {
  Q2Rows t{};
  if (KIND == Q2S_MUL) {
    t.x0 = a.c0, t.y0 = b.c0;
    t.x1 = a.c1, t.y1 = b.c1;
    t.x2 = f29_add(a.c0, a.c1), t.y2 = f29_add(b.c0, b.c1);
  } else if (KIND == Q2S_SQR) {
    t.x0 = f29_add(a.c0, a.c1), t.y0 = f29_sub(b.c0, b.c1);
    t.x1 = f29_add(a.c0, a.c0), t.y1 = b.c1;
  } else if (KIND == Q2S_MULF) {
    t.x0 = a.c0, t.y0 = b.c0;
    t.x1 = a.c1, t.y1 = b.c0;
  }
  return t;
}
template <int KIND>
FTS_HD void q2s_col(const Q2Rows& t, int k, int64_t& re, uint64_t& im, int64_t& u, int64_t& v) {
  if (KIND == Q2S_NONE) return;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int j = k - i;
    if (j < 0 || j > 8) continue;
    if (KIND == Q2S_MUL) {
      u += (int64_t)t.x0.l[i] * t.y0.l[j];
      v += (int64_t)t.x1.l[i] * t.y1.l[j];
      im += w29_p(t.x2.l[i], t.y2.l[j]);
    } else {
      re += (int64_t)t.x0.l[i] * t.y0.l[j];
      im += w29_p(t.x1.l[i], t.y1.l[j]);
    }
  }
}
// 32-bit equivalent of a term, for opcounts (as q2_mulb and q2_sqrb count theirs)
constexpr int q2s_mads(int kind) { return kind == Q2S_MUL ? 192 : (kind == Q2S_NONE ? 0 : 128); }

template <int K1, int K2, bool ADD>
FTS_HD q2 q2_scan(const q2& a, const q2& b, const q2& c, const q2& d, const q2& f) {
  FTS_COUNT_MAD(q2s_mads(K1) + q2s_mads(K2));
  FTS_SCHED_FENCE();
  const Q2Rows t1 = q2s_rows<K1>(a, b), t2 = q2s_rows<K2>(c, d);
  Scan2 s;
  s.ar = s.ai = 0;
  q2 r;
#pragma unroll
  for (int k = 0; k < 17; k++) {
    int64_t re = s.ar, u = 0, v = 0;
    uint64_t im = (uint64_t)s.ai;
    q2s_col<K1>(t1, k, re, im, u, v);
    q2s_col<K2>(t2, k, re, im, u, v);
    if (K1 == Q2S_MUL || K2 == Q2S_MUL) {
      re += u - v;
      im -= (uint64_t)(u + v);
    }
    s.ar = re;
    s.ai = (int64_t)im;
    scan2_reduce<ADD>(s, k, f, r);
  }
  r.c0.l[8] = (int32_t)s.ar + (ADD ? f.c0.l[8] : 0);
  r.c1.l[8] = (int32_t)s.ai + (ADD ? f.c1.l[8] : 0);
  return r;
}
// a b / R + f
FTS_HD q2 q2s_mul_add(const q2& a, const q2& b, const q2& f) { return q2_scan<Q2S_MUL, Q2S_NONE, true>(a, b, a, a, f); }
// (a b + c d) / R
FTS_HD q2 q2s_mul2(const q2& a, const q2& b, const q2& c, const q2& d) {
  return q2_scan<Q2S_MUL, Q2S_MUL, false>(a, b, c, d, a);
}
// a b / R + f with b = c a (Q2S_SQR)
FTS_HD q2 q2s_sqr_add(const q2& a, const q2& b, const q2& f) { return q2_scan<Q2S_SQR, Q2S_NONE, true>(a, b, a, a, f); }
// a s / R (s in Fp)
FTS_HD q2 q2s_mulf(const q2& a, const f29& s) {
  const q2 b = {s, s};
  return q2_scan<Q2S_MULF, Q2S_NONE, false>(a, b, a, a, a);
}
FTS_HD void pin2q(q2& a) {
  pin29(a.c0);
  pin29(a.c1);
}

FTS_HD q2 q2_lin2b(const q2& a, int32_t ca, const q2& b, int32_t cb) {
  return {f29_lin2(a.c0, ca, b.c0, cb), f29_lin2(a.c1, ca, b.c1, cb)};
}
FTS_HD q2 q2_subr(const q2& a, const q2& b) { return {f29_sub(a.c0, b.c0), f29_sub(a.c1, b.c1)}; }
FTS_HD bool q2_rzero(const q2& a) { return f29_reduced_zero(a.c0) && f29_reduced_zero(a.c1); }
FTS_HD q2 q2_one_b() { return {f29_breduce(f29_from_fp(fe_one<ModP>())), q2_zero().c1}; }

// x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2
struct x2q {
  q2 x, y, zz, zzz;
  bool inf;
};

// 2 (x, y) for an affine point (balanced), mdbl-2008-s-1 (a = 0); (B, L) in
// comments.  U and M are squared, so they stay reduced (a square takes L <= 1.9).
FTS_HD x2q x2q_dbl_aff(const q2& x, const q2& y) {
  const q2 U = q2_lin2b(y, 2, y, 0);                       // (0.51, 1)
  const q2 V = q2_sqrb(U);                                 // (0.51, 1)
  const q2 W = q2_mulb(U, V);                              // (0.51, 1)
  const q2 S = q2_mulb(x, V);                              // (0.51, 1)
  const q2 M = q2_lin2b(q2_sqrb(x), 3, x, 0);              // (0.51, 1)
  const q2 X3 = q2s_sqr_add(M, M, q2_neg(q2_add(S, S)));   // 0.01 + 0.5 + 1.02: (1.53, 1), column 32
  const q2 Y3 = q2s_mul2(M, q2_subr(S, X3), W, q2_neg(y)); // 2 (0.51 x 2.04 + 0.27) / 169 + 0.5: (0.52, 1), column 32 + 16
  return {X3, Y3, V, W, false};
}

// p + (x2, y2), (x2, y2) affine (balanced, B <= 0.52) and not the identity:
// madd-2008-s in seven single reductions and the two fused ones of X3 and Y3.
// The accumulator's coordinates have balanced limbs (L = 1) with |X| <= 2.2 p
// and |Y|, |ZZ|, |ZZZ| <= 0.6 p -- this routine's outputs, x2q_dbl_aff's and
// the entry values; (B, L) of every intermediate in comments.
// P = U2 - X vanishes iff the x coordinates agree, and then the sum is a
// doubling (R = 0) or the identity.  The test comes after the fact, as
// x29_madd's: P and R are not reduced values (B > 1), but ZZ3 = ZZ PP is
// (B < 1) and vanishes iff P does (ZZ != 0); R is then reduced for its own test.
FTS_HD x2q x2q_madd(const x2q& p, const q2& x2, const q2& y2, bool* dbl = nullptr) {
  if (p.inf) {
    const q2 one = q2_one_b();
    return {x2, y2, one, one, false};
  }
  const q2 nY = q2_neg(p.y);
  const q2 P = q2s_mul_add(x2, p.zz, q2_neg(p.x));         // 0.01 + 0.5 + 2.2: (2.71, 1), column 16
  const q2 R = q2s_mul_add(y2, p.zzz, nY);                 // 0.01 + 0.5 + 0.6: (1.11, 1)
  const q2 PP = q2_sqrb(P);                                // 2 x 7.4 / 169 + 0.5: (0.59, 1), column 32
  const q2 ZZ3 = q2_mulb(p.zz, PP);                        // (0.51, 1)
  // the compiler tests ZZ3 here whatever the source order, and the operands that
  // cross that branch would be multiplied as sign-extended 64-bit copies (pin32)
  q2 Pq = P, PPq = PP, Rq = R, X1 = p.x, nY1 = nY, ZZZ1 = p.zzz;
  pin2q(Pq);
  pin2q(PPq);
  pin2q(Rq);
  pin2q(X1);
  pin2q(nY1);
  pin2q(ZZZ1);
  const q2 PPP = q2_mulb(Pq, PPq);                         // 2 x 1.6 / 169 + 0.5: (0.52, 1)
  const q2 ZZZ3 = q2_mulb(ZZZ1, PPP);                      // (0.51, 1)
  const q2 Q = q2_mulb(X1, PPq);                           // 2 x 1.3 / 169 + 0.5: (0.52, 1)
  const q2 X3 = q2s_sqr_add(Rq, Rq, q2_neg(q2_add(PPP, q2_add(Q, Q))));  // 0.02 + 0.5 + 0.52 + 1.04: (2.08, 1), column 32
  const q2 Y3 = q2s_mul2(Rq, q2_subr(Q, X3), nY1, PPP);    // 2 (1.11 x 2.6 + 0.32) / 169 + 0.5: (0.54, 1), column 32 + 16
  // an exceptional sum hands back these coordinates unread (the flags say what
  // it is), so the accumulator does not stay live through the products
  if (q2_rzero(ZZ3)) {
    if (q2_rzero(q2_lin2b(Rq, 1, Rq, 0))) {
      if (dbl) {  // the caller redoes the lane in the 32-bit code
        *dbl = true;
        return {X3, Y3, ZZ3, ZZZ3, false};
      }
      return x2q_dbl_aff(x2, y2);
    }
    return {X3, Y3, ZZ3, ZZZ3, true};
  }
  return {X3, Y3, ZZ3, ZZZ3, false};
}

// to 32-bit Jacobian without an inversion: Z' = ZZ ZZZ, X' = X ZZ ZZZ^2,
// Y' = Y ZZZ^4 (X'/Z'^2 = X/ZZ and Y'/Z'^3 = Y/ZZZ since ZZ^3 = ZZZ^2)
FTS_HD g2j x2q_to_g2j(const x2q& p) {
  if (p.inf) return jac_inf<fp2>();
  const q2 t = q2_sqrb(p.zzz);
  const q2 X = q2_mulb(q2_mulb(p.x, p.zz), t);
  const q2 Y = q2_mulb(p.y, q2_sqrb(t));
  const q2 Z = q2_mulb(p.zz, p.zzz);
  return {q2_to_fp2(X), q2_to_fp2(Y), q2_to_fp2(Z)};
}

// job_g2_part (dev/jobs.h) on this form: lane q of a job sums the table points
// of the (base, window) positions q, q + 4, ...
FTS_HD void job_g2_part_x29(const G2Job& g, int q, const uint32_t (*scal)[8], const G2Dev* tab, G2PartDev& out) {
  x2q acc;
  acc.inf = true;
  acc.x = acc.y = acc.zz = acc.zzz = q2_zero();
  bool dbl = false;
#pragma nounroll
  for (int p = q; p < 3 * G2TAB_WINDOWS; p += 4) {
    int f = p / G2TAB_WINDOWS, w = p % G2TAB_WINDOWS;
    if (f < g.nfix) {
      int32_t d = sdigit_at(scal[g.fscal[f]], G2TAB_C, w);
      if (d) {
        g2a T = g2_load(tab[((size_t)g.fbase[f] * G2TAB_WINDOWS + w) * G2TAB_DIGITS + (uint32_t)(d < 0 ? -d : d) - 1]);
        const q2 x2 = q2_from_fp2(T.x);
        q2 y2 = q2_from_fp2(T.y);
        if (d < 0) y2 = q2_neg(y2);
        acc = x2q_madd(acc, x2, y2, &dbl);
        if (dbl) break;
      }
    }
  }
  if (dbl) {
    job_g2_part(g, q, scal, tab, out);  // a running sum met its next table point
    return;
  }
  g2part_store(out, x2q_to_g2j(acc));
}

}  // namespace fts
