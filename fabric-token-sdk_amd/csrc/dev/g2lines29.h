// The pair-2 line chain of k_g2lines1 (one lane per membership digit) on the
// carry-free balanced form: the 88 Miller lines of t' evaluated at R (65
// doublings, 21 NAF additions, 2 Frobenius lines) with q2 values and the
// scanned sums of Fp2 products of dev/g2x29.h (q2_scan), written in EvLineDev's
// balanced planes as the 32-bit chain (job_g2lines_parts) writes them.
//
// Same points as the 32-bit chain, and the same lines up to one factor in Fp
// per line.  T is homogeneous projective, so any common factor of (X : Y : Z)
// is free, and every later line is homogeneous in T's coordinates: the
// doubling runs on 4 T so that no halving is needed, the addition on -T.  A
// line scaled by an element of Fp multiplies the Miller value by an element
// the final exponentiation sends to 1, so every GT byte is identical
// (tests/test_sextet.py test_g2_lines_carry_free checks them).  The multiples
// of xP and yP the lines take are formed once per job (G2LP).
//
// Bounds: T's coordinates between steps have balanced limbs and |value| <=
// 0.7 p, and every line coefficient is balanced with |value| <= 0.52 p; sums
// and small multiples of such values are formed limb by limb without a sweep
// where they are only multiplied.  Each step documents the (B, L) of its
// intermediates against q2_scan's contract; both steps map the bound of T to
// itself (their outputs are at most 0.55 p), so it holds along the 88-step
// chain and any longer one (tests/native/g2fused_main.cpp feeds 1,000 steps).
#pragma once
#include "g2x29.h"

namespace fts {

// Constants of the line chain in the balanced R = 2^261 form (from
// dev/constants.h by q2_from_fp2 / f29_breduce; tests/native/sx_emu.cpp
// sxe_g2l29_consts re-derives them): 3 b' (b' = 3 / (9 + u)), the twist
// Frobenius factors of pi(Q) and -pi^2(Q), one.  As literals they are scalar
// operands, not lane VGPRs.
static constexpr int32_t G2L29_CONST[9][9] = {
  {-253769606, 6731155, -156399417, 46225477, -175165556, 162336334, -209914092, -192467748, -1389658},  // 3 b' c0
  {31837202, -172120824, -128414024, 15984953, -118312780, 62914239, -210424777, 247765560, 1563920},  // 3 b' c1
  {203985993, 99656738, 260427116, -196420981, 88012806, 31651349, 187173606, 203914975, -774555},  // TW_FROB_X c0
  {-250335503, 187804872, -44558148, -133497832, -94169217, -176792772, -242256849, 104485019, 1269326},  // TW_FROB_X c1
  {44173617, 40868432, -156996498, -175615513, 213596584, -200916108, -28519026, -208385841, -1252753},  // TW_FROB_Y c0
  {-106543147, -100798548, -40739557, 220163168, 145517765, -5938662, -212924673, 161949719, 1410845},  // TW_FROB_Y c1
  {-120801391, -145023941, 193189603, 244240497, -226312478, 69340805, -1834625, -184005301, 1478938},  // TW_FROB2_X
  {176370655, 199481511, 128831276, -21759002, -178483129, 45989682, 237679608, -86689705, -903222},  // TW_FROB2_Y
  {-176370655, -199481511, -128831276, 21759002, 178483129, -45989682, -237679608, 86689705, 903222},  // one
};
enum { G2C_B3 = 0, G2C_FX = 2, G2C_FY = 4, G2C_F2X = 6, G2C_F2Y = 7, G2C_ONE = 8 };
FTS_HD f29 g2c_f(int i) {
  f29 r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = G2L29_CONST[i][k];
  return r;
}
FTS_HD q2 g2c_q(int i) { return {g2c_f(i), g2c_f(i + 1)}; }
FTS_HD q2 q2_one29() { return {g2c_f(G2C_ONE), q2_zero().c1}; }

// The multiples of P's coordinates the evaluated lines take, formed once per
// job: -yP and -xP (balanced, negated limb by limb) and 3 xP (unnormalised:
// L = 3, B = 1.56, a multiplicand only)
struct G2LP {
  f29 nyP, nxP, xP3;
};
FTS_HD G2LP g2l_pmults(const f29& yP, const f29& xP) {
  return {f29_neg(yP), f29_neg(xP), f29_add(xP, f29_add(xP, xP))};
}

// Each step hands its three evaluated coefficients to emit(c, value) (c = 0:
// c0, 1: c3, 2: c4) as soon as they are formed, so that none of them stays live
// through the rest of the step.  Every coefficient leaves a reduction with no
// linear term, so it is balanced with B <= 0.52 as the Miller kernels expect.
//
// Both steps take and return T = (X, Y, Z) with balanced limbs (L = 1) and
//   |X|, |Y|, |Z| <= 0.7 p
// (B, L of every intermediate in comments; "column" is the budget of dev/g2x29.h
// q2_scan, at most 118) and return them <= 0.55 p.  The chain starts from
// (Qx, Qy, 1), all <= 0.52 p.
//
// T <- 4 (2T) = 2T; the line (-H, 3J, I) evaluated: c0 = -H yP, c3 = 3 X^2 xP,
// c4 = K = E - B.  With B = Y^2, H = 2 Y Z = Y (2Z), E = 3 b' Z^2 (E = K + B):
//   4 X3 = 2 X Y (B - 3E) = (X 2Y)(-2E - K),
//   4 Y3 = (B + 3E)^2 - 12 E^2 = 4 B^2 - 3 K^2 = (2B)(2B) - K (3K),
//   4 Z3 = 4 B H = (2B)(2H):
// the factors 2 and 4 are limb-wise multiples of a multiplicand, B - 3E and
// 4 Y3 take no reduction of their own terms, and K is the one carry sweep left
// (it leaves as a line coefficient, E and B feed the products).
// 3S + 7M + 2 Fp2 x Fp in eleven reductions and one sweep.
template <class Emit>
FTS_HD void g2l_dbl(q2& X, q2& Y, q2& Z, const G2LP& P, const Emit& emit) {
  const q2 B = q2_sqrb(Y);                                 // 2 x 0.49 / 169 + 0.5: (0.51, 1), column 32
  const q2 H = q2_mulb(Y, q2_add(Z, Z));                   // (0.51, 1), column 32
  emit(0, q2s_mulf(H, P.nyP));                             // (0.51, 1), column 8
  emit(1, q2s_mulf(q2_sqrb(X), P.xP3));                    // X^2: (0.51, 1); 0.51 x 1.56 / 169 + 0.5: (0.51, 1), column 24
  const q2 E = q2_mulb(q2_sqrb(Z), g2c_q(G2C_B3));         // Z^2, E: (0.51, 1)
  const q2 K = q2_lin2b(E, 1, B, -1);                      // (0.5001, 1)
  emit(2, K);
  const q2 M2 = q2_mulb(X, q2_add(Y, Y));                  // (0.51, 1), column 32
  const q2 Wn = q2_neg(q2_add(q2_add(E, E), K));           // -2E - K = B - 3E: (1.53, 3), a multiplicand only
  const q2 B2 = q2_add(B, B);                              // (1.02, 2)
  const q2 K3n = q2_neg(q2_add(K, q2_add(K, K)));          // (1.51, 3)
  X = q2_mulb(M2, Wn);                                     // 2 x 0.51 x 1.53 / 169 + 0.5: (0.51, 1), column 48
  Y = q2s_mul2(B2, B2, K, K3n);                            // 2 (1.05 + 0.76) / 169 + 0.5: (0.53, 1), column 64 + 48
  Z = q2_mulb(B2, q2_add(H, H));                           // 2 x 1.02 x 1.02 / 169 + 0.5: (0.52, 1), column 64
}

// T <- T + (Qx, Qy) ((Qx, Qy) affine, balanced, B <= 0.52), the projective
// triple of the 32-bit chain times -1; the line (L, -O, Qx O - L Qy) evaluated:
// c0 = L yP, c3 = -O xP, c4 = Qx O - L Qy.  With L' = -L = Qx Z - X,
// O = Y - Qy Z, D = L'^2, E' = L' D, G = X D, H = -E' - 2G + Z O^2:
//   X3 = L' H,  Y3 = (H - G) O - Y E',  Z3 = E' Z.
// 2S + 11M + 2 Fp2 x Fp in thirteen reductions, no sweep: O, L' and H take
// their linear terms in the reduction, c4 and Y3 are sums of two products.
template <class Emit>
FTS_HD void g2l_add(q2& X, q2& Y, q2& Z, const q2& Qx, const q2& Qy, const G2LP& P, const Emit& emit) {
  const q2 O = q2s_mul_add(q2_neg(Qy), Z, Y);              // 0.01 + 0.5 + 0.7: (1.21, 1), column 16
  const q2 Lp = q2s_mul_add(Qx, Z, q2_neg(X));             // (1.21, 1)
  emit(0, q2s_mulf(Lp, P.nyP));                            // 0.63 / 169 + 0.5: (0.51, 1), column 8
  emit(1, q2s_mulf(O, P.nxP));                             // (0.51, 1)
  emit(2, q2s_mul2(Qx, O, Lp, Qy));                        // 2 (0.63 + 0.63) / 169 + 0.5001: (0.516, 1), column 32
  const q2 D = q2_sqrb(Lp);                                // 2 x 1.47 / 169 + 0.5: (0.52, 1), column 32
  const q2 Ep = q2_mulb(Lp, D);                            // (0.51, 1)
  const q2 G = q2_mulb(X, D);                              // (0.51, 1)
  const q2 nE = q2_neg(Ep);
  // Z O^2 / R - E' - 2G: O^2 is (0.52, 1); H: 0.01 + 0.5 + 0.51 + 1.02: (2.04, 1)
  const q2 H = q2s_mul_add(Z, q2_sqrb(O), q2_subr(nE, q2_add(G, G)));
  X = q2_mulb(Lp, H);                                      // 2 x 1.21 x 2.04 / 169 + 0.5: (0.53, 1), column 16
  const q2 Y3 = q2s_mul2(q2_subr(H, G), O, Y, nE);         // 2 (2.55 x 1.21 + 0.7 x 0.51) / 169 + 0.5: (0.55, 1), column 32 + 16
  Z = q2_mulb(Ep, Z);                                      // (0.51, 1)
  Y = Y3;
}

FTS_HD void evline_put_b(EvLineDev* base, uint32_t s, int c, uint32_t idx, uint32_t njobs, const f29& b) {
  int32_t* o = (int32_t*)base + evl_off(s, c, idx, njobs);
#pragma unroll
  for (int i = 0; i < 9; i++) o[i] = b.l[i];
  o[9] = 0;
}

// The four partial sums of t' added in the 32-bit Jacobian form and written
// over part 0, and the norm N(Z) = Z0^2 + Z1^2 of the sum (in Fp, zero only
// for Z = 0: -1 is not a square mod p) parked in part 1's first eight words,
// for the launch's batched inversion (k_g2_sum, k_g2_binv, dev/binv.h)
FTS_HD void job_g2_sum(G2PartDev* part, uint32_t idx, uint32_t njobs) {
  g2j acc = g2part_load(part[idx]);
#pragma nounroll
  for (int q = 1; q < 4; q++) acc = jac_add_inl(acc, g2part_load(part[(size_t)q * njobs + idx]));
  g2part_store(part[idx], acc);
  const fp nz = fe_sqr(acc.z.c0) + fe_sqr(acc.z.c1);
#pragma unroll
  for (int i = 0; i < 8; i++) part[njobs + idx].w[i] = nz.v[i];
}
// t' in affine form from the sum and N(Z)^-1 (part 1 after k_g2_binv):
// Z^-1 = conj(Z) N(Z)^-1, as f2_inv_inl, then jac_to_aff_inl's products
FTS_HD g2a g2_sum_aff(const G2PartDev* part, uint32_t idx, uint32_t njobs) {
  const g2j acc = g2part_load(part[idx]);
  g2a r;
  if (is_zero(acc.z)) {
    r.x = zero_of<fp2>();
    r.y = zero_of<fp2>();
    r.inf = true;
    return r;
  }
  fp ni;
#pragma unroll
  for (int i = 0; i < 8; i++) ni.v[i] = part[njobs + idx].w[i];
  const fp2 zi = {acc.z.c0 * ni, fe_neg(acc.z.c1 * ni)};
  const fp2 zi2 = sqr(zi);
  r.x = acc.x * zi2;
  r.y = acc.y * zi2 * zi;
  r.inf = false;
  return r;
}

// job_g2lines_parts (dev/jobs.h) with the line chain on this form: t' (Q,
// affine) is written to the G2 output, then the lines
FTS_HD void g2lines_chain_x29(const g2a& Q, const G2Job& g, const PairJob& j, G2Dev* g2out, const G1Dev* pts,
                              EvLineDev* lines, uint32_t idx, uint32_t njobs) {
  G2Dev d;
  g2_store(d, Q);
  g2out[g.out] = d;
  const g1a P = g1_load(pts[j.p2]);
  const bool use = !(P.inf || Q.inf);
  const G2LP pm = g2l_pmults(f29_breduce(f29_from_fp(P.y)), f29_breduce(f29_from_fp(P.x)));
  const q2 Qx = q2_from_fp2(Q.x), Qy = q2_from_fp2(Q.y);
  q2 X = Qx, Y = Qy, Z = q2_one29();
#pragma nounroll
  for (int s = 0; s < MILLER_LINES; s++) {
    const int t = MILLER_STEPS.t[s];
    // a pair with an infinity point contributes 1 (gnark's MillerLoop skips it)
    auto emit = [&](int c, const q2& v) {
      const q2 w = use ? v : (c == 0 ? q2_one29() : q2_zero());
      evline_put_b(lines, (uint32_t)s, 2 * c, idx, njobs, w.c0);
      evline_put_b(lines, (uint32_t)s, 2 * c + 1, idx, njobs, w.c1);
    };
    if (t == STEP_DBL) {
      g2l_dbl(X, Y, Z, pm, emit);
    } else {
      q2 Ax = Qx, Ay = Qy;
      if (t == STEP_FROB1 || t == STEP_FROB2) {
        // t' re-read from the output just written (this lane's own store): no
        // 32-bit copy of it stays live through the loop
        const g2a Qr = g2_load(g2out[g.out]);
        const g2a A = t == STEP_FROB1 ? tw_frob(Qr) : tw_frob2_neg(Qr);
        Ax = q2_from_fp2(A.x);
        Ay = q2_from_fp2(A.y);
      } else if (t == STEP_SUB) {
        Ay = q2_neg(Qy);
      }
      g2l_add(X, Y, Z, Ax, Ay, pm, emit);
    }
  }
}
// the four partial sums added and normalised in the 32-bit code (one
// inversion per lane), then the chain (tests/native/sx_emu.cpp's cross-reference)
FTS_HD void job_g2lines_parts_x29(const G2Job& g, const PairJob& j, const G2PartDev* part, G2Dev* g2out,
                                  const G1Dev* pts, EvLineDev* lines, uint32_t idx, uint32_t njobs) {
  g2j acc = g2part_load(part[idx]);
#pragma nounroll
  for (int q = 1; q < 4; q++) acc = jac_add_inl(acc, g2part_load(part[(size_t)q * njobs + idx]));
  g2lines_chain_x29(jac_to_aff_inl(acc), g, j, g2out, pts, lines, idx, njobs);
}
// the same after job_g2_sum and the batched inversion
FTS_HD void job_g2lines_summed_x29(const G2Job& g, const PairJob& j, const G2PartDev* part, G2Dev* g2out,
                                   const G1Dev* pts, EvLineDev* lines, uint32_t idx, uint32_t njobs) {
  g2lines_chain_x29(g2_sum_aff(part, idx, njobs), g, j, g2out, pts, lines, idx, njobs);
}

}  // namespace fts
