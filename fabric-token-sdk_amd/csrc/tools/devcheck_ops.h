// TEST-ONLY: one dispatcher over the arithmetic primitives of dev/fp.h,
// dev/fp_wide.h, dev/fp29.h, dev/sha256.h and dev/p256.h.  dc_apply<OP> reads
// an op's operands as raw 32-bit words and writes its result words; the same
// header is compiled for the device (tools/devcheck.hip, one lane per vector)
// and for the host (tests/native/devcheck_host.cpp), and tests/test_devcheck.py
// compares every word of both with big-integer references
// (tests/devcheck_ref.py).  No HIP-only constructs here: g++ compiles it too.
//
// Adding an op: one DC_OPS line (name, input words, output words), its branch
// in dc_apply, and in tests/devcheck_ref.py its vectors, its reference and a
// mutant that the vectors must tell apart (test_every_op_has_vectors fails
// until the Python side knows the op).
#pragma once
#include "../dev/fp_wide.h"
#include "../dev/fp29.h"
#include "../dev/g2lines29.h"
#include "../dev/p256.h"
#include "../dev/sha256.h"

namespace fts {

// the _ch ops chain the statement ((a o b) o a) o b: the primitive sits between
// other asm statements of one kernel (carry-register liveness across them)
#define DC_FIELD_OPS(X, F)                                                                              \
  X(F##_add, 16, 8) X(F##_sub, 16, 8) X(F##_mul, 16, 8) X(F##_cios, 16, 8)                              \
  X(F##_add_ch, 16, 8) X(F##_sub_ch, 16, 8) X(F##_mul_ch, 16, 8) X(F##_cios_ch, 16, 8)                  \
  X(F##_neg, 8, 8) X(F##_dbl, 8, 8) X(F##_sqr, 8, 8) X(F##_from_int, 8, 8) X(F##_to_int, 8, 8)          \
  X(F##_geq_mod, 8, 1)

static constexpr int DC_W2_MAX = 6;                      // terms of a lazily reduced sum
static constexpr int DC_W2_IN = 1 + DC_W2_MAX * 32;      // k, then k x (a.c0 a.c1 b.c0 b.c1)
static constexpr int DC_BYTES_PAD = 32;                  // sentinel bytes either side of a 32-byte target

#define DC_OPS(X)                                                                                       \
  DC_FIELD_OPS(X, fp)                                                                                   \
  DC_FIELD_OPS(X, fr)                                                                                   \
  X(fp_inv_var, 8, 8) X(fp_inv_sg30, 8, 8) X(fp_inv_sg62, 8, 8) X(fp_inv_eea, 8, 8)                     \
  X(mul_wide, 16, 16) X(redc_wide, 16, 8) X(w2_sum, DC_W2_IN, 16)                                       \
  X(f29_from_fp, 8, 9) X(f29_to_fp, 9, 8) X(f29_roundtrip, 8, 8) X(f29_norm, 9, 9) X(f29_reduce, 9, 9)  \
  X(f29_mul, 18, 9) X(f29_mul_c, 18, 9) X(f29_sqr, 9, 9) X(f29_sqr_c, 9, 9)                             \
  X(f29_is_zero, 9, 1) X(f29_reduced_zero, 9, 1)                                                        \
  X(be32_load, 28, 8) X(be32_store, 12, 24)                                                             \
  X(pf_add, 16, 8) X(pf_sub, 16, 8) X(pf_mul, 16, 8)                                                    \
  X(pf_add_ch, 16, 8) X(pf_sub_ch, 16, 8) X(pf_mul_ch, 16, 8)                                           \
  X(pf_neg, 8, 8) X(pf_from_int, 8, 8) X(pf_to_int, 8, 8) X(pf_inv, 8, 8)                               \
  X(pn_mul, 16, 8) X(pn_mul_ch, 16, 8) X(pn_from_int, 8, 8) X(pn_to_int, 8, 8) X(pn_inv, 8, 8)          \
  X(u256_geq, 16, 1)

enum DcOp : int {
#define DC_X(name, nin, nout) DC_##name,
  DC_OPS(DC_X)
#undef DC_X
  DC_OP_COUNT
};

struct DcInfo {
  const char* name;
  uint32_t nin, nout;
};
inline const DcInfo* dc_table() {
  static const DcInfo t[DC_OP_COUNT] = {
#define DC_X(name, nin, nout) {#name, nin, nout},
      DC_OPS(DC_X)
#undef DC_X
  };
  return t;
}

template <class T>
FTS_HD T dc_ld8(const uint32_t* in) {
  T r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = in[i];
  return r;
}
template <class T>
FTS_HD void dc_st8(uint32_t* out, const T& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = a.v[i];
}
FTS_HD f29 dc_ld29(const uint32_t* in) {
  f29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = (int32_t)in[i];
  return r;
}
FTS_HD void dc_st29(uint32_t* out, const f29& a) {
#pragma unroll
  for (int i = 0; i < 9; i++) out[i] = (uint32_t)a.l[i];
}

struct DcAdd {
  template <class T>
  FTS_HD T operator()(const T& a, const T& b) const { return a + b; }
};
struct DcSub {
  template <class T>
  FTS_HD T operator()(const T& a, const T& b) const { return a - b; }
};
struct DcMul {
  template <class T>
  FTS_HD T operator()(const T& a, const T& b) const { return a * b; }
};
struct DcCios {
  template <class M>
  FTS_HD Fe<M> operator()(const Fe<M>& a, const Fe<M>& b) const { return mont_mul_cios(a, b); }
};
template <class T, class O>
FTS_HD void dc_bin(const uint32_t* in, uint32_t* out, bool chain, O o) {
  const T a = dc_ld8<T>(in), b = dc_ld8<T>(in + 8);
  T r = o(a, b);
  if (chain) r = o(o(r, a), b);
  dc_st8(out, r);
}

// the 14 ops of DC_FIELD_OPS for Fe<M>, k = op - first op of the field
template <class M>
FTS_HD void dc_field(int k, const uint32_t* in, uint32_t* out) {
  typedef Fe<M> F;
  switch (k) {
    case 0: case 4: dc_bin<F>(in, out, k >= 4, DcAdd()); break;
    case 1: case 5: dc_bin<F>(in, out, k >= 4, DcSub()); break;
    case 2: case 6: dc_bin<F>(in, out, k >= 4, DcMul()); break;
    case 3: case 7: dc_bin<F>(in, out, k >= 4, DcCios()); break;
    case 8: dc_st8(out, fe_neg(dc_ld8<F>(in))); break;
    case 9: dc_st8(out, fe_dbl(dc_ld8<F>(in))); break;
    case 10: dc_st8(out, fe_sqr(dc_ld8<F>(in))); break;
    case 11: {
      uint32_t a[8];
      for (int i = 0; i < 8; i++) a[i] = in[i];
      dc_st8(out, fe_from_int<M>(a));
      break;
    }
    case 12: {
      uint32_t r[8];
      fe_to_int(r, dc_ld8<F>(in));
      for (int i = 0; i < 8; i++) out[i] = r[i];
      break;
    }
    default: {
      uint32_t a[8];
      for (int i = 0; i < 8; i++) a[i] = in[i];
      out[0] = fe_geq_mod<M>(a) ? 1u : 0u;
    }
  }
}

template <int OP>
FTS_HD void dc_apply(const uint32_t* in, uint32_t* out) {
  if constexpr (OP >= DC_fp_add && OP <= DC_fp_geq_mod) {
    dc_field<ModP>(OP - DC_fp_add, in, out);
  } else if constexpr (OP >= DC_fr_add && OP <= DC_fr_geq_mod) {
    dc_field<ModR>(OP - DC_fr_add, in, out);
  } else if constexpr (OP == DC_fp_inv_var) {
    dc_st8(out, fp_inv_var(dc_ld8<fp>(in)));
  } else if constexpr (OP == DC_fp_inv_sg30) {
    dc_st8(out, fp_inv_sg<30>(dc_ld8<fp>(in)));
  } else if constexpr (OP == DC_fp_inv_sg62) {
    dc_st8(out, fp_inv_sg<62>(dc_ld8<fp>(in)));
  } else if constexpr (OP == DC_fp_inv_eea) {
    dc_st8(out, fp_inv_eea(dc_ld8<fp>(in)));
  } else if constexpr (OP == DC_mul_wide) {
    uint32_t a[8], b[8], r[16];
    for (int i = 0; i < 8; i++) {
      a[i] = in[i];
      b[i] = in[8 + i];
    }
    mul_wide(r, a, b);
    for (int i = 0; i < 16; i++) out[i] = r[i];
  } else if constexpr (OP == DC_redc_wide) {
    uint32_t t[16];
    for (int i = 0; i < 16; i++) t[i] = in[i];
    dc_st8(out, redc_wide(t));
  } else if constexpr (OP == DC_w2_sum) {
    Wide2 w;
    w2_init(w);
    const uint32_t k = in[0] < (uint32_t)DC_W2_MAX ? in[0] : (uint32_t)DC_W2_MAX;
#pragma nounroll
    for (uint32_t t = 0; t < k; t++) {
      const uint32_t* q = in + 1 + 32 * t;
      const fp2 a = {dc_ld8<fp>(q), dc_ld8<fp>(q + 8)}, b = {dc_ld8<fp>(q + 16), dc_ld8<fp>(q + 24)};
      w2_mac(w, a, b);
    }
    const fp2 r = w2_reduce(w);
    dc_st8(out, r.c0);
    dc_st8(out + 8, r.c1);
  } else if constexpr (OP == DC_f29_from_fp) {
    dc_st29(out, f29_from_fp(dc_ld8<fp>(in)));
  } else if constexpr (OP == DC_f29_to_fp) {
    dc_st8(out, f29_to_fp(dc_ld29(in)));
  } else if constexpr (OP == DC_f29_roundtrip) {
    dc_st8(out, f29_to_fp(f29_from_fp(dc_ld8<fp>(in))));
  } else if constexpr (OP == DC_f29_norm) {
    dc_st29(out, f29_norm(dc_ld29(in)));
  } else if constexpr (OP == DC_f29_reduce) {
    dc_st29(out, f29_reduce(dc_ld29(in)));
  } else if constexpr (OP == DC_f29_mul) {
    dc_st29(out, f29_mul(dc_ld29(in), dc_ld29(in + 9)));
  } else if constexpr (OP == DC_f29_mul_c) {
    dc_st29(out, f29_mul_c(dc_ld29(in), dc_ld29(in + 9)));
  } else if constexpr (OP == DC_f29_sqr) {
    dc_st29(out, f29_sqr(dc_ld29(in)));
  } else if constexpr (OP == DC_f29_sqr_c) {
    dc_st29(out, f29_sqr_c(dc_ld29(in)));
  } else if constexpr (OP == DC_f29_is_zero) {
    out[0] = f29_is_zero(dc_ld29(in)) ? 1u : 0u;
  } else if constexpr (OP == DC_f29_reduced_zero) {
    out[0] = f29_reduced_zero(dc_ld29(in)) ? 1u : 0u;
  } else if constexpr (OP == DC_be32_load) {
    // in: byte offset (0..31), 3 words of padding, a 96-byte buffer (16-byte
    // aligned when the vector is): 32 big-endian bytes read at buffer + offset
    uint32_t r[8];
    be32_to_limbs_g(r, reinterpret_cast<const uint8_t*>(in + 4) + (in[0] & 31u));
    for (int i = 0; i < 8; i++) out[i] = r[i];
  } else if constexpr (OP == DC_be32_store) {
    // in: byte offset (0..31), 3 words of padding, 8 limbs; out: a 96-byte
    // buffer the caller filled, 32 bytes written at buffer + 32 + offset
    uint32_t a[8];
    for (int i = 0; i < 8; i++) a[i] = in[4 + i];
    limbs_to_be32_g(reinterpret_cast<uint8_t*>(out) + DC_BYTES_PAD + (in[0] & 31u), a);
  } else if constexpr (OP == DC_pf_add || OP == DC_pf_add_ch) {
    dc_bin<pf>(in, out, OP == DC_pf_add_ch, DcAdd());
  } else if constexpr (OP == DC_pf_sub || OP == DC_pf_sub_ch) {
    dc_bin<pf>(in, out, OP == DC_pf_sub_ch, DcSub());
  } else if constexpr (OP == DC_pf_mul || OP == DC_pf_mul_ch) {
    dc_bin<pf>(in, out, OP == DC_pf_mul_ch, DcMul());
  } else if constexpr (OP == DC_pf_neg) {
    dc_st8(out, pf_neg(dc_ld8<pf>(in)));
  } else if constexpr (OP == DC_pf_from_int || OP == DC_pn_from_int) {
    uint32_t a[8];
    for (int i = 0; i < 8; i++) a[i] = in[i];
    if (OP == DC_pf_from_int)
      dc_st8(out, pf_from_int(a));
    else
      dc_st8(out, pn_from_int(a));
  } else if constexpr (OP == DC_pf_to_int) {
    uint32_t r[8];
    pf_to_int(r, dc_ld8<pf>(in));
    for (int i = 0; i < 8; i++) out[i] = r[i];
  } else if constexpr (OP == DC_pf_inv) {
    dc_st8(out, pf_inv(dc_ld8<pf>(in)));
  } else if constexpr (OP == DC_pn_mul || OP == DC_pn_mul_ch) {
    dc_bin<pn>(in, out, OP == DC_pn_mul_ch, DcMul());
  } else if constexpr (OP == DC_pn_to_int) {
    uint32_t r[8];
    pn_to_int(r, dc_ld8<pn>(in));
    for (int i = 0; i < 8; i++) out[i] = r[i];
  } else if constexpr (OP == DC_pn_inv) {
    dc_st8(out, pn_inv(dc_ld8<pn>(in)));
  } else {
    static_assert(OP == DC_u256_geq, "dc_apply: op without a branch");
    uint32_t a[8], b[8];
    for (int i = 0; i < 8; i++) {
      a[i] = in[i];
      b[i] = in[8 + i];
    }
    out[0] = u256_geq(a, b) ? 1u : 0u;
  }
}

// ---- the fused G1 formulas of dev/fp29.h against the 32-bit ones of
// dev/curve.h (tests/test_gpu_g1_fused.py), a table of its own beside DC_OPS:
// an op reads an accumulator in raw 29-bit limbs (j29: X Y Z, x29: X Y ZZ ZZZ),
// its infinity flag and, for the additions, an affine operand (x2 y2 in
// limbs); it writes the new routine's result as a 32-bit Jacobian point (24
// words) and then the 32-bit formula's on the same operands (24 words).  The
// two are the same projective point in different scalings.
#define DC_G1_OPS(X) X(g1f_dbl, 28, 48) X(g1f_madd, 46, 48) X(g1f_xmadd, 55, 48)

enum DcG1Op : int {
#define DC_X(name, nin, nout) DC_##name,
  DC_G1_OPS(DC_X)
#undef DC_X
  DC_G1_OP_COUNT
};
inline const DcInfo* dc_g1_table() {
  static const DcInfo t[DC_G1_OP_COUNT] = {
#define DC_X(name, nin, nout) {#name, nin, nout},
      DC_G1_OPS(DC_X)
#undef DC_X
  };
  return t;
}
FTS_HD void dc_stj(uint32_t* out, const g1j& p) {
  dc_st8(out, p.x);
  dc_st8(out + 8, p.y);
  dc_st8(out + 16, p.z);
}
template <int OP>
FTS_HD void dc_g1_apply(const uint32_t* in, uint32_t* out) {
  if constexpr (OP == DC_g1f_dbl) {
    const j29 p = {dc_ld29(in), dc_ld29(in + 9), dc_ld29(in + 18), in[27] != 0};
    dc_stj(out, j29_to(j29_dbl(p)));
    dc_stj(out + 24, jac_dbl(j29_to(p)));
  } else if constexpr (OP == DC_g1f_madd) {
    const j29 p = {dc_ld29(in), dc_ld29(in + 9), dc_ld29(in + 18), in[27] != 0};
    const f29 x2 = dc_ld29(in + 28), y2 = dc_ld29(in + 37);
    dc_stj(out, j29_to(j29_madd(p, x2, y2)));
    dc_stj(out + 24, jac_add_aff(j29_to(p), g1a{f29_to_fp(x2), f29_to_fp(y2), false}));
  } else {
    static_assert(OP == DC_g1f_xmadd, "dc_g1_apply: op without a branch");
    const x29 p = {dc_ld29(in), dc_ld29(in + 9), dc_ld29(in + 18), dc_ld29(in + 27), in[36] != 0};
    const f29 x2 = dc_ld29(in + 37), y2 = dc_ld29(in + 46);
    dc_stj(out, j29_to(x29_to_j29(x29_madd(p, x2, y2))));
    dc_stj(out + 24, jac_add_aff(j29_to(x29_to_j29(p)), g1a{f29_to_fp(x2), f29_to_fp(y2), false}));
  }
}

// ---- the fused G2 formulas of dev/g2x29.h and dev/g2lines29.h against the
// 32-bit ones of dev/pairing.h and dev/curve.h (tests/test_gpu_g2_fused.py), a
// table of its own as DC_G1_OPS.  Operands are raw 29-bit limbs (an Fp2 value:
// c0 then c1, 18 words); results are canonical 32-bit Montgomery words (an Fp2
// value: 16 words).
//   g2f_dbl   in: T = X Y Z, yP, xP.  out: the new T and the three evaluated
//             coefficients c0 c3 c4 of g2l_dbl (96 words), then dbl_step_inl's
//             T and its coefficients times yP, xP, 1 (96 words).
//   g2f_add   in: T, Qx Qy, yP, xP.  out: as g2f_dbl, for g2l_add / add_step_inl.
//   g2f_xmadd in: the accumulator X Y ZZ ZZZ, its infinity flag, x2 y2.  out:
//             x2q_madd's sum as a 32-bit Jacobian point (48 words; of the
//             accumulator when the doubling flag came back), jac_add_aff's on
//             the same operands (48 words), the doubling flag.
// A step's new T is the reference's as a homogeneous projective point, and a
// line is the reference's times one factor in Fp.
#define DC_G2_OPS(X) X(g2f_dbl, 72, 192) X(g2f_add, 108, 192) X(g2f_xmadd, 109, 97)

enum DcG2Op : int {
#define DC_X(name, nin, nout) DC_##name,
  DC_G2_OPS(DC_X)
#undef DC_X
  DC_G2_OP_COUNT
};
inline const DcInfo* dc_g2_table() {
  static const DcInfo t[DC_G2_OP_COUNT] = {
#define DC_X(name, nin, nout) {#name, nin, nout},
      DC_G2_OPS(DC_X)
#undef DC_X
  };
  return t;
}
FTS_HD q2 dc_ldq(const uint32_t* in) { return {dc_ld29(in), dc_ld29(in + 9)}; }
FTS_HD void dc_st2(uint32_t* out, const fp2& a) {
  dc_st8(out, a.c0);
  dc_st8(out + 8, a.c1);
}
template <int OP>
FTS_HD void dc_g2_apply(const uint32_t* in, uint32_t* out) {
  if constexpr (OP == DC_g2f_dbl || OP == DC_g2f_add) {
    constexpr int o = OP == DC_g2f_add ? 36 : 0;  // Qx Qy sit between T and P
    q2 X = dc_ldq(in), Y = dc_ldq(in + 18), Z = dc_ldq(in + 36);
    const f29 yP = dc_ld29(in + 54 + o), xP = dc_ld29(in + 63 + o);
    g2p T = {q2_to_fp2(X), q2_to_fp2(Y), q2_to_fp2(Z)};
    auto emit = [&](int c, const q2& v) { dc_st2(out + 48 + 16 * c, q2_to_fp2(v)); };
    LineCoef ref;
    if constexpr (OP == DC_g2f_add) {
      const q2 Qx = dc_ldq(in + 54), Qy = dc_ldq(in + 72);
      g2l_add(X, Y, Z, Qx, Qy, g2l_pmults(yP, xP), emit);
      ref = add_step_inl(T, g2a{q2_to_fp2(Qx), q2_to_fp2(Qy), false});
    } else {
      g2l_dbl(X, Y, Z, g2l_pmults(yP, xP), emit);
      ref = dbl_step_inl(T);
    }
    dc_st2(out, q2_to_fp2(X));
    dc_st2(out + 16, q2_to_fp2(Y));
    dc_st2(out + 32, q2_to_fp2(Z));
    dc_st2(out + 96, T.x);
    dc_st2(out + 112, T.y);
    dc_st2(out + 128, T.z);
    dc_st2(out + 144, f2_mul_fp(ref.r0, f29_to_fp(yP)));
    dc_st2(out + 160, f2_mul_fp(ref.r1, f29_to_fp(xP)));
    dc_st2(out + 176, ref.r2);
  } else {
    static_assert(OP == DC_g2f_xmadd, "dc_g2_apply: op without a branch");
    const x2q p = {dc_ldq(in), dc_ldq(in + 18), dc_ldq(in + 36), dc_ldq(in + 54), in[72] != 0};
    const q2 x2 = dc_ldq(in + 73), y2 = dc_ldq(in + 91);
    bool dbl = false;
    const x2q s = x2q_madd(p, x2, y2, &dbl);
    const g2j a = x2q_to_g2j(dbl ? p : s), b = jac_add_aff(x2q_to_g2j(p), g2a{q2_to_fp2(x2), q2_to_fp2(y2), false});
    dc_st2(out, a.x);
    dc_st2(out + 16, a.y);
    dc_st2(out + 32, a.z);
    dc_st2(out + 48, b.x);
    dc_st2(out + 64, b.y);
    dc_st2(out + 80, b.z);
    out[96] = dbl ? 1u : 0u;
  }
}

// SHA-256 of one message given as nseg (offset, length) segments of an arena:
// out[0..7] the digest bytes as they lie in memory, out[8..15] digest_mod_r
FTS_HD void dc_sha(const uint8_t* arena, const uint32_t* segs, uint32_t nseg, uint32_t* out) {
  Sha256 s;
  s.init();
#pragma nounroll
  for (uint32_t k = 0; k < nseg; k++) s.update(arena + segs[2 * k], segs[2 * k + 1]);
  uint8_t d[32];
  s.final(d);
  for (int i = 0; i < 8; i++)
    out[i] = (uint32_t)d[4 * i] | ((uint32_t)d[4 * i + 1] << 8) | ((uint32_t)d[4 * i + 2] << 16) |
             ((uint32_t)d[4 * i + 3] << 24);
  uint32_t r[8];
  digest_mod_r(r, d);
  for (int i = 0; i < 8; i++) out[8 + i] = r[i];
}

}  // namespace fts
