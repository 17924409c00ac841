// TEST-ONLY: the sextet pairing routines of dev/sx29.h as a table of ops, one
// sextet (six lanes) per job.  dc_sx_apply<OP> is lane k's program: it reads
// the job's operands as raw words, runs the sq_* routines with the barriers and
// the slot exchange of its context, and returns the lane's result in raw limbs.
// The same header is compiled
//   - for the device (tools/devcheck.hip, k_devcheck_sx): 64 lanes per
//     workgroup, ten sextets and the ghost lanes 60..63, the production
//     prologue (SQ_KERNEL_PROLOGUE_B of launch.h) and its LDS regions;
//   - for the host (tests/native/sx_emu.cpp, sxe_sx_ops): six threads and a
//     pthread barrier per job.
// tests/sx_ref.py holds the vectors, the Fp12 references and the mutants;
// tests/test_sx_ops.py (host) and tests/test_gpu_sx_ops.py (device) compare
// every lane's value mod p with the reference and check the limb bounds.
//
// A job's operands, in words (an Fp2 value: 9 limbs of c0, then 9 of c1, signed
// 29-bit limbs, Montgomery radix 2^261; an Fp12 value: lane 0..5's Fp2
// coefficient of w^k; a line record: r0 r1 r2; an Fp value: 9 limbs):
//   sx_mulv, sx_mulv24   a, b                          -> a b  (30 / 24 slots)
//   sx_sqr, sx_cyc_sqr, sx_inv, sx_conj, sx_frob1..3,
//   sx_expt, sx_fexp_easy                a             -> the routine's value
//   sx_mul_line_r        f, l0 l1 l3                   -> f (l0 + l1 w + l3 w^3)
//   sx_fixed_line        f, record, yP, xP, inf        -> sq_fixed_line
//   sx_fixed_line_n      f, record (r0 unused), xq, yi, inf -> sq_fixed_line_n (unreduced)
//   sx_miller3           f, 3 x (record, l0 l1 l3), xq, yi, inf -> three turns of
//                        sq_sqr, sq_fixed_line_n, sq_mul_line_r with nothing
//                        republished in between (the verifier's Miller step)
//   sx_xpow_turn         r, b -> conj(conj(r^2) b): sq_cyc_sqr, the publication
//                        of b, conjugate, sq_mul, conjugate (sq_expt's body)
// Every op writes 108 words: lane k's 18 limbs at 18 k.
//
// Adding an op: one DC_SX_OPS line (name, input words, LDS slots, slot of the
// second operand's group, waves per SIMD of the kernel), its branch in
// dc_sx_apply, and in tests/sx_ref.py its vectors, reference and mutants
// (test_every_sx_op_has_vectors fails until the Python side knows the op).
#pragma once
#include "sx29.h"

namespace fts {

static constexpr int DC_SX_F12 = 108, DC_SX_LINE = 54, DC_SX_OUT = 108;

#define DC_SX_OPS(X)                                                                      \
  X(sx_mulv, 2 * DC_SX_F12, SX_SLOTS_FEXP, SX_B, 2)                                       \
  X(sx_mulv24, 2 * DC_SX_F12, 24, 12, 2)                                                  \
  X(sx_sqr, DC_SX_F12, SX_SLOTS_MILLER_F, SX_B, 2)                                        \
  X(sx_cyc_sqr, DC_SX_F12, 24, 12, 2)                                                     \
  X(sx_inv, DC_SX_F12, SX_SLOTS_FEXP, SX_B, 2)                                          \
  X(sx_conj, DC_SX_F12, SX_SLOTS_FEXP, SX_B, 2)                                           \
  X(sx_frob1, DC_SX_F12, SX_SLOTS_FEXP, SX_B, 2)                                          \
  X(sx_frob2, DC_SX_F12, SX_SLOTS_FEXP, SX_B, 2)                                          \
  X(sx_frob3, DC_SX_F12, SX_SLOTS_FEXP, SX_B, 2)                                          \
  X(sx_mul_line_r, DC_SX_F12 + DC_SX_LINE, SX_SLOTS_MILLER_F, SX_B, 2)                    \
  X(sx_fixed_line, DC_SX_F12 + DC_SX_LINE + 19, SX_SLOTS_MILLER_F, SX_B, 2)               \
  X(sx_fixed_line_n, DC_SX_F12 + DC_SX_LINE + 19, SX_SLOTS_MILLER_F, SX_B, 2)             \
  X(sx_expt, DC_SX_F12, 24, 12, 2)                                                        \
  X(sx_fexp_easy, DC_SX_F12, SX_SLOTS_FEXP, SX_B, 2)                                    \
  X(sx_miller3, DC_SX_F12 + 3 * 2 * DC_SX_LINE + 19, SX_SLOTS_MILLER_F, SX_B, 2)          \
  X(sx_xpow_turn, 2 * DC_SX_F12, 24, 12, 2)

enum DcSxOp : int {
#define DC_X(name, nin, ns, bofs, waves) DC_##name,
  DC_SX_OPS(DC_X)
#undef DC_X
  DC_SX_OP_COUNT
};

struct DcSxInfo {
  const char* name;
  uint32_t nin, slots, bofs;
};
inline const DcSxInfo* dc_sx_table() {
  static const DcSxInfo t[DC_SX_OP_COUNT] = {
#define DC_X(name, nin, ns, bofs, waves) {#name, (uint32_t)(nin), (uint32_t)(ns), (uint32_t)(bofs)},
      DC_SX_OPS(DC_X)
#undef DC_X
  };
  return t;
}

FTS_HD f29 dc_sx_ld29(const uint32_t* in) {
  f29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = (int32_t)in[i];
  return r;
}
FTS_HD q2 dc_sx_ldq(const uint32_t* in) { return {dc_sx_ld29(in), dc_sx_ld29(in + 9)}; }
// a line record where it lies in the operand words (as the Miller kernels read
// theirs from the context's line table: a copy in registers, selected by lane
// role, would live in scratch)
FTS_HD const LineCoef29& dc_sx_ldline(const uint32_t* in) {
  static_assert(sizeof(LineCoef29) == 4 * DC_SX_LINE, "a line record is 54 words");
  return *reinterpret_cast<const LineCoef29*>(in);
}
FTS_HD void dc_sx_stq(uint32_t* out, const q2& a) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    out[i] = (uint32_t)a.c0.l[i];
    out[9 + i] = (uint32_t)a.c1.l[i];
  }
}

// lane x.k's program of op OP on the job whose operands start at `in`; pk: the
// lane's park planes (sx_expt only: slot 0 and the odd powers' 4..6)
template <int OP, class X, class P>
FTS_HD q2 dc_sx_apply(const X& x, const uint32_t* in, const P& pk) {
  const int k = x.k;
  const q2 a = dc_sx_ldq(in + 18 * k);
  if constexpr (OP == DC_sx_mulv || OP == DC_sx_mulv24) {
    return sq_mulv(x, a, dc_sx_ldq(in + DC_SX_F12 + 18 * k));
  } else if constexpr (OP == DC_sx_sqr) {
    return sq_sqr(x, a);
  } else if constexpr (OP == DC_sx_cyc_sqr) {
    return sq_cyc_sqr(x, a);
  } else if constexpr (OP == DC_sx_inv) {
    return sq_inv(x, a);
  } else if constexpr (OP == DC_sx_conj) {
    return sq_conj(k, a);
  } else if constexpr (OP == DC_sx_frob1) {
    return sq_frob1(k, a);
  } else if constexpr (OP == DC_sx_frob2) {
    return sq_frob2(k, a);
  } else if constexpr (OP == DC_sx_frob3) {
    return sq_frob3(k, a);
  } else if constexpr (OP == DC_sx_mul_line_r) {
    const uint32_t* l = in + DC_SX_F12;
    return sq_mul_line_r(x, a, dc_sx_ldq(l), dc_sx_ldq(l + 18), dc_sx_ldq(l + 36));
  } else if constexpr (OP == DC_sx_fixed_line || OP == DC_sx_fixed_line_n) {
    const uint32_t* q = in + DC_SX_F12;
    const f29 u = dc_sx_ld29(q + DC_SX_LINE), v = dc_sx_ld29(q + DC_SX_LINE + 9);
    const bool inf = q[DC_SX_LINE + 18] != 0;
    if constexpr (OP == DC_sx_fixed_line)
      return sq_fixed_line(x, a, dc_sx_ldline(q), u, v, inf);
    else
      return sq_fixed_line_n(x, a, dc_sx_ldline(q), u, v, inf);
  } else if constexpr (OP == DC_sx_expt) {
    pk.put(0, a);
    return sq_expt(x, pk, 0, 4);
  } else if constexpr (OP == DC_sx_fexp_easy) {
    return sq_fexp_easy(x, q2_to_fp2(a));
  } else if constexpr (OP == DC_sx_miller3) {
    const uint32_t* tail = in + DC_SX_F12 + 3 * 2 * DC_SX_LINE;
    const f29 xq = dc_sx_ld29(tail), yi = dc_sx_ld29(tail + 9);
    const bool inf = tail[18] != 0;
    q2 f = a;
#pragma nounroll
    for (int t = 0; t < 3; t++) {
      const uint32_t* s = in + DC_SX_F12 + t * 2 * DC_SX_LINE;
      f = sq_sqr(x, f);
      f = sq_fixed_line_n(x, f, dc_sx_ldline(s), xq, yi, inf);
      f = sq_mul_line_r(x, f, dc_sx_ldq(s + DC_SX_LINE), dc_sx_ldq(s + DC_SX_LINE + 18), dc_sx_ldq(s + DC_SX_LINE + 36));
    }
    return f;
  } else {
    static_assert(OP == DC_sx_xpow_turn, "dc_sx_apply: op without a branch");
    q2 r = sq_cyc_sqr(x, a);
    sq_pub(x, X::B, dc_sx_ldq(in + DC_SX_F12 + 18 * k));
    return sq_conj(k, sq_mul(x, sq_conj(k, r)));
  }
}

}  // namespace fts
