// TEST-ONLY stand-alone driver (own main) for the variable-base G1 chain of
// dev/jobs.h on the carry-free form: g1_mul_glv16_halves (window table in
// balanced 29-bit limbs with beta x stored, built by j29_dbl / j29_madd, empty
// steps skipped) and g1_var_point.  It only RUNS the code and prints operands
// and affine results; tests/test_g1_chain.py holds the reference, a
// big-integer double-and-add, and the assertions.
//
// Lines (every number in hex, points as the 64 bytes x || y, "-" for infinity):
//   halves <P> <zin> <k1> <n1> <k2> <n2> <result>   (-1)^n1 k1 V + (-1)^n2 k2 phi(V), V = (P.x zin^2 : P.y zin^3 : zin)
//   mul <P> <k> <result>                            k P through glv_split
//   consts <beta> <lambda>                          phi(x, y) = (beta x, y) = lambda (x, y)
//   var <horner> <vneg> <k> <count> {<P_t> <w_t> <neg_t>} <result>   job_g1_part, part 3
// Built a second time with -fsanitize=signed-integer-overflow,undefined: a
// 64-bit column that overflows aborts that run.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../fabric-token-sdk_amd/csrc/dev/jobs.h"

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
  v[0] |= 1;            // not zero
  return fe_from_int<ModP>(v);
}
void rnd_scalar(uint32_t s[8]) {
  for (int i = 0; i < 8; i++) s[i] = (uint32_t)rnd();
  s[7] &= 0x0fffffffu;  // < 2^252 < r
}

g1a gen() { return {fe_one<ModP>(), fe_one<ModP>() + fe_one<ModP>(), false}; }
const int POOL = 64;
g1a pool[POOL];
void fill_pool() {
  for (int i = 0; i < POOL; i++) {
    uint32_t s[8];
    rnd_scalar(s);
    pool[i] = jac_to_aff(aff_mul(gen(), s));
  }
}
g1a rnd_point() { return pool[rnd() % POOL]; }

void put_point(const g1a& a) {
  if (a.inf) {
    printf(" -");
    return;
  }
  uint8_t b[64];
  g1_to_bytes(b, a);
  printf(" ");
  for (int i = 0; i < 64; i++) printf("%02x", b[i]);
}
void put_words(const uint32_t* w, int n) {
  printf(" ");
  for (int i = n - 1; i >= 0; i--) printf("%08x", w[i]);
}
void put_fp(const fp& a) {
  uint32_t t[8];
  fe_to_int(t, a);
  put_words(t, 8);
}

void halves_case(const uint32_t k1[4], bool n1, const uint32_t k2[4], bool n2, bool with_z) {
  const g1a P = rnd_point();
  const fp z = with_z ? rnd_fp() : fe_one<ModP>(), z2 = sqr(z);
  const g1a V = {P.x * z2, P.y * (z2 * z), false};
  G1Tab29 tb[8];
  const g1j got = g1_mul_glv16_halves(V, z, k1, n1, k2, n2, tb, 1);
  printf("halves");
  put_point(P);
  put_fp(z);
  put_words(k1, 4);
  printf(" %d", (int)n1);
  put_words(k2, 4);
  printf(" %d", (int)n2);
  put_point(jac_to_aff(got));
  printf("\n");
}

void halves_section() {
  // 0, 1, every window digit 8 / -8 (g1fused_main.cpp's nibble patterns), bit
  // 127 set (window 32 holds a digit), 2^128 - 1, the top 8, 12 and 124 bits zero
  uint32_t hs[10][4] = {{0, 0, 0, 0},
                        {1, 0, 0, 0},
                        {0x78787878u, 0x78787878u, 0x78787878u, 0x78787878u},
                        {0x87878788u, 0x78787878u, 0x78787878u, 0xf8787878u},
                        {0, 0, 0, 0x80000000u},
                        {0, 0, 0, 0},
                        {~0u, ~0u, ~0u, ~0u},
                        {0, 0, 0, 0},
                        {0, 0, 0, 0},
                        {0, 0, 0, 0}};
  for (int i = 0; i < 4; i++) hs[5][i] = hs[7][i] = hs[8][i] = (uint32_t)rnd();
  hs[5][3] |= 0x80000000u;
  hs[7][3] &= 0x00ffffffu;
  hs[8][3] &= 0x000fffffu;
  hs[9][0] = 2 + (uint32_t)(rnd() % 14);
  int c = 0;
  for (int a = 0; a < 10; a++)
    for (int b = 0; b < 10; b++)
      for (int sg = 0; sg < 4; sg++) halves_case(hs[a], (sg & 1) != 0, hs[b], (sg & 2) != 0, (c++ % 3) == 1);
}

void mul_section() {
  uint32_t ks[203][8] = {{0}, {1}, {0}};
  fe_to_int(ks[2], fe_zero<ModR>() - fe_one<ModR>());  // r - 1
  for (int t = 3; t < 203; t++) rnd_scalar(ks[t]);
  for (int t = 0; t < 203; t++) {
    const g1a P = rnd_point();
    G1Tab29 tb[8];
    printf("mul");
    put_point(P);
    put_words(ks[t], 8);
    put_point(jac_to_aff(g1_mul_glv16(P, ks[t], tb, 1)));
    printf("\n");
  }
}

// one variable part through job_g1_part (part 3 of a one-job batch)
void var_case(int horner, int vneg, const std::vector<g1a>& P, const std::vector<uint64_t>& w,
              const std::vector<int>& neg) {
  const uint32_t cnt = (uint32_t)P.size();
  std::vector<G1Dev> pts(cnt);
  std::vector<VTerm> vt(cnt);
  for (uint32_t t = 0; t < cnt; t++) {
    g1_store(pts[t], P[t]);
    vt[t].pt = t;
    vt[t].w_lo = (uint32_t)w[t];
    vt[t].w_hi = (uint32_t)(w[t] >> 32);
    vt[t].flags = ((horner && t == 0) ? VT_HORNER : 0) | (neg[t] ? VT_NEG : 0);
  }
  G1Job j{};
  j.vcount = cnt;
  j.vscal = 0;
  j.vneg = (uint32_t)vneg;
  uint32_t scal[1][8];
  rnd_scalar(scal[0]);
  G1JDev part[4];
  job_g1_part(&j, 1, 3, vt.data(), pts.data(), scal, nullptr, part, nullptr);
  printf("var %d %d", horner, vneg);
  put_words(scal[0], 8);
  printf(" %u", cnt);
  for (uint32_t t = 0; t < cnt; t++) {
    put_point(P[t]);
    printf(" %llx %d", (unsigned long long)w[t], neg[t]);
  }
  put_point(jac_to_aff(g1j_load(part[3])));
  printf("\n");
}

void var_section() {
  for (int vneg = 0; vneg < 2; vneg++) {
    // a single unit-weight point
    var_case(0, vneg, {rnd_point()}, {1}, {0});
    var_case(1, vneg, {rnd_point()}, {16}, {0});
    // PP-A: Horner weights (100, 1), joint double-and-add
    var_case(1, vneg, {rnd_point(), rnd_point()}, {100, 100}, {0, 0});
    // PP-B: Horner with b = 16 over 16 digits
    {
      std::vector<g1a> P;
      for (int t = 0; t < 16; t++) P.push_back(rnd_point());
      var_case(1, vneg, P, std::vector<uint64_t>(16, 16), std::vector<int>(16, 0));
    }
    // explicit weights, the top one -2^63 (VT_NEG), and a lone negated term
    var_case(0, vneg, {rnd_point(), rnd_point(), rnd_point()}, {1ull << 63, 10000, 1}, {1, 0, 0});
    var_case(0, vneg, {rnd_point()}, {1}, {1});
    // equal and opposite points meet in the joint sum: P + P and P - P
    {
      const g1a A = rnd_point();
      var_case(0, vneg, {A, A}, {1, 1}, {0, 0});
      var_case(0, vneg, {A, A}, {1, 1}, {0, 1});
      var_case(0, vneg, {A, A, rnd_point()}, {5, 5, 3}, {0, 1, 0});
    }
  }
}

}  // namespace

int main() {
  fill_pool();
  // the endomorphism's constants as the code holds them (the test checks that they pair up)
  uint32_t lam[8];
  fe_to_int(lam, fe_const<ModR>(GLV_LAMBDA));
  printf("consts");
  put_fp(fe_const<ModP>(GLV_BETA));
  put_words(lam, 8);
  printf("\n");
  halves_section();
  mul_section();
  var_section();
  return 0;
}
