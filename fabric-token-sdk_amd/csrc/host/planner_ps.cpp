// Pointcheval-Sanders verification passes: see planner_ps.h.
#include "planner_ps.h"

#include <string.h>

namespace ftsh {

namespace {

uint32_t put_wire(Plan& pl, const uint8_t* p, size_t n) {
  pl.wire.resize((pl.wire.size() + 15) & ~(size_t)15, 0);
  uint32_t off = (uint32_t)pl.wire.size();
  pl.wire.insert(pl.wire.end(), p, p + n);
  return off;
}
uint32_t zr(Plan& pl, uint32_t raw) {
  ZrJob j;
  j.raw = raw;
  j.len = 32;
  j.out = pl.n_scal++;
  pl.zr.push_back(j);
  return j.out;
}
uint32_t point(Plan& pl, uint32_t raw) {
  DecodeJob j;
  j.raw = raw;
  j.len = 64;
  j.out = pl.n_pts++;
  j.bytes = NONE;
  j.b64 = NONE;
  pl.dec.push_back(j);
  return j.out;
}
void check(Plan& pl, uint8_t kind, uint8_t code, uint32_t a, uint32_t b) {
  Check c;
  c.kind = kind;
  c.code = code;
  c.pad = 0;
  c.a = a;
  c.b = b;
  pl.ck.push_back(c);
}

}  // namespace

void plan_ps_item(Plan& pl, const PsIn& in) {
  // the scalar 1 of c = 1 in P1 = sigbf P - c S and t' = c PK0 + ..: once per piece
  if (pl.zr.empty()) {
    uint8_t one[32] = {0};
    one[31] = 1;
    zr(pl, put_wire(pl, one, 32));
  }
  const uint32_t s_one = pl.zr[0].out;
  const uint32_t w_m = put_wire(pl, in.m, 32), w_h = put_wire(pl, in.h, 32);
  const uint32_t w_r = put_wire(pl, in.r, 64), w_s = put_wire(pl, in.s, 64);
  const uint32_t s_m = zr(pl, w_m), s_h = zr(pl, w_h);
  const uint32_t R = point(pl, w_r), S = point(pl, w_s);
  TxChecks tc;
  tc.wf_start = (uint32_t)pl.ck.size();
  tc.wf_count = 2;
  tc.rg_start = tc.wf_start + 2;
  tc.rg_count = 0;
  tc.mode = 1;
  check(pl, CK_PTS, E_PARSE, R, 2);
  // P1 = -S (pairs with Q)
  G1Job g;
  memset(&g, 0, sizeof(g));
  g.nfix = 0;
  g.vstart = (uint32_t)pl.vt.size();
  g.vcount = 1;
  VTerm v;
  v.pt = S;
  v.w_lo = 1;
  v.w_hi = 0;
  v.flags = 0;
  pl.vt.push_back(v);
  g.vscal = s_one;
  g.vneg = 1;
  g.out = pl.n_g1out++;
  g.bytes = NONE;
  g.b64 = NONE;
  pl.g1p.push_back(g);
  // t' = PK0 + m PK1 + h PK2 (pairs with R)
  G2Job g2;
  memset(&g2, 0, sizeof(g2));
  g2.nfix = 3;
  g2.fbase[0] = G2B_PK0;
  g2.fscal[0] = s_one;
  g2.fbase[1] = G2B_PK1;
  g2.fscal[1] = s_m;
  g2.fbase[2] = G2B_PK2;
  g2.fscal[2] = s_h;
  g2.out = pl.n_g2out++;
  pl.g2.push_back(g2);
  pl.pr.push_back({g.out, R, g2.out, NONE, NONE});
  check(pl, CK_GT, (uint8_t)E_PS_SIGNATURE, (uint32_t)pl.pr.size() - 1, 0);
  pl.tx.push_back(tc);
}

void plan_ps_items(size_t n, const PsIn* items, PlanWork& w, WorkPool& pool) {
  size_t np = plan_piece_count(n, pool.size());
  if (w.pieces.size() < np) w.pieces.resize(np);
  w.used = np;
  pool.run(np, [&](size_t c) {
    Plan& p = w.pieces[c];
    p.clear();
    size_t lo = n * c / np, hi = n * (c + 1) / np;
    for (size_t i = lo; i < hi; i++) plan_ps_item(p, items[i]);
  });
}

void ps_hash_index(uint64_t i, uint8_t m_be[32], uint8_t h_be[32]) {
  uint32_t mi[8] = {(uint32_t)i, (uint32_t)(i >> 32), 0, 0, 0, 0, 0, 0};
  limbs_to_be32(m_be, mi);  // Zr.Bytes(): 32 bytes big-endian
  uint8_t d[32];
  Sha256 s;
  s.init();
  s.update(m_be, 32);
  s.final(d);
  uint32_t hm[8];
  digest_mod_r(hm, d);
  limbs_to_be32(h_be, hm);
}

}  // namespace ftsh
