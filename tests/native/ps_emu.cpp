// TEST-ONLY: the Pointcheval-Sanders verification pass on the CPU -- the
// product's planner (host/planner_ps.cpp, relocated through host/planner.cpp's
// flat plan) and the device job functions of dev/jobs.h in the order the
// runtime launches them, ending in the sextet unity test (sx_gt_lane_one /
// sx_gt_votes_one on a wave of ten jobs) and job_verdict_gt.  The product
// library contains no CPU execution path; this file is never part of it.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/dev/jobs.h"
#include "../../fabric-token-sdk_amd/csrc/host/planner.h"
#include "../../fabric-token-sdk_amd/csrc/host/planner_ps.h"

using namespace fts;
using namespace ftsh;

namespace {

struct PsEmu {
  PPInfo pp;
  std::vector<G2Dev> g2tab;  // PK0, PK1, PK2: |d| 2^(C w) B as job_tab_g2 defines them
  std::vector<LineCoef> qlines;
  std::vector<G1Dev> sig;    // decoded SignedValues: R_0, S_0, R_1, S_1, ..
  int fexp = 0;
};

// the table of job_tab_g2 by successive additions (a scalar multiplication per
// entry is too slow for a sanitizer build)
void build_g2tab(const G2Dev* bases, int nb, std::vector<G2Dev>& tab) {
  tab.resize((size_t)nb * G2TAB_WINDOWS * G2TAB_DIGITS);
  for (int b = 0; b < nb; b++) {
    g2a Bw = g2_load(bases[b]);
    for (int w = 0; w < G2TAB_WINDOWS; w++) {
      G2Dev* t = &tab[((size_t)b * G2TAB_WINDOWS + w) * G2TAB_DIGITS];
      g2j acc = jac_from_aff(Bw);
      for (int d = 1; d <= G2TAB_DIGITS; d++) {
        if (d == 2) acc = jac_dbl(acc);
        if (d > 2) acc = jac_add_aff(acc, Bw);
        g2_store(t[d - 1], Bw.inf ? Bw : jac_to_aff(acc));
      }
      if (!Bw.inf) Bw = jac_to_aff(jac_dbl(acc));  // 2 x 2^(C-1) 2^(C w) B
    }
  }
}

// the unity bytes of n pair jobs as k_fexp_hard_one computes them: waves of ten
// sextets, lane 6 s + k votes on coefficient k of job (wave, s), ghost lanes
// and sextets past n vote true
void unity_bytes(const std::vector<F12Dev>& g, uint8_t* gt_ok) {
  const size_t n = g.size();
  for (size_t w0 = 0; w0 < n; w0 += 10) {
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t sx = lane / 6;
      const size_t job = w0 + sx;
      bool vote = true;
      if (sx < 10 && job < n) {
        const int k = (int)(lane - 6 * sx);
        const uint32_t* wd = &g[job].w[16 * sx_f12_index(k)];
        fp2 c;
        for (int i = 0; i < 8; i++) {
          c.c0.v[i] = wd[i];
          c.c1.v[i] = wd[8 + i];
        }
        vote = sx_gt_lane_one(k, c);
      }
      if (vote) ballot |= 1ull << lane;
    }
    for (uint32_t sx = 0; sx < 10 && w0 + sx < n; sx++) gt_ok[w0 + sx] = sx_gt_votes_one(ballot, sx) ? 1 : 0;
  }
}

}  // namespace

extern "C" {

void* ps_emu_create(const uint8_t* pp, size_t len) {
  PsEmu* c = new PsEmu();
  if (!parse_pp(pp, len, "zkatdlog", c->pp).empty()) {
    delete c;
    return nullptr;
  }
  G2Dev g2[4];
  for (int k = 0; k < 4; k++) {
    std::vector<uint8_t> raw = k < 3 ? c->pp.pk[k] : c->pp.q;
    raw.resize(std::max<size_t>(raw.size(), 128), 0);
    if (!decode_g2(raw.data(), 128, g2[k], nullptr)) {
      delete c;
      return nullptr;
    }
  }
  build_g2tab(g2, 3, c->g2tab);
  c->qlines.resize(MILLER_LINES);
  precompute_lines(c->qlines.data(), g2_load(g2[3]));
  const size_t nsig = c->pp.sig_r.size();
  c->sig.resize(2 * nsig);
  for (size_t k = 0; k < 2 * nsig; k++) {
    std::vector<uint8_t> raw = (k & 1) ? c->pp.sig_s[k / 2] : c->pp.sig_r[k / 2];
    raw.resize(std::max<size_t>(raw.size(), 64) + 64, 0);
    DecodeJob j{0, 64, (uint32_t)k, NONE, NONE};
    if (!job_decode(j, raw.data(), c->sig.data(), nullptr)) {
      delete c;
      return nullptr;
    }
  }
  return c;
}
void ps_emu_destroy(void* h) { delete (PsEmu*)h; }
void ps_emu_set_fexp(void* h, int variant) { ((PsEmu*)h)->fexp = variant; }

// sigs: n records of 192 bytes (m | h | r | s, ftz_ps_sig); planned in
// `threads` pieces when n allows (plan_piece_count), so the relocation of
// every index -- CK_GT's pair job among them -- runs as in the product
int ps_emu_verify(void* h, size_t n, const uint8_t* sigs, int32_t* codes, int threads) {
  PsEmu* c = (PsEmu*)h;
  if (n == 0) return 0;
  std::vector<PsIn> items(n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t* g = sigs + 192 * i;
    items[i] = {g, g + 32, g + 64, g + 128};
  }
  WorkPool pool(std::max(1, threads));
  PlanWork w;
  plan_ps_items(n, items.data(), w, pool);
  FlatPlan fp;
  if (!flat_layout(w, false, fp).empty() || fp.n_items != n) return -1;
  std::vector<uint8_t> blob(fp.bytes);
  flat_write(w, fp, blob.data(), std::vector<uint8_t>(C_SIZE, 0).data(), pool);
  Plan p;
  plan_unflatten(fp, blob.data(), p);
  if (p.g2.size() != p.pr.size() || !p.hpre.empty() || !p.hmain.empty() || p.tx.size() != n) return -1;
  std::vector<uint8_t> wire = p.wire;
  wire.resize(wire.size() + WIRE_TAIL, 0);
  std::vector<G1Dev> pts(p.n_pts);
  std::vector<uint8_t> pt_ok(p.n_pts, 1), canon(p.n_scal), gt_ok(p.pr.size());
  std::vector<uint32_t> scalv(8 * (size_t)p.n_scal);
  uint32_t(*scal)[8] = reinterpret_cast<uint32_t(*)[8]>(scalv.data());
  std::vector<G1Dev> g1out(p.n_g1out);
  std::vector<G2Dev> g2out(p.n_g2out);
  std::vector<F12Dev> fbuf(p.pr.size()), gt(p.pr.size());
  for (auto& j : p.dec) pt_ok[j.out] = job_decode(j, wire.data(), pts.data(), nullptr);
  for (auto& j : p.zr) job_zr(j, wire.data(), scal, canon.data());
  for (auto& j : p.g1p) job_g1(j, p.vt.data(), pts.data(), scal, nullptr, g1out.data(), nullptr);
  for (auto& j : p.g2) job_g2(j, scal, c->g2tab.data(), g2out.data());
  for (size_t i = 0; i < p.pr.size(); i++) {
    if (p.pr[i].bytes != NONE || p.pr[i].p3 != NONE || p.pr[i].q2 != p.g2[i].out) return -1;
    job_miller(p.pr[i], c->qlines.data(), g1out.data(), pts.data(), g2out.data(), fbuf.data(), (uint32_t)i);
    f12_store(gt[i], final_exp(f12_load(fbuf[i]), c->fexp));
  }
  unity_bytes(gt, gt_ok.data());
  for (size_t i = 0; i < n; i++) codes[i] = job_verdict_gt(p.tx[i], p.ck.data(), pt_ok.data(), gt_ok.data());
  return 0;
}

// ftz_pp_audit_signed_values restated: entry i with m = i and h = HashToZr(i's
// 32 bytes), and E_PS_SIGNATURE for an entry holding the point at infinity
int ps_emu_audit(void* h, int32_t* codes, size_t cap, size_t* count) {
  PsEmu* c = (PsEmu*)h;
  const size_t n = c->pp.sig_r.size();
  *count = n;
  if (cap < n) return -1;
  std::vector<uint8_t> sigs(192 * n, 0);
  for (size_t i = 0; i < n; i++) {
    uint8_t* g = &sigs[192 * i];
    ps_hash_index(i, g, g + 32);
    memcpy(g + 64, c->pp.sig_r[i].data(), std::min<size_t>(64, c->pp.sig_r[i].size()));
    memcpy(g + 128, c->pp.sig_s[i].data(), std::min<size_t>(64, c->pp.sig_s[i].size()));
  }
  int rc = ps_emu_verify(h, n, sigs.data(), codes, 1);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++)
    if (g1_load(c->sig[2 * i]).inf || g1_load(c->sig[2 * i + 1]).inf) codes[i] = E_PS_SIGNATURE;
  return 0;
}

// The sextet unity predicate on one GT value given as twelve 32-byte big-endian
// Fp coefficients in F12Dev word order (Fp2 word q = coefficients 2 q, 2 q + 1),
// placed as sextet `sx` of a wave.  Bit 0: the verdict with every other lane of
// the wave voting true; bit 1: with every other lane voting false (the two
// must agree: a sextet reads its own six bits only).
int ps_emu_unity(const uint8_t* coef, uint32_t sx) {
  uint64_t own = 0;
  for (int k = 0; k < 6; k++) {
    const uint8_t* b = coef + 64 * sx_f12_index(k);
    uint32_t t[8];
    fp2 cf;
    be32_to_limbs(t, b);
    cf.c0 = fe_from_int<ModP>(t);
    be32_to_limbs(t, b + 32);
    cf.c1 = fe_from_int<ModP>(t);
    if (sx_gt_lane_one(k, cf)) own |= 1ull << (6 * sx + k);
  }
  const uint64_t mask = 63ull << (6 * sx);
  return (sx_gt_votes_one(own | ~mask, sx) ? 1 : 0) | (sx_gt_votes_one(own, sx) ? 2 : 0);
}

}  // extern "C"
