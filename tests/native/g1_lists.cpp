// TEST-ONLY: structure of the k_g1_part work lists and of the shared variable
// partials in a flattened verifier plan (host/planner.h g1_part_lists, dev/jobs.h
// G1Job.sh_first / sh_count).  Built with the planner by tests/test_g1_shared.py.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/dev/jobs.h"
#include "../../fabric-token-sdk_amd/csrc/host/planner.h"
#include "../../include/ftsamd.h"

using namespace fts;
using namespace ftsh;

namespace {

std::string check_side(const Plan& p, const std::vector<G1Job>& jobs, const std::vector<uint32_t>& fl,
                       const std::vector<uint32_t>& vl, uint32_t* stats) {
  const size_t n = jobs.size();
  char buf[160];
  auto fail = [&](const char* what, size_t a, size_t b) {
    snprintf(buf, sizeof buf, "%s (%zu, %zu)", what, a, b);
    return std::string(buf);
  };
  // every (job, fixed term) exactly once, in the fixed list only
  std::vector<uint8_t> seen(4 * n, 0);
  for (uint32_t i : fl) {
    if (i >= 3 * n) return fail("fixed list entry out of range", i, n);
    if (i / n >= jobs[i % n].nfix) return fail("fixed list holds an idle term", i / n, i % n);
    if (seen[i]++) return fail("fixed term listed twice", i / n, i % n);
  }
  size_t nf = 0;
  for (const G1Job& j : jobs) nf += j.nfix;
  if (fl.size() != nf) return fail("fixed list misses terms", fl.size(), nf);
  // every own chain exactly once
  for (uint32_t i : vl) {
    if (i < 3 * n || i >= 4 * n) return fail("variable list entry out of range", i, n);
    const G1Job& j = jobs[i - 3 * n];
    if (j.vscal == NONE || j.sh_count) return fail("variable list holds a job without a chain", i - 3 * n, j.sh_count);
    if (seen[i]++) return fail("chain listed twice", i - 3 * n, 0);
  }
  size_t nv = 0, nshare = 0, nwide = 0;
  for (size_t k = 0; k < n; k++) {
    const G1Job& j = jobs[k];
    if (j.vscal != NONE && !j.sh_count) nv++;
    if (j.vscal != NONE && !j.sh_count && j.vcount > G1_SHARE_MAX) nwide++;
    if (!j.sh_count) continue;
    nshare++;
    if (j.sh_count > G1_SHARE_MAX) return fail("shares more siblings than the cap", k, j.sh_count);
    if (j.vscal == NONE || j.vcount != j.sh_count) return fail("sharing job without its own terms", k, j.vcount);
    if ((size_t)j.sh_first + j.sh_count > k) return fail("siblings do not precede the job", k, j.sh_first);
    for (uint32_t s = 0; s < j.sh_count; s++) {
      const G1Job& q = jobs[j.sh_first + s];
      if (q.sh_count || q.vscal != j.vscal || q.vneg != j.vneg || q.vcount != 1)
        return fail("sibling of another scalar, sign or shape", k, s);
      const VTerm &a = p.vt[j.vstart + s], &b = p.vt[q.vstart];
      if (a.pt != b.pt || a.flags || b.flags || a.w_lo != 1 || a.w_hi || b.w_lo != 1 || b.w_hi)
        return fail("sibling is not the job's unit-weight term", k, s);
    }
  }
  if (vl.size() != nv) return fail("variable list misses chains", vl.size(), nv);
  stats[0] += (uint32_t)n;
  stats[1] += (uint32_t)nshare;
  stats[2] += (uint32_t)fl.size();
  stats[3] += (uint32_t)vl.size();
  stats[4] += (uint32_t)nwide;
  return "";
}

}  // namespace

// Plans the transfers (merged through the flat plan, `threads` pieces at 32
// items a piece) and checks both job arrays; stats: jobs, sharing jobs, fixed
// list entries, variable list entries, own chains wider than the cap.
extern "C" int g1l_check(const uint8_t* pp_json, size_t pp_len, size_t n, const ftz_transfer* tx, int threads,
                         uint32_t* stats, char* err, size_t errlen) {
  PPInfo pp;
  std::string e = parse_pp(pp_json, pp_len, "zkatdlog", pp);
  std::vector<TransferIn> t(n);
  for (size_t i = 0; i < n; i++)
    t[i] = {tx[i].inputs, tx[i].n_in, tx[i].outputs, tx[i].n_out, tx[i].proof, tx[i].proof_len};
  Plan p;
  memset(stats, 0, 5 * sizeof(uint32_t));
  if (e.empty()) {
    plan_transfers(pp, n, t.data(), p, threads);
    e = check_side(p, p.g1, p.g1fl, p.g1vl, stats);
  }
  if (e.empty()) e = check_side(p, p.g1p, p.g1pfl, p.g1pvl, stats);
  if (e.empty()) return 0;
  snprintf(err, errlen, "%s", e.c_str());
  return 1;
}
