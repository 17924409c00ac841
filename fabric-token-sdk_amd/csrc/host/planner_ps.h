// Host planner of Pointcheval-Sanders verification passes (pssign.SignVerifier
// .Verify, crypto/pssign/sign.go:125-160): items -> the flat job arrays of
// dev/jobs.h, as host/planner.cpp plans the membership verification it is a
// special case of (c = 1, sigbf = 0).
#pragma once
#include "planner.h"

namespace ftsh {

// One signature on one message: m, h as 32 big-endian bytes, R, S as 64-byte
// gnark G1 encodings (the layout of ftz_ps_sig).
struct PsIn {
  const uint8_t* m;
  const uint8_t* h;
  const uint8_t* r;
  const uint8_t* s;
};

// Appends item `in` to the plan:
//   decode R, S;  scalars m, h (ZrJob: reduced mod r) and the piece's constant 1;
//   P1 = -S (a G1 job of the pairing chain: no fixed term, -(1) S);
//   t' = 1 PK0 + m PK1 + h PK2 (G2 job);  pair job (P1 with Q, R with t'),
//   bytes NONE: a PS pass writes no GT bytes and plans no hash job;
//   checks: CK_PTS E_PARSE over (R, S), then CK_GT E_PS_SIGNATURE on the pair job.
void plan_ps_item(Plan& pl, const PsIn& in);
// n items into w's pieces on the pool (as plan_items)
void plan_ps_items(size_t n, const PsIn* items, PlanWork& w, WorkPool& pool);
// HashToZr(32-byte big-endian i) as 32 big-endian bytes: the h that
// GenerateRangeProofParameters signs next to m = i (setup.go:168-184, :198-206)
void ps_hash_index(uint64_t i, uint8_t m_be[32], uint8_t h_be[32]);

}  // namespace ftsh
