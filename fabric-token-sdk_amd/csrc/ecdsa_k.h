// Kernel declarations of ECDSA P-256 verification (k_ecdsa.hip), kept apart
// from launch.h so the P-256 code stays out of the pairing translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "dev/p256.h"

using namespace fts;

// One pass over n signatures (jobs sorted: the n_reg registered-key jobs first,
// then the ad-hoc ones):
//   k_ecdsa_pre   n lanes   SHA-256 of the message, range checks, s^-1, u1, u2
//   k_ecdsa_part  2n lanes  lanes [0, n): u1 G; lanes [n, 2n): u2 Q (table or windowed)
//   k_ecdsa_fin   n lanes   the final addition and the x == r comparison
// u: 2n scalars (u1 then u2); part: 2n points; vt: P256_VT_WORDS * (n - n_reg) words.
__global__ void k_ecdsa_pre(const EcdsaJob* jobs, uint32_t n, const uint8_t* blob, uint32_t (*u)[8], uint8_t* ok);
__global__ void k_ecdsa_part(const EcdsaJob* jobs, uint32_t n, uint32_t n_reg, const uint8_t* blob,
                             const uint32_t (*u)[8], const P256Aff* tabs, uint32_t* vt, P256Jac* part);
__global__ void k_ecdsa_fin(const EcdsaJob* jobs, uint32_t n, const uint8_t* blob, const P256Jac* part, uint8_t* ok);
