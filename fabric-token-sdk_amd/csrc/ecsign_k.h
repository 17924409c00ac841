// Kernel declarations of ECDSA P-256 signing (k_ecsign.hip), beside ecdsa_k.h.
#pragma once
#include <hip/hip_runtime.h>

#include "dev/ecsign.h"

using namespace fts;

// One pass over n signatures; keys: the handle's private scalars (limbs), by signer index:
//   k_ecsign_pre   n lanes   SHA-256 of the message, the RFC 6979 nonce k, e = the digest
//   k_ecsign_part  4n lanes  lanes [p n, (p + 1) n): windows 8p .. 8p + 7 of k G from G's table
//   k_ecsign_fin   n lanes   the sum of the parts, r, s = k^-1 (e + r d) made low; then k is zeroed
// k, e: n scalars each; part: ECSIGN_PARTS * n points; rs: n x 64 bytes (r || s big-endian); ok: n bytes.
__global__ void k_ecsign_pre(const EcsignJob* jobs, uint32_t n, const uint8_t* blob, const uint32_t (*keys)[8],
                             uint32_t (*k)[8], uint32_t (*e)[8]);
__global__ void k_ecsign_part(uint32_t n, const uint32_t (*k)[8], const P256Aff* tab, P256Jac* part);
__global__ void k_ecsign_fin(const EcsignJob* jobs, uint32_t n, const uint32_t (*keys)[8], const P256Jac* part,
                             uint32_t (*k)[8], const uint32_t (*e)[8], uint8_t* rs, uint8_t* ok);
