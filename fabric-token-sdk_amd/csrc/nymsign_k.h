// Kernel declarations of idemix pseudonym signing on BN254 (k_nymsign.hip), beside ecsign_k.h.
#pragma once
#include <hip/hip_runtime.h>

#include "dev/nymsign.h"

using namespace fts;

// One pass over n signatures; keys: the handle's user secrets (limbs), by signer index:
//   k_nymsign_pre   n lanes   SHA-256 of the message, the DRBG, r_sk, r_rnym and nonce (limbs, < r)
//   k_nymsign_part  NYMSIGN_PARTS n lanes, part-major: lanes [p n, (p + 1) n) run base p / NYMSIGN_SLICES
//                   (0: HSk with s0, 1: HRand with s1), windows (p % NYMSIGN_SLICES) * NYMSIGN_PART_WINDOWS on
//   k_nymsign_fin   n lanes   t = the sum of the parts, the transcript hash, ProofC and the two responses;
//                   then the lane's r_sk, r_rnym and nonce slots are zeroed
// r_sk, r_rnym, nonce: n scalars each; part: NYMSIGN_PARTS * n points; out: n x 128 bytes; ok: n bytes.
__global__ void k_nymsign_pre(const NymSignJob* jobs, uint32_t n, const uint8_t* blob, const uint32_t (*keys)[8],
                              uint32_t (*r_sk)[8], uint32_t (*r_rnym)[8], uint32_t (*nonce)[8]);
__global__ void k_nymsign_part(uint32_t n, const uint32_t (*s0)[8], const uint32_t (*s1)[8], const QDev* tab,
                               QJDev* part);
__global__ void k_nymsign_fin(const NymSignJob* jobs, uint32_t n, uint8_t* blob, const uint32_t (*keys)[8],
                              const QJDev* part, uint32_t (*r_sk)[8], uint32_t (*r_rnym)[8], uint32_t (*nonce)[8],
                              uint8_t* out, uint8_t* ok);
// MakeNym: Nym_i = sk HSk + RNym_i HRand through k_nymsign_part on (sk, RNym_i):
//   k_nym_make_pre  n lanes   s0[i] = keys[signer], s1[i] = the i-th of r_nyms (n x 32 bytes big-endian)
//   k_nym_make_fin  n lanes   the sum of the parts as 64 bytes of RawBytes; then s0[i] and s1[i] are zeroed
__global__ void k_nym_make_pre(uint32_t n, const uint32_t (*keys)[8], int32_t signer, const uint8_t* r_nyms,
                               uint32_t (*s0)[8], uint32_t (*s1)[8]);
__global__ void k_nym_make_fin(uint32_t n, const QJDev* part, uint32_t (*s0)[8], uint32_t (*s1)[8], uint8_t* nyms);
