// ECDSA P-256 signing kernels (dev/ecsign.h, ecsign_k.h).  A signature is one
// lane in k_ecsign_pre and k_ecsign_fin and ECSIGN_PARTS = 4 lanes in
// k_ecsign_part (part-major, so a wave runs one range of windows): a pass is at
// most 4,096 signatures, 64 waves on 1,024 SIMDs with one lane each.
#include "ecsign_k.h"

__global__ void __launch_bounds__(64) k_ecsign_pre(const EcsignJob* jobs, uint32_t n, const uint8_t* blob,
                                                   const uint32_t (*keys)[8], uint32_t (*k)[8], uint32_t (*e)[8]) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const EcsignJob j = jobs[i];
  Sha256 h;
  h.init();
  h.update(blob + j.msg, j.msg_len);
  uint8_t dg[32];
  h.final(dg);
  uint32_t ee[8], d[8], kk[8], ent[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t[8];
  be32_to_limbs(ee, dg);
#pragma unroll
  for (int w = 0; w < 8; w++) d[w] = keys[j.signer][w];
  if (j.entropy) {
    be32_to_limbs_g(t, blob + j.entropy);
    limbs_to_words(ent, t);
  }
  ecsign_nonce(kk, d, ee, ent, j.entropy != 0);
#pragma unroll
  for (int w = 0; w < 8; w++) {
    k[i][w] = kk[w];
    e[i][w] = ee[w];
  }
}

__global__ void __launch_bounds__(64) k_ecsign_part(uint32_t n, const uint32_t (*k)[8], const P256Aff* tab,
                                                    P256Jac* part) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ECSIGN_PARTS * n) return;
  const uint32_t p = i / n, s = i - p * n;
  uint32_t kk[8];
#pragma unroll
  for (int w = 0; w < 8; w++) kk[w] = k[s][w];
  p256_store(part[i], p256_fixed_mul_uniform(tab, kk, (int)p * ECSIGN_PART_WINDOWS, ECSIGN_PART_WINDOWS));
}

__global__ void __launch_bounds__(64) k_ecsign_fin(const EcsignJob* jobs, uint32_t n, const uint32_t (*keys)[8],
                                                   const P256Jac* part, uint32_t (*k)[8], const uint32_t (*e)[8],
                                                   uint8_t* rs, uint8_t* ok) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  p256j R = p256_load(part[i]);
#pragma nounroll
  for (uint32_t p = 1; p < ECSIGN_PARTS; p++) R = p256_add(R, p256_load(part[(size_t)p * n + i]));
  uint32_t kk[8], ee[8], d[8], r[8], s[8];
  const int32_t signer = jobs[i].signer;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    kk[w] = k[i][w];
    ee[w] = e[i][w];
    d[w] = keys[signer][w];
  }
  bool good = ecsign_finish(R, kk, ee, d, r, s);
  limbs_to_be32_g(rs + (size_t)i * 64, r);
  limbs_to_be32_g(rs + (size_t)i * 64 + 32, s);
  ok[i] = good ? 1 : 0;
#pragma unroll
  for (int w = 0; w < 8; w++) k[i][w] = 0;
}
