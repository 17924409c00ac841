// Idemix pseudonym signing kernels on BN254 (dev/nymsign.h, nymsign_k.h).  A
// signature is one lane in k_nymsign_pre and k_nymsign_fin and NYMSIGN_PARTS
// lanes in k_nymsign_part (part-major, so a wave runs one base and one range
// of windows): a pass is at most 4,096 signatures, 64 waves on 1,024 SIMDs
// with one lane each.
#include "nymsign_k.h"

__global__ void __launch_bounds__(64) k_nymsign_pre(const NymSignJob* jobs, uint32_t n, const uint8_t* blob,
                                                    const uint32_t (*keys)[8], uint32_t (*r_sk)[8],
                                                    uint32_t (*r_rnym)[8], uint32_t (*nonce)[8]) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const NymSignJob j = jobs[i];
  uint32_t dg[8], sk[8], rn[8], ent[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t[8];
  nymsign_msg_digest(dg, blob + j.msg, j.msg_len);
#pragma unroll
  for (int w = 0; w < 8; w++) sk[w] = keys[j.signer][w];
  be32_to_limbs_g(rn, blob + j.rnym);
  if (j.entropy) {
    be32_to_limbs_g(t, blob + j.entropy);
    nymsign_words(ent, t);
  }
  uint32_t a[8], b[8], c[8];
  nymsign_randomness(a, b, c, sk, rn, dg, ent, j.entropy != 0);
#pragma unroll
  for (int w = 0; w < 8; w++) {
    r_sk[i][w] = a[w];
    r_rnym[i][w] = b[w];
    nonce[i][w] = c[w];
  }
}

__global__ void __launch_bounds__(64) k_nymsign_part(uint32_t n, const uint32_t (*s0)[8], const uint32_t (*s1)[8],
                                                     const QDev* tab, QJDev* part) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NYMSIGN_PARTS * n) return;
  const uint32_t p = i / n, s = i - p * n;
  const uint32_t base = p / NYMSIGN_SLICES, slice = p - base * NYMSIGN_SLICES;
  const uint32_t(*sc)[8] = base ? s1 : s0;
  uint32_t kk[8];
#pragma unroll
  for (int w = 0; w < 8; w++) kk[w] = sc[s][w];
  qj_store(part[i], q1_fixed_mul_uniform<fp>(tab + (size_t)base * NYM_TAB_PER_BASE, kk,
                                             (int)slice * NYMSIGN_PART_WINDOWS, NYMSIGN_PART_WINDOWS));
}

__global__ void __launch_bounds__(64) k_nymsign_fin(const NymSignJob* jobs, uint32_t n, uint8_t* blob,
                                                    const uint32_t (*keys)[8], const QJDev* part,
                                                    uint32_t (*r_sk)[8], uint32_t (*r_rnym)[8], uint32_t (*nonce)[8],
                                                    uint8_t* out, uint8_t* ok) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const NymSignJob j = jobs[i];
  uint32_t sk[8], a[8], b[8], c[8];
#pragma unroll
  for (int w = 0; w < 8; w++) {
    sk[w] = keys[j.signer][w];
    a[w] = r_sk[i][w];
    b[w] = r_rnym[i][w];
    c[w] = nonce[i][w];
  }
  job_nymsign_fin(j, blob, nymsign_sum_parts(part, n, i), sk, a, b, c, out + (size_t)i * NYMSIGN_RAW_BYTES);
  ok[i] = 1;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    r_sk[i][w] = 0;
    r_rnym[i][w] = 0;
    nonce[i][w] = 0;
  }
}

__global__ void __launch_bounds__(64) k_nym_make_pre(uint32_t n, const uint32_t (*keys)[8], int32_t signer,
                                                     const uint8_t* r_nyms, uint32_t (*s0)[8], uint32_t (*s1)[8]) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t rn[8];
  be32_to_limbs_g(rn, r_nyms + (size_t)i * 32);
#pragma unroll
  for (int w = 0; w < 8; w++) {
    s0[i][w] = keys[signer][w];
    s1[i][w] = rn[w];
  }
}

__global__ void __launch_bounds__(64) k_nym_make_fin(uint32_t n, const QJDev* part, uint32_t (*s0)[8],
                                                     uint32_t (*s1)[8], uint8_t* nyms) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1_to_bytes_g(nyms + (size_t)i * 64, nymsign_to_aff(nymsign_sum_parts(part, n, i)));
#pragma unroll
  for (int w = 0; w < 8; w++) {
    s0[i][w] = 0;
    s1[i][w] = 0;
  }
}
