// ECDSA P-256 verification kernels (dev/p256.h, ecdsa_k.h).  A signature is
// one lane in k_ecdsa_pre and k_ecdsa_fin and two lanes in k_ecdsa_part
// (part-major: lanes [0, n) run u1 G, lanes [n, 2n) run u2 Q, so a wave runs
// one kind of part): batches are a few thousand signatures on 1,024 SIMDs.
#include "ecdsa_k.h"

__global__ void __launch_bounds__(64) k_ecdsa_pre(const EcdsaJob* jobs, uint32_t n, const uint8_t* blob,
                                                  uint32_t (*u)[8], uint8_t* ok) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const EcdsaJob j = jobs[i];
  uint32_t r[8], s[8], u1[8], u2[8];
  be32_to_limbs_g(r, blob + j.sc);
  be32_to_limbs_g(s, blob + j.sc + 32);
  bool in_range = ecdsa_rs_in_range(r, s);
  ok[i] = in_range ? 1 : 0;
  if (!in_range) {  // the host filters these; the later kernels still find defined scalars
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = r[k] = (k == 0);
  }
  Sha256 h;
  h.init();
  h.update(blob + j.msg, j.msg_len);
  uint8_t d[32];
  h.final(d);
  ecdsa_scalars(d, r, s, u1, u2);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    u[i][k] = u1[k];
    u[n + i][k] = u2[k];
  }
}

__global__ void __launch_bounds__(64) k_ecdsa_part(const EcdsaJob* jobs, uint32_t n, uint32_t n_reg,
                                                   const uint8_t* blob, const uint32_t (*u)[8],
                                                   const P256Aff* tabs, uint32_t* vt, P256Jac* part) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n) return;
  uint32_t k[8];
#pragma unroll
  for (int w = 0; w < 8; w++) k[w] = u[i][w];
  if (i < n) {
    p256_store(part[i], p256_fixed_mul(tabs, k));
    return;
  }
  const EcdsaJob j = jobs[i - n];
  if (j.key >= 0) {
    p256_store(part[i], p256_fixed_mul(tabs + (size_t)j.key * P256_TAB_ENTRIES, k));
    return;
  }
  if (i - n < n_reg) {  // outside the ad-hoc range (the host sorts the jobs, so never): it has no table slot
    p256_store(part[i], p256_inf());
    return;
  }
  uint32_t qx[8], qy[8];
  be32_to_limbs_g(qx, blob + j.sc + 64);
  be32_to_limbs_g(qy, blob + j.sc + 96);
  // ad-hoc jobs follow the registered ones: lane (i - n) - n_reg of n - n_reg
  p256_store(part[i], p256_var_mul(pf_from_int(qx), pf_from_int(qy), k, vt, n - n_reg, i - n - n_reg));
}

__global__ void __launch_bounds__(64) k_ecdsa_fin(const EcdsaJob* jobs, uint32_t n, const uint8_t* blob,
                                                  const P256Jac* part, uint8_t* ok) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t r[8];
  be32_to_limbs_g(r, blob + jobs[i].sc);
  bool acc = ecdsa_accept(p256_load(part[i]), p256_load(part[n + i]), r);
  ok[i] = (ok[i] && acc) ? 1 : 0;
}
