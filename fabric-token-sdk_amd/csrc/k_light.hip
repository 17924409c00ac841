// Kernel translation unit (one per kernel family keeps hipcc builds parallel).
#include <hip/hip_runtime.h>

#include "dev/jobs.h"
#include "launch.h"

using namespace fts;

#define JOB_KERNEL_PROLOGUE(n)                          \
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; \
  if (i >= (n)) return;

__global__ void __launch_bounds__(256) k_decode(const DecodeJob* jobs, uint32_t n, const uint8_t* wire,
                                                G1Dev* pts, uint8_t* pt_ok, uint8_t* arena) {
  JOB_KERNEL_PROLOGUE(n);
  DecodeJob j = jobs[i];
  pt_ok[j.out] = job_decode(j, wire, pts, arena);
}

__global__ void __launch_bounds__(256) k_zr(const ZrJob* jobs, uint32_t n, const uint8_t* wire,
                                            uint32_t (*scal)[8], uint8_t* canon) {
  JOB_KERNEL_PROLOGUE(n);
  job_zr(jobs[i], wire, scal, canon);
}

__global__ void __launch_bounds__(256) k_scalar(const ScalJob* jobs, uint32_t n, uint32_t (*scal)[8],
                                                const uint32_t* list) {
  JOB_KERNEL_PROLOGUE(n);
  job_scalar(jobs[i], scal, list);
}

__global__ void __launch_bounds__(128) k_hash(const HashJob* jobs, uint32_t n, const Seg* segs,
                                              const uint8_t* arena, uint32_t (*scal)[8],
                                              const uint8_t* canon, uint8_t* ok) {
  JOB_KERNEL_PROLOGUE(n);
  ok[i] = job_hash(jobs[i], segs, arena, scal, canon);
}

__global__ void __launch_bounds__(256) k_verdict(const TxChecks* tx, uint32_t n, const Check* ck,
                                                 const uint8_t* pt_ok, const uint8_t* hash_ok, int32_t* codes,
                                                 uint32_t* bitmap) {
  JOB_KERNEL_PROLOGUE(n);
  int32_t c = job_verdict(tx[i], ck, pt_ok, hash_ok);
  codes[i] = c;
  if (c == E_OK) atomicOr(&bitmap[i >> 5], 1u << (i & 31));
}

// the verdicts of a Pointcheval-Sanders pass (CK_GT: the unity bytes of k_fexp_hard_one)
__global__ void __launch_bounds__(256) k_verdict_gt(const TxChecks* tx, uint32_t n, const Check* ck,
                                                    const uint8_t* pt_ok, const uint8_t* gt_ok, int32_t* codes,
                                                    uint32_t* bitmap) {
  JOB_KERNEL_PROLOGUE(n);
  int32_t c = job_verdict_gt(tx[i], ck, pt_ok, gt_ok);
  codes[i] = c;
  if (c == E_OK) atomicOr(&bitmap[i >> 5], 1u << (i & 31));
}

// ---- prover
__global__ void __launch_bounds__(128) k_rand(const RandJob* jobs, uint32_t n, const uint8_t* arena,
                                              uint32_t (*scal)[8]) {
  JOB_KERNEL_PROLOGUE(n);
  job_rand(jobs[i], arena, scal);
}

__global__ void __launch_bounds__(256) k_emit(const EmitJob* jobs, uint32_t n, const uint32_t (*scal)[8],
                                              uint8_t* arena) {
  JOB_KERNEL_PROLOGUE(n);
  job_emit(jobs[i], scal, arena);
}

// one workgroup per copy job (the prover's device-initialised arena / output
// pools, dev/jobs.h CopyJob): lanes stride over its bytes
__global__ void __launch_bounds__(64) k_copy(const CopyJob* jobs, uint32_t n, const uint8_t* wire, uint8_t* arena,
                                             uint8_t* out) {
  if (blockIdx.x >= n) return;
  CopyJob j = jobs[blockIdx.x];
  for (uint32_t b = threadIdx.x; b < j.len; b += blockDim.x) job_copy_byte(j, b, wire, arena, out);
}

// one workgroup per inner document: threads stride over its 3-byte groups.
// level 0 runs the jobs without B64_L2 (inner documents into the outer proof;
// for the generating calls the outer proof stays in the arena and owners /
// issuer go into the action and metadata documents there), level 1 those with
// it (the outer proof into the action's Proof hole, the documents' finished
// pieces and the commitments into the output); a workgroup of the other level
// leaves at once.
__global__ void __launch_bounds__(256) k_b64(const B64Job* jobs, uint32_t n, uint8_t* arena, uint8_t* out,
                                             uint32_t level) {
  if (blockIdx.x >= n) return;
  B64Job j = jobs[blockIdx.x];
  if (((j.len & B64_L2) != 0) != (level != 0)) return;
  uint32_t units = job_b64_units(j);
  for (uint32_t u = threadIdx.x; u < units; u += blockDim.x) job_b64_unit(j, u, arena, out);
}

// context construction

__global__ void k_pp_decode(const uint8_t* raw, const uint32_t* g1off, uint32_t n1, const uint32_t* g2off,
                            uint32_t n2, G1Dev* g1, G2Dev* g2, uint8_t* g1bytes, uint8_t* g2bytes, uint8_t* ok) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n1) {
    DecodeJob j;
    j.raw = g1off[i];
    j.len = 64;
    j.out = i;
    j.bytes = NONE;
    j.b64 = NONE;
    ok[i] = job_decode(j, raw, g1, nullptr);
    g1a a = g1_load(g1[i]);
    g1_to_bytes(g1bytes + 64 * i, a);
  } else if (i < n1 + n2) {
    uint32_t k = i - n1;
    ok[i] = decode_g2(raw + g2off[k], 128, g2[k], g2bytes + 128 * k);
  }
}
