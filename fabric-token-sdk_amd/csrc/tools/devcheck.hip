// TEST-ONLY device primitive conformance harness (tests/test_devcheck.py): each
// op of tools/devcheck_ops.h as its own kernel, one vector per lane, operands
// read from and results written to global memory so that nothing folds at
// compile time.  The host supplies the operands and gets the raw result words.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "devcheck_ops.h"

using namespace fts;

static constexpr uint32_t DC_SENTINEL = 0xA5A5A5A5u;

template <int OP, uint32_t NIN, uint32_t NOUT>
__global__ void __launch_bounds__(256) k_devcheck(uint32_t n, const uint32_t* in, uint32_t* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  dc_apply<OP>(in + (size_t)j * NIN, out + (size_t)j * NOUT);
}

template <int OP, uint32_t NIN, uint32_t NOUT>
__global__ void __launch_bounds__(256) k_devcheck_g1(uint32_t n, const uint32_t* in, uint32_t* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  dc_g1_apply<OP>(in + (size_t)j * NIN, out + (size_t)j * NOUT);
}

__global__ void __launch_bounds__(256) k_devcheck_sha(uint32_t n, const uint8_t* arena, const uint32_t* first,
                                                      const uint32_t* segs, uint32_t* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  dc_sha(arena, segs + 2 * (size_t)first[j], first[j + 1] - first[j], out + (size_t)j * 16);
}

// the table of ops: returns their number; for 0 <= op < that, the name (at
// most 31 characters) and the words read and written per vector
extern "C" int ftz_devcheck_info(int op, char name[32], uint32_t* nin, uint32_t* nout) {
  if (op >= 0 && op < DC_OP_COUNT) {
    const DcInfo& e = dc_table()[op];
    strncpy(name, e.name, 31);
    name[31] = 0;
    *nin = e.nin;
    *nout = e.nout;
  }
  return DC_OP_COUNT;
}

// Runs op on n vectors (in: n * nin words) in workgroups of `block` lanes (64
// or 256).  out holds nout words for every lane of every workgroup, the idle
// lanes of the last one included: it is filled with 0xA5A5A5A5 before the
// launch and copied back whole, so the caller can check that the lanes past n
// wrote nothing.  Returns 0, or -(HIP error code), or -1000 for bad arguments.
extern "C" int ftz_devcheck(int device, int op, uint32_t n, uint32_t block, const uint32_t* in, uint32_t* out) {
  if (op < 0 || op >= DC_OP_COUNT || n == 0 || (block != 64 && block != 256) || !in || !out) return -1000;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  const DcInfo& info = dc_table()[op];
  const uint32_t blocks = (n + block - 1) / block;
  const size_t in_bytes = (size_t)n * info.nin * 4, out_bytes = (size_t)blocks * block * info.nout * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  if ((e = hipMalloc(&din, in_bytes)) == hipSuccess && (e = hipMalloc(&dout, out_bytes)) == hipSuccess &&
      (e = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemset(dout, DC_SENTINEL & 0xFF, out_bytes)) == hipSuccess) {
    switch (op) {
#define DC_X(name, nin, nout)                                           \
  case DC_##name:                                                       \
    k_devcheck<DC_##name, nin, nout><<<blocks, block>>>(n, din, dout); \
    break;
      DC_OPS(DC_X)
#undef DC_X
    }
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
      e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return -(int)e;
}

// The G1 table (DC_G1_OPS), as ftz_devcheck_info / ftz_devcheck are for DC_OPS
extern "C" int ftz_devcheck_g1_info(int op, char name[32], uint32_t* nin, uint32_t* nout) {
  if (op >= 0 && op < DC_G1_OP_COUNT) {
    const DcInfo& e = dc_g1_table()[op];
    strncpy(name, e.name, 31);
    name[31] = 0;
    *nin = e.nin;
    *nout = e.nout;
  }
  return DC_G1_OP_COUNT;
}
extern "C" int ftz_devcheck_g1(int device, int op, uint32_t n, uint32_t block, const uint32_t* in, uint32_t* out) {
  if (op < 0 || op >= DC_G1_OP_COUNT || n == 0 || (block != 64 && block != 256) || !in || !out) return -1000;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  const DcInfo& info = dc_g1_table()[op];
  const uint32_t blocks = (n + block - 1) / block;
  const size_t in_bytes = (size_t)n * info.nin * 4, out_bytes = (size_t)blocks * block * info.nout * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  if ((e = hipMalloc(&din, in_bytes)) == hipSuccess && (e = hipMalloc(&dout, out_bytes)) == hipSuccess &&
      (e = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemset(dout, DC_SENTINEL & 0xFF, out_bytes)) == hipSuccess) {
    switch (op) {
#define DC_X(name, nin, nout)                                              \
  case DC_##name:                                                          \
    k_devcheck_g1<DC_##name, nin, nout><<<blocks, block>>>(n, din, dout); \
    break;
      DC_G1_OPS(DC_X)
#undef DC_X
    }
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
      e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return -(int)e;
}

// SHA-256 of n messages: message j is the segments first[j] .. first[j + 1] - 1
// of segs ((offset, length) pairs into the arena; the arena's device copy is
// 256-byte aligned, so an offset's alignment is the address's).  out: 16 words
// per lane of every workgroup (the digest bytes, then digest_mod_r), sentinel-
// filled and copied back whole as ftz_devcheck's.
extern "C" int ftz_devcheck_sha(int device, uint32_t n, uint32_t block, const uint8_t* arena, uint32_t arena_len,
                                const uint32_t* first, const uint32_t* segs, uint32_t* out) {
  if (n == 0 || (block != 64 && block != 256) || !arena || !first || !segs || !out) return -1000;
  const uint32_t nseg = first[n];
  for (uint32_t k = 0; k < nseg; k++)
    if ((uint64_t)segs[2 * k] + segs[2 * k + 1] > arena_len) return -1000;
  for (uint32_t j = 0; j < n; j++)
    if (first[j] > first[j + 1]) return -1000;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  const uint32_t blocks = (n + block - 1) / block;
  const size_t out_bytes = (size_t)blocks * block * 16 * 4;
  uint8_t* da = nullptr;
  uint32_t *df = nullptr, *ds = nullptr, *dout = nullptr;
  if ((e = hipMalloc(&da, arena_len + 16)) == hipSuccess && (e = hipMalloc(&df, (size_t)(n + 1) * 4)) == hipSuccess &&
      (e = hipMalloc(&ds, (size_t)(nseg + 1) * 8)) == hipSuccess && (e = hipMalloc(&dout, out_bytes)) == hipSuccess &&
      (e = hipMemcpy(da, arena, arena_len, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(df, first, (size_t)(n + 1) * 4, hipMemcpyHostToDevice)) == hipSuccess &&
      (nseg == 0 || (e = hipMemcpy(ds, segs, (size_t)nseg * 8, hipMemcpyHostToDevice)) == hipSuccess) &&
      (e = hipMemset(dout, DC_SENTINEL & 0xFF, out_bytes)) == hipSuccess) {
    k_devcheck_sha<<<blocks, block>>>(n, da, df, ds, dout);
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
      e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(da);
  (void)hipFree(df);
  (void)hipFree(ds);
  (void)hipFree(dout);
  return -(int)e;
}
