// TEST-ONLY device primitive conformance harness (tests/test_devcheck.py): each
// op of tools/devcheck_ops.h as its own kernel, one vector per lane, operands
// read from and results written to global memory so that nothing folds at
// compile time.  The host supplies the operands and gets the raw result words.
// Further sections, each with entry points of its own:
//   DC_G1_OPS / DC_G2_OPS   the fused G1 and G2 formulas (ftz_devcheck_g1, _g2)
//   ftz_devcheck_g1_chain, _g1_jobs, _g2_jobs   the G1 and G2 stages as launched
//   DC_SX_OPS (dev/devcheck_sx.h)   the sextet pairing routines of dev/sx29.h,
//       six lanes per job in the production prologue: ftz_devcheck_sx_info,
//       ftz_devcheck_sx (tests/test_gpu_sx_ops.py)
// The pairing stage itself (k_qlines, k_miller*, launch_fexp on described jobs)
// is tools/devpair.hip, a shared object of its own.
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

// ---- the variable-base G1 chain as the verifier runs it (tests/test_gpu_g1_chain.py):
// k_g1_part and k_g1_combine themselves (k_g1.hip compiled into this tool) over
// a job array the caller describes, and the window loop on chosen GLV halves
// (g1_mul_glv16_halves: glv_split's own halves never reach the top window), both
// with the per-batch window table laid out [entry][job] as the runtime's.  Each
// returns the device's affine points and the host build's of the same code.
#include "../k_g1.hip"

static void dc_aff_words(uint32_t* out, const g1j& p) {
  G1Dev d;
  g1_store(d, jac_to_aff(p));
  memcpy(out, &d, sizeof(d));
}

static constexpr uint32_t DC_CHAIN_IN = 34;  // X[8] Y[8] Z[8] (Montgomery words), k1[4], n1, k2[4], n2
struct DcChainIn {
  g1a p;
  fp z;
  uint32_t k1[4], k2[4];
  bool n1, n2;
};
FTS_HD DcChainIn dc_chain_ld(const uint32_t* q) {
  DcChainIn c;
  c.p = {dc_ld8<fp>(q), dc_ld8<fp>(q + 8), false};
  c.z = dc_ld8<fp>(q + 16);
  for (int i = 0; i < 4; i++) {
    c.k1[i] = q[24 + i];
    c.k2[i] = q[29 + i];
  }
  c.n1 = q[28] != 0;
  c.n2 = q[33] != 0;
  return c;
}
__global__ void __launch_bounds__(128) k_devcheck_g1_chain(uint32_t n, const uint32_t* in, uint32_t* out,
                                                           G1Tab29* vtab) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const DcChainIn c = dc_chain_ld(in + (size_t)j * DC_CHAIN_IN);
  dc_stj(out + (size_t)j * 24, g1_mul_glv16_halves(c.p, c.z, c.k1, c.n1, c.k2, c.n2, vtab + j, n));
}

// n vectors of DC_CHAIN_IN words, one lane each in workgroups of 128 (k_g1_part's).
// out: n x 32 words, the device's affine point (x[8] y[8], all-zero: infinity)
// then the host's.
extern "C" int ftz_devcheck_g1_chain(int device, uint32_t n, const uint32_t* in, uint32_t* out) {
  if (n == 0 || n > 65536 || !in || !out) return -1000;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  const size_t in_bytes = (size_t)n * DC_CHAIN_IN * 4, res_bytes = (size_t)n * 24 * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  G1Tab29* dtab = nullptr;
  uint32_t* res = new uint32_t[(size_t)n * 24];
  if ((e = hipMalloc(&din, in_bytes)) == hipSuccess && (e = hipMalloc(&dout, res_bytes)) == hipSuccess &&
      (e = hipMalloc(&dtab, sizeof(G1Tab29) * G1VTAB_ENTRIES * n)) == hipSuccess &&
      (e = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemset(dout, 0, res_bytes)) == hipSuccess) {
    k_devcheck_g1_chain<<<(n + 127) / 128, 128>>>(n, din, dout, dtab);
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
      e = hipMemcpy(res, dout, res_bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dtab);
  if (e == hipSuccess)
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t* r = res + (size_t)j * 24;
      dc_aff_words(out + (size_t)j * 32, g1j{dc_ld8<fp>(r), dc_ld8<fp>(r + 8), dc_ld8<fp>(r + 16)});
      const DcChainIn c = dc_chain_ld(in + (size_t)j * DC_CHAIN_IN);
      G1Tab29 loc[G1VTAB_ENTRIES];
      dc_aff_words(out + (size_t)j * 32 + 16, g1_mul_glv16_halves(c.p, c.z, c.k1, c.n1, c.k2, c.n2, loc, 1));
    }
  delete[] res;
  return -(int)e;
}

// n G1 jobs without fixed-base terms through k_g1_part + k_g1_combine.
//   jobs:   n x 6 words: vstart, vcount, vscal (0xFFFFFFFF: no variable part), vneg, sh_first, sh_count
//   vterms: n_vt x 4 words (VTerm);  pts: n_pts x 16 words (G1Dev);  scal: n_scal x 8 words (< r)
// Every index is checked against its array before anything runs (-1000).
// out: n x 32 words, the device's g1out entry of job j then job_g1's on the host.
extern "C" int ftz_devcheck_g1_jobs(int device, uint32_t n, const uint32_t* jobs, uint32_t n_vt, const uint32_t* vterms,
                                    uint32_t n_pts, const uint32_t* pts, uint32_t n_scal, const uint32_t* scal,
                                    uint32_t* out) {
  if (n == 0 || n > 65536 || n_vt > 65536 || n_pts > 65536 || n_scal > 65536 || !jobs || !vterms || !pts || !scal || !out)
    return -1000;
  G1Job* hj = new G1Job[n];
  uint32_t* vlist = new uint32_t[n];
  uint32_t nvl = 0;
  bool ok = true;
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t* q = jobs + (size_t)j * 6;
    G1Job g{};
    g.vstart = q[0];
    g.vcount = q[1];
    g.vscal = q[2];
    g.vneg = q[3] ? 1u : 0u;
    g.sh_first = q[4];
    g.sh_count = q[5];
    g.out = j;
    g.bytes = g.b64 = NONE;
    if (g.vscal != NONE) {
      ok = ok && g.vscal < n_scal && g.vcount >= 1 && g.vstart <= n_vt && g.vcount <= n_vt - g.vstart;
      if (g.sh_count) {  // earlier jobs that run their own chain
        ok = ok && g.sh_first <= j && g.sh_count <= j - g.sh_first;
        for (uint32_t s = 0; ok && s < g.sh_count; s++)
          ok = hj[g.sh_first + s].vscal != NONE && hj[g.sh_first + s].sh_count == 0;
      } else {
        vlist[nvl++] = 3 * n + j;
      }
    } else {
      ok = ok && g.sh_count == 0;
    }
    hj[j] = g;
  }
  for (uint32_t t = 0; t < n_vt; t++) ok = ok && vterms[4 * (size_t)t] < n_pts;
  hipError_t e = hipSuccess;
  if (ok) e = hipSetDevice(device);
  G1Job* dj = nullptr;
  uint32_t *dvl = nullptr, *dvt = nullptr, *dpts = nullptr, *dscal = nullptr;
  G1JDev* dpart = nullptr;
  G1Tab29* dtab = nullptr;
  G1Dev *dg1 = nullptr, *dpn = nullptr;
  G1Dev* res = new G1Dev[n];
  if (ok && e == hipSuccess && (e = hipMalloc(&dj, sizeof(G1Job) * n)) == hipSuccess &&
      (e = hipMalloc(&dvl, 4 * (size_t)n)) == hipSuccess && (e = hipMalloc(&dvt, 16 * (size_t)(n_vt + 1))) == hipSuccess &&
      (e = hipMalloc(&dpts, 64 * (size_t)(n_pts + 1))) == hipSuccess &&
      (e = hipMalloc(&dscal, 32 * (size_t)(n_scal + 1))) == hipSuccess &&
      (e = hipMalloc(&dpart, sizeof(G1JDev) * 4 * n)) == hipSuccess &&
      (e = hipMalloc(&dtab, sizeof(G1Tab29) * G1VTAB_ENTRIES * n)) == hipSuccess &&
      (e = hipMalloc(&dg1, sizeof(G1Dev) * n)) == hipSuccess && (e = hipMalloc(&dpn, sizeof(G1Dev) * n)) == hipSuccess &&
      (e = hipMemcpy(dj, hj, sizeof(G1Job) * n, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dvl, vlist, 4 * (size_t)n, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dvt, vterms, 16 * (size_t)n_vt, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dpts, pts, 64 * (size_t)n_pts, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dscal, scal, 32 * (size_t)n_scal, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemset(dpart, 0, sizeof(G1JDev) * 4 * n)) == hipSuccess &&
      (e = hipMemset(dg1, 0xA5, sizeof(G1Dev) * n)) == hipSuccess) {
    if (const uint32_t lanes = g1_part_lanes(0, nvl))
      k_g1_part<<<(lanes + 127) / 128, 128>>>(dj, n, nullptr, 0, dvl, nvl, reinterpret_cast<const VTerm*>(dvt),
                                             reinterpret_cast<const G1Dev*>(dpts),
                                             reinterpret_cast<const uint32_t(*)[8]>(dscal), nullptr, dpart, dtab);
    k_g1_combine<<<(n + COMBINE_NT - 1) / COMBINE_NT, COMBINE_NT>>>(dj, n, dpart, dg1, nullptr, dpn);
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
      e = hipMemcpy(res, dg1, sizeof(G1Dev) * n, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dj);
  (void)hipFree(dvl);
  (void)hipFree(dvt);
  (void)hipFree(dpts);
  (void)hipFree(dscal);
  (void)hipFree(dpart);
  (void)hipFree(dtab);
  (void)hipFree(dg1);
  (void)hipFree(dpn);
  if (ok && e == hipSuccess) {
    G1Dev* host = new G1Dev[n];
    for (uint32_t j = 0; j < n; j++)
      job_g1(hj[j], reinterpret_cast<const VTerm*>(vterms), reinterpret_cast<const G1Dev*>(pts),
             reinterpret_cast<const uint32_t(*)[8]>(scal), nullptr, host, nullptr);
    for (uint32_t j = 0; j < n; j++) {
      memcpy(out + (size_t)j * 32, &res[j], 64);
      memcpy(out + (size_t)j * 32 + 16, &host[j], 64);
    }
    delete[] host;
  }
  delete[] res;
  delete[] vlist;
  delete[] hj;
  return ok ? -(int)e : -1000;
}

// ---- the G2 table (DC_G2_OPS), as ftz_devcheck_g1_info / ftz_devcheck_g1 are for DC_G1_OPS
template <int OP, uint32_t NIN, uint32_t NOUT>
__global__ void __launch_bounds__(256) k_devcheck_g2(uint32_t n, const uint32_t* in, uint32_t* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  dc_g2_apply<OP>(in + (size_t)j * NIN, out + (size_t)j * NOUT);
}
extern "C" int ftz_devcheck_g2_info(int op, char name[32], uint32_t* nin, uint32_t* nout) {
  if (op >= 0 && op < DC_G2_OP_COUNT) {
    const DcInfo& e = dc_g2_table()[op];
    strncpy(name, e.name, 31);
    name[31] = 0;
    *nin = e.nin;
    *nout = e.nout;
  }
  return DC_G2_OP_COUNT;
}
extern "C" int ftz_devcheck_g2(int device, int op, uint32_t n, uint32_t block, const uint32_t* in, uint32_t* out) {
  if (op < 0 || op >= DC_G2_OP_COUNT || n == 0 || (block != 64 && block != 256) || !in || !out) return -1000;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  const DcInfo& info = dc_g2_table()[op];
  const uint32_t blocks = (n + block - 1) / block;
  const size_t in_bytes = (size_t)n * info.nin * 4, out_bytes = (size_t)blocks * block * info.nout * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  if ((e = hipMalloc(&din, in_bytes)) == hipSuccess && (e = hipMalloc(&dout, out_bytes)) == hipSuccess &&
      (e = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemset(dout, DC_SENTINEL & 0xFF, out_bytes)) == hipSuccess) {
    switch (op) {
#define DC_X(name, nin, nout)                                              \
  case DC_##name:                                                          \
    k_devcheck_g2<DC_##name, nin, nout><<<blocks, block>>>(n, din, dout); \
    break;
      DC_G2_OPS(DC_X)
#undef DC_X
    }
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
      e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return -(int)e;
}

// ---- the G2 stage as the verifier runs it (tests/test_gpu_g2_fused.py): k_tab_g2
// for the window table of the four bases, then k_g2_part, k_g2_sum, k_g2_binv
// and k_g2lines1 themselves (k_g2.hip compiled into this tool) with the
// runtime's launch shapes, over n membership jobs the caller describes.
//   jobs:  n x 5 words: nfix (1..3), the scalar index of each of the three
//          fixed terms (term f is base f; unused ones ignored), the pts index of R
//   bases: 4 x 32 words (G2Dev);  scal: n_scal x 8 words (< r);  pts: n_pts x 16
//          words (G1Dev, all-zero: infinity)
// Every index is checked before anything runs (-1000).
//   g2out: n x 64 words, the device's t' (G2Dev, all-zero: infinity) then the
//          host's from the 32-bit code (job_g2_part, job_g2lines_parts)
//   lines_dev, lines_host: 88 x 6 x n x 10 words each (EvLineDev planes,
//          evl_off): the device's evaluated lines and the 32-bit host chain's
#include "../k_g2.hip"

extern "C" int ftz_devcheck_g2_jobs(int device, uint32_t n, const uint32_t* jobs, const uint32_t* bases, uint32_t n_scal,
                                    const uint32_t* scal, uint32_t n_pts, const uint32_t* pts, uint32_t* g2out,
                                    int32_t* lines_dev, int32_t* lines_host) {
  if (n == 0 || n > 4096 || n_scal == 0 || n_scal > 65536 || n_pts == 0 || n_pts > 65536 || !jobs || !bases || !scal ||
      !pts || !g2out || !lines_dev || !lines_host)
    return -1000;
  G2Job* hj = new G2Job[n];
  PairJob* hp = new PairJob[n];
  bool ok = true;
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t* q = jobs + (size_t)j * 5;
    G2Job g{};
    ok = ok && q[0] >= 1 && q[0] <= 3 && q[4] < n_pts;
    g.nfix = (uint8_t)q[0];
    for (int f = 0; f < 3; f++) {
      g.fbase[f] = (uint8_t)f;
      g.fscal[f] = f < (int)q[0] ? q[1 + f] : 0;
      ok = ok && g.fscal[f] < n_scal;
    }
    g.out = j;
    hj[j] = g;
    hp[j] = PairJob{0, q[4], j, 0, NONE};
  }
  const uint32_t t2 = G2B_COUNT * G2TAB_WINDOWS * G2TAB_DIGITS;
  const size_t line_words = (size_t)MILLER_LINES * 6 * n * EVL_REC;
  hipError_t e = hipSuccess;
  if (ok) e = hipSetDevice(device);
  G2Job* dj = nullptr;
  PairJob* dp = nullptr;
  uint32_t *dscal = nullptr, *dpts = nullptr;
  G2Dev *dbases = nullptr, *dtab = nullptr, *dout = nullptr;
  G2PartDev* dpart = nullptr;
  EvLineDev* dlines = nullptr;
  G2Dev* htab = new G2Dev[t2];
  G2Dev* res = new G2Dev[n];
  if (ok && e == hipSuccess && (e = hipMalloc(&dj, sizeof(G2Job) * n)) == hipSuccess &&
      (e = hipMalloc(&dp, sizeof(PairJob) * n)) == hipSuccess && (e = hipMalloc(&dscal, 32 * (size_t)n_scal)) == hipSuccess &&
      (e = hipMalloc(&dpts, 64 * (size_t)n_pts)) == hipSuccess && (e = hipMalloc(&dbases, sizeof(G2Dev) * G2B_COUNT)) == hipSuccess &&
      (e = hipMalloc(&dtab, sizeof(G2Dev) * (size_t)t2)) == hipSuccess && (e = hipMalloc(&dout, sizeof(G2Dev) * n)) == hipSuccess &&
      (e = hipMalloc(&dpart, sizeof(G2PartDev) * 4 * (size_t)n)) == hipSuccess &&
      (e = hipMalloc(&dlines, line_words * 4)) == hipSuccess &&
      (e = hipMemcpy(dj, hj, sizeof(G2Job) * n, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dp, hp, sizeof(PairJob) * n, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dscal, scal, 32 * (size_t)n_scal, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dpts, pts, 64 * (size_t)n_pts, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemcpy(dbases, bases, sizeof(G2Dev) * G2B_COUNT, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemset(dout, 0xA5, sizeof(G2Dev) * n)) == hipSuccess &&
      (e = hipMemset(dlines, 0xA5, line_words * 4)) == hipSuccess) {
    const uint32_t(*sc)[8] = reinterpret_cast<const uint32_t(*)[8]>(dscal);
    k_tab_g2<<<(t2 + 63) / 64, 64>>>(dbases, t2, dtab);
    k_g2_part<<<(4 * n + 63) / 64, 64>>>(dj, n, sc, dtab, dpart);
    k_g2_sum<<<(n + 63) / 64, 64>>>(n, dpart);
    k_g2_binv<<<(n + 255) / 256, 256>>>(n, dpart);
    k_g2lines1<<<(n + 63) / 64, 64>>>(dj, dp, n, dpart, dout, reinterpret_cast<const G1Dev*>(dpts), dlines);
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess &&
        (e = hipMemcpy(res, dout, sizeof(G2Dev) * n, hipMemcpyDeviceToHost)) == hipSuccess &&
        (e = hipMemcpy(lines_dev, dlines, line_words * 4, hipMemcpyDeviceToHost)) == hipSuccess)
      e = hipMemcpy(htab, dtab, sizeof(G2Dev) * (size_t)t2, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dj);
  (void)hipFree(dp);
  (void)hipFree(dscal);
  (void)hipFree(dpts);
  (void)hipFree(dbases);
  (void)hipFree(dtab);
  (void)hipFree(dout);
  (void)hipFree(dpart);
  (void)hipFree(dlines);
  if (ok && e == hipSuccess) {
    // the host's 32-bit code on the device's table (its entries are the
    // runtime's own k_tab_g2 points; t' does not depend on their form)
    const uint32_t(*sc)[8] = reinterpret_cast<const uint32_t(*)[8]>(scal);
    G2PartDev* part = new G2PartDev[4 * (size_t)n];
    G2Dev* host = new G2Dev[n];
    for (uint32_t j = 0; j < n; j++)
      for (int q = 0; q < 4; q++) job_g2_part(hj[j], q, sc, htab, part[(size_t)q * n + j]);
    for (uint32_t j = 0; j < n; j++)
      job_g2lines_parts(hj[j], hp[j], part, host, reinterpret_cast<const G1Dev*>(pts),
                        reinterpret_cast<EvLineDev*>(lines_host), j, n);
    for (uint32_t j = 0; j < n; j++) {
      memcpy(g2out + (size_t)j * 64, &res[j], 128);
      memcpy(g2out + (size_t)j * 64 + 32, &host[j], 128);
    }
    delete[] host;
    delete[] part;
  }
  delete[] res;
  delete[] htab;
  delete[] hp;
  delete[] hj;
  return ok ? -(int)e : -1000;
}

// ---- the sextet table (DC_SX_OPS of dev/devcheck_sx.h, tests/test_gpu_sx_ops.py):
// one kernel per op, launched as the runtime launches its sextet kernels -- 64
// lanes per workgroup, (n + 9) / 10 workgroups, the prologue of launch.h with
// the op's slot count and second-operand offset -- so the lane-to-sextet map,
// the ghost lanes 60..63, the LDS region stride and SyncWave are the production
// ones.  A lane of a sextet past n runs the last job's program in its own
// region (as in production) and stores nothing.
#include "../dev/devcheck_sx.h"

template <int OP, int NIN, int NS, int BOFS, int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_devcheck_sx(uint32_t n, const uint32_t* in, uint32_t* out,
                                                          int32_t* park) {
  SQ_KERNEL_PROLOGUE_B(n, NS, BOFS)
  const Park pk{park, blockIdx.x * 64 + threadIdx.x, gridDim.x * 64, !ghost_};
  const q2 r = dc_sx_apply<OP>(x, in + (size_t)jc * NIN, pk);
  if (valid) dc_sx_stq(out + ((size_t)job_ * 6 + x.k) * 18, r);
}

// the table: returns the number of ops; for 0 <= op < that, the name, the words
// read per job, the words written per job (108) and the LDS layout
extern "C" int ftz_devcheck_sx_info(int op, char name[32], uint32_t* nin, uint32_t* nout, uint32_t* slots,
                                    uint32_t* bofs) {
  if (op >= 0 && op < DC_SX_OP_COUNT) {
    const DcSxInfo& e = dc_sx_table()[op];
    strncpy(name, e.name, 31);
    name[31] = 0;
    *nin = e.nin;
    *nout = DC_SX_OUT;
    *slots = e.slots;
    *bofs = e.bofs;
  }
  return DC_SX_OP_COUNT;
}

// Runs op on n jobs (in: n * nin words).  out holds 108 words for every sextet
// of every workgroup, the idle ones of the last workgroup included: filled with
// 0xA5A5A5A5 before the launch and copied back whole.  The park planes
// (fexp_park_bytes(n)) are scratch.  Returns 0, -(HIP error code) or -1000.
extern "C" int ftz_devcheck_sx(int device, int op, uint32_t n, const uint32_t* in, uint32_t* out) {
  if (op < 0 || op >= DC_SX_OP_COUNT || n == 0 || n > 65536 || !in || !out) return -1000;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  const DcSxInfo& info = dc_sx_table()[op];
  const uint32_t blocks = (n + SX_JOBS_PER_WAVE - 1) / SX_JOBS_PER_WAVE;
  const size_t in_bytes = (size_t)n * info.nin * 4, out_bytes = (size_t)blocks * SX_JOBS_PER_WAVE * DC_SX_OUT * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  int32_t* dpark = nullptr;
  if ((e = hipMalloc(&din, in_bytes)) == hipSuccess && (e = hipMalloc(&dout, out_bytes)) == hipSuccess &&
      (e = hipMalloc(&dpark, fexp_park_bytes(n))) == hipSuccess &&
      (e = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice)) == hipSuccess &&
      (e = hipMemset(dpark, DC_SENTINEL & 0xFF, fexp_park_bytes(n))) == hipSuccess &&
      (e = hipMemset(dout, DC_SENTINEL & 0xFF, out_bytes)) == hipSuccess) {
    switch (op) {
#define DC_X(name, nin, ns, bofs, waves)                                                          \
  case DC_##name:                                                                                 \
    k_devcheck_sx<DC_##name, nin, ns, bofs, waves><<<blocks, 64>>>(n, din, dout, dpark); \
    break;
      DC_SX_OPS(DC_X)
#undef DC_X
    }
    if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
      e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dpark);
  return -(int)e;
}
