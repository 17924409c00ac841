// TEST-ONLY: the pairing stage as the runtime launches it, over jobs the caller
// describes (tests/test_gpu_pair_stage.py).  k_g2.hip, k_miller.hip and
// k_fexp.hip are compiled into this tool, so the kernels, their launch shapes
// and launch_fexp are the production ones.  A shared object of its own beside
// libftsdevcheck.so: the two pairing translation units are the slowest to
// compile, and build.py builds the tools side by side.
//
//   ftz_devcheck_pair_jobs   k_qlines for the fixed Q; the G2 stage (k_tab_g2,
//       k_g2_part, k_g2_sum, k_g2_binv, k_g2lines1) for t' and the evaluated
//       pair-2 lines; the host's g1_pnorm of every P1, uploaded; then k_miller
//       or k_miller_n -- chosen by the caller, not by whether Q's lines can be
//       normalised -- and launch_fexp, exact or Fuentes-Castaneda, writing GT
//       bytes or the unity byte.
//   ftz_devcheck_pair3_jobs  the same for the prover's k_miller_f3 with three
//       fixed G2 arguments Q, PK1, PK2.
// Outputs.  Job j's 384 GT bytes lie at arena offset DP_GAP + j * DP_STRIDE; the
// arena has such a place for every sextet of every workgroup, is filled with
// 0xA5 and is returned whole, as is the unity array (one byte per sextet).
// *guard comes back as a bit mask of what changed that must not: 1 an F12Dev of
// a sextet past n, 2 a park plane entry of a ghost lane 60..63.  (The park
// entries of the idle sextets of the last workgroup are scratch: those lanes
// run the last job's program and park its values, as in production.)
// Returns 0, -(HIP error code), -1000 for bad arguments, -1001 when a fixed
// line with r0 = 0 rules out the normalised kernel that was asked for.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../k_g2.hip"
#include "../k_miller.hip"
#include "../k_fexp.hip"

static constexpr uint32_t DP_GAP = 64, DP_STRIDE = 384 + DP_GAP;

namespace {

// device buffers of one call: the first HIP error sticks and skips the rest
struct DpMem {
  std::vector<void*> all;
  hipError_t e = hipSuccess;
  // n elements: copied from src, or filled with the byte `fill` (0xA5: sentinel)
  template <class T>
  T* get(size_t n, const void* src, int fill = 0xA5) {
    T* p = nullptr;
    if (e != hipSuccess) return nullptr;
    const size_t bytes = sizeof(T) * (n ? n : 1);
    if ((e = hipMalloc(&p, bytes)) != hipSuccess) return nullptr;
    all.push_back(p);
    e = src ? hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice) : hipMemset(p, fill, bytes);
    return p;
  }
  ~DpMem() {
    for (void* p : all) (void)hipFree(p);
  }
};

// the host's normalised evaluation point of an affine P (g1_pnorm with Z = 1)
G1Dev dp_pnorm(const G1Dev& d) {
  G1Dev out;
  memset(&out, 0, sizeof(out));
  const g1a p = g1_load(d);
  if (!p.inf) g1_pnorm(g1j{p.x, p.y, fe_one<ModP>()}, fp_inv(p.y), out);
  return out;
}

struct DpOut {
  F12Dev* dfbuf;
  uint8_t *darena, *dok;
  int32_t* dpark;
  uint32_t slots;
};
DpOut dp_outputs(DpMem& m, uint32_t n) {
  const uint32_t slots = (n + SX_JOBS_PER_WAVE - 1) / SX_JOBS_PER_WAVE * SX_JOBS_PER_WAVE;
  DpOut o;
  o.slots = slots;
  o.dfbuf = m.get<F12Dev>(slots, nullptr);
  o.darena = m.get<uint8_t>(DP_GAP + (size_t)slots * DP_STRIDE, nullptr);
  o.dok = m.get<uint8_t>(slots, nullptr);
  o.dpark = m.get<int32_t>(fexp_park_bytes(n) / 4, nullptr);
  return o;
}
void dp_pair_jobs(std::vector<PairJob>& hp, uint32_t n) {
  for (uint32_t j = 0; j < n; j++) hp[j].bytes = DP_GAP + j * DP_STRIDE;
}
// the final exponentiation, then the outputs and the guards
hipError_t dp_finish(DpMem& m, const DpOut& o, const PairJob* dp, uint32_t n, int exact, int unity, uint8_t* arena_out,
                     uint8_t* unity_out, uint32_t* guard) {
  launch_fexp(exact != 0, dp, n, o.dfbuf, o.darena, o.dpark, 0, unity ? o.dok : nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) return e;
  std::vector<F12Dev> fb(o.slots);
  std::vector<int32_t> park(fexp_park_bytes(n) / 4);
  if ((e = hipMemcpy(arena_out, o.darena, DP_GAP + (size_t)o.slots * DP_STRIDE, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(unity_out, o.dok, o.slots, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(fb.data(), o.dfbuf, sizeof(F12Dev) * o.slots, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(park.data(), o.dpark, park.size() * 4, hipMemcpyDeviceToHost)) != hipSuccess)
    return e;
  uint32_t g = 0;
  for (uint32_t j = n; j < o.slots; j++)
    for (uint32_t w : fb[j].w) g |= w != 0xA5A5A5A5u ? 1u : 0u;
  const size_t lanes = (size_t)(o.slots / SX_JOBS_PER_WAVE) * 64;
  for (size_t i = 0; i < park.size(); i++)
    if (i % lanes % 64 >= 6 * SX_JOBS_PER_WAVE && (uint32_t)park[i] != 0xA5A5A5A5u) g |= 2u;
  *guard = g;
  return hipSuccess;
}

}  // namespace

//   miller: 0 k_miller (the unnormalised lines), 1 k_miller_n
//   exact:  1 the exact final exponentiation, 0 the Fuentes-Castaneda multiple
//   unity:  1 the unity kernels (one byte per job), 0 the GT bytes
//   q:      the fixed Q (G2Dev, 32 words);  p1: n x 16 words (G1Dev, all-zero: infinity)
//   jobs, bases, scal, pts: pair 2 as ftz_devcheck_g2_jobs takes it (n x 5
//           words: nfix, three scalar indices, the pts index of R; 4 bases)
//   arena_out: DP_GAP + slots x DP_STRIDE bytes, unity_out: slots bytes, for
//           slots = the job count rounded up to whole workgroups of ten
extern "C" int ftz_devcheck_pair_jobs(int device, uint32_t n, int miller, int exact, int unity, const uint32_t* q,
                                      const uint32_t* p1, const uint32_t* jobs, const uint32_t* bases, uint32_t n_scal,
                                      const uint32_t* scal, uint32_t n_pts, const uint32_t* pts, uint8_t* arena_out,
                                      uint8_t* unity_out, uint32_t* guard) {
  if (n == 0 || n > 4096 || n_scal == 0 || n_scal > 65536 || n_pts == 0 || n_pts > 65536 || !q || !p1 || !jobs ||
      !bases || !scal || !pts || !arena_out || !unity_out || !guard)
    return -1000;
  std::vector<G2Job> hj(n);
  std::vector<PairJob> hp(n);
  std::vector<G1Dev> pn(n);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t* w = jobs + (size_t)j * 5;
    if (w[0] < 1 || w[0] > 3 || w[4] >= n_pts) return -1000;
    G2Job g{};
    g.nfix = (uint8_t)w[0];
    for (int f = 0; f < 3; f++) {
      g.fbase[f] = (uint8_t)f;
      g.fscal[f] = f < (int)w[0] ? w[1 + f] : 0;
      if (g.fscal[f] >= n_scal) return -1000;
    }
    g.out = j;
    hj[j] = g;
    hp[j] = PairJob{j, w[4], j, 0, NONE};
    pn[j] = dp_pnorm(reinterpret_cast<const G1Dev*>(p1)[j]);
  }
  dp_pair_jobs(hp, n);
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  const uint32_t t2 = G2B_COUNT * G2TAB_WINDOWS * G2TAB_DIGITS;
  DpMem m;
  G2Job* dj = m.get<G2Job>(n, hj.data());
  PairJob* dp = m.get<PairJob>(n, hp.data());
  uint32_t* dscal = m.get<uint32_t>(8 * (size_t)n_scal, scal);
  G1Dev* dpts = m.get<G1Dev>(n_pts, pts);
  G1Dev* dg1 = m.get<G1Dev>(n, p1);
  G1Dev* dpn = m.get<G1Dev>(n, pn.data());
  G2Dev* dbases = m.get<G2Dev>(G2B_COUNT, bases);
  G2Dev* dq = m.get<G2Dev>(1, q);
  G2Dev* dtab = m.get<G2Dev>(t2, nullptr);
  G2Dev* dg2 = m.get<G2Dev>(n, nullptr);
  G2PartDev* dpart = m.get<G2PartDev>(4 * (size_t)n, nullptr);
  EvLineDev* dlines = m.get<EvLineDev>((size_t)MILLER_LINES * n, nullptr);
  LineCoef* dl = m.get<LineCoef>(MILLER_LINES, nullptr);
  LineCoef29* dl29 = m.get<LineCoef29>(MILLER_LINES, nullptr);
  LineCoef29* dl29n = m.get<LineCoef29>(MILLER_LINES, nullptr);
  int* dn = m.get<int>(2, nullptr, 0);
  const DpOut o = dp_outputs(m, n);
  if (m.e != hipSuccess) return -(int)m.e;
  const uint32_t(*sc)[8] = reinterpret_cast<const uint32_t(*)[8]>(dscal);
  k_qlines<<<1, 64>>>(dq, dl, dl29, dl29n, dn, dn + 1);
  int nl[2] = {0, 0};
  if ((e = hipGetLastError()) != hipSuccess || (e = hipMemcpy(nl, dn, 8, hipMemcpyDeviceToHost)) != hipSuccess)
    return -(int)e;
  if (nl[0] != MILLER_LINES) return -1000;
  if (miller && !nl[1]) return -1001;
  k_tab_g2<<<(t2 + 63) / 64, 64>>>(dbases, t2, dtab);
  k_g2_part<<<(4 * n + 63) / 64, 64>>>(dj, n, sc, dtab, dpart);
  k_g2_sum<<<(n + 63) / 64, 64>>>(n, dpart);
  k_g2_binv<<<(n + 255) / 256, 256>>>(n, dpart);
  k_g2lines1<<<(n + 63) / 64, 64>>>(dj, dp, n, dpart, dg2, dpts, dlines);
  const uint32_t nb = o.slots / SX_JOBS_PER_WAVE;
  if (miller)
    k_miller_n<<<nb, 64>>>(dp, n, dl29n, dlines, dg1, dpn, o.dfbuf);
  else
    k_miller<<<nb, 64>>>(dp, n, dl29, dlines, dg1, o.dfbuf);
  if ((e = hipGetLastError()) != hipSuccess) return -(int)e;
  return -(int)dp_finish(m, o, dp, n, exact, unity, arena_out, unity_out, guard);
}

// The prover's fixed-pair product f(C, Q) f(A, PK1) f(B, PK2) through k_miller_f3:
//   q3:   Q, PK1, PK2 (3 x 32 words);  pts3: n x 3 x 16 words, job j's C, A, B
// Outputs as ftz_devcheck_pair_jobs.  -1001 if a line of one of the three has r0 = 0.
extern "C" int ftz_devcheck_pair3_jobs(int device, uint32_t n, int exact, int unity, const uint32_t* q3,
                                       const uint32_t* pts3, uint8_t* arena_out, uint8_t* unity_out, uint32_t* guard) {
  if (n == 0 || n > 4096 || !q3 || !pts3 || !arena_out || !unity_out || !guard) return -1000;
  std::vector<PairJob> hp(n);
  std::vector<G1Dev> pn(3 * (size_t)n);
  for (uint32_t j = 0; j < n; j++) hp[j] = PairJob{3 * j, 3 * j + 1, NONE, 0, 3 * j + 2};
  for (size_t i = 0; i < pn.size(); i++) pn[i] = dp_pnorm(reinterpret_cast<const G1Dev*>(pts3)[i]);
  dp_pair_jobs(hp, n);
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return -(int)e;
  DpMem m;
  PairJob* dp = m.get<PairJob>(n, hp.data());
  G1Dev* dg1 = m.get<G1Dev>(3 * (size_t)n, pts3);
  G1Dev* dpn = m.get<G1Dev>(3 * (size_t)n, pn.data());
  G2Dev* dq = m.get<G2Dev>(3, q3);
  LineCoef* dl = m.get<LineCoef>(MILLER_LINES, nullptr);
  LineCoef29* dl29 = m.get<LineCoef29>(MILLER_LINES, nullptr);
  LineCoef29* dl29n = m.get<LineCoef29>(3 * (size_t)MILLER_LINES, nullptr);  // Q's, then PK1's, then PK2's
  int* dn = m.get<int>(6, nullptr, 0);
  const DpOut o = dp_outputs(m, n);
  if (m.e != hipSuccess) return -(int)m.e;
  for (int t = 0; t < 3; t++) k_qlines<<<1, 64>>>(dq + t, dl, dl29, dl29n + t * MILLER_LINES, dn + 2 * t, dn + 2 * t + 1);
  int nl[6] = {0, 0, 0, 0, 0, 0};
  if ((e = hipGetLastError()) != hipSuccess || (e = hipMemcpy(nl, dn, 24, hipMemcpyDeviceToHost)) != hipSuccess)
    return -(int)e;
  for (int t = 0; t < 3; t++) {
    if (nl[2 * t] != MILLER_LINES) return -1000;
    if (!nl[2 * t + 1]) return -1001;
  }
  k_miller_f3<<<o.slots / SX_JOBS_PER_WAVE, 64>>>(dp, n, dl29n, dl29n + MILLER_LINES, dg1, dpn, o.dfbuf);
  if ((e = hipGetLastError()) != hipSuccess) return -(int)e;
  return -(int)dp_finish(m, o, dp, n, exact, unity, arena_out, unity_out, guard);
}
