// The device side of host/sigpipe.h, shared by ecdsa_rt.hip and idemix_rt.hip:
// what every pipeline slot carries, how a pass begins and ends in it, the
// signer-key registry of the two signing handles and the pool loop.
//
// One rule for errors: a slot is marked in flight (sig_pass_begin) before the
// first call that enqueues on its stream, so its collector always waits for
// the stream (sig_pass_end) before the call returns or the staging blob is
// written again -- also when an enqueue failed half way.  Such a pass, or one
// whose stream reports an error, has no results; the signing collectors still
// wipe what it may have left behind.
#pragma once
#include "host/sigpipe.h"
#include "rt_internal.h"

// f(i) for i in [0, n) on the pool, 64 items per piece
template <class F>
void par_for(WorkPool* pool, size_t n, F f) {
  pool->run((n + 63) / 64, [&](size_t p) {
    for (size_t i = p * 64; i < n && i < (p + 1) * 64; i++) f(i);
  });
}

// What the slots of all four pipelines have in common; each adds its buffers.
struct SigSlot {
  hipStream_t st = nullptr;
  bool busy = false;          // a pass is, or may be, enqueued on st
  bool enqueued = false;      // ... and every call of it was: the submit sets it after its last enqueue
  std::vector<uint32_t> idx;  // call-relative indices of the pass's items
  hipError_t open() { return st ? hipSuccess : hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
  void close() {
    if (!st) return;
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    st = nullptr;
  }
};

// The pass over the call's items a + idx[0..m) (idx = nullptr: [a, a + m))
// begins: until sig_pass_end the stream may hold work that uses the slot's buffers.
inline void sig_pass_begin(SigSlot& q, size_t a, const uint32_t* idx, size_t m) {
  q.idx.resize(m);
  for (size_t k = 0; k < m; k++) q.idx[k] = (uint32_t)(a + (idx ? idx[k] : k));
  q.busy = true;
  q.enqueued = false;
}

// Wait for a busy slot's pass.  FTZ_SUCCESS: its results are in the slot's buffers.
inline int sig_pass_end(SigSlot& q) {
  q.busy = false;
  HC(hipStreamSynchronize(q.st));
  return q.enqueued ? FTZ_SUCCESS : FTZ_E_DEVICE;  // the failed enqueue has set the error text
}

// collect the verdicts (one byte per item of the pass in h_ok) of a verifying slot's pass
inline int sig_collect_verdicts(SigSlot& q, const uint8_t* h_ok, int32_t* codes) {
  if (!q.busy) return FTZ_SUCCESS;
  int rc = sig_pass_end(q);
  for (size_t k = 0; rc == FTZ_SUCCESS && k < q.idx.size(); k++)
    codes[q.idx[k]] = h_ok[k] ? FTZ_OK : FTZ_ERR_SIGNATURE;
  return rc;
}

// Private scalars of a signing handle's signers, on the device only: `max`
// keys of 8 limbs, allocated and zeroed with the first one.  The handle's
// mutex is held and none of its passes is in flight when these are called.
struct SignerKeys {
  DBuf<uint32_t> d;
  int32_t n = 0;
  const uint32_t (*keys() const)[8] { return reinterpret_cast<const uint32_t(*)[8]>(d.p); }
  hipError_t add(int device, size_t max, const uint32_t limbs[8], int32_t* signer) {
    hipError_t he = hipSetDevice(device);
    if (he == hipSuccess && !d.p) {
      he = d.alloc(max * 8);
      if (he == hipSuccess) he = hipMemset(d.p, 0, d.n * sizeof(uint32_t));
    }
    if (he == hipSuccess) he = hipMemcpy(d.p + (size_t)n * 8, limbs, 8 * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (he == hipSuccess) *signer = n++;
    return he;
  }
  void wipe() {
    if (d.p) (void)hipMemset(d.p, 0, d.n * sizeof(uint32_t));
  }
};
