// HMAC-SHA-256 (RFC 2104) with a 32-byte key, per lane, and the HMAC_DRBG of
// RFC 6979 section 3.2 on top of it (the deterministic ECDSA nonce of
// dev/ecsign.h).  Values are big-endian 32-bit words as SHA-256 sees them:
// word 0 holds the first four bytes.  Built on Sha256 (dev/sha256.h), which it
// leaves as it is.
//
// Two ways in: hmac256() streams bytes of any length through Sha256's block
// buffer (runtime-indexed, so it lives in scratch memory on the device: for
// public data).  The DRBG's messages have fixed layouts, and they hold the
// private key: Rfc6979 builds their blocks with constant indices only, so the
// key, K and V stay in registers.
#pragma once
#include "sha256.h"

namespace fts {

// the hash states after the ipad / opad block of a 32-byte key (8 words)
struct HmacKey {
  uint32_t ist[8], ost[8];
  FTS_HD void set(const uint32_t k[8]) {
    uint32_t blk[16];
    Sha256 h;
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = (i < 8 ? k[i] : 0u) ^ 0x36363636u;
    h.init();
    h.compress_words(blk);
#pragma unroll
    for (int i = 0; i < 8; i++) ist[i] = h.h[i];
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] ^= 0x36363636u ^ 0x5c5c5c5cu;
    h.init();
    h.compress_words(blk);
#pragma unroll
    for (int i = 0; i < 8; i++) ost[i] = h.h[i];
  }
  // the outer hash of an inner digest: digest || 0x80 || zeros || (64 + 32) * 8 bits
  FTS_HD void outer(uint32_t out[8], const uint32_t inner[8]) const {
    uint32_t blk[16];
    Sha256 h;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      blk[i] = inner[i];
      h.h[i] = ost[i];
    }
    blk[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; i++) blk[i] = 0;
    blk[15] = 768;
    h.compress_words(blk);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = h.h[i];
  }
  // HMAC of a message given as NB whole blocks that already hold the padding
  // and the length (which counts the 64 bytes of the ipad block)
  template <int NB>
  FTS_HD void mac_blocks(uint32_t out[8], const uint32_t* m) const {
    Sha256 h;
#pragma unroll
    for (int i = 0; i < 8; i++) h.h[i] = ist[i];
#pragma unroll
    for (int b = 0; b < NB; b++) h.compress_words(m + 16 * b);
    uint32_t inner[8];
#pragma unroll
    for (int i = 0; i < 8; i++) inner[i] = h.h[i];
    outer(out, inner);
  }
};

// HMAC_K(data) over plain bytes of any length
FTS_HD void hmac256(const uint32_t key[8], const uint8_t* data, uint32_t n, uint32_t out[8]) {
  HmacKey k;
  k.set(key);
  Sha256 h;
  h.init();
#pragma unroll
  for (int i = 0; i < 8; i++) h.h[i] = k.ist[i];
  h.total = 64;
  h.update(data, n);
  uint8_t dg[32];
  h.final(dg);
  uint32_t inner[8];
#pragma unroll
  for (int i = 0; i < 8; i++)
    inner[i] = ((uint32_t)dg[4 * i] << 24) | ((uint32_t)dg[4 * i + 1] << 16) | ((uint32_t)dg[4 * i + 2] << 8) |
               dg[4 * i + 3];
  k.outer(out, inner);
}

// The HMAC_DRBG of RFC 6979 3.2 for qlen = hlen = 256: T is one HMAC output, so
// every candidate is V itself.
//   init (steps b-g): V = 01.., K = 00..; twice, with tag 0x00 then 0x01:
//     K = HMAC_K(V || tag || x || z [|| extra]), V = HMAC_K(V)
//   where x = int2octets(private key), z = bits2octets(h1), and extra is the
//   additional data k' of section 3.6 (32 bytes) when given.
//   next (step h.2): V = HMAC_K(V), the candidate.
//   retry (step h.3, after a refused candidate): K = HMAC_K(V || 0x00), V = HMAC_K(V).
struct Rfc6979 {
  uint32_t K[8], V[8];

  // V = HMAC_K(V): one block, V || 0x80 || zeros || (64 + 32) * 8
  FTS_HD void step_v() {
    HmacKey hk;
    hk.set(K);
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = i < 8 ? V[i] : 0u;
    m[8] = 0x80000000u;
    m[15] = 768;
    hk.mac_blocks<1>(V, m);
  }
  // K = HMAC_K(V || tag || s[0 .. NS) words), V = HMAC_K(V).  The tag byte
  // shifts the words after it by 8 bits; 33 + 4 NS bytes, then 0x80, zeros and
  // the length fill NB blocks.
  template <int NS>
  FTS_HD void step_k(uint32_t tag, const uint32_t* s) {
    constexpr int BYTES = 33 + 4 * NS;
    constexpr int NB = (BYTES + 9 + 63) / 64;
    HmacKey hk;
    hk.set(K);
    uint32_t m[16 * NB];
#pragma unroll
    for (int i = 0; i < 16 * NB; i++) m[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = V[i];
    uint32_t carry = tag << 24;  // the byte waiting for the top of the next word
#pragma unroll
    for (int i = 0; i < NS; i++) {
      m[8 + i] = carry | (s[i] >> 8);
      carry = s[i] << 24;
    }
    m[8 + NS] = carry | 0x00800000u;
    m[16 * NB - 1] = (64 + BYTES) * 8;
    hk.mac_blocks<NB>(K, m);
    step_v();
  }
  // extra: read when has_extra (a flag, not a null pointer: a pointer that may be null keeps the
  // caller's array in scratch memory)
  FTS_HD void init(const uint32_t x[8], const uint32_t z[8], const uint32_t extra[8], bool has_extra) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      K[i] = 0;
      V[i] = 0x01010101u;
    }
    uint32_t s[24];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      s[i] = x[i];
      s[8 + i] = z[i];
      s[16 + i] = has_extra ? extra[i] : 0u;
    }
#pragma nounroll
    for (uint32_t tag = 0; tag < 2; tag++) {
      if (has_extra)
        step_k<24>(tag, s);
      else
        step_k<16>(tag, s);
    }
  }
  FTS_HD void next() { step_v(); }
  FTS_HD void retry() { step_k<0>(0, nullptr); }
};

}  // namespace fts
