// TEST-ONLY host build of the P-256 field / curve / ECDSA job code (dev/p256.h)
// and the x509 decoders (host/x509id.cpp), for tests/test_ecdsa.py.  Integers
// cross the boundary as 32 bytes big-endian.
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../fabric-token-sdk_amd/csrc/dev/p256.h"
#include "../../fabric-token-sdk_amd/csrc/host/x509id.h"

using namespace fts;

namespace {
pf pf_raw(const uint8_t* b) {
  pf x;
  be32_to_limbs(x.v, b);
  return x;
}
void pf_raw_out(uint8_t* o, const pf& x) { limbs_to_be32(o, x.v); }
pf pf_in(const uint8_t* b) {
  uint32_t t[8];
  be32_to_limbs(t, b);
  return pf_from_int(t);
}
void pf_out(uint8_t* o, const pf& x) {
  uint32_t t[8];
  pf_to_int(t, x);
  limbs_to_be32(o, t);
}
p256j jac_in(const uint8_t* b) {
  p256j p;
  p.x = pf_in(b);
  p.y = pf_in(b + 32);
  p.z = pf_in(b + 64);
  return p;
}
// affine X || Y; returns 1 for the point at infinity
int aff_out(uint8_t* o, const p256j& p) {
  if (p256_is_inf(p)) {
    memset(o, 0, 64);
    return 1;
  }
  pf zi = pf_inv(p.z);
  pf zi2 = pf_sqr(zi);
  pf_out(o, p.x * zi2);
  pf_out(o + 32, p.y * zi2 * zi);
  return 0;
}
const P256Aff* table_for(const uint8_t* xy) {
  static std::map<std::string, std::vector<P256Aff>> cache;
  uint8_t g[64];
  if (!xy) {
    pf_out(g, pf_const(P256_GX));
    pf_out(g + 32, pf_const(P256_GY));
    xy = g;
  }
  std::string key((const char*)xy, 64);
  auto f = cache.find(key);
  if (f == cache.end()) {
    std::vector<P256Aff> t(P256_TAB_ENTRIES);
    p256_build_table(pf_in(xy), pf_in(xy + 32), t.data());
    f = cache.emplace(key, std::move(t)).first;
  }
  return f->second.data();
}
}  // namespace

extern "C" {

// raw Montgomery-domain operations on values < p: 0 a b R^-1, 1 a^2 R^-1, 2 a + b, 3 a - b (mod p)
void ecdsa_emu_pf(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  pf x = pf_raw(a), y = pf_raw(b);
  pf_raw_out(out, op == 0 ? x * y : op == 1 ? pf_sqr(x) : op == 2 ? x + y : x - y);
}
// the conversions: 0 to Montgomery form, 1 back
void ecdsa_emu_pf_conv(int op, const uint8_t* a, uint8_t* out) {
  if (op == 0) {
    pf_raw_out(out, pf_in(a));
  } else {
    pf_out(out, pf_raw(a));
  }
}
// scalar field: 0 raw Montgomery product a b R^-1 mod n (a, b < n); 1 a^-1 mod n (canonical in and out);
// 2 a mod n for any 256-bit a (through the Montgomery form)
void ecdsa_emu_pn(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  uint32_t t[8];
  if (op == 0) {
    pn x, y;
    be32_to_limbs(x.v, a);
    be32_to_limbs(y.v, b);
    pn r = x * y;
    limbs_to_be32(out, r.v);
    return;
  }
  be32_to_limbs(t, a);
  pn x = pn_from_int(t);
  if (op == 1) x = pn_inv(x);
  pn_to_int(t, x);
  limbs_to_be32(out, t);
}
// points as Jacobian X || Y || Z (canonical integers): 0 2P, 1 P + (Qx, Qy) mixed, 2 P + Q complete
int ecdsa_emu_point(int op, const uint8_t* p, const uint8_t* q, uint8_t* out) {
  p256j a = jac_in(p);
  if (op == 0) return aff_out(out, p256_dbl(a));
  p256j b = jac_in(q);
  if (op == 1) return aff_out(out, p256_add_aff(a, b.x, b.y));
  return aff_out(out, p256_add(a, b));
}
int ecdsa_emu_on_curve(const uint8_t* xy) { return p256_on_curve(pf_in(xy), pf_in(xy + 32)) ? 1 : 0; }
int ecdsa_emu_xmatch(const uint8_t* X, const uint8_t* Z, const uint8_t* r) {
  uint32_t t[8];
  be32_to_limbs(t, r);
  return p256_x_matches(pf_in(X), pf_in(Z), t) ? 1 : 0;
}
// k B from the window table of B = xy (null: G)
int ecdsa_emu_fixed(const uint8_t* xy, const uint8_t* k, uint8_t* out) {
  uint32_t t[8];
  be32_to_limbs(t, k);
  return aff_out(out, p256_fixed_mul(table_for(xy), t));
}
// k Q by the windowed variable-base multiplication, as lane `lane` of `lanes`
int ecdsa_emu_var(const uint8_t* xy, const uint8_t* k, uint32_t lanes, uint32_t lane, uint8_t* out) {
  uint32_t t[8];
  be32_to_limbs(t, k);
  std::vector<uint32_t> vt((size_t)P256_VT_WORDS * lanes, 0xdeadbeefu);
  return aff_out(out, p256_var_mul(pf_in(xy), pf_in(xy + 32), t, vt.data(), lanes, lane));
}
int ecdsa_emu_decode_sig(const uint8_t* sig, size_t len, uint8_t* r, uint8_t* s) {
  return ftsh::decode_ecdsa_signature(sig, len, r, s);
}
int ecdsa_emu_identity(const uint8_t* id, size_t len, uint8_t* xy) {
  return ftsh::decode_x509_identity(id, len, xy);
}
// The whole job as the runtime and the kernels split it.  registered_xy != null:
// the registered-key route (its table); else the ad-hoc route (decode `id`).
int ecdsa_emu_verify(const uint8_t* id, size_t id_len, const uint8_t* registered_xy, const uint8_t* msg,
                     size_t msg_len, const uint8_t* sig, size_t sig_len) {
  uint8_t xy[64], rb[32], sb[32];
  int code = 0;
  if (!registered_xy) code = ftsh::decode_x509_identity(id, id_len, xy);
  if (code == 0) code = ftsh::decode_ecdsa_signature(sig, sig_len, rb, sb);
  if (code) return code;
  uint32_t r[8], s[8], u1[8], u2[8];
  be32_to_limbs(r, rb);
  be32_to_limbs(s, sb);
  if (!ecdsa_rs_in_range(r, s)) return FTZ_ERR_SIGNATURE;
  Sha256 h;
  h.init();
  h.update(msg, (uint32_t)msg_len);
  uint8_t d[32];
  h.final(d);
  ecdsa_scalars(d, r, s, u1, u2);
  p256j a = p256_fixed_mul(table_for(nullptr), u1), b;
  if (registered_xy) {
    b = p256_fixed_mul(table_for(registered_xy), u2);
  } else {
    std::vector<uint32_t> vt((size_t)P256_VT_WORDS * 5);
    b = p256_var_mul(pf_in(xy), pf_in(xy + 32), u2, vt.data(), 5, 3);
  }
  return ecdsa_accept(a, b, r) ? FTZ_OK : FTZ_ERR_SIGNATURE;
}
}
