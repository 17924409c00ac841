// Host decoding for x509 ECDSA signature verification (x509id.h).
#include "x509id.h"

#include <string.h>

#include <vector>

#include "../dev/p256.h"
#include "idemix.h"

namespace ftsh {

namespace {

// Go 1.18 encoding/asn1 parseTagAndLength on a one-byte tag: definite, minimal
// lengths; the element must lie inside [0, n)
bool tlv(const uint8_t* b, size_t n, size_t& off, uint8_t& tag, size_t& len) {
  if (off >= n) return false;
  tag = b[off++];
  if ((tag & 0x1f) == 0x1f) return false;  // high-tag-number form: none of the expected tags
  if (off >= n) return false;
  uint8_t c = b[off++];
  size_t L = 0;
  if (c & 0x80) {
    int nb = c & 0x7f;
    if (nb == 0) return false;  // indefinite length
    for (int k = 0; k < nb; k++) {
      if (off >= n) return false;
      if (L >= (1u << 23)) return false;
      L = (L << 8) | b[off++];
      if (L == 0) return false;  // superfluous leading zeros
    }
    if (L < 0x80) return false;  // non-minimal length
  } else {
    L = c;
  }
  if (L > n - off) return false;
  len = L;
  return true;
}

// an element with tag `want`: its content; off moves past it
bool expect(const uint8_t* b, size_t n, size_t& off, uint8_t want, const uint8_t*& p, size_t& len) {
  uint8_t tag;
  if (!tlv(b, n, off, tag, len) || tag != want) return false;
  p = b + off;
  off += len;
  return true;
}

// parseBigInt of an INTEGER's content into 32 bytes big-endian; false when the
// encoding is refused; *in_256 = the value is in [0, 2^256)
bool der_int(const uint8_t* p, size_t n, uint8_t out[32], bool* in_256) {
  if (n == 0) return false;  // empty integer
  if (n >= 2 && ((p[0] == 0 && (p[1] & 0x80) == 0) || (p[0] == 0xff && (p[1] & 0x80) == 0x80)))
    return false;  // not minimally encoded
  *in_256 = false;
  if (p[0] & 0x80) return true;  // negative
  if (p[0] == 0) {
    p++;
    n--;
  }
  if (n > 32) return true;
  memset(out, 0, 32 - n);
  if (n) memcpy(out + 32 - n, p, n);
  *in_256 = true;
  return true;
}

int fail(std::string* why, int code, const char* text) {
  if (why) *why = text;
  return code;
}

const uint8_t OID_EC_PUBLIC_KEY[] = {0x2a, 0x86, 0x48, 0xce, 0x3d, 0x02, 0x01};
const uint8_t OID_PRIME256V1[] = {0x2a, 0x86, 0x48, 0xce, 0x3d, 0x03, 0x01, 0x07};

// SubjectPublicKeyInfo content (inside its SEQUENCE)
int spki(const uint8_t* b, size_t n, uint8_t xy[64], std::string* why) {
  size_t off = 0, al, l;
  const uint8_t *alg, *p;
  if (!expect(b, n, off, 0x30, alg, al)) return fail(why, FTZ_ERR_UNSUPPORTED, "public key: no algorithm identifier");
  size_t k = 0;
  if (!expect(alg, al, k, 0x06, p, l)) return fail(why, FTZ_ERR_UNSUPPORTED, "public key: no algorithm OID");
  if (l != sizeof(OID_EC_PUBLIC_KEY) || memcmp(p, OID_EC_PUBLIC_KEY, l) != 0)
    return fail(why, FTZ_ERR_UNSUPPORTED, "public key: not an ECDSA key (verified in Go)");
  if (!expect(alg, al, k, 0x06, p, l) || k != al)
    return fail(why, FTZ_ERR_UNSUPPORTED, "public key: curve parameters are not one named curve");
  if (l != sizeof(OID_PRIME256V1) || memcmp(p, OID_PRIME256V1, l) != 0)
    return fail(why, FTZ_ERR_UNSUPPORTED, "public key: ECDSA on another curve than P-256 (verified in Go)");
  if (!expect(b, n, off, 0x03, p, l) || off != n)
    return fail(why, FTZ_ERR_UNSUPPORTED, "public key: no BIT STRING at the end of the key info");
  // a P-256 key from here on: elliptic.Unmarshal's rules
  if (l != 66 || p[0] != 0) return fail(why, FTZ_ERR_IDENTITY, "public key: the point is not 65 whole bytes");
  p++;
  if (p[0] != 0x04) return fail(why, FTZ_ERR_IDENTITY, "public key: the point is not in uncompressed form");
  uint32_t x[8], y[8];
  fts::be32_to_limbs(x, p + 1);
  fts::be32_to_limbs(y, p + 33);
  if (fts::u256_geq(x, fts::P256_P) || fts::u256_geq(y, fts::P256_P))
    return fail(why, FTZ_ERR_IDENTITY, "public key: coordinate not below p");
  if (!fts::p256_on_curve(fts::pf_from_int(x), fts::pf_from_int(y)))
    return fail(why, FTZ_ERR_IDENTITY, "public key: the point is not on P-256");
  memcpy(xy, p + 1, 64);
  return FTZ_OK;
}

int b64_val(uint8_t c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}

// One PEM block in the canonical form (pem.EncodeToMemory, openssl): the BEGIN
// line, base64 lines of 64 characters (the last one shorter or equal), the END
// line, each ended by '\n' (the last '\n' optional); nothing else
bool pem_block(const uint8_t* b, size_t n, std::string& type, std::vector<uint8_t>& der) {
  static const char BEGIN[] = "-----BEGIN ", END[] = "-----END ", DASH[] = "-----";
  if (n < 11 || memcmp(b, BEGIN, 11) != 0) return false;
  size_t i = 11;
  while (i < n && b[i] != '-' && b[i] != '\n' && b[i] != '\r' && b[i] != ':') i++;
  type.assign((const char*)b + 11, i - 11);
  if (type.empty() || n - i < 6 || memcmp(b + i, DASH, 5) != 0 || b[i + 5] != '\n') return false;
  i += 6;
  std::vector<uint8_t> chars;
  bool last = false;
  for (;;) {
    if (n - i >= 9 && memcmp(b + i, END, 9) == 0) break;
    if (last) return false;  // a short line was not the last one
    size_t k = i;
    while (k < n && b[k] != '\n') k++;
    if (k == n || k == i || k - i > 64) return false;
    if (k - i < 64) last = true;
    chars.insert(chars.end(), b + i, b + k);
    i = k + 1;
  }
  i += 9;
  if (n - i < type.size() + 5 || memcmp(b + i, type.data(), type.size()) != 0) return false;
  i += type.size();
  if (memcmp(b + i, DASH, 5) != 0) return false;
  i += 5;
  if (!(i == n || (i + 1 == n && b[i] == '\n'))) return false;
  // base64.StdEncoding: whole quanta, '=' only as the last one or two characters
  if (chars.empty() || chars.size() % 4) return false;
  size_t pad = 0;
  if (chars[chars.size() - 1] == '=') pad++;
  if (pad && chars[chars.size() - 2] == '=') pad++;
  der.clear();
  for (size_t q = 0; q < chars.size(); q += 4) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) {
      bool is_pad = q + 4 == chars.size() && k >= 4 - (int)pad;
      int d = is_pad ? 0 : b64_val(chars[q + k]);
      if (d < 0) return false;
      v = (v << 6) | (uint32_t)d;
    }
    der.push_back((uint8_t)(v >> 16));
    der.push_back((uint8_t)(v >> 8));
    der.push_back((uint8_t)v);
  }
  der.resize(der.size() - pad);
  return true;
}

}  // namespace

int decode_ecdsa_signature(const uint8_t* sig, size_t len, uint8_t r[32], uint8_t s[32]) {
  size_t off = 0, sl, l;
  const uint8_t *seq, *p;
  if (!expect(sig, len, off, 0x30, seq, sl)) return FTZ_ERR_SIGNATURE;
  size_t k = 0;
  bool r_ok, s_ok;
  if (!expect(seq, sl, k, 0x02, p, l) || !der_int(p, l, r, &r_ok)) return FTZ_ERR_SIGNATURE;
  if (!expect(seq, sl, k, 0x02, p, l) || !der_int(p, l, s, &s_ok)) return FTZ_ERR_SIGNATURE;
  if (!r_ok || !s_ok) return FTZ_ERR_SIGNATURE;
  uint32_t rl[8], sl8[8];
  fts::be32_to_limbs(rl, r);
  fts::be32_to_limbs(sl8, s);
  return fts::ecdsa_rs_in_range(rl, sl8) ? FTZ_OK : FTZ_ERR_SIGNATURE;
}

size_t encode_ecdsa_signature(const uint8_t r[32], const uint8_t s[32], uint8_t out[72]) {
  size_t n = 2;  // the SEQUENCE header: its content is at most 70 bytes, one length byte
  for (const uint8_t* v : {r, s}) {
    size_t lead = 0;
    while (lead < 31 && v[lead] == 0) lead++;  // zero keeps one byte
    const bool pad = (v[lead] & 0x80) != 0;
    out[n++] = 0x02;
    out[n++] = (uint8_t)(32 - lead + (pad ? 1 : 0));
    if (pad) out[n++] = 0;
    memcpy(out + n, v + lead, 32 - lead);
    n += 32 - lead;
  }
  out[0] = 0x30;
  out[1] = (uint8_t)(n - 2);
  return n;
}

int decode_x509_identity(const uint8_t* id, size_t len, uint8_t xy[64], std::string* why) {
  std::vector<PbField> fs;
  std::string e = pb_scan(id, len, fs);
  if (!e.empty()) return fail(why, FTZ_ERR_IDENTITY, "failed unmarshalling to msp serialized identity");
  const uint8_t* pem = nullptr;
  size_t pem_len = 0;
  for (const PbField& f : fs) {
    if (f.wt != 2) continue;  // a known field with another wire type is an unknown field
    if (f.num == 1 && !utf8_valid(f.p, f.len))
      return fail(why, FTZ_ERR_IDENTITY, "failed unmarshalling to msp serialized identity: invalid UTF-8");
    if (f.num == 2) {
      pem = f.p;
      pem_len = f.len;
    }
  }
  std::string type;
  std::vector<uint8_t> der;
  if (!pem || !pem_block(pem, pem_len, type, der))
    return fail(why, FTZ_ERR_UNSUPPORTED, "identity: not one canonical PEM block (verified in Go)");
  const uint8_t* b = der.data();
  size_t n = der.size(), off = 0, l;
  const uint8_t* p;
  if (type == "PUBLIC KEY") {
    if (!expect(b, n, off, 0x30, p, l) || off != n)
      return fail(why, FTZ_ERR_UNSUPPORTED, "public key: not one SubjectPublicKeyInfo");
    return spki(p, l, xy, why);
  }
  if (type != "CERTIFICATE") return fail(why, FTZ_ERR_UNSUPPORTED, "identity: PEM block type verified in Go");
  const char* walk = "certificate: unexpected structure (verified in Go)";
  if (!expect(b, n, off, 0x30, p, l) || off != n) return fail(why, FTZ_ERR_UNSUPPORTED, walk);
  const uint8_t* tbs;
  size_t tl, k = 0;
  if (!expect(p, l, k, 0x30, tbs, tl)) return fail(why, FTZ_ERR_UNSUPPORTED, walk);
  k = 0;
  const uint8_t* q;
  size_t ql;
  if (tl && tbs[0] == 0xa0 && !expect(tbs, tl, k, 0xa0, q, ql)) return fail(why, FTZ_ERR_UNSUPPORTED, walk);
  // serial, signature algorithm, issuer, validity, subject
  static const uint8_t tags[5] = {0x02, 0x30, 0x30, 0x30, 0x30};
  for (uint8_t t : tags)
    if (!expect(tbs, tl, k, t, q, ql)) return fail(why, FTZ_ERR_UNSUPPORTED, walk);
  if (!expect(tbs, tl, k, 0x30, q, ql)) return fail(why, FTZ_ERR_UNSUPPORTED, walk);
  return spki(q, ql, xy, why);
}

}  // namespace ftsh
