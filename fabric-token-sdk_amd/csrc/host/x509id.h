// Host side of x509 ECDSA signature verification: the wire formats around
// edsaVerifier.Verify (token/core/identity/msp/x509/ecdsa.go:70-101), decoded
// as the reference's Go libraries decode them:
//   * the signature: asn1.Unmarshal(sigma, &ecdsaSignature{R, S *big.Int}) with
//     Go 1.18 encoding/asn1 rules -- 0x30 with a definite, minimal length, two
//     0x02 INTEGERs, each non-empty and minimally encoded; bytes after S inside
//     the SEQUENCE and bytes after the SEQUENCE are ignored (Go discards `rest`);
//     negative values and magnitudes over 32 bytes parse and then fail the
//     range check (1 <= r < n, 1 <= s <= (n-1)/2);
//   * the identity: MSPIdentityDeserializer.DeserializeVerifier ->
//     NewIdentityFromBytes (ecdsa.go:130-147): proto msp.SerializedIdentity
//     (field 2 = IdBytes; unknown fields skipped, the last value of a repeated
//     field wins), IdBytes one PEM block, "PUBLIC KEY" (PKIX
//     SubjectPublicKeyInfo) or "CERTIFICATE" (the key of
//     tbsCertificate.subjectPublicKeyInfo; as in the reference the
//     certificate's own signature, validity and chain are not checked).
// Only what is certain is accepted.  FTZ_ERR_UNSUPPORTED ("verify in Go"), never
// a guess, for: a PEM block that is not in the canonical form pem.EncodeToMemory
// and openssl write (headers, leading garbage, other line lengths or spacing),
// any other block type, an ECDSA key on another named curve (the reference
// verifies P-224/384/521 too), an RSA key, and a certificate or key structure
// that departs from the expected DER walk.  FTZ_ERR_IDENTITY for an
// unmarshalable proto and for a P-256 key whose point is malformed (unused
// bits, not 65 bytes, not 0x04-prefixed, a coordinate >= p) or off the curve.
// Known gap: Go's x509.ParseCertificate is stricter than this structural walk
// (it rejects, e.g., malformed names, extensions or validity times that the
// walk steps over).  Callers should therefore register only identities their Go
// deserializer has already accepted -- for the auditor and the issuers that
// happens when the public parameters are loaded.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../../include/ftsamd.h"

namespace ftsh {

// FTZ_OK with r, s (32 bytes big-endian, in range), or FTZ_ERR_SIGNATURE
int decode_ecdsa_signature(const uint8_t* sig, size_t len, uint8_t r[32], uint8_t s[32]);

// The writer's side (edsaSigner.Sign, ecdsa.go:50-64, utils.MarshalECDSASignature):
// SEQUENCE of two minimal INTEGERs -- leading zero bytes stripped, a 0x00 pad
// when the top bit is set.  r, s: 32 bytes big-endian, any values; returns the
// length written, at most 72 (71 for a low s).
size_t encode_ecdsa_signature(const uint8_t r[32], const uint8_t s[32], uint8_t out[72]);

// FTZ_OK with the affine point X || Y (32 bytes big-endian each, on P-256), or
// FTZ_ERR_IDENTITY / FTZ_ERR_UNSUPPORTED with the reason in *why (optional)
int decode_x509_identity(const uint8_t* id, size_t len, uint8_t xy[64], std::string* why = nullptr);

}  // namespace ftsh
