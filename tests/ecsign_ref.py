"""Python-int restatement of the batch signer (dev/ecsign.h, dev/hmac256.h):
edsaSigner.Sign (identity/msp/x509/ecdsa.go:50-64) with the nonce of RFC 6979
section 3.2 for P-256 / SHA-256 (qlen = hlen = 256), optionally with the
additional data k' of section 3.6, then ToLowS and DER.  Pinned by RFC 6979
A.2.5 in tests/test_ecsign.py."""
import hashlib
import hmac

import p256_ref as R

N = R.N


def _hmac(key, data):
    return hmac.new(key, data, hashlib.sha256).digest()


def drbg_init(d, h1, extra=b""):
    """(K, V) after steps b-g; h1 = the message digest, extra = k' (b"" or 32 bytes)"""
    x = d.to_bytes(32, "big")
    z = (int.from_bytes(h1, "big") % N).to_bytes(32, "big")  # bits2octets
    K, V = b"\x00" * 32, b"\x01" * 32
    for tag in (b"\x00", b"\x01"):
        K = _hmac(K, V + tag + x + z + extra)
        V = _hmac(K, V)
    return K, V


def drbg_retry(K, V):
    """step h.3 after a refused candidate"""
    K = _hmac(K, V + b"\x00")
    return K, _hmac(K, V)


def nonce(d, msg, extra=None):
    K, V = drbg_init(d, hashlib.sha256(msg).digest(), extra or b"")
    while True:
        V = _hmac(K, V)
        k = int.from_bytes(V, "big")
        if 1 <= k < N:
            return k
        K, V = drbg_retry(K, V)


def sign_rs(d, msg, extra=None):
    """(r, s), s low"""
    return R.sign(d, msg, nonce(d, msg, extra))


def sign(d, msg, extra=None):
    """the DER signature"""
    return R.encode_signature(*sign_rs(d, msg, extra))


def public_key(d):
    return R.mul(R.G, d)


def identity_of(d):
    """proto(msp.SerializedIdentity) around the PUBLIC KEY block of d G"""
    return R.serialized_identity(R.pem_encode("PUBLIC KEY", R.spki_der(*public_key(d))))
