"""Python-int restatement of the batch pseudonym signer (dev/nymsign.h,
dev/hmac256.h): IBM/idemix NewNymSignature on BN254 with r_sk, r_rnym and the
nonce drawn from the HMAC-SHA-256 DRBG of RFC 6979 section 3.2 instead of
crypto/rand (only the generator is that RFC's: 512 bits reduced mod r per
value, no retry loop).  The signature itself is the oracle's
(ftsoracle.idemix.bn_nym_sign with the derived values)."""
import hashlib
import hmac
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "py"))
from ftsoracle import bn254 as C  # noqa: E402
from ftsoracle import idemix as I  # noqa: E402

R = C.R
P = C.P


def _hmac(key, data):
    return hmac.new(key, data, hashlib.sha256).digest()


def drbg_outputs(x, z, extra, count):
    """HMAC_DRBG init (K = 00.., V = 01..; two rounds K = HMAC_K(V || tag || x || z || extra),
    V = HMAC_K(V)) and `count` outputs V = HMAC_K(V)"""
    K, V = b"\x00" * 32, b"\x01" * 32
    for tag in (b"\x00", b"\x01"):
        K = _hmac(K, V + tag + x + z + extra)
        V = _hmac(K, V)
    out = []
    for _ in range(count):
        V = _hmac(K, V)
        out.append(V)
    return out


def seed(msg, entropy=None):
    """z: SHA-256(msg), or SHA-256(SHA-256(msg) || entropy) when hedged"""
    z = hashlib.sha256(msg).digest()
    return hashlib.sha256(z + entropy).digest() if entropy is not None else z


def randomness(sk, r_nym, msg, entropy=None):
    """(r_sk, r_rnym, nonce)"""
    v = drbg_outputs(sk.to_bytes(32, "big"), seed(msg, entropy), r_nym.to_bytes(32, "big"), 6)
    return tuple(int.from_bytes(v[2 * k] + v[2 * k + 1], "big") % R for k in range(3))


def sign(ipk, sk, r_nym, nym, msg, entropy=None):
    """the 136-byte NymSignature proto; nym: the oracle's point (x, y)"""
    return I.bn_nym_sign(ipk, sk, r_nym, nym, msg, *randomness(sk, r_nym, msg, entropy))


def make_nym(ipk, sk, r_nym):
    return I.bn_make_nym(ipk, sk, r_nym)


def nym_bytes(nym):
    """NymX || NymY"""
    return C.g1_bytes(nym)


def owner_of(nym):
    """asn1(RawOwner{"si", SerializedIdentity}) around the nym, as tests/golden/make_idemix_bn254.py builds it"""
    role = I.pb_field(1, 2, b"idemix") + I.pb_field(2, 0, 2)
    ou = I.pb_field(1, 2, b"idemix") + I.pb_field(2, 2, b"org1.department1") + I.pb_field(3, 2, b"")
    return I.raw_owner_encode(b"si", I.bn_serialize_idemix_identity(nym, ou=ou, role=role), 0x13)


def expand(seed_bytes, n):
    """the SHA-256 counter stream of the idemix fixtures' bench entries (tests/golden/make_idemix.py expand)"""
    out = b""
    c = 0
    while len(out) < n:
        out += hashlib.sha256(seed_bytes + c.to_bytes(4, "big")).digest()
        c += 1
    return out[:n]
