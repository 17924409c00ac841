"""Pure-Python restatement of x509 ECDSA P-256 verification as the reference
runs it (token/core/identity/msp/x509/ecdsa.go): affine P-256 on Python ints,
the Go-rule DER signature and identity decoders, and verify(identity, msg, sig)
-> FTZ code.  Independent of the C++ / HIP code under test: it shares no source
with it, and tests/golden/ecdsa_golden.json holds openssl-made signatures that
pin it."""
import base64
import hashlib

P = 2**256 - 2**224 + 2**192 + 2**96 - 1
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
G = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
     0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)
HALF_N = (N - 1) // 2

OK, ERR_SIGNATURE, ERR_UNSUPPORTED, ERR_IDENTITY = 0, 10, 11, 13


def on_curve(pt):
    x, y = pt
    return (y * y - x * x * x + 3 * x - B) % P == 0


def add(p1, p2):
    """affine addition; None is the point at infinity"""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lm = (3 * x1 * x1 - 3) * pow(2 * y1, -1, P) % P
    else:
        lm = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lm * lm - x1 - x2) % P
    return (x3, (lm * (x1 - x3) - y1) % P)


def mul(pt, k):
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


# ---------------------------------------------------------------- DER (Go 1.18 encoding/asn1)
class DerError(Exception):
    pass


def tlv(b, off):
    """(tag, content start, content end) of the element at off"""
    if off >= len(b):
        raise DerError("truncated")
    tag = b[off]
    off += 1
    if tag & 0x1f == 0x1f or off >= len(b):
        raise DerError("tag")
    c = b[off]
    off += 1
    if c & 0x80:
        nb = c & 0x7f
        if nb == 0:
            raise DerError("indefinite length")
        ln = 0
        for _ in range(nb):
            if off >= len(b) or ln >= 1 << 23:
                raise DerError("length")
            ln = (ln << 8) | b[off]
            off += 1
            if ln == 0:
                raise DerError("leading zeros in length")
        if ln < 0x80:
            raise DerError("non-minimal length")
    else:
        ln = c
    if ln > len(b) - off:
        raise DerError("data truncated")
    return tag, off, off + ln


def expect(b, off, want):
    tag, s, e = tlv(b, off)
    if tag != want:
        raise DerError("tag %#x, want %#x" % (tag, want))
    return b[s:e], e


def der_int(c):
    if len(c) == 0:
        raise DerError("empty integer")
    if len(c) >= 2 and ((c[0] == 0 and c[1] & 0x80 == 0) or (c[0] == 0xff and c[1] & 0x80)):
        raise DerError("integer not minimally encoded")
    return int.from_bytes(c, "big", signed=True)


def parse_signature(sig):
    """asn1.Unmarshal(sigma, &ecdsaSignature{R, S}): (r, s) or DerError"""
    seq, _ = expect(sig, 0, 0x30)  # bytes after the SEQUENCE: `rest`, discarded
    rc, off = expect(seq, 0, 0x02)
    sc, off = expect(seq, off, 0x02)  # bytes after S inside the SEQUENCE are ignored
    return der_int(rc), der_int(sc)


def encode_int(v):
    n = max(1, (v.bit_length() + 8) // 8) if v >= 0 else (((-v - 1).bit_length() + 8) // 8)
    return v.to_bytes(n, "big", signed=True)


def encode_len(n):
    if n < 0x80:
        return bytes([n])
    b = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(b)]) + b


def encode_tlv(tag, content):
    return bytes([tag]) + encode_len(len(content)) + content


def encode_signature(r, s):
    return encode_tlv(0x30, encode_tlv(0x02, encode_int(r)) + encode_tlv(0x02, encode_int(s)))


# ---------------------------------------------------------------- identity
class Unsupported(Exception):
    pass


class IdentityError(Exception):
    pass


def _varint(b, i):
    v = 0
    for k in range(10):
        if i >= len(b):
            raise IdentityError("EOF")
        c = b[i]
        i += 1
        if k == 9 and c > 1:
            raise IdentityError("varint overflow")
        v |= (c & 0x7f) << (7 * k)
        if c < 0x80:
            return v, i
    raise IdentityError("varint overflow")


def _skip_group(b, i, num, depth=0):
    while True:
        if i >= len(b):
            raise IdentityError("EOF")
        t, i = _varint(b, i)
        n2, wt = t >> 3, t & 7
        if n2 < 1 or n2 > (1 << 29) - 1:
            raise IdentityError("field number")
        if wt == 4:
            if n2 != num:
                raise IdentityError("end group")
            return i
        i = _skip(b, i, n2, wt, depth + 1)


def _skip(b, i, num, wt, depth=0):
    if wt == 0:
        return _varint(b, i)[1]
    if wt in (1, 5):
        k = 8 if wt == 1 else 4
        if len(b) - i < k:
            raise IdentityError("EOF")
        return i + k
    if wt == 2:
        ln, i = _varint(b, i)
        if ln > len(b) - i:
            raise IdentityError("EOF")
        return i + ln
    if wt == 3:
        return _skip_group(b, i, num, depth)
    raise IdentityError("wire type")


def serialized_identity_idbytes(raw):
    """proto.Unmarshal(raw, &msp.SerializedIdentity{}) -> IdBytes"""
    i, idb = 0, b""
    while i < len(raw):
        t, i = _varint(raw, i)
        num, wt = t >> 3, t & 7
        if num < 1 or num > (1 << 29) - 1 or wt == 4:
            raise IdentityError("tag")
        if wt == 2:
            ln, i = _varint(raw, i)
            if ln > len(raw) - i:
                raise IdentityError("EOF")
            val = raw[i:i + ln]
            i += ln
            if num == 1:
                try:
                    val.decode("utf-8")
                except UnicodeDecodeError:
                    raise IdentityError("invalid UTF-8")
            if num == 2:
                idb = val
        else:
            i = _skip(raw, i, num, wt)
    return idb


def pem_block(data):
    """(type, DER) of one PEM block in the canonical form, else Unsupported"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) < 3 or not (lines[0].startswith(b"-----BEGIN ") and lines[0].endswith(b"-----")):
        raise Unsupported("PEM")
    typ = lines[0][11:-5]
    if not typ or any(c in typ for c in b"-:\r") or lines[-1] != b"-----END " + typ + b"-----":
        raise Unsupported("PEM")
    body = lines[1:-1]
    alphabet = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")
    for k, ln in enumerate(body):
        if len(ln) == 0 or len(ln) > 64 or (len(ln) < 64 and k != len(body) - 1):
            raise Unsupported("PEM line length")
    text = b"".join(body)
    stripped = text.rstrip(b"=")
    if len(text) % 4 or len(text) - len(stripped) > 2 or any(c not in alphabet for c in stripped):
        raise Unsupported("PEM base64")
    return typ.decode(), base64.b64decode(text)


OID_EC = bytes.fromhex("2a8648ce3d0201")
OID_P256 = bytes.fromhex("2a8648ce3d030107")


def spki_point(c):
    """content of a SubjectPublicKeyInfo SEQUENCE -> (x, y)"""
    try:
        alg, off = expect(c, 0, 0x30)
        oid, k = expect(alg, 0, 0x06)
        if oid != OID_EC:
            raise Unsupported("not ECDSA")
        curve, k = expect(alg, k, 0x06)
        if k != len(alg):
            raise Unsupported("parameters")
        if curve != OID_P256:
            raise Unsupported("curve")
        bits, off = expect(c, off, 0x03)
        if off != len(c):
            raise Unsupported("trailing")
    except DerError:
        raise Unsupported("structure")
    if len(bits) != 66 or bits[0] != 0 or bits[1] != 4:
        raise IdentityError("point encoding")
    x, y = int.from_bytes(bits[2:34], "big"), int.from_bytes(bits[34:], "big")
    if x >= P or y >= P or not on_curve((x, y)):
        raise IdentityError("point")
    return x, y


def public_key(identity):
    """DeserializeVerifier(identity) -> (x, y); raises IdentityError / Unsupported"""
    typ, der = pem_block(serialized_identity_idbytes(identity))
    try:
        if typ == "PUBLIC KEY":
            c, off = expect(der, 0, 0x30)
            if off != len(der):
                raise Unsupported("trailing")
            return spki_point(c)
        if typ != "CERTIFICATE":
            raise Unsupported(typ)
        cert, off = expect(der, 0, 0x30)
        if off != len(der):
            raise Unsupported("trailing")
        tbs, _ = expect(cert, 0, 0x30)
        k = 0
        if tbs[:1] == b"\xa0":
            _, k = expect(tbs, 0, 0xa0)
        for tag in (0x02, 0x30, 0x30, 0x30, 0x30):
            _, k = expect(tbs, k, tag)
        c, _ = expect(tbs, k, 0x30)
        return spki_point(c)
    except DerError:
        raise Unsupported("structure")


def identity_code(identity):
    try:
        public_key(identity)
    except IdentityError:
        return ERR_IDENTITY
    except Unsupported:
        return ERR_UNSUPPORTED
    return OK


# ---------------------------------------------------------------- verification
def verify_rs(q, msg, r, s):
    """go1.18 ecdsa.Verify behind the low-S rule; True = accept"""
    if not (1 <= r < N and 1 <= s <= HALF_N):
        return False
    e = int.from_bytes(hashlib.sha256(msg).digest(), "big")
    w = pow(s, -1, N)
    pt = add(mul(G, e * w % N), mul(q, r * w % N))
    return pt is not None and pt[0] % N == r


def signature_code(q, msg, sig):
    try:
        r, s = parse_signature(sig)
    except DerError:
        return ERR_SIGNATURE
    return OK if verify_rs(q, msg, r, s) else ERR_SIGNATURE


def verify(identity, msg, sig):
    """FTZ code of DeserializeVerifier(identity).Verify(msg, sig)"""
    try:
        q = public_key(identity)
    except IdentityError:
        return ERR_IDENTITY
    except Unsupported:
        return ERR_UNSUPPORTED
    return signature_code(q, msg, sig)


def sign(d, msg, k):
    """low-S signature (r, s) with nonce k"""
    e = int.from_bytes(hashlib.sha256(msg).digest(), "big")
    r = mul(G, k)[0] % N
    s = pow(k, -1, N) * (e + r * d) % N
    assert r and s
    return r, min(s, N - s)


def serialized_identity(id_bytes, mspid=b""):
    out = b""
    if mspid:
        out += b"\x0a" + bytes([len(mspid)]) + mspid
    ln = len(id_bytes)
    v = b""
    while True:
        c = ln & 0x7f
        ln >>= 7
        v += bytes([c | (0x80 if ln else 0)])
        if not ln:
            break
    return out + b"\x12" + v + id_bytes


def pem_encode(typ, der):
    b = base64.b64encode(der)
    lines = [b[i:i + 64] for i in range(0, len(b), 64)]
    return b"-----BEGIN " + typ.encode() + b"-----\n" + b"\n".join(lines) + b"\n-----END " + typ.encode() + b"-----\n"


def spki_der(x, y, curve_oid=OID_P256, point=None):
    pt = point if point is not None else b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")
    alg = encode_tlv(0x30, encode_tlv(0x06, OID_EC) + encode_tlv(0x06, curve_oid))
    return encode_tlv(0x30, alg + encode_tlv(0x03, b"\x00" + pt))
