#!/usr/bin/env python3
"""Write tests/golden/ecdsa_golden.json: the fixture of tests/test_ecdsa.py and
tests/test_ecdsa_gpu.py.  Run once on a CPU and committed; tests never run it.

The `openssl` CLI makes the keys, the "PUBLIC KEY" and "CERTIFICATE" PEM blocks
and the `dgst -sha256 -sign` signatures (an implementation independent of this
project's, normalised to low-S as the reference's signer does); p256_ref crafts
the adversarial cases.  Every case records the code the reference would give
(0 accept, 10 signature, 11 verify-in-Go, 13 identity), computed by p256_ref
and asserted here against the intent of the case.

Layout: keys[name] = {identity, xy} (identities a test may register);
cases[] = {name, key | identity, msg, sig, expect[, xy][, openssl]} (hex)."""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import p256_ref as R  # noqa: E402

OK, SIG, UNSUP, IDENT = R.OK, R.ERR_SIGNATURE, R.ERR_UNSUPPORTED, R.ERR_IDENTITY
rng = random.Random(20260501)


def ossl(*args, stdin=None):
    return subprocess.run(["openssl"] + list(args), input=stdin, check=True, capture_output=True).stdout


def low_s(sig):
    r, s = R.parse_signature(sig)
    return R.encode_signature(r, min(s, R.N - s))


def e_of(msg):
    return int.from_bytes(hashlib.sha256(msg).digest(), "big")


def key_identity(d):
    x, y = R.mul(R.G, d)
    return R.serialized_identity(R.pem_encode("PUBLIC KEY", R.spki_der(x, y))), (x, y)


def main():
    keys, cases = {}, []
    tmp = tempfile.mkdtemp()
    kp, msgf = os.path.join(tmp, "k.pem"), os.path.join(tmp, "m")

    def add_key(name, identity):
        x, y = R.public_key(identity)
        keys[name] = {"identity": identity.hex(), "xy": (x.to_bytes(32, "big") + y.to_bytes(32, "big")).hex()}

    def case(name, who, msg, sig, want, **kw):
        identity = bytes.fromhex(keys[who]["identity"]) if who in keys else who
        got = R.verify(identity, msg, sig)
        assert got == want, (name, got, want)
        c = {"name": name, "msg": msg.hex(), "sig": sig.hex(), "expect": want}
        if who in keys:
            c["key"] = who
        else:
            c["identity"] = identity.hex()
            if R.identity_code(identity) == OK:
                x, y = R.public_key(identity)
                c["xy"] = (x.to_bytes(32, "big") + y.to_bytes(32, "big")).hex()
        c.update(kw)
        assert name not in [q["name"] for q in cases]
        cases.append(c)

    # ---- openssl: key A as PUBLIC KEY and as a self-signed CERTIFICATE
    ossl("ecparam", "-name", "prime256v1", "-genkey", "-noout", "-out", kp)
    pub_pem = ossl("ec", "-in", kp, "-pubout")
    cert_pem = ossl("req", "-new", "-x509", "-key", kp, "-subj", "/CN=auditor.example.com/O=org1", "-days", "3650")
    add_key("pub", R.serialized_identity(pub_pem))
    add_key("cert", R.serialized_identity(cert_pem, mspid=b"Org1MSP"))
    assert keys["pub"]["xy"] == keys["cert"]["xy"]
    pub = bytes.fromhex(keys["pub"]["identity"])

    def ossl_sign(msg):
        with open(msgf, "wb") as f:
            f.write(msg)
        return low_s(ossl("dgst", "-sha256", "-sign", kp, msgf))

    # message lengths on the SHA-256 padding boundaries, both identity forms
    for ln in (0, 55, 56, 64, 119, 120, 1000):
        msg = bytes(rng.randrange(256) for _ in range(ln))
        case("openssl_len%d_pub" % ln, "pub", msg, ossl_sign(msg), OK, openssl=True)
        case("openssl_len%d_cert" % ln, "cert", msg, ossl_sign(msg), OK, openssl=True)
    for i in range(8):
        msg = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 300)))
        case("openssl_rand%d" % i, "pub", msg, ossl_sign(msg), OK, openssl=True)

    msg = b"token request bytes || anchor"
    good = ossl_sign(msg)
    r, s = R.parse_signature(good)
    case("good", "pub", msg, good, OK, openssl=True)

    # ---- range and low-S
    sig = R.encode_signature
    case("r_zero", "pub", msg, sig(0, s), SIG)
    case("s_zero", "pub", msg, sig(r, 0), SIG)
    case("r_eq_n", "pub", msg, sig(R.N, s), SIG)
    case("s_eq_n", "pub", msg, sig(r, R.N), SIG)
    case("r_plus_n", "pub", msg, sig(r + R.N, s), SIG)  # 33 significant bytes, = r mod n
    case("s_plus_n", "pub", msg, sig(r, s + R.N), SIG)
    case("r_33_bytes", "pub", msg, sig(r + (1 << 256), s), SIG)
    case("s_33_bytes", "pub", msg, sig(r, s + (1 << 256)), SIG)
    case("r_negative", "pub", msg, sig(-r, s), SIG)
    case("s_negative", "pub", msg, sig(r, -s), SIG)
    case("r_minus_n", "pub", msg, sig(r - R.N, s), SIG)
    case("high_s", "pub", msg, sig(r, R.N - s), SIG)  # valid for plain ECDSA, refused by the low-S rule
    # s = (n-1)/2 exactly on a valid signature: choose k, solve d = (s k - e) / r
    m2 = b"low-S boundary"
    k = rng.randrange(1, R.N)
    r2 = R.mul(R.G, k)[0] % R.N
    d_half = (R.HALF_N * k - e_of(m2)) * pow(r2, -1, R.N) % R.N
    ident, _ = key_identity(d_half)
    add_key("half", ident)
    case("s_half_n", "half", m2, sig(r2, R.HALF_N), OK)
    case("s_half_n_flipped", "half", m2, sig(r2, R.N - R.HALF_N), SIG)  # = (n-1)/2 + 1: high-S
    case("s_half_n_plus_1", "pub", msg, sig(r, R.HALF_N + 1), SIG)

    # ---- message and key
    case("wrong_msg", "pub", msg + b"!", good, SIG)
    case("wrong_key", "half", msg, good, SIG)
    case("flip_r", "pub", msg, sig(r ^ (1 << 77), s), SIG)
    case("flip_s", "pub", msg, sig(r, s ^ (1 << 3)), SIG)
    fm = bytearray(msg)
    fm[5] ^= 0x10
    case("flip_msg", "pub", bytes(fm), good, SIG)

    # ---- u1 G = u2 Q: d = e / r, s = 2 e / k (valid; the final addition is a doubling)
    m3 = b"doubling case"
    while True:
        k = rng.randrange(1, R.N)
        r3 = R.mul(R.G, k)[0] % R.N
        s3 = 2 * e_of(m3) * pow(k, -1, R.N) % R.N
        if s3 <= R.HALF_N:
            break
    d_dbl = e_of(m3) * pow(r3, -1, R.N) % R.N
    ident, q = key_identity(d_dbl)
    w = pow(s3, -1, R.N)
    assert R.mul(R.G, e_of(m3) * w % R.N) == R.mul(q, r3 * w % R.N)
    add_key("dbl", ident)
    case("doubling", "dbl", m3, sig(r3, s3), OK)
    # ---- u1 G = -u2 Q: d = -e / r, any s in range: the sum is infinity
    m4 = b"cancelling case"
    r4 = rng.randrange(1, R.N)
    d_can = (-e_of(m4)) * pow(r4, -1, R.N) % R.N
    ident, q = key_identity(d_can)
    s4 = rng.randrange(1, R.HALF_N)
    w = pow(s4, -1, R.N)
    assert R.add(R.mul(R.G, e_of(m4) * w % R.N), R.mul(q, r4 * w % R.N)) is None
    add_key("cancel", ident)
    case("cancelling", "cancel", m4, sig(r4, s4), SIG)
    case("cancelling_s1", "cancel", m4, sig(r4, 1), SIG)

    # ---- DER
    ri, si = R.encode_tlv(0x02, R.encode_int(r)), R.encode_tlv(0x02, R.encode_int(s))
    body = ri + si
    case("der_nonminimal_length", "pub", msg, b"\x30\x81" + bytes([len(body)]) + body, SIG)
    case("der_indefinite_length", "pub", msg, b"\x30\x80" + body + b"\x00\x00", SIG)
    case("der_nonminimal_int", "pub", msg, R.encode_tlv(0x30, R.encode_tlv(0x02, b"\x00" + R.encode_int(r)) + si), SIG)
    case("der_nonminimal_negative_int", "pub", msg, R.encode_tlv(0x30, R.encode_tlv(0x02, b"\xff\xff") + si), SIG)
    case("der_empty_int", "pub", msg, R.encode_tlv(0x30, b"\x02\x00" + si), SIG)
    case("der_wrong_seq_tag", "pub", msg, b"\x31" + good[1:], SIG)
    case("der_primitive_seq", "pub", msg, b"\x10" + good[1:], SIG)
    case("der_wrong_int_tag", "pub", msg, R.encode_tlv(0x30, b"\x03" + ri[1:] + si), SIG)
    case("der_truncated", "pub", msg, good[:-1], SIG)
    case("der_only_r", "pub", msg, R.encode_tlv(0x30, ri), SIG)
    case("der_empty", "pub", msg, b"", SIG)
    case("der_trailing_inside", "pub", msg, R.encode_tlv(0x30, body + b"\x05\x00\xde\xad"), OK)
    case("der_trailing_after", "pub", msg, good + b"\x00\x01\x02", OK)
    long_body = body + b"\x04\x81\x90" + bytes(0x90)
    case("der_long_form_length", "pub", msg, R.encode_tlv(0x30, long_body), OK)  # 0x81 length, minimal

    # ---- identities (each with the good signature of key A)
    ax, ay = R.public_key(pub)
    pem = R.pem_encode
    ser = R.serialized_identity
    case("id_unknown_fields", ser(pub_pem) + b"\x18\x07" + b"\x7a\x03abc" + b"\x25\x01\x02\x03\x04", msg, good, OK)
    case("id_repeated_field2", b"\x12\x03zzz" + ser(pub_pem), msg, good, OK)
    case("id_repeated_field2_last_bad", ser(pub_pem) + b"\x12\x03zzz", msg, good, UNSUP)
    case("id_field2_as_varint", b"\x10\x05", msg, good, UNSUP)
    case("id_empty", b"", msg, good, UNSUP)
    case("id_garbage_proto", b"\x12\xff\xff\xff", msg, good, IDENT)
    case("id_truncated_proto", ser(pub_pem)[:-3], msg, good, IDENT)
    case("id_bad_utf8_mspid", b"\x0a\x02\xc3\x28" + ser(pub_pem), msg, good, IDENT)
    y_bad = (ay + 1) % R.P
    case("id_off_curve", ser(pem("PUBLIC KEY", R.spki_der(ax, y_bad))), msg, good, IDENT)
    x0 = next(x for x in range(1, 1000) if pow((x**3 - 3 * x + R.B) % R.P, (R.P - 1) // 2, R.P) == 1)
    y0 = pow((x0**3 - 3 * x0 + R.B) % R.P, (R.P + 1) // 4, R.P)
    assert R.on_curve((x0, y0))
    case("id_x_geq_p", ser(pem("PUBLIC KEY", R.spki_der(x0 + R.P, y0))), msg, good, IDENT)
    comp = bytes([2 + (ay & 1)]) + ax.to_bytes(32, "big")
    case("id_compressed_point", ser(pem("PUBLIC KEY", R.spki_der(0, 0, point=comp))), msg, good, IDENT)
    pt = b"\x04" + ax.to_bytes(32, "big") + ay.to_bytes(32, "big")
    alg = R.encode_tlv(0x30, R.encode_tlv(0x06, R.OID_EC) + R.encode_tlv(0x06, R.OID_P256))
    case("id_unused_bits", ser(pem("PUBLIC KEY", R.encode_tlv(0x30, alg + R.encode_tlv(0x03, b"\x01" + pt)))),
         msg, good, IDENT)
    case("id_infinity_point", ser(pem("PUBLIC KEY", R.spki_der(0, 0, point=b"\x00"))), msg, good, IDENT)
    case("id_spki_trailing", ser(pem("PUBLIC KEY", R.spki_der(ax, ay) + b"\x00")), msg, good, UNSUP)
    k384 = os.path.join(tmp, "k384.pem")
    ossl("ecparam", "-name", "secp384r1", "-genkey", "-noout", "-out", k384)
    case("id_p384", ser(ossl("ec", "-in", k384, "-pubout")), msg, good, UNSUP)
    case("id_p384_cert", ser(ossl("req", "-new", "-x509", "-key", k384, "-subj", "/CN=p384", "-days", "3650")),
         msg, good, UNSUP)
    krsa = os.path.join(tmp, "rsa.pem")
    ossl("genrsa", "-out", krsa, "2048")
    case("id_rsa", ser(ossl("rsa", "-in", krsa, "-pubout")), msg, good, UNSUP)
    case("id_private_key_block", ser(ossl("pkcs8", "-topk8", "-nocrypt", "-in", kp)), msg, good, UNSUP)
    case("id_ec_private_key_block", ser(open(kp, "rb").read()), msg, good, UNSUP)
    first, rest = pub_pem.split(b"\n", 1)
    case("id_pem_headers", ser(first + b"\nComment: auditor\n\n" + rest), msg, good, UNSUP)
    case("id_pem_leading_garbage", ser(b"junk\n" + pub_pem), msg, good, UNSUP)
    case("id_pem_crlf", ser(pub_pem.replace(b"\n", b"\r\n")), msg, good, UNSUP)
    case("id_pem_trailing_text", ser(pub_pem + b"more\n"), msg, good, UNSUP)
    case("id_pem_no_final_newline", ser(pub_pem[:-1]), msg, good, OK)
    case("id_cert_truncated_der", ser(pem("CERTIFICATE", R.pem_block(cert_pem)[1][:-7])), msg, good, UNSUP)
    # an identity failure comes before the signature is looked at
    case("id_off_curve_bad_sig", ser(pem("PUBLIC KEY", R.spki_der(ax, y_bad))), msg, b"", IDENT)

    out = {"about": "generated by tests/gen_ecdsa_golden.py (openssl + p256_ref); codes: 0 accept, 10 signature, "
                    "11 verify in Go, 13 identity", "keys": keys, "cases": cases}
    path = os.path.join(HERE, "golden", "ecdsa_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases, %d keys, %d bytes" % (len(cases), len(keys), os.path.getsize(path)))


if __name__ == "__main__":
    main()
