#!/usr/bin/env python3
"""Fixture maker for Pointcheval-Sanders verification
(tests/golden/ps_golden.json), from tests/ps_ref.py.

Parameters: ftsoracle.zkat.setup(base 8, exponent 2) under a fixed seed; the
secret key is kept in the file so that tests can sign fresh messages.  Every
case carries the wire inputs of one ftz_ps_sig (m, h: 32 bytes; r, s: 64 bytes,
hex) and the code ps_ref.ps_code gives it.

    python tests/gen_ps_golden.py
"""
import base64
import json
import os

import ps_ref as S

C, Z, R, P = S.C, S.Z, S.R, S.P
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = b"ps-golden-base8"


def b32(v):
    return int(v).to_bytes(32, "big")


def main():
    pp = Z.setup(8, 2, Z.Rand(SEED))
    cases = []

    def add(name, kind, m, h, r, s):
        """m, h: ints below 2^256; r, s: points, None, or 64 raw bytes"""
        rb = r if isinstance(r, bytes) else C.g1_bytes(r)
        sb = s if isinstance(s, bytes) else C.g1_bytes(s)
        code = S.ps_code(pp, b32(m), b32(h), rb, sb)
        assert code == S.ps_code(pp, b32(m), b32(h), rb, sb, C.FE_FUENTES)  # unity does not depend on the variant
        cases.append({"name": name, "kind": kind, "m": b32(m).hex(), "h": b32(h).hex(), "r": rb.hex(), "s": sb.hex(),
                      "code": code})
        return code

    sv = pp.signed_values
    for i in range(8):
        assert add("signed_value_%d" % i, "signed_value", i, Z.ps_hash(i), *sv[i]) == 0
    for k, r in enumerate((2, R - 1, 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766)):
        i = 1 + 2 * k
        assert add("randomized_%d" % k, "randomized", i, Z.ps_hash(i), C.g1_mul(sv[i][0], r), C.g1_mul(sv[i][1], r)) == 0
    for name, m in (("m_r_minus_1", R - 1), ("m_2_64", 1 << 64)):
        assert add(name, "fresh", m, Z.ps_hash(m), *S.ps_sign(pp, m, 7)) == 0
    assert add("m_off_by_one", "wrong_m", 4, Z.ps_hash(3), *sv[3]) == 14
    assert add("h_off_by_one", "wrong_h", 3, (Z.ps_hash(3) + 1) % R, *sv[3]) == 14
    assert add("s_negated", "s_negated", 5, Z.ps_hash(5), sv[5][0], C.g1_neg(sv[5][1])) == 14
    Rr, Sr = S.ps_sign(pp, 6, 11)
    assert add("r_s_swapped", "swapped", 6, Z.ps_hash(6), Sr, Rr) == 14
    assert add("s_of_other_index", "other_s", 3, Z.ps_hash(3), sv[3][0], sv[5][1]) == 14
    assert add("both_infinity", "both_infinity", 2, Z.ps_hash(2), None, None) == 0
    assert add("r_infinity", "r_infinity", 2, Z.ps_hash(2), None, sv[2][1]) == 14
    assert add("s_infinity", "s_infinity", 2, Z.ps_hash(2), sv[2][0], None) == 14
    # R compressed: X with the flag of its Y (10: the smaller root, 11: the larger), 32 ignored bytes after it
    for k, r in enumerate((3, 5)):
        Rp, Sp = S.ps_sign(pp, 4, r)
        big = Rp[1] > (-Rp[1]) % P
        comp = bytearray(b32(Rp[0]) + bytes(32))
        comp[0] |= 0xC0 if big else 0x80
        assert C.g1_from_bytes(bytes(comp)) == Rp
        assert add("r_compressed_%d" % k, "compressed", 4, Z.ps_hash(4), bytes(comp), Sp) == 0
    Rp, Sp = sv[1]
    assert add("r_off_curve", "off_curve", 1, Z.ps_hash(1), b32(Rp[0]) + b32((Rp[1] + 1) % P), Sp) == 1
    # coordinates >= p are reduced (fp.SetBytes); x + p, y + p must stay clear of the two flag bits
    r = 2
    while True:
        Rp, Sp = S.ps_sign(pp, 7, r)
        if Rp[0] + P < 1 << 254 and Rp[1] + P < 1 << 254:
            break
        r += 1
    assert add("r_coordinates_ge_p", "ge_p", 7, Z.ps_hash(7), b32(Rp[0] + P) + b32(Rp[1] + P), Sp) == 0
    assert add("m_h_plus_r", "plus_r", 6 + R, Z.ps_hash(6) + R, *sv[6]) == 0
    out = {"comment": "Pointcheval-Sanders verification (pssign.SignVerifier.Verify, sign.go:125-160); made by "
                      "tests/gen_ps_golden.py from tests/ps_ref.py; code: 0 accept, 1 FTZ_ERR_PARSE, "
                      "14 FTZ_ERR_PS_SIGNATURE",
           "seed": SEED.decode(), "base": 8, "exponent": 2, "sk": ["%064x" % k for k in pp._sk],
           "pp": base64.b64encode(pp.to_json()).decode(), "cases": cases}
    path = os.path.join(HERE, "golden", "ps_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
