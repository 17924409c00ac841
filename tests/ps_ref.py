"""Pointcheval-Sanders verification restated from pssign.SignVerifier.Verify
(crypto/pssign/sign.go:125-160) for one message, over ftsoracle.bn254:

    H = PK0 + m PK1 + h PK2
    e = FExp(Pairing2(Q, -S, H, R));  accept iff e is one in GT

h is an argument (the reference's callers pass hashMessages(m) = HashToZr of
m's 32 bytes, ftsoracle.zkat.ps_hash).  miller_loop skips a pair holding a
point at infinity, as gnark's does ([EXT] in bn254.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "py"))
from ftsoracle import bn254 as C  # noqa: E402
from ftsoracle import zkat as Z  # noqa: E402

R = C.R
P = C.P
OK, ERR_PARSE, ERR_PS = 0, 1, 14


def ps_verify(pp, m, h, Rp, Sp, variant=None):
    """True iff the reference returns nil.  m, h: ints (any size: G2 scalar
    multiplication is modulo the group order); Rp, Sp: affine points or None."""
    H = C.g2_add(C.g2_add(pp.sign_pk[0], C.g2_mul(pp.sign_pk[1], m % R)), C.g2_mul(pp.sign_pk[2], h % R))
    f = C.miller_loop([(C.g1_neg(Sp), pp.q), (Rp, H)])
    return C.f12_eq(C.final_exp(f, variant), C.F12_ONE)


def ps_code(pp, m, h, r_bytes, s_bytes, variant=None):
    """The per-item code of ftz_verify_ps_signatures for wire inputs: m, h as
    32 big-endian bytes, r, s as 64-byte gnark encodings."""
    try:
        Rp = C.g1_from_bytes(r_bytes)
        Sp = C.g1_from_bytes(s_bytes)
    except C.DecodeError:
        return ERR_PARSE
    return OK if ps_verify(pp, int.from_bytes(m, "big"), int.from_bytes(h, "big"), Rp, Sp, variant) else ERR_PS


def ps_sign(pp, m, r=1):
    """A signature on m under pp._sk with R = r G (setup signs with r = 1)."""
    sk = pp._sk
    e = (sk[0] + sk[1] * m + sk[2] * Z.ps_hash(m % (1 << 256))) % R
    Rp = C.g1_mul(C.G1_GEN, r % R)
    return Rp, C.g1_mul(Rp, e)
