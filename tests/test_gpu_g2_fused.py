"""The fused G2 formulas on the device (dev/g2x29.h q2_scan and x2q_madd,
dev/g2lines29.h g2l_dbl and g2l_add: one reduction per sum of Fp2 products,
linear terms folded into it) against the 32-bit device formulas (dev/pairing.h
dbl_step_inl / add_step_inl, dev/curve.h jac_add_aff on Fp2), through the G2 op
table of the devcheck tool (csrc/tools/devcheck_ops.h DC_G2_OPS): one operand
set per lane, both results written by the same lane.  The comparison is the one
of tests/native/g2fused_main.cpp: the new point is the reference's projectively
(cross-multiplied mod p), and a line is the reference's times one factor
lambda in Fp (lambda = one coefficient's ratio has a zero u-component, the two
other coefficients are lambda times the reference's).

Operands (the generator of g2fused_main.cpp restated): 4,096 random ones in
the representations the contracts accept, the edge cases of the addition (the
accumulator at infinity, P + P: the doubling flag, P + (-P)), and coordinates
at the extremes of the contracts (every limb +-2^28, limb 8 at its stated
maximum; the accumulator's ZZ and ZZZ are then z^2 and z^3 of an extreme z).
The formulas are polynomial identities in the coordinates, so the operands
need not lie on the curve.  n is not a multiple of the workgroup, and
the lanes past n must leave their output words alone.

test_stage_matches_32bit_host_code runs k_g2_part, k_g2_sum, k_g2_binv and
k_g2lines1 themselves as the pipeline launches them (ftz_devcheck_g2_jobs) on
130 jobs -- two waves and a partial one -- with one, two and three fixed terms,
all-zero scalars (t' at infinity), one R at infinity and scalars whose window
digits are negative: t' must equal the host's 32-bit code byte for byte, and
every line the 32-bit chain's up to its factor in Fp.

Then one 64-transfer PP-A verification through the C ABI against the golden
verdicts.
"""
import ctypes
import os
import random
import struct

import pytest

from conftest import case_tuple

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftsdevcheck.so")
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R261, R256 = 1 << 261, 1 << 256
B28, B29 = 1 << 28, 1 << 29
# limb 8 at the value bounds (p / 2^232 = 3171406.45): 0.7 p for a coordinate of T, 0.52 p for an affine operand or
# a coordinate of P, 2.2 p and 0.6 p for the accumulator of x2q_madd; less one for what the limbs below can add
IN_T, IN_AFF, IN_AX, IN_A = 2219983, 1649130, 6977093, 1902842
SENTINEL = 0xA5A5A5A5
N_RANDOM = 4096
MILLER_LINES, EVL_REC = 88, 10
C13, WINDOWS = 13, 20


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_eq(a, b):
    return (a[0] - b[0]) % P == 0 and (a[1] - b[1]) % P == 0


def f2_zero(a):
    return a[0] % P == 0 and a[1] % P == 0


def limbs(v):
    """the 9 balanced limbs of the integer v: limbs 0..7 in [-2^28, 2^28), limb 8 the signed rest"""
    out = []
    for _ in range(8):
        d = ((v + B28) % B29) - B28
        out.append(d)
        v = (v - d) >> 29
    return out + [v]


def rep(rng, a, kmax=0):
    """balanced limbs of a representative of the element a: a R mod p, centred, plus up to kmax multiples of p"""
    v = a * R261 % P
    if v > P // 2:
        v -= P
    return limbs(v + rng.randint(-kmax, kmax) * P)


def rep2(rng, a, kmax=0):
    return rep(rng, a[0], kmax) + rep(rng, a[1], kmax)


def elem2(ls):
    """the Fp2 element two limb vectors stand for (Montgomery radix 2^261)"""
    inv = pow(R261, -1, P)
    return tuple(sum(x << (29 * i) for i, x in enumerate(ls[9 * c:9 * c + 9])) * inv % P for c in range(2))


def rnd2(rng):
    return (rng.randrange(P), rng.randrange(P))


def corner(signs, top):
    return [(-B28 if (signs >> i) & 1 else B28) for i in range(8)] + [top]


def corner2(s0, s1, top0, top1):
    return corner(s0, top0) + corner(s1, top1)


def vectors():
    """[(inputs of g2f_dbl, g2f_add, g2f_xmadd, what the sum of the addition must be)]"""
    rng = random.Random(0x6732)
    rows = []

    def add(X, Y, Z, Qx, Qy, yP, xP, acc, inf=0, expect="finite"):
        rows.append((X + Y + Z + yP + xP, X + Y + Z + Qx + Qy + yP + xP, acc + [inf] + Qx + Qy, expect))

    def accumulator(x, y, z):
        zz = f2_mul(z, z)
        zzz = f2_mul(zz, z)
        # |X| <= 2.2 p: the centred value plus or minus p
        return rep2(rng, f2_mul(x, zz), 1) + rep2(rng, f2_mul(y, zzz)) + rep2(rng, zz) + rep2(rng, zzz)

    for _ in range(N_RANDOM):
        T = [rep2(rng, rnd2(rng)) for _ in range(3)]
        add(*T, rep2(rng, rnd2(rng)), rep2(rng, rnd2(rng)), rep(rng, rng.randrange(P)), rep(rng, rng.randrange(P)),
            accumulator(rnd2(rng), rnd2(rng), rnd2(rng)))
    for k in range(24):
        x, y, z = rnd2(rng), rnd2(rng), (rng.randrange(1, P), rng.randrange(P))
        T = [rep2(rng, rnd2(rng)) for _ in range(3)]
        P2 = [rep(rng, rng.randrange(P)), rep(rng, rng.randrange(P))]
        if k % 3 == 0:  # the accumulator at infinity: whatever its coordinates hold
            add(*T, rep2(rng, x), rep2(rng, y), *P2, accumulator(rnd2(rng), rnd2(rng), z), inf=1)
        elif k % 3 == 1:  # P + P
            add(*T, rep2(rng, x), rep2(rng, y), *P2, accumulator(x, y, z), expect="dbl")
        else:  # P + (-P)
            add(*T, rep2(rng, x), rep2(rng, y), *P2, accumulator(x, (-y[0], -y[1]), z), expect="inf")
    pats = [0x00, 0xFF, 0x55, 0xAA, 0x0F, 0xC3]
    for a in range(6):
        for b in range(6):
            for c in range(6):
                s = -1 if (a + c) & 1 else 1
                t, u = s * IN_T, s * IN_AFF
                # ZZ^3 = ZZZ^2 is what makes an XYZZ accumulator a point: ZZ = z^2, ZZZ = z^3 of an extreme z
                # (balanced), next to the extreme X and Y
                z = elem2(corner2(pats[b], pats[c], -s * IN_A, s * IN_A))
                zz = f2_mul(z, z)
                acc = (corner2(pats[a], pats[b], s * IN_AX, -s * IN_AX) + corner2(pats[c], pats[a], s * IN_A, s * IN_A)
                       + rep2(rng, zz) + rep2(rng, f2_mul(zz, z)))
                add(corner2(pats[a], pats[b], t, -t), corner2(pats[c], pats[a] ^ pats[b], -t, -t),
                    corner2(pats[b], pats[c], t, t), corner2(pats[c], pats[a], u, -u), corner2(pats[a] ^ 0xFF, pats[b], -u, u),
                    corner(pats[c], u), corner(pats[b], -u), acc)
    return rows


def words(ls):
    return [x & 0xFFFFFFFF for x in ls]


def fp2s(w, count):
    """count Fp2 values of 16 words each (c0 then c1)"""
    return [(sum(x << (32 * i) for i, x in enumerate(w[16 * c:16 * c + 8])),
             sum(x << (32 * i) for i, x in enumerate(w[16 * c + 8:16 * c + 16]))) for c in range(count)]


def hom_same(a, b):
    """(X : Y : Z) the same homogeneous projective point, neither the zero triple"""
    if all(f2_zero(c) for c in a) or all(f2_zero(c) for c in b):
        return False
    return all(f2_eq(f2_mul(a[i], b[j]), f2_mul(b[i], a[j])) for i, j in ((0, 2), (1, 2), (0, 1)))


def jac_same(a, b):
    (x1, y1, z1), (x2, y2, z2) = a, b
    if f2_zero(z1) or f2_zero(z2):
        return f2_zero(z1) and f2_zero(z2)
    za, zb = f2_mul(z1, z1), f2_mul(z2, z2)
    return f2_eq(f2_mul(x1, zb), f2_mul(x2, za)) and f2_eq(f2_mul(y1, f2_mul(zb, z2)), f2_mul(y2, f2_mul(za, z1)))


def line_same(got, want):
    """got = lambda want for one non-zero lambda in Fp"""
    k = max((i for i in range(3) if not f2_zero(want[i])), default=None)
    if k is None:
        return all(f2_zero(c) for c in got)
    t = f2_mul(got[k], (want[k][0], -want[k][1]))  # lambda N(want[k])
    if t[1] % P or not t[0] % P:
        return False
    return all(f2_eq(f2_mul(got[i], want[k]), f2_mul(got[k], want[i])) for i in range(3))


@pytest.fixture(scope="module")
def devlib():
    lib = ctypes.CDLL(LIB)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.ftz_devcheck_g2_info.argtypes = [ctypes.c_int, ctypes.c_char_p, u32p, u32p]
    lib.ftz_devcheck_g2.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p,
                                    ctypes.c_char_p]
    lib.ftz_devcheck_g2_jobs.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32,
                                         ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p,
                                         ctypes.c_char_p, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def rows():
    return vectors()


@pytest.mark.parametrize("op, name, nin, nout", [(0, "g2f_dbl", 72, 192), (1, "g2f_add", 108, 192),
                                                 (2, "g2f_xmadd", 109, 97)])
def test_fused_formula_matches_32bit_device_code(devlib, rows, op, name, nin, nout):
    buf, a, b = ctypes.create_string_buffer(32), ctypes.c_uint32(), ctypes.c_uint32()
    assert devlib.ftz_devcheck_g2_info(-1, buf, a, b) == 3
    devlib.ftz_devcheck_g2_info(op, buf, a, b)
    assert (buf.value.decode(), a.value, b.value) == (name, nin, nout)
    n, block = len(rows), 256
    assert n >= N_RANDOM + 64 and n % block  # a partial last workgroup
    ins = [words(r[op]) for r in rows]
    assert all(len(v) == nin for v in ins)
    packed = struct.pack("<%dI" % (n * nin), *[w for v in ins for w in v])
    lanes = -(-n // block) * block
    out = ctypes.create_string_buffer(lanes * nout * 4)
    assert devlib.ftz_devcheck_g2(0, op, n, block, packed, out) == 0
    got = struct.unpack("<%dI" % (lanes * nout), out.raw)
    assert all(w == SENTINEL for w in got[n * nout:]), "a lane past n wrote"
    bad = []
    for j, r in enumerate(rows):
        w = got[nout * j:nout * (j + 1)]
        if op < 2:
            v = fp2s(w, 12)
            ok = hom_same(v[0:3], v[6:9]) and line_same(v[3:6], v[9:12])
        else:
            v = fp2s(w, 6)
            if r[3] == "dbl":
                ok = w[96] == 1
            else:
                ok = w[96] == 0 and jac_same(v[0:3], v[3:6]) and f2_zero(v[2]) == (r[3] == "inf")
        if not ok:
            bad.append(j)
    assert not bad, "%s: %d of %d lanes differ, first %d" % (name, len(bad), n, bad[0])


def mont_words(v):
    v = v * R256 % P
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def sdigits(k):
    """the signed 13-bit window digits the table sums take"""
    out, carry = [], 0
    for w in range(WINDOWS):
        raw = ((k >> (C13 * w)) & ((1 << C13) - 1)) + carry
        carry = 0
        if raw > 1 << (C13 - 1):
            raw -= 1 << C13
            carry = 1
        out.append(raw)
    return out


def test_stage_matches_32bit_host_code(devlib):
    from ftsoracle import bn254 as C

    rng = random.Random(0x6733)
    n = 130
    bases = [C.g2_mul(C.G2_GEN, rng.randrange(1, R)) for _ in range(4)]
    pts = [C.g1_mul(C.G1_GEN, rng.randrange(1, R)) for _ in range(7)] + [None]  # the last R is at infinity
    scal = [0] + [rng.randrange(R) for _ in range(23)]
    assert any(d < 0 for k in scal for d in sdigits(k))
    jobs = []
    for j in range(n):
        nfix = 1 + j % 3
        s = [rng.randrange(1, len(scal)) for _ in range(3)]
        if j % 16 == 5:  # t' at infinity: every term's scalar is zero
            s = [0, 0, 0]
        jobs.append([nfix] + s + [len(pts) - 1 if j == 77 else rng.randrange(len(pts) - 1)])
    assert {q[0] for q in jobs} == {1, 2, 3}
    bw = b"".join(struct.pack("<32I", *(mont_words(b[0][0]) + mont_words(b[0][1]) + mont_words(b[1][0]) + mont_words(b[1][1])))
                  for b in bases)
    pw = b"".join(struct.pack("<16I", *((mont_words(p[0]) + mont_words(p[1])) if p else [0] * 16)) for p in pts)
    sw = b"".join(struct.pack("<8I", *[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]) for k in scal)
    jw = struct.pack("<%dI" % (5 * n), *[w for q in jobs for w in q])
    nl = MILLER_LINES * 6 * n * EVL_REC
    g2out = ctypes.create_string_buffer(n * 64 * 4)
    ld, lh = ctypes.create_string_buffer(nl * 4), ctypes.create_string_buffer(nl * 4)
    assert devlib.ftz_devcheck_g2_jobs(0, n, jw, bw, len(scal), sw, len(pts), pw, g2out, ld, lh) == 0
    out = struct.unpack("<%dI" % (n * 64), g2out.raw)
    dev, host = struct.unpack("<%di" % nl, ld.raw), struct.unpack("<%di" % nl, lh.raw)
    infs = 0
    for j, q in enumerate(jobs):
        assert out[64 * j:64 * j + 32] == out[64 * j + 32:64 * j + 64], "t' of job %d" % j
        tinf = not any(out[64 * j:64 * j + 32])
        assert tinf == all(scal[q[1 + f]] == 0 for f in range(q[0]))
        # t' of the first jobs against the oracle's sum of their terms
        if j < 5:
            want = None
            for f in range(q[0]):
                want = C.g2_add(want, C.g2_mul(bases[f], scal[q[1 + f]]))
            assert want is not None and not tinf
            assert list(out[64 * j:64 * j + 32]) == (mont_words(want[0][0]) + mont_words(want[0][1])
                                                      + mont_words(want[1][0]) + mont_words(want[1][1]))
        infs += tinf or q[4] == len(pts) - 1
    assert infs >= 9

    def coef(buf, s, c, j):
        o = ((s * 6 + c) * n + j) * EVL_REC
        assert buf[o + 9] == 0
        return sum(x << (29 * i) for i, x in enumerate(buf[o:o + 9]))

    bad = []
    for j in range(n):
        for s in range(MILLER_LINES):
            g = [(coef(dev, s, 2 * c, j), coef(dev, s, 2 * c + 1, j)) for c in range(3)]
            h = [(coef(host, s, 2 * c, j), coef(host, s, 2 * c + 1, j)) for c in range(3)]
            if not line_same(g, h):
                bad.append((j, s))
    assert not bad, "%d lines differ, first %r" % (len(bad), bad[0])


def test_pp_a_transfers_match_golden_verdicts(golden):
    import zkatdlog

    js = golden["pp_a"]["pp"].encode()
    cases = [c for c in golden["pp_a"]["cases"] if c["kind"] == "transfer"]
    sel = [k % len(cases) for k in range(64)]
    with zkatdlog.Context(js, device=0) as ctx:
        assert list(ctx.verify_transfers([case_tuple(cases[k]) for k in sel])) == [cases[k]["expect"] for k in sel]
