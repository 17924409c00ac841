"""The variable-base G1 chain on the device (dev/jobs.h g1_mul_glv16_halves on
the carry-free form: window table in 29-bit limbs laid out [entry][job], empty
window steps skipped when a ballot finds no lane of the wave needing them)
through the devcheck tool, 130 lanes each time: two full waves and two lanes.

test_jobs_match_host_emulation runs k_g1_part + k_g1_combine themselves
(ftz_devcheck_g1_jobs) on 130 jobs: single points, the PP-A weights (100, 1),
a PP-B Horner, a VT_NEG term, jobs without a variable part, jobs whose variable
part is the sum of shared siblings (sh_count), vneg, and one lane with k = 0.
Every g1out entry must equal the host build's job_g1 word for word.

test_halves_match_host_emulation runs the window loop on chosen GLV halves
(ftz_devcheck_g1_chain).  A non-zero digit in window 32 needs a half of at
least 2^127, which no scalar reaches through glv_split (its halves stay below
0.87 x 2^127), so that case cannot be given to k_g1_part as a job and is
given here: wave 0 holds exactly one lane with a window-32 digit and one lane
with both halves 0 (the skip of the top window is refused by that wave and
taken by waves 1 and 2); wave 2's two lanes have short halves, so their
accumulators stay at infinity over many windows and the doublings are skipped
wave-wide.  The device's affine points must equal the host build's word for
word, and both a big-integer double-and-add.
"""
import ctypes
import os
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftsdevcheck.so")
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R256 = 1 << 256
NONE = 0xFFFFFFFF
VT_HORNER, VT_NEG = 1, 2
N = 130
INF = None


def add(a, b):
    if a is INF:
        return b
    if b is INF:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return INF
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(a):
    return INF if a is INF else (a[0], -a[1] % P)


def mul(k, a):
    acc = INF
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, a)
    return acc


def words(v, n=8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def mont(v):
    return words(v * R256 % P)


def aff_words(a):
    """a G1Dev: Montgomery x, y; all-zero for infinity"""
    return [0] * 16 if a is INF else mont(a[0]) + mont(a[1])


def booth16(k, i):
    v = ((k << 1) >> (4 * i)) & 31
    return (v & 1) + ((v >> 1) & 7) - 8 * (v >> 4)


@pytest.fixture(scope="module")
def devlib():
    lib = ctypes.CDLL(LIB)
    u32 = ctypes.c_uint32
    lib.ftz_devcheck_g1_chain.argtypes = [ctypes.c_int, u32, ctypes.c_char_p, ctypes.c_char_p]
    lib.ftz_devcheck_g1_jobs.argtypes = [ctypes.c_int, u32, ctypes.c_char_p, u32, ctypes.c_char_p, u32, ctypes.c_char_p,
                                         u32, ctypes.c_char_p, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def points():
    """a pool of curve points (multiples of the generator), shared by both tests"""
    rng = random.Random(0x6732)
    return [mul(rng.randrange(1, R), (1, 2)) for _ in range(24)]


def pack(ws):
    return struct.pack("<%dI" % len(ws), *ws)


def test_halves_match_host_emulation(devlib, points):
    rng = random.Random(0x6733)
    rows = []
    for j in range(N):
        k1, k2 = rng.randrange(1 << 127), rng.randrange(1 << 127)  # no digit in window 32
        if j == 3:
            k1 |= 1 << 127
        if j == 9:
            k1 = k2 = 0
        if j == 17:
            k1, k2 = (1 << 128) - 1, 0x78787878787878787878787878787878  # top digit and all +-8
        if j in (70, 71):
            k1 >>= 12 * (j - 69)
            k2 >>= 8
        if j >= 128:  # wave 2: nothing above window 21 in either lane
            k1 >>= 40 if j == 128 else 124
            k2 >>= 60 if j == 128 else 48
        z = rng.randrange(1, P) if j % 3 == 1 else 1
        rows.append((points[j % len(points)], z, k1, j & 1, k2, (j >> 1) & 1))
    assert [j for j, r in enumerate(rows) if booth16(r[2], 32) or booth16(r[4], 32)] == [3, 17]
    ins = []
    for (x, y), z, k1, n1, k2, n2 in rows:
        ins += mont(x * z * z % P) + mont(y * z * z * z % P) + mont(z) + words(k1, 4) + [n1] + words(k2, 4) + [n2]
    out = ctypes.create_string_buffer(N * 32 * 4)
    assert devlib.ftz_devcheck_g1_chain(0, N, pack(ins), out) == 0
    got = struct.unpack("<%dI" % (N * 32), out.raw)
    bad = [j for j in range(N) if got[32 * j:32 * j + 16] != got[32 * j + 16:32 * j + 32]]
    assert not bad, "device and host differ in %d of %d lanes, first %d" % (len(bad), N, bad[0])
    # big-integer reference: phi = lambda for one of the two primitive cube roots of unity mod r
    lam = next(w for w in (pow(g, (R - 1) // 3, R) for g in range(2, 50)) if w != 1)
    ok = {lam: 0, lam * lam % R: 0}
    for j, (pt, z, k1, n1, k2, n2) in enumerate(rows):
        for l in ok:
            want = mul(((-k1 if n1 else k1) + (-k2 if n2 else k2) * l) % R, pt)
            ok[l] += tuple(got[32 * j:32 * j + 16]) == tuple(aff_words(want))
    assert max(ok.values()) == N, ok
    assert tuple(got[32 * 9:32 * 9 + 16]) == (0,) * 16


def test_jobs_match_host_emulation(devlib, points):
    rng = random.Random(0x6734)
    scal = [rng.randrange(R) for _ in range(40)]
    scal[5] = 0
    scal[6] = 1
    scal[7] = R - 1
    jobs, vterms = [], []

    def job(terms, vscal, vneg=0, sh_first=0, sh_count=0):
        jobs.append((len(vterms), len(terms), vscal, vneg, sh_first, sh_count))
        vterms.extend(terms)

    for j in range(N):
        if j % 11 == 10:  # the sum of the three jobs before it, which share its scalar and sign
            s, vn = jobs[-1][2], jobs[-1][3]
            assert all(q[2] == s and q[3] == vn and q[1] == 1 for q in jobs[-3:])
            job([(vterms[q[0]][0], 1, 0, 0) for q in jobs[-3:]], s, vn, j - 3, 3)
        elif j % 11 in (7, 8, 9):  # siblings: one unit-weight point each
            job([(rng.randrange(len(points)), 1, 0, 0)], 20 + j // 11, (j // 11) & 1)
        elif j % 11 == 0:
            jobs.append((0, 0, NONE, 0, 0, 0))  # no variable part
        elif j % 11 == 1:  # PP-A: Horner with b = 100, two terms
            job([(rng.randrange(len(points)), 100, 0, VT_HORNER), (rng.randrange(len(points)), 100, 0, 0)], j % 40, j & 1)
        elif j % 11 == 2 and j < 30:  # PP-B: Horner with b = 16, 16 terms
            job([(rng.randrange(len(points)), 16, 0, VT_HORNER if t == 0 else 0) for t in range(16)], j % 40, 0)
        elif j % 11 == 3:  # explicit weights, the top one -2^63
            job([(rng.randrange(len(points)), 0, 1 << 31, VT_NEG), (rng.randrange(len(points)), 10000, 0, 0),
                 (rng.randrange(len(points)), 1, 0, 0)], j % 40, (j >> 2) & 1)
        else:
            job([(rng.randrange(len(points)), 1, 0, 0)], j % 40, (j >> 1) & 1)
    assert len(jobs) == N
    own = [j for j, q in enumerate(jobs) if q[2] != NONE and not q[5]]
    assert len(own) > 64 and any(jobs[j][2] == 5 for j in own[:64])  # k = 0 sits in the first wave of chains
    out = ctypes.create_string_buffer(N * 32 * 4)
    rc = devlib.ftz_devcheck_g1_jobs(0, N, pack([w for q in jobs for w in q]), len(vterms),
                                     pack([w for t in vterms for w in t]), len(points),
                                     pack([w for a in points for w in aff_words(a)]), len(scal),
                                     pack([w for s in scal for w in words(s)]), out)
    assert rc == 0
    got = struct.unpack("<%dI" % (N * 32), out.raw)
    bad = [j for j in range(N) if got[32 * j:32 * j + 16] != got[32 * j + 16:32 * j + 32]]
    assert not bad, "device and host differ in %d of %d jobs, first %d" % (len(bad), N, bad[0])
    # and a big-integer reference for every job
    for j, (vstart, vcount, vscal, vneg, _, sh_count) in enumerate(jobs):
        want = INF
        if vscal != NONE:
            terms = vterms[vstart:vstart + vcount]
            V = INF
            for i, (pt, w_lo, w_hi, flags) in enumerate(terms):
                c = terms[0][1] ** (vcount - 1 - i) if terms[0][3] & VT_HORNER else w_lo | (w_hi << 32)
                V = add(V, mul(c, neg(points[pt]) if flags & VT_NEG else points[pt]))
            want = mul(scal[vscal], neg(V) if vneg else V)
        assert tuple(got[32 * j:32 * j + 16]) == tuple(aff_words(want)), j
    assert sum(q[5] != 0 for q in jobs) >= 10 and sum(q[2] == NONE for q in jobs) >= 10
