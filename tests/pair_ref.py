"""Jobs and references for the pairing stage on the device
(csrc/tools/devpair.hip, tests/test_gpu_pair_stage.py).

A job pairs P1 with the fixed Q and R with t' = sum s_f B_f.  Every point is a
known multiple of its generator -- P1 = a G1, Q = q G2, R = r G1, B_f = b_f G2
-- so by bilinearity the exact GT value is g^(a q + r t mod R) with t = sum s_f
b_f and g = pairing(G1_GEN, G2_GEN): one pairing per module, independent of the
oracle's Miller loop.  The Fuentes-Castaneda variant holds that value to the
power 2 X (6 X^2 + 3 X + 1).  The prover's three fixed pairs give g^(c q + a k1
+ b k2).  The product's order of pairs and the absence of any sign are the
pipeline's: dev/jobs.h job_miller is miller_2(qlines(Q), P1, R, t'), and
tests/test_pair_ref.py checks the reference against that code on the CPU.
"""
import functools
import random
import struct

from ftsoracle import bn254 as C

P, R = C.P, C.R
R256 = 1 << 256
GAP, STRIDE = 64, 448          # devpair.hip DP_GAP, DP_STRIDE: job j's 384 GT bytes at GAP + j * STRIDE
FUENTES = 2 * C.X * (6 * C.X * C.X + 3 * C.X + 1)
JOB_COUNTS = (1, 10, 11, 21)   # one sextet, a full wave, a second workgroup of one job, a third of one job
N_JOBS = 21


def mont_words(v):
    v = v * R256 % P
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def g1_words(p):
    return struct.pack("<16I", *((mont_words(p[0]) + mont_words(p[1])) if p else [0] * 16))


def g2_words(p):
    return struct.pack("<32I", *(mont_words(p[0][0]) + mont_words(p[0][1]) + mont_words(p[1][0]) + mont_words(p[1][1])))


def g1_of(k):
    return C.g1_mul(C.G1_GEN, k) if k % R else None


@functools.lru_cache(maxsize=None)
def _g_powers():
    """g^(2^i), g = pairing(G1_GEN, G2_GEN) with the exact final exponentiation"""
    out = [C.pairing(C.G1_GEN, C.G2_GEN, C.FE_EXACT)]
    for _ in range(R.bit_length() - 1):
        out.append(C.f12_sqr(out[-1]))
    return out


@functools.lru_cache(maxsize=None)
def gt_bytes_of(e, exact=True):
    """the GT bytes of g^e (exact) or of that value to the Fuentes-Castaneda power"""
    e = (e if exact else e * FUENTES) % R
    f = C.F12_ONE
    for i, gp in enumerate(_g_powers()):
        if (e >> i) & 1:
            f = C.f12_mul(f, gp)
    return C.gt_bytes(f)


class PairJobs:
    """N_JOBS two-pair jobs: (kind, a, r, nfix, scalar indices) and the secrets behind the points"""

    # job 0 alone (n = 1), job 9 (the sextet the ghost lanes shadow), job 10 (alone in the second workgroup at
    # n = 11) and job 20 (alone in the third at n = 21) are the unity cases
    KINDS = ["cancel", "near", "random", "p1_inf", "r_inf", "t_inf", "all_inf", "random", "random", "cancel",
             "cancel", "random", "all_inf", "p1_r_inf", "random", "near", "t_inf", "random", "p1_inf", "random", "near"]

    def __init__(self):
        rng = random.Random("pair-stage")
        self.q = rng.randrange(1, R)
        self.b = [rng.randrange(1, R) for _ in range(4)]
        self.scal = [0] + [rng.randrange(1, R) for _ in range(15)]
        self.jobs = []
        for j, kind in enumerate(self.KINDS):
            nfix = 1 + j % 3
            s = [rng.randrange(1, len(self.scal)) for _ in range(3)]
            a, r = rng.randrange(1, R), rng.randrange(1, R)
            if kind in ("t_inf", "all_inf"):
                s = [0, 0, 0]
            if kind in ("p1_inf", "all_inf", "p1_r_inf"):
                a = 0
            if kind in ("r_inf", "all_inf", "p1_r_inf"):
                r = 0
            t = sum(self.scal[s[f]] * self.b[f] for f in range(nfix)) % R
            if kind in ("cancel", "near"):  # a q + r t = 0, or = 1 (the exponent off by one), no point at infinity
                a = ((kind == "near") - r * t) * pow(self.q, -1, R) % R
                assert a and r and t
            self.jobs.append((kind, a, r, nfix, s, (a * self.q + r * t) % R))
        assert len(self.jobs) == N_JOBS
        self.Q = C.g2_mul(C.G2_GEN, self.q)
        self.bases = [C.g2_mul(C.G2_GEN, b) for b in self.b]
        self.p1 = [g1_of(j[1]) for j in self.jobs]
        self.pts = [g1_of(j[2]) for j in self.jobs]

    def exponent(self, j):
        return self.jobs[j][5]

    def unity(self, j):
        return 1 if self.exponent(j) == 0 else 0

    def packed(self, n, start=0):
        """ftz_devcheck_pair_jobs' arrays for the n jobs from `start` on"""
        sel = slice(start, start + n)
        jw = b"".join(struct.pack("<5I", nfix, *s, j) for j, (_, _, _, nfix, s, _) in enumerate(self.jobs[sel]))
        return dict(q=g2_words(self.Q), p1=b"".join(g1_words(p) for p in self.p1[sel]), jobs=jw,
                    bases=b"".join(g2_words(b) for b in self.bases), n_scal=len(self.scal),
                    scal=b"".join(struct.pack("<8I", *[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]) for k in self.scal),
                    n_pts=n, pts=b"".join(g1_words(p) for p in self.pts[sel]))


class Pair3Jobs:
    """N_JOBS jobs of the prover's three fixed pairs: f(C, Q) f(A, PK1) f(B, PK2)"""

    KINDS = ["cancel", "near", "random", "c_inf", "a_inf", "b_inf", "all_inf", "random", "random", "cancel",
             "cancel", "random", "all_inf", "random", "random", "near", "c_inf", "random", "b_inf", "random", "near"]

    def __init__(self):
        rng = random.Random("pair3-stage")
        self.k = [rng.randrange(1, R) for _ in range(3)]  # Q, PK1, PK2
        self.jobs = []
        for kind in self.KINDS:
            m = [rng.randrange(1, R) for _ in range(3)]   # C, A, B
            if kind == "all_inf":
                m = [0, 0, 0]
            elif kind.endswith("_inf"):
                m["cab".index(kind[0])] = 0
            if kind in ("cancel", "near"):
                m[0] = ((kind == "near") - (m[1] * self.k[1] + m[2] * self.k[2])) * pow(self.k[0], -1, R) % R
                assert m[0]
            self.jobs.append((kind, m, sum(x * y for x, y in zip(m, self.k)) % R))
        assert len(self.jobs) == N_JOBS
        self.q3 = [C.g2_mul(C.G2_GEN, k) for k in self.k]
        self.pts3 = [[g1_of(x) for x in m] for _, m, _ in self.jobs]

    def exponent(self, j):
        return self.jobs[j][2]

    def unity(self, j):
        return 1 if self.exponent(j) == 0 else 0

    def packed(self, n, start=0):
        return dict(q3=b"".join(g2_words(q) for q in self.q3),
                    pts3=b"".join(g1_words(p) for t in self.pts3[start:start + n] for p in t))


@functools.lru_cache(maxsize=None)
def pair_jobs():
    return PairJobs()


@functools.lru_cache(maxsize=None)
def pair3_jobs():
    return Pair3Jobs()


STARTS = {1: (0, 1, 2)}  # a single job is run three times: a cancelling product, its neighbour, a random job


def check_outputs(jobs, n, exact, unity, arena, ok, guard, what, start=0):
    """one call's outputs against the references (the n jobs from `start` on): their GT bytes or unity bytes,
    every other byte untouched"""
    slots = -(-n // 10) * 10
    assert len(arena) == GAP + slots * STRIDE and len(ok) == slots
    assert guard == 0, what + ": guard %d (1: an F12 value past n, 2: a ghost lane's park entry)" % guard
    for j in range(slots):
        got = arena[GAP + j * STRIDE:GAP + j * STRIDE + 384]
        if j < n and not unity:
            assert got == gt_bytes_of(jobs.exponent(start + j), exact), \
                "%s: GT bytes of job %d (%s)" % (what, start + j, jobs.jobs[start + j][0])
        else:
            assert got == b"\xa5" * 384, "%s: arena place of sextet %d written" % (what, j)
        gap = arena[GAP + j * STRIDE + 384:GAP + (j + 1) * STRIDE]
        assert gap == b"\xa5" * GAP, "%s: bytes behind job %d changed" % (what, j)
        if j < n and unity:
            assert ok[j] == jobs.unity(start + j), \
                "%s: unity byte of job %d (%s)" % (what, start + j, jobs.jobs[start + j][0])
        else:
            assert ok[j] == 0xA5, "%s: unity byte of sextet %d written" % (what, j)
    assert arena[:GAP] == b"\xa5" * GAP
