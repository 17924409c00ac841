"""Vectors, Fp12 references and mutants for the sextet op table of
csrc/dev/devcheck_sx.h (DC_SX_OPS), as devcheck_ref.py is for DC_OPS.

A job's words are the tool's: an Fp value is 9 signed 29-bit limbs standing for
V = sum l_i 2^(29 i), the field value V / 2^261 mod p; an Fp2 value is c0 then
c1; an Fp12 value is lane k's Fp2 coefficient f_k of f = sum f_k w^k at word
18 k.  The map to the oracle's tower is dev/sextet.h's (f_0 = C0.B0, f_1 =
C1.B0, f_2 = C0.B1, ...: bn254._to_w / _from_w).  A reference decodes the words
to field values, computes with ftsoracle.bn254 (f12_mul, f12_inv, f12_frob,
f12_pow) and returns the six Fp2 values the lanes must hold: comparisons are
exact, value mod p against value mod p.

Representatives.  Every routine states what it accepts (dev/sx29.h); IN_BOUND
holds that bound in hundredths of p and the vectors push representatives to it:
values shifted by multiples of p up to the bound, limbs 0..7 at +2^28 and -2^28
in both sign patterns, values at +-(p - 1) / 2.  OUT_BOUND is what the header
states for the result (see the table); limbs 0..7 of every result are balanced.
"""
import functools
import random
import struct
from fractions import Fraction

from ftsoracle import bn254 as C

P = C.P
RADIX = 1 << 261
RINV = pow(RADIX, -1, P)
B28 = 1 << 28
SENTINEL = 0xA5A5A5A5
TOP_P = P >> 232  # limb 8 of p
N_JOBS = 153      # per op: fifteen full workgroups of ten sextets and one of three
JOB_COUNTS = (1, 10, 11, 23)  # one sextet, a full wave, a second workgroup of one job, a partial third

F12, LINE, OUT = 108, 54, 108
# name -> words per job (the header's table: test_every_sx_op_has_vectors)
NIN = {"sx_mulv": 2 * F12, "sx_mulv24": 2 * F12, "sx_sqr": F12, "sx_cyc_sqr": F12, "sx_inv": F12, "sx_conj": F12,
       "sx_frob1": F12, "sx_frob2": F12, "sx_frob3": F12, "sx_mul_line_r": F12 + LINE,
       "sx_fixed_line": F12 + LINE + 19, "sx_fixed_line_n": F12 + LINE + 19, "sx_expt": F12, "sx_fexp_easy": F12,
       "sx_miller3": F12 + 6 * LINE + 19, "sx_xpow_turn": 2 * F12}
# (LDS slots, slot of the second operand's group): the layout each op runs in
LAYOUT = {n: (30, 18) for n in NIN}
LAYOUT.update({n: (24, 12) for n in ("sx_mulv24", "sx_cyc_sqr", "sx_expt", "sx_xpow_turn")})
LAYOUT.update({n: (18, 18) for n in ("sx_sqr", "sx_mul_line_r", "sx_fixed_line", "sx_fixed_line_n", "sx_miller3")})

# What the Fp12 operand f may be, in hundredths of p (dev/sx29.h):
#   100  the routines of the final exponentiation take operands within 1 p (sx29.h opening comment and sq_mul)
#   72   sq_expt raises a parked value, <= 0.72 ("Value bounds of the final exponentiation")
#   52   sq_inv / sq_fexp_easy start from q2_from_fp2 of the Miller value: p/2 + e, taken as 0.52 p (fp29.h:354-356)
#   68   sq_sqr in the verifier chain squares the line product's m <= 0.68 (sq_fixed_line_sum's comment)
#   78   the fixed lines take sq_sqr's result <= 0.78 (same comment)
#   300  sq_mul_line_r takes the unreduced sum of sq_fixed_line_sum, |g| <= 3 (same comment)
IN_BOUND = {n: 100 for n in NIN}
IN_BOUND.update({"sx_expt": 72, "sx_inv": 52, "sx_fexp_easy": 52,
                 "sx_sqr": 68, "sx_miller3": 68, "sx_fixed_line": 78, "sx_fixed_line_n": 78, "sx_mul_line_r": 300})
REDUCED = 52  # a second operand, a line coefficient, a multiplicand: reduced values


def _pb(n, a, b):
    """A reduced sum of n field products of operands within a p and b p (xi-wrapped ones counted ten times):
    |r| <= 1/2 + n a b p / R with p / R < 1 / 168.9 (sx29.h, opening comment)."""
    return Fraction(1, 2) + n * Fraction(a) * Fraction(b) / Fraction("168.9")


_LIN = Fraction(1, 2) + Fraction(2, 10809)  # f29_lin2 / f29_lin4: p/2 + 2^-13.4 p (fp29.h:354, test_sx_bounds.py)
# |value| of a result in units of p, each from the comment of dev/sx29.h it cites.  M(a, b) = 1/2 + 102 a b / 168.9
# is the bound written at sq_mul (lane 0: 2 + 10 x 10 field products of |a| |b|)
OUT_BOUND = {
    "sx_mulv": _pb(102, 1, 1), "sx_mulv24": _pb(102, 1, 1),   # sq_mul's comment, operands of 1 p
    "sx_inv": Fraction(66, 100),        # "Value bounds of the final exponentiation": f^-1 = M(L, 0.51) = 0.66
    "sx_fexp_easy": Fraction(72, 100),  # same table: m = M(0.506, 0.70) = 0.72
    "sx_expt": Fraction(72, 100),       # same table: the result of sq_expt of a <= 0.72
    "sx_xpow_turn": _pb(102, _LIN, 1),  # sq_cyc_sqr's L, then sq_mul by b <= 1
    "sx_sqr": _pb(102, "0.68", "0.68"),               # sq_fixed_line_sum's comment: 1/2 + 102 a^2 / 168.9 (<= 0.78)
    "sx_cyc_sqr": _LIN,                                # f29_lin4 (the last line of sq_cyc_sqr)
    "sx_conj": Fraction(1),                            # the operand's own bound
    "sx_frob1": _pb(2, 1, _LIN), "sx_frob2": _pb(2, 1, _LIN), "sx_frob3": _pb(2, 1, _LIN),  # F(a): one Fp2 product
    "sx_mul_line_r": _pb(42, "0.52", 3),               # same comment: 1/2 + 2 x 0.52 (1 + 10 + 10) |g| / 168.9
    "sx_fixed_line": _pb(42, "0.52", "0.78"),
    "sx_fixed_line_n": Fraction("1.123") * Fraction("0.78") + Fraction(1, 2),  # same comment: |g| <= 1.123 |f| + 1/2
    "sx_miller3": Fraction(68, 100),                   # same comment: the chain ends on m <= 0.68
}
PASSES_OPERAND = ("sx_conj", "sx_fixed_line_n")  # sq_conj negates or returns f; sq_fixed_line_n returns f when inf
LIMB8_BOUND = {"sx_fixed_line_n": 1 << 24, "sx_miller3": 1 << 24}  # sq_fixed_line_sum's comment: |g| <= 3 means |limb 8| < 2^24


# ------------------------------------------------------------------ words
def s32(w):
    return w - (1 << 32) if w & 0x80000000 else w


def val(limbs):
    return sum(v << (29 * i) for i, v in enumerate(limbs))


def limbs_of(v):
    """the balanced form of the integer v: limbs 0..7 in [-2^28, 2^28), limb 8 the signed rest"""
    out = []
    for _ in range(8):
        lo = ((v + B28) & ((1 << 29) - 1)) - B28
        out.append(lo)
        v = (v - lo) >> 29
    return out + [v]


def centered(v):
    v %= P
    return v - P if v > P // 2 else v


def mont(v):
    """the centered integer that stands for the field value v"""
    return centered(v * RADIX)


def dec(limbs):
    return val(limbs) * RINV % P


def reps(v, bound):
    """every integer congruent to mont(v) within bound / 100 p"""
    c = mont(v)
    return [c + m * P for m in range(-4, 5) if 100 * abs(c + m * P) <= bound * P]


def enc(v, bound, mode, rng):
    """limbs of the field value v: 'c' centred, 'far' the representative of largest magnitude within the bound,
    'rnd' any of them"""
    if mode == "c":
        return limbs_of(mont(v))
    r = reps(v, bound)
    return limbs_of(max(r, key=abs) if mode == "far" else rng.choice(r))


def edge_limbs(signs, top):
    """limbs 0..7 at +2^28 or -2^28 by the bits of signs, limb 8 = top"""
    return [(-B28 if (signs >> i) & 1 else B28) for i in range(8)] + [top]


def rd_fp(words, off):
    return dec([s32(w) for w in words[off:off + 9]])


def rd_q2(words, off):
    return (rd_fp(words, off), rd_fp(words, off + 9))


def rd_f12(words, off):
    return [rd_q2(words, off + 18 * k) for k in range(6)]


def pack(words):
    return struct.pack("<%dI" % len(words), *[w & 0xFFFFFFFF for w in words])


# ------------------------------------------------------------------ Fp12 in the w-power basis
W_ZERO = [C.F2_ZERO] * 6
W_ONE = [C.F2_ONE] + [C.F2_ZERO] * 5


def w_unit(k):
    return [C.F2_ONE if i == k else C.F2_ZERO for i in range(6)]


def tow(c):
    return C._from_w(list(c))


def wco(a):
    return [tuple(x) for x in C._to_w(a)]


def w_mul(a, b, drop=None, swap=None):
    """schoolbook product over w (dev/sextet.h: c_k = sum a_i b_(k-i), xi on the wrapped terms).  drop = (i, j):
    the xi of that wrapped term left out (a wrong entry of the wrap table)"""
    out = [C.F2_ZERO] * 6
    for i in range(6):
        for j in range(6):
            t = C.f2_mul(a[i], b[j])
            if i + j >= 6 and (i, j) != drop:
                t = C.f2_mul_xi(t)
            out[(i + j) % 6] = C.f2_add(out[(i + j) % 6], t)
    return out


def w_conj(a, keep=None):
    """conjugation over Fp6: odd lanes negated (keep: that odd lane's sign forgotten)"""
    return [C.f2_neg(x) if (k & 1) and k != keep else x for k, x in enumerate(a)]


@functools.lru_cache(maxsize=None)
def gamma(n, k):
    """the constant of lane k in the n-th Frobenius: (w^k)^(p^n) = gamma w^k"""
    return wco(C.f12_frob(tow(w_unit(k)), n))[k]


def w_frob(a, n, wrong=None):
    """lane k: conj^n(a_k) gamma(n, k) (wrong = (k, k2): lane k takes lane k2's constant)"""
    out = []
    for k, x in enumerate(a):
        g = gamma(n, wrong[1] if wrong and wrong[0] == k else k)
        out.append(C.f2_mul(C.f2_conj(x) if n & 1 else x, g))
    return out


def w_line(l0, l1, l3):
    return [l0, l1, C.F2_ZERO, l3, C.F2_ZERO, C.F2_ZERO]


def cyclotomic(f):
    """the easy part f^((p^6 - 1)(p^2 + 1)), tower form"""
    m = C.f12_mul(C.f12_conj(f), C.f12_inv(f))
    return C.f12_mul(C.f12_frob(m, 2), m)


# ------------------------------------------------------------------ references (words -> six Fp2 values)
def _fixed(words, off, f, normalised, mul=w_mul):
    r0, r1, r2 = (rd_q2(words, off + 18 * i) for i in range(3))
    u, v, inf = rd_fp(words, off + LINE), rd_fp(words, off + LINE + 9), words[off + LINE + 18] != 0
    if inf:
        return f
    if normalised:  # 1 + r1 xq w + r2 yi w^3
        return mul(f, w_line(C.F2_ONE, C.f2_muls(r1, u), C.f2_muls(r2, v)))
    return mul(f, w_line(C.f2_muls(r0, u), C.f2_muls(r1, v), r2))  # r0 yP + r1 xP w + r2 w^3


def _t_mul(a, b):
    return wco(C.f12_mul(tow(a), tow(b)))


def gs_sqr(a, no_xi=None):
    """Granger-Scott squaring as sq_cyc_sqr computes it: a polynomial map of ANY Fp12 operand, the square for a
    cyclotomic one.  The Fp4 pairs are (a_p, a_(p+3)): the even lane 2 p holds 3 (a_p^2 + xi a_(p+3)^2) - 2 a_(2p),
    the pair's odd lane k = 3, 5, 1 holds 6 q + 2 a_k with q = a_p a_(p+3), times xi on lane 1.
    no_xi: the lane whose xi is left out (a wrong lane select)"""
    out = [None] * 6
    for p, k in ((0, 3), (1, 5), (2, 1)):
        u, v = a[p], a[p + 3]
        vv = C.f2_sqr(v)
        even = C.f2_add(C.f2_sqr(u), vv if no_xi == 2 * p else C.f2_mul_xi(vv))
        out[2 * p] = C.f2_sub(C.f2_muls(even, 3), C.f2_muls(a[2 * p], 2))
        q = C.f2_mul(u, v)
        if k == 1 and no_xi != 1:
            q = C.f2_mul_xi(q)
        out[k] = C.f2_add(C.f2_muls(q, 6), C.f2_muls(a[k], 2))
    return out


def ref(name, words, mul=_t_mul, conj=w_conj, frob=None, cyc=gs_sqr):
    """mul / conj / frob / cyc: the pieces a mutant replaces"""
    a = rd_f12(words, 0)
    fr = frob or (lambda x, n: wco(C.f12_frob(tow(x), n)))
    if name in ("sx_mulv", "sx_mulv24"):
        return mul(a, rd_f12(words, F12))
    if name == "sx_sqr":
        return mul(a, a)
    if name == "sx_cyc_sqr":
        return cyc(a)
    if name == "sx_inv":
        return wco(C.f12_inv(tow(a)))
    if name == "sx_conj":
        return conj(a)
    if name in ("sx_frob1", "sx_frob2", "sx_frob3"):
        return fr(a, int(name[-1]))
    if name == "sx_mul_line_r":
        return mul(a, w_line(*(rd_q2(words, F12 + 18 * i) for i in range(3))))
    if name in ("sx_fixed_line", "sx_fixed_line_n"):
        return _fixed(words, F12, a, name == "sx_fixed_line_n", mul)
    if name == "sx_expt":
        return wco(C.f12_pow(tow(a), C.X))
    if name == "sx_fexp_easy":
        m = mul(conj(a), wco(C.f12_inv(tow(a))))
        return mul(fr(m, 2), m)
    if name == "sx_miller3":
        tail = F12 + 6 * LINE
        f = a
        for t in range(3):
            s = F12 + t * 2 * LINE
            f = mul(f, f)
            f = _fixed(list(words[s:s + LINE]) + list(words[tail:tail + 19]), 0, f, True, mul)
            f = mul(f, w_line(*(rd_q2(words, s + LINE + 18 * i) for i in range(3))))
        return f
    assert name == "sx_xpow_turn", name
    return conj(mul(conj(cyc(a)), rd_f12(words, F12)))


def _swapped(i, j):
    def m(name, words):
        out = list(ref(name, words))
        out[i], out[j] = out[j], out[i]
        return out
    return m


def _swapped_in(i, j):
    """lanes i and j of the first operand exchanged (two regions' or two lanes' slots mixed up)"""
    def m(name, words):
        w = list(words)
        w[18 * i:18 * i + 18], w[18 * j:18 * j + 18] = words[18 * j:18 * j + 18], words[18 * i:18 * i + 18]
        return ref(name, w)
    return m


WRAPPED = [(i, j) for i in range(6) for j in range(6) if i + j >= 6]
_MULS = ("sx_mulv", "sx_mulv24", "sx_sqr", "sx_mul_line_r", "sx_fixed_line", "sx_fixed_line_n",
         "sx_miller3", "sx_xpow_turn", "sx_fexp_easy")
# (op, what, mutant(name, words) -> six Fp2 values): the op's vectors must tell each from the reference
MUTANTS = []
for _n in NIN:
    MUTANTS.append((_n, "result lanes 1 and 3 swapped", _swapped(1, 3)))
    MUTANTS.append((_n, "result lanes 0 and 4 swapped", _swapped(0, 4)))
    MUTANTS.append((_n, "operand lanes 2 and 5 swapped", _swapped_in(2, 5)))
for _n in ("sx_mulv", "sx_mulv24"):  # every entry of the wrap table
    for _d in WRAPPED:
        MUTANTS.append((_n, "xi dropped on a_%d b_%d" % _d,
                        lambda name, words, d=_d: ref(name, words, mul=lambda a, b: w_mul(a, b, drop=d))))
for _n in _MULS:
    if _n in ("sx_mul_line_r", "sx_fixed_line", "sx_fixed_line_n", "sx_miller3"):
        _ds = [(5, 1), (3, 3), (4, 3)]  # the line has coefficients 0, 1 and 3 only
    else:
        _ds = [(5, 1), (3, 3), (2, 4)]
    for _d in _ds:
        MUTANTS.append((_n, "xi dropped on a_%d b_%d" % _d,
                        lambda name, words, d=_d: ref(name, words, mul=lambda a, b: w_mul(a, b, drop=d))))
for _n in ("sx_cyc_sqr", "sx_xpow_turn"):  # the pair and lane map of sq_cyc_sqr
    for _k in (0, 1, 2, 4):
        MUTANTS.append((_n, "xi left out on lane %d of the cyclotomic squaring" % _k,
                        lambda name, words, k=_k: ref(name, words, cyc=lambda a: gs_sqr(a, no_xi=k))))
for _n in ("sx_conj", "sx_xpow_turn", "sx_fexp_easy"):
    for _k in (1, 3, 5):
        MUTANTS.append((_n, "conjugation sign forgotten on lane %d" % _k,
                        lambda name, words, k=_k: ref(name, words, conj=lambda a: w_conj(a, keep=k))))
for _n in ("sx_frob1", "sx_frob2", "sx_frob3", "sx_fexp_easy"):
    for _k in range(1, 6):  # lane 0's constant is one in every power
        MUTANTS.append((_n, "Frobenius constant of lane %d on lane %d" % ((_k + 1) % 6, _k),
                        lambda name, words, k=_k: ref(name, words, frob=lambda a, n: w_frob(a, n, (k, (k + 1) % 6)))))


# ------------------------------------------------------------------ vectors
def _rand_fp2(rng):
    return (rng.randrange(P), rng.randrange(P))


def _rand_w(rng):
    return [_rand_fp2(rng) for _ in range(6)]


def _structured(rng):
    """(label, element): 0, 1, -1, elements of Fp, Fp2 and Fp6 (odd lanes zero), w^k"""
    z = C.F2_ZERO
    out = [("zero", list(W_ZERO)), ("one", list(W_ONE)), ("minus_one", [(P - 1, 0)] + [z] * 5),
           ("fp", [(rng.randrange(1, P), 0)] + [z] * 5), ("fp2", [_rand_fp2(rng)] + [z] * 5),
           ("fp6", [_rand_fp2(rng), z, _rand_fp2(rng), z, _rand_fp2(rng), z])]
    return out + [("w^%d" % k, w_unit(k)) for k in range(6)]


def _near_half(rng):
    """a field value whose centred integer lies within 0.02 p of +-p/2: it has two representatives within 0.52 p"""
    v = rng.choice((1, -1)) * (P // 2 - rng.randrange(P // 50))
    return v * RINV % P


def enc_q2(x, bound, mode, rng):
    return enc(x[0], bound, mode, rng) + enc(x[1], bound, mode, rng)


def enc_f12(a, bound, mode, rng):
    out = []
    for x in a:
        out += enc_q2(x, bound, mode, rng)
    return out


def edge_f12(rng, bound):
    """every limb 0..7 of every coefficient at +-2^28 (all +, all -, both alternations), limb 8 up to the bound"""
    top = bound * TOP_P // 100 - 2 if bound > 52 else TOP_P // 2 - 1
    out = []
    for _ in range(12):
        signs = rng.choice((0x00, 0xFF, 0x55, 0xAA))
        out += edge_limbs(signs, rng.choice((top, -top, rng.randrange(-top, top + 1))))
    return out


def _operands(name, rng, cyc):
    """N_JOBS encodings of the op's Fp12 operand f (label, 108 words)"""
    bound = IN_BOUND[name]
    out = []
    if name == "sx_expt":  # a power is only checked on cyclotomic values, which cannot be chosen limb by limb
        out.append(("one", enc_f12(W_ONE, bound, "c", rng)))
    else:
        if cyc:
            # sq_cyc_sqr is a polynomial map (gs_sqr), so any operand is a test: every limb 0..7 of a_p and a_(p+3)
            # at the same extreme, so that the even lanes' sums a_p + a_(p+3) have every limb at +-2^29
            top = bound * TOP_P // 100 - 2
            for s, signs in enumerate((0x00, 0xFF, 0x55, 0xAA)):
                for t in (top, -top):
                    out.append(("pairs%d%s" % (s, "+" if t > 0 else "-"), edge_limbs(signs, t) * 12))
        for lab, a in _structured(rng):
            if lab == "zero" and name in ("sx_inv", "sx_fexp_easy"):
                continue  # no inverse
            out.append((lab, enc_f12(a, bound, "c", rng)))
            far = enc_f12(a, bound, "far", rng)
            if far != out[-1][1]:
                out.append((lab + "/far", far))
        for s in range(6):
            out.append(("edge%d" % s, edge_f12(rng, bound)))
        for s in range(6):
            out.append(("half%d" % s, enc_f12([(_near_half(rng), _near_half(rng)) for _ in range(6)], bound,
                                             ("far", "rnd", "c")[s % 3], rng)))
    modes = ("c", "far", "rnd")
    while len(out) < N_JOBS:
        is_cyc = cyc and (name == "sx_expt" or len(out) % 4 != 0)
        a = wco(cyclotomic(tow(_rand_w(rng)))) if is_cyc else _rand_w(rng)
        m = modes[len(out) % 3]
        out.append((("cyclo/" if is_cyc else "random/") + m, enc_f12(a, bound, m, rng)))
    return out[:N_JOBS]


def _coef(rng, i):
    """a line coefficient or a point's multiplicand (reduced): random, near +-p/2 in either representative, edge"""
    kind = i % 5
    if kind == 3:
        return enc(_near_half(rng), 52, "far", rng)
    if kind == 4:
        return edge_limbs(rng.choice((0x00, 0xFF, 0x55, 0xAA)), rng.choice((1, -1)) * (TOP_P // 2 - 1))
    return enc(rng.randrange(P), 52, "c", rng)


def _line_words(rng, i, n):
    out = []
    for t in range(n):
        out += _coef(rng, i + t)
    return out


class SxOp:
    def __init__(self, name):
        self.name, self.nin, self.nout = name, NIN[name], OUT

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        """[(label, words)], N_JOBS of them, in a fixed shuffled order (so that the first 1, 10, 11 and 23 are a
        mix, and the ten sextets of any wave hold different operands)"""
        name = self.name
        rng = random.Random("sx:" + name)
        cyc = name in ("sx_cyc_sqr", "sx_expt", "sx_xpow_turn")
        jobs = []
        if name in ("sx_mulv", "sx_mulv24"):
            for i in range(6):
                for j in range(6):  # w^i w^j = w^((i + j) mod 6), times xi when i + j >= 6
                    jobs.append(("unit%d%d" % (i, j), enc_f12(w_unit(i), 52, "c", rng) + enc_f12(w_unit(j), 52, "c", rng)))
            st = _structured(rng)
            for (la, a), (lb, b) in zip(st, st[3:] + st[:3]):
                jobs.append((la + "*" + lb, enc_f12(a, 52, "c", rng) + enc_f12(b, 52, "c", rng)))
            bound = IN_BOUND[name]
            for s in range(8):
                jobs.append(("edge%d" % s, edge_f12(rng, bound) + edge_f12(rng, bound)))
            for s in range(6):  # reduced operands at +-p/2: what the header's opening comment once bounded by 0.52 p
                h = [[(_near_half(rng), _near_half(rng)) for _ in range(6)] for _ in range(2)]
                jobs.append(("half%d" % s, enc_f12(h[0], REDUCED, "far", rng) + enc_f12(h[1], REDUCED, "rnd", rng)))
            while len(jobs) < N_JOBS:
                m = ("far", "rnd", "c")[len(jobs) % 3]
                jobs.append(("random/" + m, enc_f12(_rand_w(rng), bound, m, rng) + enc_f12(_rand_w(rng), bound, m, rng)))
        else:
            for i, (lab, f) in enumerate(_operands(name, rng, cyc)):
                w = list(f)
                if name == "sx_xpow_turn":
                    b = wco(cyclotomic(tow(_rand_w(rng)))) if i % 7 else W_ONE
                    w += enc_f12(b, IN_BOUND[name], "far", rng)
                elif name == "sx_mul_line_r":
                    w += _line_words(rng, i, 6)
                elif name in ("sx_fixed_line", "sx_fixed_line_n"):
                    w += _line_words(rng, i, 6) + _coef(rng, i + 1) + _coef(rng, i + 2) + [1 if i % 5 == 2 else 0]
                    lab += "/inf" if i % 5 == 2 else ""
                elif name == "sx_miller3":
                    for t in range(3):
                        w += _line_words(rng, i + t, 6) + _line_words(rng, i + 2 * t, 6)
                    w += _coef(rng, i + 1) + _coef(rng, i + 2) + [1 if i % 9 == 4 else 0]
                    lab += "/inf" if i % 9 == 4 else ""
                jobs.append((lab, w))
        assert len(jobs) == N_JOBS and all(len(w) == self.nin for _, w in jobs), self.name
        rng.shuffle(jobs)
        return tuple((lab, tuple(x & 0xFFFFFFFF for x in w)) for lab, w in jobs)

    def labels(self):
        return [lab for lab, _ in self.jobs()]

    def vectors(self):
        return [w for _, w in self.jobs()]

    def packed(self, n=None):
        return b"".join(pack(w) for w in self.vectors()[:n])

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return tuple(tuple(ref(self.name, w)) for w in self.vectors())


OPS = {name: SxOp(name) for name in NIN}


# ------------------------------------------------------------------ checks
def operand_in_contract(name, words):
    """the first operand's limbs and values are inside what the routine states it accepts"""
    for k in range(12):
        l = [s32(w) for w in words[9 * k:9 * k + 9]]
        if not all(-B28 <= v <= B28 for v in l[:8]) or 100 * abs(val(l)) > IN_BOUND[name] * P:
            return False
    return True


def check_job(name, label, want, got_words):
    """one job's 108 result words: every lane's value mod p, and the stated bounds"""
    assert len(got_words) == OUT
    for k in range(6):
        for c in range(2):
            l = [s32(w) for w in got_words[18 * k + 9 * c:18 * k + 9 * c + 9]]
            where = "%s [%s] lane %d c%d" % (name, label, k, c)
            assert dec(l) == want[k][c], where + ": value"
            # a carry sweep leaves [-2^28, 2^28); an operand handed through or negated keeps sx29.h:7's [-2^28, 2^28]
            top = B28 if name in PASSES_OPERAND else B28 - 1
            assert all(-B28 <= v <= top for v in l[:8]), where + ": limbs 0..7 not balanced"
            assert Fraction(abs(val(l)), P) <= OUT_BOUND[name], where + ": |value| = %.4f p" % (abs(val(l)) / P)
            if name in LIMB8_BOUND:
                assert abs(l[8]) < LIMB8_BOUND[name], where + ": limb 8"


def check_op(name, got, n=None):
    """got: the flat result words of the op's first n jobs"""
    o = OPS[name]
    n = N_JOBS if n is None else n
    assert len(got) == n * OUT, name
    for j in range(n):
        check_job(name, o.labels()[j], o.expected()[j], got[j * OUT:(j + 1) * OUT])
