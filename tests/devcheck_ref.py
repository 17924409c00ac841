"""Vectors, big-integer references and mutant references for the device
primitive conformance harness (fabric-token-sdk_amd/csrc/tools/devcheck_ops.h).

Python integers and hashlib only.  Every op of the header's table has an entry
in OPS: its group, its vectors (tuples of input words, built once and cached)
and its reference (the output words of one vector).  MUTANTS lists plausible
wrong implementations; tests/test_devcheck.py::test_vectors_kill_mutants
asserts that each op's vectors tell every mutant from the true reference.

R = 2^256 throughout: a field op's operands are raw limb values below the
modulus (the Montgomery representative is just an integer), and
  mul(a, b) = a b / R,  from_int(a) = a R,  to_int(a) = a / R,  inv(a) = R^2 / a.
"""
import functools
import hashlib
import random
import struct

M32 = 0xFFFFFFFF
RR = 1 << 256
P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47  # BN254 base field
RO = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # BN254 group order
PF = 2**256 - 2**224 + 2**192 + 2**96 - 1                                # P-256 base field
PN = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551  # P-256 group order
SENTINEL = 0xA5A5A5A5
W2_MAX = 6
W2_IN = 1 + W2_MAX * 32


def words(x, n=8):
    assert 0 <= x < 1 << (32 * n), hex(x)
    return tuple((x >> (32 * i)) & M32 for i in range(n))


def val(ws):
    return sum(w << (32 * i) for i, w in enumerate(ws))


def edges(m):
    """E(m): the values at which carry chains and final subtractions go wrong."""
    v = [0, 1, 2, 3, m - 1, m - 2, m - 3, (m - 1) // 2, (m + 1) // 2]
    for k in range(1, 8):
        v += [(1 << 32 * k) - 1, 1 << 32 * k, (1 << 32 * k) + 1, m - (1 << 32 * k)]
    v += [1 << 253, (1 << 253) + 1]
    low7 = ((m >> 224) << 224) | ((1 << 224) - 1)  # seven low limbs all ones
    v.append(low7 if low7 < m else low7 - (1 << 224))
    v += [M32 << 32 * k for k in range(8)]                                   # one limb all ones
    v += [(RR - 1) ^ (M32 << 32 * k) for k in range(8)]                      # one limb all zeros
    v += [int("55" * 32, 16), int("aa" * 32, 16)]
    v += [RR % m, RR * RR % m, m - RR % m]
    out = []
    for x in v:
        x %= m
        if x not in out:
            out.append(x)
    return out


def randoms(m, n, seed):
    """n values below m, at least a quarter of them in [2^253, m)"""
    rng = random.Random(seed)
    lo = min(1 << 253, m // 2)
    return [rng.randrange(lo, m) if i % 4 == 0 else rng.randrange(m) for i in range(n)]


def pairs(m, seed):
    e = edges(m)
    ra, rb = randoms(m, 4096, seed), randoms(m, 4096, seed + 1)
    return [(a, b) for a in e for b in e] + list(zip(ra, rb))


# ------------------------------------------------------------------ registry
class Op:
    def __init__(self, name, group, nin, nout, gen, ref):
        self.name, self.group, self.nin, self.nout, self._gen, self._ref = name, group, nin, nout, gen, ref

    @functools.lru_cache(maxsize=None)
    def vectors(self):
        v = [tuple(x) for x in self._gen()]
        if len(v) % 64 == 0:  # the harness runs n lanes in blocks of 64 or 256: keep a partial last block
            v.append(v[0])
        assert v and all(len(x) == self.nin and all(0 <= w <= M32 for w in x) for x in v), self.name
        return v

    def ref(self, vec):
        out = tuple(self._ref(vec))
        assert len(out) == self.nout, self.name
        return out

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return [self.ref(v) for v in self.vectors()]

    def packed(self):
        return b"".join(struct.pack("<%dI" % self.nin, *v) for v in self.vectors())


OPS = {}


def op(name, group, nin, nout, gen, ref):
    assert name not in OPS
    OPS[name] = Op(name, group, nin, nout, gen, ref)


def binary(f):  # reference of a two-operand op on 8-word values
    return lambda v: words(f(val(v[:8]), val(v[8:])))


def chained(f):  # ((a o b) o a) o b
    return lambda v: words(f(f(f(val(v[:8]), val(v[8:])), val(v[:8])), val(v[8:])))


def unary(f):
    return lambda v: words(f(val(v)))


def pair_vectors(m, seed):
    return lambda: [words(a) + words(b) for a, b in pairs(m, seed)]


def single_vectors(m, seed, extra=(), n=512, full=False):
    def gen():
        rng = random.Random(seed)
        xs = edges(m) + list(extra) + [rng.randrange(RR if full else m) for _ in range(n)]
        if not full:
            xs += randoms(m, 64, seed + 7)
        return [words(x) for x in xs]
    return gen


# ------------------------------------------------ 1. Fe<ModP>, Fe<ModR> (dev/fp.h)
def field_ops(prefix, m, group, seed):
    ri = pow(RR, -1, m)
    add = lambda a, b: (a + b) % m
    sub = lambda a, b: (a - b) % m
    mul = lambda a, b: a * b * ri % m
    for k, (n, f) in enumerate([("add", add), ("sub", sub), ("mul", mul), ("cios", mul)]):
        op("%s_%s" % (prefix, n), group, 16, 8, pair_vectors(m, seed + 10 * k), binary(f))
        op("%s_%s_ch" % (prefix, n), group, 16, 8, pair_vectors(m, seed + 10 * k + 5), chained(f))
    return add, sub, mul


def from_int_extra(m):
    return [RR - 1, 5 * m, 5 * m + 1, 5 * m - 1, 1 << 255, m, m + 1, 2 * m, 2 * m - 1, 4 * m, 4 * m - 1, RR - m]


for _prefix, _m, _seed in (("fp", P, 100), ("fr", RO, 200)):
    _add, _sub, _mul = field_ops(_prefix, _m, "fe", _seed)
    op(_prefix + "_neg", "fe", 8, 8, single_vectors(_m, _seed + 50), unary(lambda a, m=_m: -a % m))
    op(_prefix + "_dbl", "fe", 8, 8, single_vectors(_m, _seed + 51), unary(lambda a, m=_m: 2 * a % m))
    op(_prefix + "_sqr", "fe", 8, 8, single_vectors(_m, _seed + 52), unary(lambda a, f=_mul: f(a, a)))
    op(_prefix + "_from_int", "fe", 8, 8, single_vectors(_m, _seed + 53, from_int_extra(_m), full=True),
       unary(lambda a, m=_m: a * RR % m))
    op(_prefix + "_to_int", "fe", 8, 8, single_vectors(_m, _seed + 54), unary(lambda a, f=_mul: f(a, 1)))
    op(_prefix + "_geq_mod", "fe", 8, 1,
       single_vectors(_m, _seed + 55, [_m, _m + 1, RR - 1, 1 << 255] + [_m ^ (1 << 32 * k) for k in range(8)]
                      + [_m + (1 << 32 * k) for k in range(7)], full=True),
       lambda v, m=_m: (int(val(v) >= m),))


# ------------------------------------------------------------- 2. inversions
SAFEGCD_EDGES = [1, 2, 3, P - 1, P - 2, (P - 1) // 2, (1 << 253) % P, 1 << 200, (1 << 30) - 1, (1 << 62) - 1]


def inv_vectors(m, seed, n):
    def gen():
        rng = random.Random(seed)
        xs = [0] + (SAFEGCD_EDGES if m == P else []) + [x for x in edges(m) if x]
        return [words(x) for x in xs + [rng.randrange(1, m) for _ in range(n)]]
    return gen


def inv_ref(m):  # Montgomery form in and out; 0 stays 0
    return unary(lambda a: RR * RR * pow(a, -1, m) % m if a else 0)


for _k, _n in enumerate(("fp_inv_var", "fp_inv_sg30", "fp_inv_sg62", "fp_inv_eea")):
    op(_n, "inv", 8, 8, inv_vectors(P, 300 + _k, 1024), inv_ref(P))


# ------------------------------------------------------ 3. dev/fp_wide.h
def mul_wide_vectors():
    rng = random.Random(400)
    e = edges(P) + [RR - 1, RR - 2, 1 << 255]
    ps = [(a, b) for a in e for b in e] + [(rng.randrange(RR), rng.randrange(RR)) for _ in range(2048)]
    return [words(a) + words(b) for a, b in ps]


op("mul_wide", "wide", 16, 16, mul_wide_vectors, lambda v: words(val(v[:8]) * val(v[8:]), 16))

REDC_BOUND = 14 * P * P
P_NEG_INV = -pow(P, -1, RR) % RR


def redc_pre(t):
    """the value before the final subtractions: (T + (-T / p mod R) p) / R"""
    return (t + (t * P_NEG_INV % RR) * P) >> 256


def redc_targets():
    """T whose pre-subtraction value is exactly u: T = u R - q p for a quotient q that keeps T in range"""
    out = []
    umax = (REDC_BOUND - 1 + (RR - 1) * P) >> 256
    for u in (P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P - 1, 3 * P, 3 * P + 1, umax, umax - 1):
        for q in (RR - 1, RR - 2, RR - (1 << 224), (RR * 9) // 10):
            t = u * RR - q * P
            if 0 <= t < REDC_BOUND:
                assert redc_pre(t) == u
                out.append(t)
    assert {redc_pre(t) for t in out} >= {2 * P - 1, 2 * P, 3 * P - 1, 3 * P, umax}
    return out


def redc_vectors():
    rng = random.Random(401)
    ts = [0, 1, REDC_BOUND - 1, REDC_BOUND - 2]
    for j in (1, 2, 3):
        ts += [j * P * RR, j * P * RR + 1, j * P * RR - 1]
    ts += redc_targets()
    ts += [a * b for a in edges(P) for b in (P - 1, P - 2, (P + 1) // 2, 1)]
    ts += [rng.randrange(REDC_BOUND) for _ in range(2048)]
    # 3 p R (+-1) lies past the documented 14 p^2 and inside what the two subtractions take: a value below 4p
    assert all(0 <= t < REDC_BOUND or t // (P * RR) == 3 or t == 3 * P * RR - 1 for t in ts)
    assert all(redc_pre(t) < 4 * P for t in ts)
    return [words(t, 16) for t in ts]


P_RI = pow(RR, -1, P)
op("redc_wide", "wide", 16, 8, redc_vectors, lambda v: words(val(v) * P_RI % P))


def w2_vectors():
    rng = random.Random(402)
    kinds = [lambda: 0, lambda: 1, lambda: P - 1, lambda: (P - 1) // 2, lambda: (P + 1) // 2,
             lambda: rng.randrange(P)]
    out = []
    for k in range(1, W2_MAX + 1):
        for ia in range(6):
            for ib in range(6):
                for ic in range(6):
                    for id_ in range(6):
                        v = [k]
                        for t in range(W2_MAX):
                            for i in (ia, ib, ic, id_):
                                v += words(kinds[i]() if t < k else rng.randrange(RR))  # past k: never read
                        out.append(v)
    return out


def w2_terms(v):
    k = v[0]
    for t in range(k):
        q = v[1 + 32 * t:33 + 32 * t]
        yield val(q[:8]), val(q[8:16]), val(q[16:24]), val(q[24:32])


def w2_ref(v):
    re = sum(a0 * b0 - a1 * b1 for a0, a1, b0, b1 in w2_terms(v))
    im = sum(a0 * b1 + a1 * b0 for a0, a1, b0, b1 in w2_terms(v))
    return words(re * P_RI % P) + words(im * P_RI % P)


op("w2_sum", "wide", W2_IN, 16, w2_vectors, w2_ref)


# ------------------------------------------------------------ 4. dev/fp29.h
U29 = (1 << 29) - 1
P29_TOP_INV = 5.873246395036766e-16  # dev/fp29_const.h
R261_INV = pow(1 << 261, -1, P)
P_NEG_INV261 = -pow(P, -1, 1 << 261) % (1 << 261)


def s32(w):
    return w - (1 << 32) if w >> 31 else w


def f29_val(ls):
    return sum(s32(w) << (29 * i) for i, w in enumerate(ls))


def f29_words(x):
    """normalised limbs of x: 0..7 in [0, 2^29), limb 8 the signed rest"""
    top = x >> 232
    assert -(1 << 31) <= top < 1 << 31
    return tuple((x >> (29 * i)) & U29 for i in range(8)) + (top & M32,)


def f29_limbs(L, B, pattern, rng):
    """signed limbs with |limb| <= L (2^29 - 1) and |value| <= B p; pattern + - a b (alternating) r(andom)"""
    lim, bp = int(L * U29), int(B * 1000) * P // 1000
    top = min(lim, (bp - lim * (((1 << 232) - 1) // U29)) >> 232)  # the low limbs reach lim sum 2^(29 i)
    assert top > 0
    ls = []
    for i in range(9):
        mag = top if i == 8 else lim
        ls.append({"+": mag, "-": -mag, "a": mag if i % 2 == 0 else -mag, "b": -mag if i % 2 == 0 else mag,
                   "r": rng.randint(-mag, mag)}[pattern])
    assert max(abs(x) for x in ls) <= lim and abs(sum(x << (29 * i) for i, x in enumerate(ls))) <= bp
    return tuple(x & M32 for x in ls)


F29_MUL_L = [(1, 1), (1, 2), (2, 1), (1, 2.5), (1.5, 1.5)]
F29_MUL_B = [(12.9, 12.9), (32, 5.2), (5.2, 32), (1, 1)]


def f29_mul_vectors():
    rng = random.Random(500)
    out = []
    for la, lb in F29_MUL_L:
        for ba, bb in F29_MUL_B:
            pats = [(x, y) for x in "+-ab" for y in "+-ab"] + [("r", "r")] * 48
            for x, y in pats:
                out.append(f29_limbs(la, ba, x, rng) + f29_limbs(lb, bb, y, rng))
    for v in out:  # the header's preconditions
        a, b = v[:9], v[9:]
        la, lb = (max(abs(s32(w)) for w in x) / U29 for x in (a, b))
        assert la * lb <= 2.5 and abs(f29_val(a) * f29_val(b)) < 169 * P * P
    return out


def f29_sqr_vectors():
    rng = random.Random(501)
    out = [f29_limbs(1, b, x, rng) for b in (12.9, 1, 2) for x in "+-ab" + "r" * 200]
    assert all(max(abs(s32(w)) for w in v) <= U29 and f29_val(v) ** 2 < 169 * P * P for v in out)
    return out


def f29_product(a, b):
    """(a b + m p) / 2^261 for the Montgomery digits m = -a b / p mod 2^261, digits in [0, 2^29)"""
    t = a * b
    return (t + (t * P_NEG_INV261 % (1 << 261)) * P) >> 261


def f29_mul_model(a, b, flip=None):
    """dev/fp29.h f29_mul limb for limb; flip = (i, j) negates the reduction term m_i p_j (a mutant)"""
    p29 = [(P >> (29 * i)) & U29 for i in range(9)]
    inv = -pow(P, -1, 1 << 29) % (1 << 29)
    acc, m, r = 0, [0] * 9, [0] * 9
    for k in range(17):
        for i in range(9):
            j = k - i
            if 0 <= j < 9:
                acc += a[i] * b[j]
        for i in range(9):
            j = k - i
            if i < k and 0 <= j < 9:
                acc += -m[i] * p29[j] if flip == (i, j) else m[i] * p29[j]
        if k < 9:
            m[k] = (acc * inv) & U29
            acc += m[k] * p29[0]
        else:
            r[k - 9] = acc & U29
        acc >>= 29
    r[8] = acc
    return tuple(x & M32 for x in r)


def f29_mul_ref(v):
    return f29_words(f29_product(f29_val(v[:9]), f29_val(v[9:])))


def f29_reduce_model(ls):
    t = float(s32(ls[8])) * 536870912.0 + float(s32(ls[7]))
    q = round(t * P29_TOP_INV)  # round half to even, as rint
    return f29_val(ls) - q * P


def f29_wide_vectors(L, B, seed, n=300):
    def gen():
        rng = random.Random(seed)
        return [f29_limbs(L, b, x, rng) for b in B for x in "+-ab" + "r" * n]
    return gen


def f29_zero_vectors():
    rng = random.Random(505)
    out = []
    for k in list(range(-40, 41)) + [rng.randint(-40, 40) for _ in range(64)]:
        for d in (0, 1, -1, 1 << 232, -(1 << 29)):
            out.append(f29_words(k * P + d))
    p29 = [(P >> (29 * i)) & U29 for i in range(9)]
    for k in (-4, -3, -2, 2, 3, 4):  # k p with unnormalised limbs, and one limb off by one
        out.append(tuple((k * x) & M32 for x in p29))
        out.append(tuple((k * x + (i == 4)) & M32 for i, x in enumerate(p29)))
    out += f29_wide_vectors(4, (40,), 506, 100)()
    return out


def f29_rzero_vectors():
    out = [(0,) * 9]
    for i in range(9):
        for x in (1, M32, 1 << 31, 1 << 28):
            out.append(tuple(x if j == i else 0 for j in range(9)))
    return out


def from_fp_vectors():
    rng = random.Random(507)
    return [words(x) for x in edges(P) + [RR - 1, P, 1 << 255] + [rng.randrange(RR) for _ in range(512)]]


def to_fp_vectors():
    rng = random.Random(508)
    out = [f29_words(32 * x) for x in edges(P)]                       # f29_from_fp's outputs
    out += [f29_words(-32 * x) for x in edges(P)]                     # and their negatives, normalised
    out += [f29_limbs(L, 160, x, rng) for L in (1, 2, 2.5) for x in "+-ab" + "r" * 100]
    assert all(max(abs(s32(w)) for w in v) <= 2.5 * U29 and abs(f29_val(v)) < 169 * P for v in out)
    return out


INV32 = pow(32, -1, P)
op("f29_from_fp", "f29", 8, 9, from_fp_vectors, lambda v: f29_words(32 * val(v)))
op("f29_to_fp", "f29", 9, 8, to_fp_vectors, lambda v: words(f29_val(v) * INV32 % P))
op("f29_roundtrip", "f29", 8, 8, lambda: [words(x) for x in edges(P) + randoms(P, 512, 509)], lambda v: tuple(v))
op("f29_norm", "f29", 9, 9, f29_wide_vectors(4, (40, 1), 502), lambda v: f29_words(f29_val(v)))
op("f29_reduce", "f29", 9, 9, f29_wide_vectors(4, (40, 26, 8, 1), 503), lambda v: f29_words(f29_reduce_model(v)))
op("f29_mul", "f29", 18, 9, f29_mul_vectors, f29_mul_ref)
op("f29_mul_c", "f29", 18, 9, f29_mul_vectors, f29_mul_ref)
op("f29_sqr", "f29", 9, 9, f29_sqr_vectors, lambda v: f29_words(f29_product(f29_val(v), f29_val(v))))
op("f29_sqr_c", "f29", 9, 9, f29_sqr_vectors, lambda v: f29_words(f29_product(f29_val(v), f29_val(v))))
op("f29_is_zero", "f29", 9, 1, f29_zero_vectors, lambda v: (int(f29_val(v) % P == 0),))
op("f29_reduced_zero", "f29", 9, 1, f29_rzero_vectors, lambda v: (int(not any(v)),))


def f29_check_bounds(name, vec, out):
    """the documented output bounds and congruences of an f29 op's result `out` (None: nothing documented)"""
    if name in ("f29_mul", "f29_mul_c", "f29_sqr", "f29_sqr_c"):
        a, b = f29_val(vec[:9]), f29_val(vec[9:] if len(vec) == 18 else vec)
        r = f29_val(out)
        return all(0 <= s32(w) <= U29 for w in out[:8]) and abs(r) < 2 * P and (r - a * b * R261_INV) % P == 0
    if name in ("f29_norm", "f29_reduce"):
        r = f29_val(out)
        ok = all(0 <= s32(w) <= U29 for w in out[:8]) and (r - f29_val(vec)) % P == 0
        return ok and (r == f29_val(vec) if name == "f29_norm" else 2 * abs(r) <= 3 * P)
    return None


# --------------------------------------------------------- 6. byte conversions
def be32_load_vectors():
    rng = random.Random(600)
    out = []
    for off in range(32):
        for x in (rng.randrange(RR), RR - 1, int("0102030405060708090a0b0c0d0e0f10" "1112131415161718191a1b1c1d1e1f20", 16)):
            buf = bytearray(rng.randrange(256) for _ in range(96))
            buf[off:off + 32] = x.to_bytes(32, "big")
            out.append((off, SENTINEL, SENTINEL, SENTINEL) + struct.unpack("<24I", bytes(buf)))
    return out


def be32_load_ref(v):
    buf = struct.pack("<24I", *v[4:])
    return words(int.from_bytes(buf[v[0]:v[0] + 32], "big"))


def be32_store_vectors():
    rng = random.Random(601)
    return [(off, SENTINEL, SENTINEL, SENTINEL) + words(x) for off in range(32)
            for x in (rng.randrange(RR), RR - 1, 0, int("0102030405060708090a0b0c0d0e0f10" * 2, 16))]


def be32_store_ref(v):
    buf = bytearray(b"\xa5" * 96)  # the 32 bytes either side of the target keep the sentinel
    buf[32 + v[0]:64 + v[0]] = val(v[4:]).to_bytes(32, "big")
    return struct.unpack("<24I", bytes(buf))


op("be32_load", "bytes", 28, 8, be32_load_vectors, be32_load_ref)
op("be32_store", "bytes", 12, 24, be32_store_vectors, be32_store_ref)


# ------------------------------------------------------------- 7. dev/p256.h
def p256_limb_patterns(m):
    """all ones / all zeros in each limb position (every branch of the multiplication-free reduction)"""
    v = []
    for k in range(8):
        v += [M32 << 32 * k, ((RR - 1) ^ (M32 << 32 * k)) % m, ((1 << 32 * (k + 1)) - 1) % m, (RR - (1 << 32 * k)) % m]
    return v


def pf_pair_vectors(seed):
    def gen():
        e = edges(PF)
        e += [x for x in p256_limb_patterns(PF) if x not in e]
        ra, rb = randoms(PF, 4096, seed), randoms(PF, 4096, seed + 1)
        return [words(a) + words(b) for a, b in [(a, b) for a in e for b in e] + list(zip(ra, rb))]
    return gen


PF_RI, PN_RI = pow(RR, -1, PF), pow(RR, -1, PN)
pf_add = lambda a, b: (a + b) % PF
pf_sub = lambda a, b: (a - b) % PF
pf_mul = lambda a, b: a * b * PF_RI % PF
pn_mul = lambda a, b: a * b * PN_RI % PN
for _k, (_n, _f) in enumerate((("add", pf_add), ("sub", pf_sub), ("mul", pf_mul))):
    op("pf_" + _n, "p256", 16, 8, pf_pair_vectors(700 + 10 * _k), binary(_f))
    op("pf_%s_ch" % _n, "p256", 16, 8, pf_pair_vectors(705 + 10 * _k), chained(_f))
op("pf_neg", "p256", 8, 8, single_vectors(PF, 740), unary(lambda a: -a % PF))
op("pf_from_int", "p256", 8, 8, single_vectors(PF, 741, [RR - 1, PF, PF + 1, RR - PF, 1 << 255], full=True),
   unary(lambda a: a * RR % PF))
op("pf_to_int", "p256", 8, 8, single_vectors(PF, 742), unary(lambda a: pf_mul(a, 1)))
op("pf_inv", "p256", 8, 8, inv_vectors(PF, 743, 256), inv_ref(PF))
op("pn_mul", "p256", 16, 8, pair_vectors(PN, 750), binary(pn_mul))
op("pn_mul_ch", "p256", 16, 8, pair_vectors(PN, 755), chained(pn_mul))
op("pn_from_int", "p256", 8, 8, single_vectors(PN, 760, [RR - 1, PN, PN + 1, PN - 1, RR - PN, 1 << 255], full=True),
   unary(lambda a: a * RR % PN))
op("pn_to_int", "p256", 8, 8, single_vectors(PN, 761), unary(lambda a: pn_mul(a, 1)))
op("pn_inv", "p256", 8, 8, inv_vectors(PN, 762, 256), inv_ref(PN))


def geq_vectors():
    rng = random.Random(770)
    e = edges(PN) + [PN, PN + 1, RR - 1, PF, PN // 2 + 1]
    ps = [(a, b) for a in e for b in e]
    for _ in range(512):
        a = rng.randrange(RR)
        ps += [(a, rng.randrange(RR)), (a, a ^ (1 << rng.randrange(256)))]
    return [words(a) + words(b) for a, b in ps]


op("u256_geq", "p256", 16, 1, geq_vectors, lambda v: (int(val(v[:8]) >= val(v[8:])),))


# ------------------------------------------------------------ 5. dev/sha256.h
SHA_LENGTHS = list(range(131)) + [183, 184, 191, 192, 247, 248, 1451]
_K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]


def sha256_model(msg, bits=None, fits=56):
    """FIPS 180-4 with the length field (`bits`) and the padding threshold (`fits`: the 0x80 byte and the
    zeros share the last block with the length when len % 64 < fits) open to the mutants"""
    rot = lambda x, n: ((x >> n) | (x << (32 - n))) & M32
    bits = 8 * len(msg) if bits is None else bits
    pad = b"\x80" + b"\0" * ((55 - len(msg)) % 64)
    if len(msg) % 64 >= fits and len(pad) < 9:
        pad += b"\0" * 64
    data = msg + pad + struct.pack(">Q", bits)
    h = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
    for o in range(0, len(data), 64):
        w = list(struct.unpack(">16I", data[o:o + 64]))
        for i in range(16, 64):
            s0 = rot(w[i - 15], 7) ^ rot(w[i - 15], 18) ^ (w[i - 15] >> 3)
            s1 = rot(w[i - 2], 17) ^ rot(w[i - 2], 19) ^ (w[i - 2] >> 10)
            w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
        a, b, c, d, e, f, g, hh = h
        for i in range(64):
            t1 = (hh + (rot(e, 6) ^ rot(e, 11) ^ rot(e, 25)) + ((e & f) ^ (~e & g)) + _K[i] + w[i]) & M32
            t2 = ((rot(a, 2) ^ rot(a, 13) ^ rot(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
            a, b, c, d, e, f, g, hh = (t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g
        h = [(x + y) & M32 for x, y in zip(h, (a, b, c, d, e, f, g, hh))]
    return struct.pack(">8I", *h)


class ShaSet:
    """messages as segment lists in one arena: arena bytes, first[n + 1], segs [(offset, length)], and per
    message its bytes and its placement's label"""

    def __init__(self):
        rng = random.Random(800)
        self.arena, self.first, self.segs, self.msgs, self.labels = bytearray(), [0], [], [], []

        def place(data, mis):
            while len(self.arena) % 16 != mis:
                self.arena.append(0xEE)
            o = len(self.arena)
            self.arena += data
            self.arena.append(0xEE)
            return (o, len(data))

        def add(label, msg, parts):
            assert b"".join(msg[a:b] for a, b, _ in parts) == msg
            self.segs += [place(msg[a:b], mis) for a, b, mis in parts]
            self.first.append(len(self.segs))
            self.msgs.append(msg)
            self.labels.append(label)

        for L in SHA_LENGTHS:
            msg = bytes(rng.randrange(256) for _ in range(L))
            for mis in range(16):  # one segment: aligned, and at every misalignment
                add("one@%d" % mis, msg, [(0, L, mis)])
            c = L // 2
            add("split+empty", msg, [(0, c, 0), (c, c, 5), (c, L, 0)])          # a zero-length segment between
            add("split3", msg, [(0, L // 3, 3), (L // 3, c, 0), (c, L, 9)])
            if L >= 64:  # an aligned multiple of 64 first, then the tail
                f = 64 * max(1, (L - 1) // 64)
                add("blocks+tail", msg, [(0, f, 0), (f, L, 0)])
            if L >= 65:  # second segment aligned and >= 64 bytes while the block is part full
                f = (L - 65) % 63 + 1
                assert 1 <= f <= L - 64
                add("partial+aligned64", msg, [(0, f, 0), (f, L, 0)])
        self.n = len(self.msgs)
        assert len(self.arena) < 1 << 22

    def fast_blocks(self, j):
        """64-byte blocks of message j that Sha256::update takes through its aligned fast path"""
        fill, nb = 0, 0
        for o, n in self.segs[self.first[j]:self.first[j + 1]]:
            if fill == 0 and o % 16 == 0:
                nb += n // 64
                n %= 64
            fill = (fill + n) % 64
        return nb

    def expected(self):
        out = []
        for m in self.msgs:
            d = hashlib.sha256(m).digest()
            out.append(struct.unpack("<8I", d) + words(int.from_bytes(d, "big") % RO))
        assert all(sha256_model(m) == hashlib.sha256(m).digest() for m in self.msgs[::97])  # the mutants' base
        return out

    def record(self):
        """the host program's record (tests/native/devcheck_host.cpp)"""
        a = bytes(self.arena)
        return (struct.pack("<4I", M32, self.n, len(a), len(self.segs)) + struct.pack("<%dI" % len(self.first), *self.first)
                + b"".join(struct.pack("<2I", *s) for s in self.segs) + a + b"\0" * (-len(a) % 4))


@functools.lru_cache(maxsize=None)
def sha_set():
    return ShaSet()


# ------------------------------------------------------------------- mutants
def redc_mutant(kind):
    def f(v):
        t = val(v)
        q = t * P_NEG_INV % RR
        u = (t + q * P) >> 256
        if kind == "carry":  # the carry of limbs 0..14 into limb 15 dropped
            u = (u - ((((t % (1 << 480)) + (q * P % (1 << 480))) >> 480) << 224)) % RR
        if kind != "p" and u >= 2 * P:
            u -= 2 * P
        if kind != "2p" and u >= P:
            u -= P
        return words(u % RR)
    return f


def w2_low_mutant(v):  # real accumulator starting at 5 p^2: wraps below zero
    re = (5 * P * P + sum(a0 * b0 - a1 * b1 for a0, a1, b0, b1 in w2_terms(v))) % (1 << 512)
    im = sum(a0 * b1 + a1 * b0 for a0, a1, b0, b1 in w2_terms(v))
    return words(re * P_RI % P) + words(im * P_RI % P)


def from_int_mutant(v):
    """fe_from_int with 4 conditional subtractions, one fewer than 2^256 - 1 needs (5, 6 and 7 are the
    same function), then the Montgomery product by R^2 with its own final subtraction"""
    a = val(v)
    for _ in range(4):
        a = a - P if a >= P else a
    t = a * (RR * RR % P)
    u = (t + (t * P_NEG_INV % RR) * P) >> 256
    return words((u - P if u >= P else u) % RR)


def pf_mul_mutant(v):  # the value before the last conditional subtraction, truncated to 256 bits
    t = val(v[:8]) * val(v[8:])
    return words(((t + (t * (-pow(PF, -1, RR) % RR) % RR) * PF) >> 256) % RR)


# (op whose vectors must kill it, description, mutant reference of one vector)
MUTANTS = [
    ("fp_add", "final subtraction on > instead of >=", binary(lambda a, b: a + b - P if a + b > P else a + b)),
    ("fr_add", "final subtraction on > instead of >=", binary(lambda a, b: a + b - RO if a + b > RO else a + b)),
    ("fp_sub", "adds m back on a <= b", binary(lambda a, b: a - b + P if a <= b else a - b)),
    ("fr_sub", "adds m back on a <= b", binary(lambda a, b: a - b + RO if a <= b else a - b)),
    ("redc_wide", "only the subtraction of p", redc_mutant("p")),
    ("redc_wide", "only the subtraction of 2p", redc_mutant("2p")),
    ("redc_wide", "carry into the top limb dropped", redc_mutant("carry")),
    ("w2_sum", "accumulator one multiple of p^2 too low", w2_low_mutant),
    ("pf_add", "carry out of 2^256 ignored",
     binary(lambda a, b: (a + b) % RR - PF if (a + b) % RR >= PF else (a + b) % RR)),
    ("pf_mul", "last conditional subtraction missing", pf_mul_mutant),
    ("f29_mul", "sign of one reduction term flipped",
     lambda v: f29_mul_model([s32(w) for w in v[:9]], [s32(w) for w in v[9:]], flip=(3, 2))),
]

# Wrong on paper, the same function in fact: the product by R^2 takes any operand below 2^256 (its value
# before the final subtraction is below a R^2 / R + p < 2p), so fe_from_int's subtractions change no output.
# test_vectors_kill_mutants asserts that no vector tells it apart, and kills the same defect where it does
# show: digest_mod_r, whose result is the reduced integer itself (SHA_MUTANTS).
EQUIVALENT_MUTANTS = [
    ("fp_from_int", "one conditional subtraction too few", from_int_mutant),
]


def sha_out(d, subs=6):
    """the harness's 16 output words for a digest: its bytes, then digest_mod_r by conditional subtractions"""
    x = int.from_bytes(d, "big")
    for _ in range(subs):
        x = x - RO if x >= RO else x
    return struct.unpack("<8I", d) + words(x)


# the hash: (description, the 16 output words of message j of the set under the mutant)
SHA_MUTANTS = [
    ("padding threshold 55 instead of 56", lambda s, j: sha_out(sha256_model(s.msgs[j], fits=55))),
    ("total not advanced on the fast path",
     lambda s, j: sha_out(sha256_model(s.msgs[j], bits=8 * (len(s.msgs[j]) - 64 * s.fast_blocks(j))))),
    ("digest_mod_r one conditional subtraction too few", lambda s, j: sha_out(hashlib.sha256(s.msgs[j]).digest(), 4)),
]

GROUPS = ["fe", "inv", "wide", "f29", "bytes", "p256"]  # and "sha", which has its own entry point
