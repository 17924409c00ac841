"""The variable-base G1 chain on the carry-free form (CPU tier): dev/jobs.h
g1_mul_glv16_halves -- window table in balanced 29-bit limbs with beta x
stored, built by j29_dbl / j29_madd and brought to a common Z, empty window
steps skipped -- and g1_var_point, against a big-integer double-and-add on the
affine result.

tests/native/g1chain_main.cpp runs the code and prints operands and results;
the reference and every assertion are here.  Cases:
  - GLV halves 0, 1, every Booth digit +-8, bit 127 set (window 32 holds a
    digit), 2^128 - 1, the top 8, 12 and 124 bits zero (the accumulator stays at
    infinity across windows), in every pair, with every combination of n1 and
    n2, a third of them on an input with Z != 1;
  - k = 0, 1, r - 1 and 200 random scalars through glv_split;
  - g1_var_point: a single point, the PP-A weights (100, 1), the PP-B Horner
    (b = 16, 16 terms), a VT_NEG term, equal and opposite points in one sum,
    each with and without vneg.
The program is built twice: plainly, and with
-fsanitize=signed-integer-overflow,undefined so that a 64-bit column that
overflows aborts the run; both print the same.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "g1chain_main.cpp")
OUT = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc", "dev")

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
INF = None


def add(a, b):
    """affine addition on y^2 = x^3 + 3 over Fp, big integers"""
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
    """k a by double-and-add from the top bit"""
    acc = INF
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, a)
    return acc


def point(tok):
    if tok == "-":
        return INF
    b = bytes.fromhex(tok)
    x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
    assert (y * y - x * x * x - 3) % P == 0
    return x, y


def booth16(k, i):
    """dev/jobs.h booth16 on the integer k"""
    v = ((k << 1) >> (4 * i)) & 31
    return (v & 1) + ((v >> 1) & 7) - 8 * (v >> 4)


def build(name, extra):
    exe = os.path.join(OUT, name)
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in deps):
        return exe
    os.makedirs(OUT, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + extra + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def lines():
    plain = build("g1chain", ["-O2"])
    san = build("g1chain_ubsan", ["-O1", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"])
    a = subprocess.run([plain], check=True, capture_output=True, text=True).stdout
    r = subprocess.run([san], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a signed overflow (or any other UB) aborts the sanitized run
    assert r.stdout == a
    return [ln.split() for ln in a.splitlines()]


@pytest.fixture(scope="module")
def glv_constants(lines):
    """(lambda, beta) of the code, checked here: cube roots of unity with phi(x, y) = (beta x, y) = lambda (x, y)"""
    beta, lam = (int(v, 16) for v in next(t for t in lines if t[0] == "consts")[1:])
    assert 1 < beta < P and pow(beta, 3, P) == 1 and 1 < lam < R and pow(lam, 3, R) == 1
    pt = next(point(t[1]) for t in lines if t[0] == "mul")
    assert mul(lam, pt) == (beta * pt[0] % P, pt[1])
    return lam, beta


def test_halves_match_double_and_add(lines, glv_constants):
    lam, beta = glv_constants
    rows = [t for t in lines if t[0] == "halves"]
    assert len(rows) == 400
    shapes = {"zero": 0, "one": 0, "eights": 0, "top": 0, "z": 0, "lead8": 0, "lead12": 0, "lead124": 0}
    signs = set()
    bad = []
    for n, t in enumerate(rows):
        pt, z, k1, n1, k2, n2, got = point(t[1]), int(t[2], 16), int(t[3], 16), int(t[4]), int(t[5], 16), int(t[6]), point(t[7])
        phi = (beta * pt[0] % P, pt[1])
        want = add(mul(k1, neg(pt) if n1 else pt), mul(k2, neg(phi) if n2 else phi))
        assert want == mul(((-k1 if n1 else k1) + (-k2 if n2 else k2) * lam) % R, pt)  # the reference agrees with itself
        if got != want:
            bad.append(n)
        signs.add((n1, n2))
        for k in (k1, k2):
            shapes["zero"] += k == 0
            shapes["one"] += k == 1
            shapes["eights"] += all(abs(booth16(k, i)) == 8 for i in range(32))
            shapes["top"] += booth16(k, 32) != 0
            shapes["lead8"] += 0 < k < 1 << 120
            shapes["lead12"] += 0 < k < 1 << 116
            shapes["lead124"] += 1 < k < 16
        shapes["z"] += z != 1
    assert not bad, "%d of %d differ, first %d" % (len(bad), len(rows), bad[0])
    assert signs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(v >= 40 for v in shapes.values()), shapes


def test_scalars_through_glv_split(lines):
    rows = [t for t in lines if t[0] == "mul"]
    assert len(rows) == 203
    ks = [int(t[2], 16) for t in rows]
    assert ks[:3] == [0, 1, R - 1] and all(k < R for k in ks)
    bad = [n for n, t in enumerate(rows) if point(t[3]) != mul(ks[n], point(t[1]))]
    assert not bad, "%d of %d differ, first %d" % (len(bad), len(rows), bad[0])
    assert point(rows[0][3]) is INF


def test_var_point_branches(lines):
    rows = [t for t in lines if t[0] == "var"]
    seen = set()
    for t in rows:
        horner, vneg, k, cnt = int(t[1]), int(t[2]), int(t[3], 16), int(t[4])
        terms = [(point(t[5 + 3 * i]), int(t[6 + 3 * i], 16), int(t[7 + 3 * i])) for i in range(cnt)]
        got = point(t[5 + 3 * cnt])
        V = INF
        for i, (pt, w, ng) in enumerate(terms):
            c = terms[0][1] ** (cnt - 1 - i) if horner else w
            V = add(V, mul(c, neg(pt) if ng else pt))
        want = mul(k, neg(V) if vneg else V)
        assert got == want, t[:5]
        b = terms[0][1]
        if cnt == 1 and not terms[0][2]:
            seen.add("single")
        elif horner and b & (b - 1) == 0:
            seen.add("horner16" if (b, cnt) == (16, 16) else "horner")
        else:
            seen.add("joint")
            if horner and (b, cnt) == (100, 2):
                seen.add("pp_a")
            if any(ng for _, _, ng in terms):
                seen.add("vt_neg")
            if V is INF:
                seen.add("cancel")
        seen.add("vneg" if vneg else "plain")
    assert seen == {"single", "horner16", "joint", "pp_a", "vt_neg", "cancel", "vneg", "plain"}
