"""The pairing side's limb primitives (dev/fp29.h, dev/sx29.h) at the edges of
their contracts, against big-integer arithmetic mod p (CPU tier).

tests/native/sx_bounds.cpp is a stand-alone program that drives
  - f29_lin2 / f29_lin4 with the integer quotient estimate (f29_quot),
  - sums of Fp2 products whose first term writes the accumulation rows
    (w29_set) instead of adding to zeroed ones,
  - the fixed line's sum formed inside the reduction (w29_reduce_add)
on extremal inputs (every limb at +-2^28 or +-2^29, worst-sign Karatsuba
sums, values at +-p/2, multiples of p, coefficient corners) and on random
balanced values, and prints every case.  It is built twice: plainly, and with
-fsanitize=undefined,signed-integer-overflow so that a signed 64-bit column
overflow on the host aborts the run; both outputs must agree and every line is
checked here for congruence mod p and for the documented limb / value bounds:
  limbs 0..7 of every result in [-2^28, 2^28);
  lin2 / lin4: |result| <= p/2 + 2^-13.4 p (fp29.h f29_quot), exactly zero
    for multiples of p;
  products: |result| <= |sum| / R + (p/2)(1 + 2^-28) (balanced Montgomery
    digits), the same words as the zeroed-rows sum;
  fixed line: value(g) = value(f) + value(r) exactly.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sx_bounds.cpp")
OUT = os.path.join(ROOT, "tests", "_build")
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 1 << 261
B28 = 1 << 28


def build(name, extra):
    exe = os.path.join(OUT, name)
    deps = [SRC] + [os.path.join(ROOT, "fabric-token-sdk_amd", "csrc", "dev", f)
                    for f in os.listdir(os.path.join(ROOT, "fabric-token-sdk_amd", "csrc", "dev")) if f.endswith(".h")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in deps):
        return exe
    os.makedirs(OUT, exist_ok=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas"] + extra + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def lines():
    plain = build("sx_bounds", [])
    san = build("sx_bounds_ubsan", ["-fsanitize=undefined,signed-integer-overflow", "-fno-sanitize-recover=all"])
    a = subprocess.run([plain], check=True, capture_output=True, text=True).stdout
    r = subprocess.run([san], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a signed overflow (or any other UB) aborts the sanitized run
    assert r.stdout == a
    return [ln.split() for ln in a.splitlines()]


def val(limbs):
    return sum(int(v) << (29 * i) for i, v in enumerate(limbs))


def take(it, n):
    return [int(next(it)) for _ in range(n)]


def balanced(limbs):
    return all(-B28 <= v < B28 for v in limbs[:8])


def lin_bound(v):
    # |v| <= p/2 + 2^-13.4 p  (2^-13.4 < 1/10809)
    return 2 * 10809 * abs(v) <= P * (10809 + 2)


def check_lin(tok, nterms):
    it = iter(tok)
    contract = int(next(it))
    c = take(it, nterms)
    xs = [take(it, 9) for _ in range(nterms)]
    r = take(it, 9)
    v = sum(ci * val(x) for ci, x in zip(c, xs))
    assert (v - val(r)) % P == 0
    assert balanced(r)
    assert lin_bound(val(r)), (c, val(r) / P)
    if contract == 2:
        assert r == [0] * 9
    return contract


def test_lin2_integer_quotient(lines):
    seen = [check_lin(t[1:], 2) for t in lines if t[0] == "lin2"]
    assert len(seen) > 1500 and 2 in seen


def test_lin4_integer_quotient(lines):
    seen = [check_lin(t[1:], 4) for t in lines if t[0] == "lin4"]
    assert len(seen) > 1500 and 2 in seen


def test_first_term_writes_products(lines):
    n_cases = 0
    for t in lines:
        if t[0] != "prod":
            continue
        it = iter(t[1:])
        _contract, n, same = take(it, 3)
        assert same == 1  # word for word the zeroed-rows sum
        re = im = 0
        for _ in range(n):
            a0, a1, b0, b1 = (val(take(it, 9)) for _ in range(4))
            re += a0 * b0 - a1 * b1
            im += a0 * b1 + a1 * b0
        r0, r1 = take(it, 9), take(it, 9)
        for want, got in ((re, r0), (im, r1)):
            assert (val(got) * R - want) % P == 0
            assert balanced(got)
            assert R * abs(val(got)) <= abs(want) + P * R // 2 + (P * R >> 28)
        n_cases += 1
    assert n_cases > 400


def test_fixed_line_sum_in_reduction(lines):
    n_cases = 0
    for t in lines:
        if t[0] != "fline":
            continue
        it = iter(t[1:])
        contract = int(next(it))
        f = [take(it, 9), take(it, 9)]
        r = [take(it, 9), take(it, 9)]
        g = [take(it, 9), take(it, 9)]
        for fc, rc, gc in zip(f, r, g):
            assert val(gc) == val(fc) + val(rc)  # (row + R f) / R = r + f, the same Montgomery digits
            assert balanced(gc)
            if contract:
                assert abs(gc[8]) < 1 << 24
        n_cases += 1
    assert n_cases > 400
