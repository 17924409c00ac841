"""The fused G1 formulas of dev/fp29.h (CPU tier): the scanned balanced products
(s29_*: one Montgomery reduction per product or per sum of two, linear terms
folded into it), the halved slope f29_half3, and j29_dbl / j29_madd / x29_madd
built on them, with g1_mul_glv16 (dev/jobs.h) on top.

tests/native/g1fused_main.cpp is a stand-alone program that compares every
routine with the 32-bit code of dev/curve.h -- jac_dbl, jac_add_aff and jac_add
as projective points (cross-multiplied), g1_mul_glv and aff_mul as affine
points -- and checks that every result is balanced within the documented
bounds, on
  - 10^4 random operands in every representation the contracts accept,
  - the point at infinity, P + P through the additions (the doubling branch)
    and P + (-P),
  - coordinates at the extremes of the contracts (every limb at +-2^28 or
    +-2^29, limb 8 at its stated maximum, the sign patterns that make a whole
    column of limb products one sign),
  - chains of 1,000 steps that feed the outputs back in,
  - scalars 0, 1, r - 1, 2^127 and 2^127 lambda, and GLV halves 0, 1, 2^127
    (the top window's digit), 2^128 - 1 and the half whose window digits are
    all -8 or 8.
It is built twice: plainly, and with -fsanitize=signed-integer-overflow,undefined
so that a 64-bit column that overflows aborts the run; both print the same.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "g1fused_main.cpp")
OUT = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc", "dev")


def build(name, extra):
    exe = os.path.join(OUT, name)
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in deps):
        return exe
    os.makedirs(OUT, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + extra + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def sections():
    plain = build("g1fused", ["-O2"])
    san = build("g1fused_ubsan", ["-O1", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"])
    a = subprocess.run([plain], check=True, capture_output=True, text=True).stdout
    r = subprocess.run([san], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a signed overflow (or any other UB) aborts the sanitized run
    assert r.stdout == a
    return {t[0]: [int(v) for v in t[1:]] for t in (ln.split() for ln in a.splitlines())}


@pytest.mark.parametrize("name, at_least", [
    ("field_random", 60000), ("field_corners", 500), ("points_random", 30000), ("points_exceptional", 5000),
    ("points_extremes", 1200), ("chains", 8000), ("glv16", 48), ("glv16_halves", 144)])
def test_section(sections, name, at_least):
    checked, bad = sections[name][:2]
    assert bad == 0 and checked >= at_least


def test_window_shapes_were_reached(sections):
    top, _, eights = sections["glv16_shapes"]
    assert top >= 2 and eights >= 1
