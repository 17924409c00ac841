"""The fused G2 formulas of dev/g2x29.h and dev/g2lines29.h (CPU tier): the
two-row scanned sums (q2_scan: one Montgomery reduction per row for a sum of up
to two Fp2 terms with a linear term folded in), x2q_madd built on them, and the
line steps g2l_dbl / g2l_add with the whole 88-step chain of k_g2lines1.

tests/native/g2fused_main.cpp is a stand-alone program that compares every
routine with the 32-bit code -- fp2 arithmetic, jac_add_aff on Fp2 as
projective points (cross-multiplied), dbl_step_inl / add_step_inl and
job_g2lines_parts: the new point equals the old one projectively and each line
equals the reference's up to one factor in Fp -- and checks that every result
is balanced within the documented bounds, on
  - 10^4 random operands in every representation the contracts accept,
  - the extremes of the contracts (every limb at +-2^28 or a multiple of it as
    allowed, limb 8 at its stated maximum, the sign patterns that make a whole
    column of limb products one sign),
  - the accumulator at infinity, P + P through x2q_madd (the doubling flag),
    P + (-P), t' at infinity and R at infinity,
  - chains of 1,000 steps that feed the outputs back in,
  - the full 88-step chain for 64 random (t', R).
It is built twice: plainly, and with -fsanitize=signed-integer-overflow,undefined
so that a 64-bit column that overflows aborts the run; both print the same.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "g2fused_main.cpp")
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
    plain = build("g2fused", ["-O2"])
    san = build("g2fused_ubsan", ["-O1", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"])
    a = subprocess.run([plain], check=True, capture_output=True, text=True).stdout
    r = subprocess.run([san], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]  # a signed overflow (or any other UB) aborts the sanitized run
    assert r.stdout == a
    return {t[0]: [int(v) for v in t[1:]] for t in (ln.split() for ln in a.splitlines())}


@pytest.mark.parametrize("name, at_least", [
    ("scan_random", 80000), ("scan_corners", 28000), ("madd_random", 10000), ("madd_exceptional", 2000),
    ("madd_extremes", 1296), ("madd_chains", 4000), ("steps_random", 20000), ("steps_extremes", 2592),
    ("steps_chains", 4000), ("chain88", 64 * 88)])
def test_section(sections, name, at_least):
    checked, bad = sections[name][:2]
    assert bad == 0 and checked >= at_least


def test_infinity_lines_were_reached(sections):
    assert sections["chain88_infinity_lines"][0] == 3 * 88
