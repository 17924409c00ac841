"""CPU: the job engine's placement rules (csrc/host/engine_policy.h: which
stream triple a device pass takes, and whether it may be enqueued behind a
running pass) driven through random arrival and completion sequences by a
stand-alone program, tests/native/engine_policy_main.cpp, built plainly and
under AddressSanitizer + UBSan.  The program asserts that no triple ever holds
more than 1 + lookahead passes, that the triples' counts differ by at most one
while a big call keeps full passes pending, that a partial pass never goes
behind a running one, and that lookahead = 0 takes the triples in the order the
engine's slots were taken before lookahead existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "engine_policy_main.cpp")
OUT = os.path.join(ROOT, "tests", "_build")


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + [SRC, "-o", exe], check=True)
    return exe


def _run(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 1000000  # the sequences were really run


@pytest.mark.parametrize("seed", [0, 1, 20260])
def test_policy_sequences(seed):
    _run(_build("engine_policy_main", ["-O2"]), seed)


def test_policy_under_sanitizers():
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    try:  # the sanitizer runtimes inside the program, where the toolchain ships them as archives
        exe = _build("engine_policy_main_san", flags + ["-static-libasan", "-static-libubsan"])
    except subprocess.CalledProcessError:
        exe = _build("engine_policy_main_san", flags)
    _run(exe, 3)
