"""CPU: the host side the four batched signature calls share
(csrc/host/sigpipe.h: the chunk splitter, the two-slot pass driver and the
message layout) driven by a stand-alone program, tests/native/sigpipe_main.cpp,
built plainly and under AddressSanitizer + UBSan.  The program compares the
splitter's boundaries with the loop the runtimes used to carry inline, asserts
through recorded submit / collect events that chunk c takes slot c & 1, that no
slot is submitted into with its pass uncollected, that every pass is collected
exactly once and that after an injected error no submit follows, both slots are
collected and the first error is returned, and checks the layout's alignment,
sharing and non-overlap for both remainders the library uses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sigpipe_main.cpp")
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


@pytest.mark.parametrize("seed", [0, 1, 20261])
def test_sigpipe_sequences(seed):
    _run(_build("sigpipe_main", ["-O2"]), seed)


def test_sigpipe_under_sanitizers():
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    try:  # the sanitizer runtimes inside the program, where the toolchain ships them as archives
        exe = _build("sigpipe_main_san", flags + ["-static-libasan", "-static-libubsan"])
    except subprocess.CalledProcessError:
        exe = _build("sigpipe_main_san", flags)
    _run(exe, 3)
