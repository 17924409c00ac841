"""CPU tier of batched Pointcheval-Sanders verification (host/planner_ps.cpp,
dev/jobs.h job_verdict_gt / sx_gt_lane_one, the audit of SignedValues).

The reference is tests/ps_ref.py (pssign.SignVerifier.Verify restated over
ftsoracle.bn254); the fixture tests/golden/ps_golden.json carries its verdict
for every case.  The planner and the device job code are compiled for the host
(tests/native/ps_emu.cpp, TEST-ONLY) and run over the fixture and over seeded
single-bit tamperings; the same pass runs in a stand-alone program under
AddressSanitizer + UBSan (tests/native/ps_main.cpp)."""
import base64
import ctypes
import json
import os
import random
import subprocess

import pytest

import ps_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ps_golden.json")
NATIVE = os.path.join(ROOT, "tests", "native")
HOST_SRCS = [os.path.join(CSRC, "host", f) for f in ("planner_ps.cpp", "planner.cpp", "gojson.cpp")]
C, Z, R, P = S.C, S.Z, S.R, S.P
KINDS = {"signed_value", "randomized", "fresh", "wrong_m", "wrong_h", "s_negated", "swapped", "other_s",
         "both_infinity", "r_infinity", "s_infinity", "compressed", "off_curve", "ge_p", "plus_r"}


def _deps():
    return [os.path.join(d, f) for d in (os.path.join(CSRC, "dev"), os.path.join(CSRC, "host"))
            for f in os.listdir(d) if f.endswith(".h")]


def _build(out, srcs, flags):
    """compile srcs into tests/_build/<out> unless it is newer than its sources"""
    path = os.path.join(BUILD, out)
    deps = srcs + _deps()
    if os.path.exists(path) and os.path.getmtime(path) >= max(os.path.getmtime(p) for p in deps):
        return path
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-pthread"] + flags + srcs + ["-o", path], check=True)
    return path


def record(c):
    return bytes.fromhex(c["m"] + c["h"] + c["r"] + c["s"])


@pytest.fixture(scope="module")
def g():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pp_raw(g):
    return base64.b64decode(g["pp"])


@pytest.fixture(scope="module")
def pp(pp_raw):
    return Z.PublicParams.from_json(pp_raw)


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(_build("libpsemu.so", [os.path.join(NATIVE, "ps_emu.cpp")] + HOST_SRCS,
                             ["-O2", "-shared", "-fPIC"]))
    cp, sz, vp, ci = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    lib.ps_emu_create.restype = vp
    lib.ps_emu_create.argtypes = [cp, sz]
    lib.ps_emu_destroy.argtypes = [vp]
    lib.ps_emu_destroy.restype = None
    lib.ps_emu_set_fexp.argtypes = [vp, ci]
    lib.ps_emu_set_fexp.restype = None
    lib.ps_emu_verify.argtypes = [vp, sz, cp, ctypes.POINTER(ctypes.c_int32), ci]
    lib.ps_emu_audit.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), sz, ctypes.POINTER(sz)]
    lib.ps_emu_unity.argtypes = [cp, ctypes.c_uint32]
    return lib


@pytest.fixture(scope="module")
def emu(lib, pp_raw):
    h = lib.ps_emu_create(pp_raw, len(pp_raw))
    assert h
    yield h
    lib.ps_emu_destroy(h)


def emu_codes(lib, h, records, threads=1, fexp=0):
    n = len(records)
    codes = (ctypes.c_int32 * max(1, n))()
    lib.ps_emu_set_fexp(h, fexp)
    assert lib.ps_emu_verify(h, n, b"".join(records), codes, threads) == 0
    lib.ps_emu_set_fexp(h, 0)
    return list(codes)[:n]


# ---------------------------------------------------------------- the reference and the fixture
def test_fixture_covers_the_cases(g, pp):
    cases = g["cases"]
    assert {c["kind"] for c in cases} == KINDS
    assert [c["name"] for c in cases[:8]] == ["signed_value_%d" % i for i in range(8)]
    assert sum(c["kind"] == "randomized" for c in cases) == 3
    by = {c["name"]: c for c in cases}
    assert int(by["m_r_minus_1"]["m"], 16) == R - 1 and int(by["m_2_64"]["m"], 16) == 1 << 64
    assert int(by["m_h_plus_r"]["m"], 16) == 6 + R and int(by["m_h_plus_r"]["h"], 16) == Z.ps_hash(6) + R
    for c in cases:
        assert len(record(c)) == 192 and c["code"] in (0, 1, 14), c["name"]
    accept = {"signed_value", "randomized", "fresh", "both_infinity", "compressed", "ge_p", "plus_r"}
    for c in cases:
        want = 0 if c["kind"] in accept else (1 if c["kind"] == "off_curve" else 14)
        assert c["code"] == want, c["name"]
    assert by["both_infinity"]["r"] == by["both_infinity"]["s"] == "00" * 64
    assert by["r_infinity"]["r"] == "00" * 64 and by["s_infinity"]["s"] == "00" * 64
    assert int(by["r_compressed_0"]["r"][:2], 16) & 0x80
    assert int(by["r_coordinates_ge_p"]["r"][:64], 16) >= P and int(by["r_coordinates_ge_p"]["r"][64:], 16) >= P
    assert [bytes.fromhex(x["s"]) for x in cases[:8]] == [C.g1_bytes(s[1]) for s in pp.signed_values]
    assert os.path.getsize(GOLDEN) < 256 * 1024


def test_reference_agrees_with_the_fixture(g, pp):
    """at most eight recomputations (the pure-Python pairing costs seconds): one
    accept of each kind and the infinity cases"""
    names = ["signed_value_5", "randomized_1", "m_r_minus_1", "r_compressed_0", "m_h_plus_r", "both_infinity",
             "r_infinity", "s_infinity"]
    by = {c["name"]: c for c in g["cases"]}
    for nm in names:
        c = by[nm]
        code = S.ps_code(pp, bytes.fromhex(c["m"]), bytes.fromhex(c["h"]), bytes.fromhex(c["r"]),
                         bytes.fromhex(c["s"]))
        assert code == c["code"], nm


# ---------------------------------------------------------------- host emulation
def test_unity_lane_predicate(lib):
    """one is one; a value differing from one in any single coefficient is not,
    whichever sextet of the wave holds it and whatever the other lanes vote"""
    one = [0] * 12
    one[0] = 1

    def run(coef, sx):
        return lib.ps_emu_unity(b"".join(int(v % P).to_bytes(32, "big") for v in coef), sx)
    rng = random.Random(5)
    for sx in range(10):
        assert run(one, sx) == 3
        assert run([v + P for v in one], sx) == 3      # reduced on the way in: still one
        assert run([rng.randrange(P) for _ in range(12)], sx) == 0
        assert run([1] * 12, sx) == 0 and run([0] * 12, sx) == 0
        for q in range(12):
            for delta in (1, P - 1, rng.randrange(2, P - 1)):
                v = list(one)
                v[q] = (v[q] + delta) % P
                assert run(v, sx) == 0, (sx, q)
    swapped = [0] * 12
    swapped[1] = 1  # (0, 1) in the constant term's Fp2: i, not one
    assert run(swapped, 0) == 0


def test_emulation_matches_the_fixture(lib, emu, g):
    recs = [record(c) for c in g["cases"]]
    want = [c["code"] for c in g["cases"]]
    for fexp in (0, 1):
        assert emu_codes(lib, emu, recs, 1, fexp) == want
    # a wave's worth and more, in several planner pieces (32 items at least each): neighbours keep their codes
    many = (recs * 4)[:100]
    assert emu_codes(lib, emu, many, 3) == (want * 4)[:100]
    for n in (1, 9, 10, 11):
        assert emu_codes(lib, emu, recs[8:8 + n]) == want[8:8 + n]
    assert emu_codes(lib, emu, []) == []


def test_emulation_rejects_single_bit_tamperings(lib, emu, g):
    """200 seeded single-bit flips of valid items: a flip in m, h, R or S never
    verifies (it rejects, or the point no longer decodes)"""
    rng = random.Random(0x5053)
    valid = [record(c) for c in g["cases"] if c["kind"] in ("signed_value", "randomized", "fresh")]
    recs, where = [], []
    for t in range(200):
        b = bytearray(valid[t % len(valid)])
        field = t % 4
        lo, hi = ((0, 32), (32, 64), (64, 128), (128, 192))[field]
        byte, bit = rng.randrange(lo, hi), rng.randrange(8)
        b[byte] ^= 1 << bit
        recs.append(bytes(b))
        where.append((field, byte, bit))
    codes = emu_codes(lib, emu, recs, 4)
    for c, w in zip(codes, where):
        assert c in ((14,) if w[0] < 2 else (1, 14)), w
    # every kind of outcome occurs, so the codes are not one constant
    assert 14 in codes and 1 in codes
    assert emu_codes(lib, emu, valid[:3]) == [0, 0, 0]


def test_emulated_audit(lib, g, pp, pp_raw):
    def audit(raw, cap=None):
        h = lib.ps_emu_create(raw, len(raw))
        assert h
        try:
            count = ctypes.c_size_t()
            n = len(Z.PublicParams.from_json(raw).signed_values) if cap is None else cap
            codes = (ctypes.c_int32 * max(1, n))()
            rc = lib.ps_emu_audit(h, codes, n, ctypes.byref(count))
            return rc, count.value, list(codes)[:n]
        finally:
            lib.ps_emu_destroy(h)
    assert audit(pp_raw) == (0, 8, [0] * 8)
    rc, count, _ = audit(pp_raw, 7)
    assert rc != 0 and count == 8
    sw = Z.PublicParams.from_json(pp_raw)
    sw.signed_values[3], sw.signed_values[5] = sw.signed_values[5], sw.signed_values[3]
    assert Z.validate_json(sw.to_json()) == ""
    assert audit(sw.to_json()) == (0, 8, [0, 0, 0, 14, 0, 14, 0, 0])
    inf = Z.PublicParams.from_json(pp_raw)
    inf.signed_values[2] = (None, None)
    assert audit(inf.to_json()) == (0, 8, [0, 0, 14, 0, 0, 0, 0, 0])
    rec = (2).to_bytes(32, "big") + Z.ps_hash(2).to_bytes(32, "big") + bytes(128)
    h = lib.ps_emu_create(pp_raw, len(pp_raw))
    try:
        assert emu_codes(lib, h, [rec]) == [0]   # the item call keeps the reference's skip
    finally:
        lib.ps_emu_destroy(h)


def test_pass_under_sanitizers(g, pp_raw, tmp_path):
    """the emulated pass over the fixture in a stand-alone ASan + UBSan program"""
    srcs = [os.path.join(NATIVE, "ps_main.cpp"), os.path.join(NATIVE, "ps_emu.cpp")] + HOST_SRCS
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    try:  # the sanitizer runtimes inside the program, where the toolchain ships them as archives
        exe = _build("ps_main", srcs, flags + ["-static-libasan", "-static-libubsan"])
    except subprocess.CalledProcessError:
        exe = _build("ps_main", srcs, flags)
    items = tmp_path / "cases.txt"
    lines = [pp_raw.hex()]
    cases = g["cases"] * 3   # 78 items: two planner pieces in the three-thread run
    for c in cases:
        lines.append("%s %s %s %s %d" % (c["m"], c["h"], c["r"], c["s"], c["code"]))
    items.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(items)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.startswith("%d cases x 2 runs, 8 audited, 0 mismatches" % len(cases))
