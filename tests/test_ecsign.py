"""CPU tier of batched ECDSA P-256 signing (dev/ecsign.h, dev/hmac256.h,
host/x509id.cpp encode_ecdsa_signature).

The reference is tests/ecsign_ref.py (RFC 6979 nonce, low-S, DER over
tests/p256_ref.py), pinned here by RFC 6979 A.2.5.  The device headers are
compiled for the host (tests/native/ecsign_emu.cpp, TEST-ONLY) and compared
byte for byte; the job and the encoder also run over the fixture in a
stand-alone program under AddressSanitizer + UBSan (tests/native/ecsign_main.cpp)."""
import ctypes
import hashlib
import hmac
import json
import os
import random
import shutil
import subprocess

import pytest

import ecsign_ref as S
import p256_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ecsign_golden.json")
NATIVE = os.path.join(ROOT, "tests", "native")
HOST_SRCS = [os.path.join(CSRC, "host", f) for f in ("x509id.cpp", "idemix.cpp", "gojson.cpp")]
P, N = R.P, R.N

RFC_X = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
RFC_UX = 0x60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6
RFC_UY = 0x7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299
RFC = {  # message -> (k, r, s as the RFC prints it)
    b"sample": (0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60,
                0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716,
                0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8),
    b"test": (0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0,
              0xF1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367,
              0x019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083),
}


def _deps():
    return [os.path.join(d, f) for d in (os.path.join(CSRC, "dev"), os.path.join(CSRC, "host"))
            for f in os.listdir(d) if f.endswith(".h")]


def _build(out, srcs, flags, extra_deps=()):
    """compile srcs into tests/_build/<out> unless it is newer than its sources"""
    path = os.path.join(BUILD, out)
    deps = srcs + _deps() + list(extra_deps)
    if os.path.exists(path) and os.path.getmtime(path) >= max(os.path.getmtime(p) for p in deps):
        return path
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-pthread"] + flags + srcs + ["-o", path], check=True)
    return path


@pytest.fixture(scope="module")
def g():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(_build("libecsignemu.so", [os.path.join(NATIVE, "ecsign_emu.cpp")] + HOST_SRCS,
                             ["-O2", "-shared", "-fPIC"]))
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    lib.ecsign_emu_hmac.argtypes = [cp, cp, sz, cp]
    lib.ecsign_emu_hmac.restype = None
    lib.ecsign_emu_nonce.argtypes = [cp, cp, sz, cp, cp]
    lib.ecsign_emu_nonce.restype = None
    lib.ecsign_emu_retry.argtypes = [cp, cp]
    lib.ecsign_emu_retry.restype = None
    lib.ecsign_emu_fixed.argtypes = [cp, ctypes.c_int, ctypes.c_int, cp]
    lib.ecsign_emu_fixed_parts.argtypes = [cp, cp]
    lib.ecsign_emu_x_mod_n.argtypes = [cp, cp]
    lib.ecsign_emu_x_mod_n.restype = None
    lib.ecsign_emu_low_s.argtypes = [cp, cp]
    lib.ecsign_emu_low_s.restype = None
    lib.ecsign_emu_encode.argtypes = [cp, cp, cp]
    lib.ecsign_emu_encode.restype = sz
    lib.ecsign_emu_decode.argtypes = [cp, sz, cp, cp]
    lib.ecsign_emu_sign.argtypes = [cp, cp, sz, cp, cp, ctypes.POINTER(sz)]
    return lib


@pytest.fixture(scope="module")
def vemu():
    """the emulated verifier of tests/test_ecdsa.py (the same build recipe and output)"""
    lib = ctypes.CDLL(_build("libecdsaemu.so", [os.path.join(NATIVE, "ecdsa_emu.cpp")] + HOST_SRCS,
                             ["-O2", "-shared", "-fPIC"]))
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    lib.ecdsa_emu_verify.argtypes = [cp, sz, cp, cp, sz, cp, sz]
    return lib


def b32(v):
    return v.to_bytes(32, "big")


def i32(b):
    return int.from_bytes(b, "big")


def emu_sign(emu, d, msg, entropy):
    sig = ctypes.create_string_buffer(72)
    ln = ctypes.c_size_t()
    assert emu.ecsign_emu_sign(b32(d), msg, len(msg), entropy, sig, ctypes.byref(ln)) == 0
    return sig.raw[:ln.value]


# ---------------------------------------------------------------- the reference itself
def test_reference_reproduces_rfc6979_a25():
    assert R.mul(R.G, RFC_X) == (RFC_UX, RFC_UY)
    for msg, (k, r, s) in RFC.items():
        assert S.nonce(RFC_X, msg) == k
        assert S.sign_rs(RFC_X, msg) == (r, min(s, N - s))
        assert R.verify(S.identity_of(RFC_X), msg, S.sign(RFC_X, msg)) == R.OK
    # "sample" exercises the flip, "test" a 32-byte INTEGER without a pad
    assert RFC[b"sample"][2] > R.HALF_N and RFC[b"test"][2] <= R.HALF_N
    der = S.sign(RFC_X, b"test")
    assert der[-34:-32] == b"\x02\x20"


def test_fixture_is_the_references_and_covers_the_issue_list(g):
    cases = g["cases"]
    assert len(cases) >= 40 and len(g["keys"]) <= 8
    for c in cases:
        k = g["keys"][c["key"]]
        ent = bytes.fromhex(c["entropy"]) if c["entropy"] else None
        assert S.sign(int(k["d"], 16), bytes.fromhex(c["msg"]), ent).hex() == c["sig"], c["name"]
    ds = {int(k["d"], 16) for k in g["keys"].values()}
    assert {1, N - 1, RFC_X} <= ds
    lens = {len(c["msg"]) // 2 for c in cases}
    assert {0, 55, 56, 63, 64, 65} <= lens and any(9000 <= x <= 10000 for x in lens)
    assert any(c["entropy"] for c in cases) and any(not c["entropy"] for c in cases)
    by = {c["name"]: c for c in cases}
    assert by["rfc_sample"]["sig"] == R.encode_signature(RFC[b"sample"][1], N - RFC[b"sample"][2]).hex()
    assert by["rfc_test"]["sig"] == R.encode_signature(*RFC[b"test"][1:]).hex()
    # one seed under two messages: the nonces (so the r values) differ
    ra = R.parse_signature(bytes.fromhex(by["seed_reuse_a"]["sig"]))[0]
    rb = R.parse_signature(bytes.fromhex(by["seed_reuse_b"]["sig"]))[0]
    assert by["seed_reuse_a"]["entropy"] == by["seed_reuse_b"]["entropy"] and ra != rb


# ---------------------------------------------------------------- HMAC and the DRBG
def test_hmac_sha256(emu):
    rng = random.Random(11)
    out = ctypes.create_string_buffer(32)
    for ln in (0, 31, 32, 55, 56, 63, 64, 65, 97, 119, 120, 128, 129):
        for key in (bytes(32), b"\xff" * 32, bytes(rng.randrange(256) for _ in range(32))):
            data = bytes(rng.randrange(256) for _ in range(ln))
            emu.ecsign_emu_hmac(key, data, ln, out)
            assert out.raw == hmac.new(key, data, hashlib.sha256).digest(), ln


def test_nonce_matches_reference(emu):
    rng = random.Random(12)
    out = ctypes.create_string_buffer(32)
    for msg, (k, _, _) in RFC.items():
        emu.ecsign_emu_nonce(b32(RFC_X), msg, len(msg), None, out)
        assert i32(out.raw) == k
    for i in range(50):
        d = rng.choice([1, N - 1, rng.randrange(1, N), rng.randrange(1, N)])
        msg = bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 55, 56, 64, 200, rng.randrange(300)])))
        ent = bytes(rng.randrange(256) for _ in range(32)) if i % 2 else None
        emu.ecsign_emu_nonce(b32(d), msg, len(msg), ent, out)
        assert i32(out.raw) == S.nonce(d, msg, ent), i
    # a digest at or above n: bits2octets reduces it, the reference does the same
    # (no SHA-256 preimage is known, so only the Python side's own reduction is checked)
    K, V = S.drbg_init(5, b32(N + 7))
    assert (K, V) == S.drbg_init(5, b32(7))


def test_drbg_retry_step(emu):
    """no real input reaches the retry: one step from given states against Python"""
    rng = random.Random(13)
    for _ in range(10):
        K0 = bytes(rng.randrange(256) for _ in range(32))
        V0 = bytes(rng.randrange(256) for _ in range(32))
        K, V = ctypes.create_string_buffer(K0, 32), ctypes.create_string_buffer(V0, 32)
        emu.ecsign_emu_retry(K, V)
        Kw, Vw = S.drbg_retry(K0, V0)
        assert K.raw == Kw
        assert V.raw == hmac.new(Kw, Vw, hashlib.sha256).digest()


# ---------------------------------------------------------------- curve and scalar pieces
def aff(out, inf):
    return None if inf else (i32(out.raw[:32]), i32(out.raw[32:]))


def test_uniform_fixed_base_product(emu):
    rng = random.Random(14)
    out = ctypes.create_string_buffer(64)
    ks = [1, N - 1, 1 << 248]
    ks += [v << (8 * j) for j, v in ((0, 0x5a), (13, 0xff), (31, 0x7f))]  # 31 zero bytes
    ks += [int("00ff" * 16, 16), int("ff00" * 16, 16) % N, int("0001" * 16, 16)]  # alternating zero bytes
    ks += [rng.randrange(1, N) for _ in range(20)]
    for k in ks:
        want = R.mul(R.G, k)
        assert aff(out, emu.ecsign_emu_fixed(b32(k), 0, 32, out)) == want, hex(k)
        assert aff(out, emu.ecsign_emu_fixed_parts(b32(k), out)) == want, hex(k)
        # each of the four 8-window parts on its own, summed by the reference
        total = None
        for p in range(4):
            part = aff(out, emu.ecsign_emu_fixed(b32(k), 8 * p, 8, out))
            chunk = (k >> (64 * p)) & (2**64 - 1)
            assert part == (R.mul(R.G, chunk << (64 * p)) if chunk else None), (hex(k), p)
            total = R.add(total, part) if (total and part) else (total or part)
        assert total == want, hex(k)


def test_x_mod_n(emu):
    out = ctypes.create_string_buffer(32)
    for x in (N - 1, N, N + 1, P - 1, 0, 1):
        emu.ecsign_emu_x_mod_n(b32(x), out)
        assert i32(out.raw) == x % N, hex(x)


def test_low_s(emu):
    out = ctypes.create_string_buffer(32)
    for s, want in ((R.HALF_N, R.HALF_N), (R.HALF_N + 1, R.HALF_N), (1, 1), (N - 1, 1), (R.HALF_N - 1, R.HALF_N - 1),
                    (R.HALF_N + 2, R.HALF_N - 1)):
        assert (N + 1) // 2 == R.HALF_N + 1
        emu.ecsign_emu_low_s(b32(s), out)
        assert i32(out.raw) == want, hex(s)


def test_der_encoder(emu, g):
    out, r2, s2 = ctypes.create_string_buffer(72), ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    vals = [1, int("7f" + "ff" * 31, 16), int("80" + "00" * 31, 16), int("ab" * 31, 16), int("12" * 31, 16), 0x80, 0xff,
            N - 1, R.HALF_N]
    pairs = [(a, b) for a in vals for b in vals]
    pairs += [R.parse_signature(bytes.fromhex(c["sig"])) for c in g["cases"]]
    for r, s in pairs:
        n = emu.ecsign_emu_encode(b32(r), b32(s), out)
        der = out.raw[:n]
        assert der == R.encode_signature(r, s), (hex(r), hex(s))
        assert R.parse_signature(der) == (r, s)
        ok = 1 <= r < N and 1 <= s <= R.HALF_N
        assert n <= (71 if s <= R.HALF_N else 72)
        assert emu.ecsign_emu_decode(der, n, r2, s2) == (0 if ok else 10)
        if ok:
            assert (i32(r2.raw), i32(s2.raw)) == (r, s)


# ---------------------------------------------------------------- the whole job
def test_job_on_every_fixture_case(emu, vemu, g, tmp_path):
    openssl = shutil.which("openssl")
    pems = {}
    for name, k in g["keys"].items():
        xy = bytes.fromhex(k["xy"])
        assert xy == b"".join(b32(v) for v in R.mul(R.G, int(k["d"], 16)))
        pems[name] = tmp_path / (name + ".pem")
        pems[name].write_bytes(R.pem_encode("PUBLIC KEY", R.spki_der(i32(xy[:32]), i32(xy[32:]))))
    for c in g["cases"]:
        k = g["keys"][c["key"]]
        d, msg = int(k["d"], 16), bytes.fromhex(c["msg"])
        ent = bytes.fromhex(c["entropy"]) if c["entropy"] else None
        sig = emu_sign(emu, d, msg, ent)
        assert sig.hex() == c["sig"], c["name"]
        ident, xy = bytes.fromhex(k["identity"]), bytes.fromhex(k["xy"])
        assert R.verify(ident, msg, sig) == R.OK, c["name"]
        assert vemu.ecdsa_emu_verify(ident, len(ident), None, msg, len(msg), sig, len(sig)) == 0, c["name"]
        assert vemu.ecdsa_emu_verify(None, 0, xy, msg, len(msg), sig, len(sig)) == 0, c["name"]
        assert vemu.ecdsa_emu_verify(None, 0, xy, msg + b"x", len(msg) + 1, sig, len(sig)) == 10, c["name"]
        if openssl:
            (tmp_path / "msg").write_bytes(msg)
            (tmp_path / "sig").write_bytes(sig)
            r = subprocess.run([openssl, "dgst", "-sha256", "-verify", str(pems[c["key"]]), "-signature",
                                str(tmp_path / "sig"), str(tmp_path / "msg")], capture_output=True, text=True)
            assert r.returncode == 0 and "Verified OK" in r.stdout, (c["name"], r.stdout, r.stderr)


def test_job_under_sanitizers(g, tmp_path):
    """the emulated job and the encoder over the fixture in a stand-alone ASan + UBSan program"""
    srcs = [os.path.join(NATIVE, "ecsign_main.cpp"), os.path.join(NATIVE, "ecsign_emu.cpp")] + HOST_SRCS
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    try:  # the sanitizer runtimes inside the program, where the toolchain ships them as archives
        exe = _build("ecsign_main", srcs, flags + ["-static-libasan", "-static-libubsan"])
    except subprocess.CalledProcessError:
        exe = _build("ecsign_main", srcs, flags)
    items = tmp_path / "cases.txt"
    items.write_text("".join("%s %s %s %s\n" % (g["keys"][c["key"]]["d"], c["msg"] or "-", c["entropy"] or "-", c["sig"])
                             for c in g["cases"]))
    r = subprocess.run([exe, str(items)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.startswith("%d cases, 0 mismatches" % len(g["cases"]))
