"""Token requests with their signatures (ftz_verify_signed_token_requests), CPU
tier: the restatement tests/signed_request_ref.py against the fixture
tests/golden/signed_requests.json, the signed message the product assembles
against der_encode_token_request, and the product's orchestration
(host/request.cpp verify_signed_token_requests) over the host builds of the
proof, idemix and ECDSA job code -- a library this file builds from
tests/native/ (reqsig_emu.cpp beside the sources of libftsemu.so) -- and, for
the merge and the message assembly alone, in the stand-alone program
tests/native/reqsig_main.cpp under AddressSanitizer + UBSan.

The ASN.1 mutation cases are the 2000 seeded mutations of
tests/test_requests.py::test_asn1_decoder_mutation_fuzz (tests/golden/
fuzz_cases.json holds proof mutations only)."""
import base64
import copy
import ctypes
import json
import os
import random
import subprocess

import pytest

import gen_signed_requests as G
import signed_request_ref as V
import signed_requests_fx as F
from ftsoracle import idemix as I
from ftsoracle import request as R
from ftsoracle import zkat as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HOST = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc", "host")
OUT = os.path.join(ROOT, "tests", "_build")
CURVE_ID = {"bn254": 1, "fp256bn": 0}


@pytest.fixture(scope="module")
def fx():
    return F.load()


@pytest.fixture(scope="module")
def zk():
    return G.corpus_zk()


@pytest.fixture(scope="module")
def ipks():
    def raw(name):
        with open(os.path.join(ROOT, "tests", "golden", name)) as f:
            return bytes.fromhex(json.load(f)["ipk"])
    return {"bn254": raw("idemix_bn254_golden.json"), "fp256bn": raw("idemix_golden.json")}


def ref_signers(cfg, ipks):
    ipk = None
    if cfg["ix"]:
        ipk = I.IssuerPKBn254(ipks["bn254"]) if cfg["curve"] == "bn254" else I.IssuerPK(ipks["fp256bn"])
    return V.Signers(ipk, V.CURVE_BN254 if cfg["curve"] == "bn254" else V.CURVE_FP256BN, cfg["ec"], cfg["auditor"],
                     cfg["issuers"])


# ------------------------------------------------------------------ the fixture and the restatement
def test_fixture_covers_every_code(fx):
    codes = {r["expect"] for r in fx["requests"]}
    assert codes >= {V.OK, V.ERR_PARSE, V.ERR_IDENTITY, V.ERR_UNSUPPORTED, V.ERR_SIGNATURE, V.ERR_ISSUER, V.ERR_INPUT,
                     V.ERR_OWNER, Z.ERR_MALFORMED, Z.ERR_WF, Z.ERR_RANGE, Z.ERR_MEMBERSHIP, Z.ERR_PANIC}
    assert sum(r["config"] == "fp256bn" for r in fx["requests"]) >= 3
    names = [r["name"] for r in fx["requests"]]
    assert len(set(names)) == len(names)


def test_restatement_gives_fixture_verdicts(fx, zk, ipks):
    pp = Z.PublicParams.from_json(fx["pp"].encode())
    for r in fx["requests"]:
        cfg = F.config(fx, r["config"])
        got = V.verify_signed_token_request(pp, ref_signers(cfg, ipks), r["raw_b"], r["binding_b"],
                                            fx["ledgers"][cfg["curve"]].get, zk=zk)
        assert list(got) == [r["expect"], r["failed_action"]], r["name"]


# ------------------------------------------------------------------ the emulation library
def build_lib():
    srcs = [os.path.join(NATIVE, f) for f in ("emu.cpp", "emu_exec.cpp", "sx_emu.cpp", "msm_emu.cpp", "idemix_emu.cpp",
                                               "ecdsa_emu.cpp", "reqsig_emu.cpp")]
    srcs += [os.path.join(HOST, f) for f in ("planner.cpp", "planner_prove.cpp", "gojson.cpp", "request.cpp",
                                              "idemix.cpp", "x509id.cpp")]
    lib = os.path.join(OUT, "libftsreqsig.so")
    deps = srcs + [os.path.join(d, f) for d in (os.path.join(ROOT, "fabric-token-sdk_amd", "csrc", "dev"), HOST)
                   for f in os.listdir(d) if f.endswith(".h")]
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(p) for p in deps):
        return lib
    os.makedirs(OUT, exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread"] + srcs
                   + ["-o", lib], check=True)
    return lib


@pytest.fixture(scope="module")
def lib():
    from zkatdlog import _abi as A
    L = ctypes.CDLL(build_lib())
    vp, sz, i32p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)
    L.emu_ctx_create.restype = vp
    L.emu_ctx_create.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p, sz]
    L.emu_ctx_destroy.argtypes = [vp]
    L.emu_idemix_create_curve.restype = vp
    L.emu_idemix_create_curve.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_char_p, sz]
    L.emu_idemix_destroy.argtypes = [vp]
    L.emu_signed_message.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p, sz, ctypes.c_char_p, sz,
                                     ctypes.POINTER(sz)]
    L.emu_verify_signed_token_requests.argtypes = [vp, vp, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(A.Bytes),
                                                   sz, sz, ctypes.POINTER(A.SignedRequest), vp, vp, sz, sz,
                                                   ctypes.c_int, i32p, i32p]
    return L


@pytest.fixture(scope="module")
def handles(lib, fx, ipks):
    err = ctypes.create_string_buffer(256)
    pp = fx["pp"].encode()
    h = {"ctx": lib.emu_ctx_create(pp, len(pp), err, 256)}
    assert h["ctx"], err.value
    for c, k in ipks.items():
        h[c] = lib.emu_idemix_create_curve(k, len(k), CURVE_ID[c], err, 256)
        assert h[c], err.value
    yield h
    for c in ipks:
        lib.emu_idemix_destroy(h[c])
    lib.emu_ctx_destroy(h["ctx"])


def emu_run(lib, handles, cfg, raws, bindings, ledger, chunk=0, inflight=0, threads=0, calls=None):
    """the emulated ftz_verify_signed_token_requests under one signer configuration"""
    from zkatdlog import _abi as A
    arr, keep = A.pack_signed_requests(raws, bindings)
    ia, ikeep = A.pack_bytes(cfg["issuers"])
    n = len(raws)
    codes = (ctypes.c_int32 * max(1, n))()
    failed = (ctypes.c_int32 * max(1, n))()
    cb = A.get_states_callback(ledger)
    if calls is not None:  # count the callbacks, not the keys
        inner = cb

        def wrap(user, m, keys, vals):
            calls.append(m)
            return inner(user, m, keys, vals)
        cb = A.GET_STATES_FN(wrap)
    aud = cfg["auditor"]
    rc = lib.emu_verify_signed_token_requests(
        handles["ctx"], handles[cfg["curve"]] if cfg["ix"] else None, 1 if cfg["ec"] else 0,
        None if aud is None else (aud if aud else b"\x00"), 0 if aud is None else len(aud), ia, len(ikeep), n, arr,
        ctypes.cast(cb, ctypes.c_void_p), None, chunk, inflight, threads, codes, failed)
    assert rc == 0
    return [(codes[k], failed[k]) for k in range(n)]


def by_config(fx):
    out = {}
    for r in fx["requests"]:
        out.setdefault(r["config"], []).append(r)
    return out


def test_signed_message_bytes(lib, fx):
    """signed = der_encode_token_request([issues, transfers, [], []]) + binding on every fixture
    request and every seeded ASN.1 mutation that decodes; what does not decode has none"""
    def check(raw, binding):
        n = ctypes.c_size_t()
        buf = ctypes.create_string_buffer(len(raw) + len(binding) + 16)
        rc = lib.emu_signed_message(raw, len(raw), binding, len(binding), buf, len(buf), ctypes.byref(n))
        try:
            f = R.der_token_request(raw)
        except R.Asn1Error:
            assert rc == -1
            return 0
        assert rc == 0
        assert buf.raw[:n.value] == R.der_encode_token_request([f[0], f[1], [], []]) + binding
        return 1
    for r in fx["requests"]:
        check(r["raw_b"], r["binding_b"])
    r = next(x for x in fx["requests"] if x["name"] == "trailing_bytes_after_sequence_not_signed")
    assert b"garbage" in r["raw_b"] and b"garbage" not in V.signed_message(r["raw_b"], b"")
    rng = random.Random(20261017)
    raws = [x for x in fx["base"]["raw"].values() if len(x) > 4]
    decoded = 0
    for k in range(2000):
        b = bytearray(rng.choice(raws))
        mode = k % 4
        if mode == 0:
            b[rng.randrange(len(b))] ^= rng.randrange(1, 256)
        elif mode == 1:
            b[rng.randrange(min(len(b), 12))] = rng.randrange(256)
        elif mode == 2:
            del b[rng.randrange(1, len(b)):]
        else:
            b += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        decoded += check(bytes(b), b"tx%d" % k if k % 3 else b"")
    assert decoded > 500


def test_emu_gives_fixture_verdicts(lib, handles, fx):
    got, want = {}, {}
    for name, rs in by_config(fx).items():
        cfg = F.config(fx, name)
        out = emu_run(lib, handles, cfg, [r["raw_b"] for r in rs], [r["binding_b"] for r in rs],
                      fx["ledgers"][cfg["curve"]])
        for r, o in zip(rs, out):
            got[r["name"]], want[r["name"]] = o, (r["expect"], r["failed_action"])
    assert got == want


@pytest.mark.parametrize("chunk,inflight,threads", [(1, 1, 0), (3, 2, 3), (7, 4, 4)])
def test_emu_pipeline_knobs(lib, handles, fx, chunk, inflight, threads):
    """every verdict whatever the chunking; the ledger is asked at most once per chunk"""
    rs = by_config(fx)["A"] * 2
    cfg = F.config(fx, "A")
    calls = []
    out = emu_run(lib, handles, cfg, [r["raw_b"] for r in rs], [r["binding_b"] for r in rs], fx["ledgers"]["bn254"],
                  chunk, inflight, threads, calls)
    assert out == [(r["expect"], r["failed_action"]) for r in rs]
    assert len(calls) <= (len(rs) + chunk - 1) // chunk + 4  # the first chunks are chunk/8, /4, /2 (at least 1)


def mutations(fx, count, seed):
    """`count` requests of configuration A with one byte of a signature, of an owner or of the
    binding changed: (raw, binding) and the ledger they need"""
    rng = random.Random(seed)
    base = fx["base"]
    pool = [r for r in fx["requests"] if r["config"] == "A" and r["expect"] == 0 and "raw" not in r
            and 1 <= len(r["transfers"]) <= 2 and len(r["issues"]) <= 1]
    ledger = dict(fx["ledgers"]["bn254"])
    out = []
    for k in range(count):
        r = copy.deepcopy({x: v for x, v in rng.choice(pool).items() if x not in ("raw_b", "binding_b")})
        binding = r["binding"].encode()
        what = k % 3
        if what == 0:
            which, i = rng.choice([(w, i) for w in ("sigs", "auditor_sigs") for i, x in enumerate(r[w]) if x])
            s = bytearray(bytes.fromhex(r[which][i]))
            s[rng.randrange(len(s))] ^= rng.randrange(1, 256)
            r[which][i] = bytes(s).hex()
        elif what == 1:
            t = rng.randrange(len(r["transfers"]))
            keys = json.loads(F.action(base, r["transfers"][t]))["Inputs"]
            key = rng.choice(keys)
            own = bytearray(bytes.fromhex(fx["owners"]["bn254"][key]))
            own[rng.randrange(len(own))] ^= rng.randrange(1, 256)
            new = "mut-%d" % k
            ledger[new] = base["ledger_b"][key].replace(F.BASE_OWNER, base64.b64encode(bytes(own)))
            r["transfers"][t] = dict(r["transfers"][t], sub=r["transfers"][t].get("sub", []) + [F.with_key(key, new)])
        else:
            b = bytearray(binding)
            b[rng.randrange(len(b))] ^= rng.randrange(1, 256)
            binding = bytes(b)
        out.append((F.raw_request(base, r), binding))
    return out, ledger


def test_emu_random_mutations(lib, handles, fx, zk, ipks):
    """300 single-byte mutations of signatures, owners and bindings, labelled by the restatement"""
    muts, ledger = mutations(fx, 300, 20261020)
    cfg = F.config(fx, "A")
    pp = Z.PublicParams.from_json(fx["pp"].encode())
    sg = ref_signers(cfg, ipks)
    want = [tuple(V.verify_signed_token_request(pp, sg, raw, b, ledger.get, zk=zk)) for raw, b in muts]
    assert V.ERR_SIGNATURE in {c for c, _ in want}
    got = emu_run(lib, handles, cfg, [m[0] for m in muts], [m[1] for m in muts], ledger, chunk=64, inflight=2,
                  threads=4)
    assert got == want


# ------------------------------------------------------------------ the stand-alone program
def fnv(*parts):
    """reqsig_main.cpp fnv: FNV-1a over each part's 8-byte little-endian length, then its bytes"""
    h = 0xCBF29CE484222325
    for p in parts:
        for c in len(p).to_bytes(8, "little") + bytes(p):
            h = ((h ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def write_job(path, fx, zk, ipks, groups, monkeypatch):
    """groups: [(configuration name, ledger, [(raw, binding)])].  Every request is labelled by the
    restatement, and every check the restatement evaluates on the way is recorded for reqsig_main:
    proofs, owner and x509 verifiers, signature checks"""
    from ftsoracle import bn254 as C
    tab = {}

    def rec_zk(pp, kind, ins, outs, proof, anonymous):
        code = zk(pp, kind, ins, outs, proof, anonymous)
        head = bytes([1 if kind == "transfer" else 0, 1 if anonymous else 0])
        tab[("zk", fnv(head, b"".join(C.g1_bytes(p) for p in ins), b"".join(C.g1_bytes(p) for p in outs), proof))] = code
        return code
    x509, owner = V._x509_verifier, V._owner_verifier

    def rec_x509(sg, identity):
        code, ver = x509(sg, identity)
        if sg.x509:
            tab[("eid", fnv(identity))] = code
        if ver is None:
            return code, ver

        def verify(msg, sig):
            c = ver(msg, sig)
            tab[("esig", fnv(identity, msg, sig))] = c
            return c
        return code, verify

    def rec_owner(sg, own):
        code, ver = owner(sg, own)
        if sg.ipk is not None:
            tab[("own", fnv(own))] = code
        if ver is None:
            return code, ver

        def verify(msg, sig):
            c = ver(msg, sig)
            tab[("osig", fnv(own, msg, sig))] = c
            return c
        return code, verify
    monkeypatch.setattr(V, "_x509_verifier", rec_x509)
    monkeypatch.setattr(V, "_owner_verifier", rec_owner)
    pp = Z.PublicParams.from_json(fx["pp"].encode())
    body = []

    def hx(b):
        return "x" + bytes(b).hex()
    total = 0
    for name, ledger, rs in groups:
        cfg = F.config(fx, name)
        sg = ref_signers(cfg, ipks)
        aud = cfg["auditor"]
        body.append("config %d %d %s %d %s" % (
            cfg["ix"], cfg["ec"], "nil" if aud is None else hx(aud), V.P.identity_code(aud) if aud else 0,
            " ".join("%s %d" % (hx(i), V.P.identity_code(i)) for i in cfg["issuers"])))
        body += ["ledger %s %s" % (hx(k.encode()), hx(v)) for k, v in ledger.items()]
        for raw, binding in rs:
            code, at = V.verify_signed_token_request(pp, sg, raw, binding, ledger.get, zk=rec_zk)
            body.append("request %s %s %d %d" % (hx(raw), hx(binding), code, at))
            total += 1
        body.append("run")
    from ftsoracle import bn254
    for v in fx["ledgers"]["bn254"].values():  # the elements gnark SetBytes refuses: off-curve ledger tokens
        try:
            tok = json.loads(v)
            raw = base64.b64decode(tok["Data"]["element"])
            if len(raw) == 64:
                bn254.g1_from_bytes(raw)
        except bn254.DecodeError:
            tab[("elem", fnv(raw))] = 0
        except (ValueError, TypeError, KeyError):
            pass
    with open(path, "w") as f:
        f.write("\n".join(["%s %016x %d" % (k[0], k[1], c) for k, c in tab.items()] + body) + "\n")
    return total


def build_main(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    srcs = [os.path.join(NATIVE, "reqsig_main.cpp"), os.path.join(HOST, "request.cpp"), os.path.join(HOST, "gojson.cpp")]
    deps = srcs + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in deps):
        return exe
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-pthread"] + flags + srcs
                   + ["-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def job(fx, zk, ipks, tmp_path_factory):
    """the fixture under every configuration, then 120 of its mutations"""
    mp = pytest.MonkeyPatch()
    try:
        groups = [(name, fx["ledgers"][F.config(fx, name)["curve"]], [(r["raw_b"], r["binding_b"]) for r in rs])
                  for name, rs in by_config(fx).items()]
        muts, ledger = mutations(fx, 120, 7)
        groups.append(("A", ledger, muts))
        path = str(tmp_path_factory.mktemp("reqsig") / "job.txt")
        total = write_job(path, fx, zk, ipks, groups, mp)
    finally:
        mp.undo()
    return path, total


def run_main(exe, job, *knobs):
    path, total = job
    r = subprocess.run([exe, path] + [str(k) for k in knobs], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.strip() == "ok %d" % total, r.stdout


@pytest.mark.parametrize("knobs", [(), (1, 1), (5, 3)])
def test_standalone_merge_and_message(job, knobs):
    run_main(build_main("reqsig_main", ["-O2"]), job, *knobs)


def test_standalone_under_sanitizers(job):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    try:  # the sanitizer runtimes inside the program, where the toolchain ships them as archives
        exe = build_main("reqsig_main_san", flags + ["-static-libasan", "-static-libubsan"])
    except subprocess.CalledProcessError:
        exe = build_main("reqsig_main_san", flags)
    run_main(exe, job)
    run_main(exe, job, 3, 2)


def test_existing_emulation_library_still_builds():
    """the fixed source list of tests/conftest.py still links: request.cpp reaches ECDSA through a hook only"""
    import conftest
    lib = ctypes.CDLL(conftest.build_emu())
    assert lib.emu_verify_token_requests_ex
