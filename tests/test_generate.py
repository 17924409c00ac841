"""CPU tier of the generating calls (include/ftsamd.h ftz_generate_transfers /
ftz_generate_issues / ftz_token_request_encode).

The generating plans (host/planner_prove.cpp plan_gen_*) and the device job
code are compiled for the host (tests/native/gen_emu.cpp, TEST-ONLY: the
existing executor plus the new emission level) and checked byte for byte
against what the oracle composes (tests/generate_fx.py); the planner and the
encoder also run in a stand-alone program under AddressSanitizer + UBSan
(tests/native/gen_main.cpp)."""
import base64
import ctypes
import json
import os
import subprocess

import pytest

import generate_fx as F
from ftsoracle import bn254 as C
from ftsoracle import gojson as J
from ftsoracle import request as R
from ftsoracle import zkat as Z
from zkatdlog import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
NATIVE = os.path.join(ROOT, "tests", "native")
HOST = [os.path.join(CSRC, "host", f) for f in ("planner.cpp", "planner_prove.cpp", "gojson.cpp", "request.cpp",
                                                 "idemix.cpp")]
EMU_SRCS = [os.path.join(NATIVE, f) for f in ("gen_emu.cpp", "emu.cpp", "sx_emu.cpp", "msm_emu.cpp",
                                              "idemix_emu.cpp")] + HOST
MAIN_SRCS = [os.path.join(NATIVE, "gen_main.cpp")] + HOST[:4]


def _build(out, srcs, flags):
    path = os.path.join(BUILD, out)
    deps = srcs + [os.path.join(NATIVE, "emu_exec.cpp"), os.path.join(ROOT, "include", "ftsamd.h")] + [
        os.path.join(d, f) for d in (os.path.join(CSRC, "dev"), os.path.join(CSRC, "host"))
        for f in os.listdir(d) if f.endswith(".h")]
    if os.path.exists(path) and os.path.getmtime(path) >= max(os.path.getmtime(p) for p in deps):
        return path
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-pthread"] + flags + srcs + ["-o", path], check=True)
    return path


@pytest.fixture(scope="module")
def pp_a(golden):
    js = golden["pp_a"]["pp"].encode()
    return js, Z.PublicParams.from_json(js)


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(_build("libgenemu.so", EMU_SRCS, ["-O2", "-shared", "-fPIC"]))
    vp, sz, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
    szp, i32p = ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int32)
    lib.emu_ctx_create.restype = vp
    lib.emu_ctx_create.argtypes = [cp, sz, cp, sz]
    lib.emu_ctx_destroy.argtypes = [vp]
    for name in ("transfers", "issues"):
        f = getattr(lib, "gen_emu_" + name)
        f.restype = ctypes.c_long
        f.argtypes = [vp, sz, vp, cp, sz, szp, cp, sz, szp, cp, i32p, cp, sz]
        f = getattr(lib, "gen_emu_%s_size" % name)
        f.restype = ctypes.c_long
        f.argtypes = [vp, sz, vp, szp, szp, cp, sz]
    lib.gen_emu_encode_request.restype = ctypes.c_long
    lib.gen_emu_encode_request.argtypes = [vp, szp, cp, sz]
    lib.gen_emu_decode_request.restype = ctypes.c_long
    lib.gen_emu_decode_request.argtypes = [cp, sz, szp, ctypes.POINTER(A.Bytes), sz]
    return lib


@pytest.fixture(scope="module")
def ctx(lib, pp_a):
    h = lib.emu_ctx_create(pp_a[0], len(pp_a[0]), ctypes.create_string_buffer(256), 256)
    assert h
    yield h
    lib.emu_ctx_destroy(h)


def sizes(lib, ctx, orders, issue=False):
    arr, keep = (A.pack_issue_orders if issue else A.pack_transfer_orders)(orders)
    na, nm = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(512)
    fn = lib.gen_emu_issues_size if issue else lib.gen_emu_transfers_size
    if fn(ctx, len(orders), ctypes.addressof(arr), ctypes.byref(na), ctypes.byref(nm), err, 512) != 0:
        raise ValueError(err.value.decode())
    return na.value, nm.value


def generate(lib, ctx, orders, issue=False, caps=None):
    """(actions, metadata lists, commitment lists, codes) as Context.generate_*"""
    orders = list(orders)
    arr, keep = (A.pack_issue_orders if issue else A.pack_transfer_orders)(orders)
    counts = [len(o["values" if issue else "out_values"]) for o in orders]
    n, tok = len(orders), sum(counts)
    err = ctypes.create_string_buffer(512)
    if caps is None:
        caps = sizes(lib, ctx, orders, issue)
    act, meta = ctypes.create_string_buffer(max(1, caps[0])), ctypes.create_string_buffer(max(1, caps[1]))
    coms = ctypes.create_string_buffer(max(1, 64 * tok))
    aoff, moff = (ctypes.c_size_t * (n + 1))(), (ctypes.c_size_t * (tok + 1))()
    codes = (ctypes.c_int32 * max(1, n))()
    fn = lib.gen_emu_issues if issue else lib.gen_emu_transfers
    r = fn(ctx, n, ctypes.addressof(arr), act, caps[0], aoff, meta, caps[1], moff, coms, codes, err, 512)
    if r != 0:
        raise ValueError(err.value.decode())
    actions = [act.raw[aoff[i]:aoff[i + 1]] for i in range(n)]
    metas, cs, t = [], [], 0
    for c in counts:
        metas.append([meta.raw[moff[t + k]:moff[t + k + 1]] for k in range(c)])
        cs.append([coms.raw[64 * (t + k):64 * (t + k + 1)] for k in range(c)])
        t += c
    assert aoff[n] <= caps[0] and moff[tok] <= caps[1]
    return actions, metas, cs, list(codes)[:n]


@pytest.fixture(scope="module")
def parity(lib, ctx, pp_a):
    """the parity orders through the emulation, with the oracle's expectations"""
    ts, te, iss, ie = F.parity_expected(pp_a[1], "pp_a")
    return ts, te, generate(lib, ctx, ts), iss, ie, generate(lib, ctx, iss, issue=True)


# ---------------------------------------------------------------- 1. byte parity
def test_parity_orders_cover_the_cases(pp_a):
    ts, _, iss, _ = F.parity_expected(pp_a[1], "pp_a")
    assert [(len(o["ids"]), len(o["out_values"])) for o in ts] == [(1, 1), (2, 2), (1, 2), (3, 1)]
    assert [len(o["values"]) for o in iss][:2] == [1, 2]
    ids = "".join(k for o in ts for k in o["ids"])
    assert all(ch in ids for ch in '"\\<\u2028')
    owners = [w for o in ts + iss for w in o["owners"]]
    assert None in owners and b"" in owners
    assert {1, 2, 3} <= {len(w) for w in owners if w} and any(len(w) > 690 for w in owners if w)
    assert ts[1]["inputs"][0] & 0x80 and len(ts[1]["inputs"]) == 128
    assert all(o["type"] == 'tok<&>"x"' for o in ts + iss)
    strings = (F.TYPE + ids).encode()  # go_json_str and go1.18 differ on these two bytes
    assert b"\x08" not in strings and b"\x0c" not in strings


def test_transfer_actions_match_the_oracle_composition(parity):
    ts, te, (actions, metas, coms, codes), _, _, _ = parity
    assert codes == [0] * len(ts)
    for i, (a, m, c, _) in enumerate(te):
        assert actions[i] == a, i
        assert metas[i] == m, i
        assert coms[i] == c, i


def test_issue_actions_match_the_oracle_composition(parity):
    _, _, _, iss, ie, (actions, metas, coms, codes) = parity
    assert codes == [0] * len(iss)
    for i, (a, m, c, _) in enumerate(ie):
        assert actions[i] == a, i
        assert metas[i] == m, i
        assert coms[i] == c, i


def test_sizes_are_exact(lib, ctx, parity):
    ts, _, (actions, metas, _, _), iss, _, (iactions, imetas, _, _) = parity
    assert sizes(lib, ctx, ts) == (sum(map(len, actions)), sum(len(m) for ms in metas for m in ms))
    assert sizes(lib, ctx, iss, issue=True) == (sum(map(len, iactions)), sum(len(m) for ms in imetas for m in ms))


# ---------------------------------------------------------------- 2. oracle round trip
def _opening(meta):
    v = json.loads(meta)
    return (v["Type"], int.from_bytes(base64.b64decode(v["Value"]["element"]), "big"),
            int.from_bytes(base64.b64decode(v["BlindingFactor"]["element"]), "big"), v["Owner"], v["Issuer"])


def test_transfer_actions_round_trip_through_the_oracle(parity, pp_a):
    pp = pp_a[1]
    ts, _, (actions, metas, coms, _), _, _, _ = parity
    for o, act, ms, cs in zip(ts, actions, metas, coms):
        a = R.decode_transfer_action(act)
        assert a["inputs"] == o["ids"]
        outs = [e.point for e in a["outputs"]]
        assert [C.g1_bytes(p) for p in outs] == cs
        assert json.loads(act)["Metadata"] == {}
        assert Z.transfer_verify(pp, o["_ins"], outs, a["proof"])[1] == Z.OK
        for k, m in enumerate(ms):
            t, v, bf, owner, issuer = _opening(m)
            assert (t, v, issuer) == (o["type"], o["out_values"][k], None)
            assert owner == (None if o["owners"][k] is None else base64.b64encode(o["owners"][k]).decode())
            assert C.g1_bytes(Z.token_commitment(pp, t, v, bf)) == cs[k]


def test_issue_actions_round_trip_through_the_oracle(parity, pp_a):
    pp = pp_a[1]
    _, _, _, iss, _, (actions, metas, coms, _) = parity
    for o, act, ms, cs in zip(iss, actions, metas, coms):
        a = R.decode_issue_action(act)
        outs = [e.point for e in a["outputs"]]
        assert a["anonymous"] is False and [C.g1_bytes(p) for p in outs] == cs
        assert Z.issue_verify(pp, outs, a["proof"], anonymous=False)[1] == Z.OK
        for k, m in enumerate(ms):
            t, v, bf, _, issuer = _opening(m)
            assert (t, v) == (o["type"], o["values"][k])
            assert issuer == (None if o["issuer"] is None else base64.b64encode(o["issuer"]).decode())
            assert C.g1_bytes(Z.token_commitment(pp, t, v, bf)) == cs[k]


# ---------------------------------------------------------------- 3. one planning call, mixed shapes
def test_mixed_batch_equals_single_orders_past_the_template_cap(lib, ctx, pp_a):
    """Interleaved shapes, owner lengths that differ within a shape, and more
    distinct length tuples in one planning piece than it keeps templates for
    (planner.h GEN_TPL_CAP = 32; 44 orders are one piece), so that the later
    tuples are planned directly: every order equals its single-order result."""
    pp = pp_a[1]
    orders = []
    for i in range(40):  # 40 distinct owner lengths of the cheap shape, ids of two escaped lengths
        orders.append(F.transfer_order(pp, 500 + i, 1, 1, ["k%d" % i if i % 2 else 'k"%d' % i], [bytes(range(i))]))
    orders.insert(3, F.transfer_order(pp, 600, 2, 2, ["a", "b"], [b"x", None]))
    orders.insert(17, F.transfer_order(pp, 601, 2, 2, ["a", "b"], [b"xyz", b""]))
    orders.insert(38, F.transfer_order(pp, 602, 1, 2, ["c"], [b"pq", F.LONG_OWNER]))
    orders.append(F.transfer_order(pp, 603, 2, 2, ["aa", "b"], [b"x", None]))
    keys = {(len(o["ids"]), len(o["out_values"]), tuple(len(J.enc_str(k)) for k in o["ids"]),
             tuple(None if w is None else len(w) for w in o["owners"])) for o in orders}
    assert len(keys) > 32 and len(orders) < 64
    actions, metas, coms, codes = generate(lib, ctx, orders)
    assert codes == [0] * len(orders)
    for i, o in enumerate(orders):
        a1, m1, c1, k1 = generate(lib, ctx, [o])
        assert (actions[i], metas[i], coms[i], codes[i]) == (a1[0], m1[0], c1[0], k1[0]), i
    # same seed and values at another index and beside other neighbours: the same bytes
    assert len({c for cs in coms for c in cs}) == sum(len(cs) for cs in coms)


# ---------------------------------------------------------------- 4. the request encoder
def _encode(lib, fields):
    keep, ptrs = [], (ctypes.c_void_p * 4)()
    counts = (ctypes.c_size_t * 4)(*[len(f) for f in fields])
    for k, f in enumerate(fields):
        ptrs[k] = A.pack_bytes_list(f, keep)
    need = lib.gen_emu_encode_request(ctypes.addressof(ptrs), counts, None, 0)
    buf = ctypes.create_string_buffer(max(1, need))
    assert lib.gen_emu_encode_request(ctypes.addressof(ptrs), counts, buf, need) == need
    return buf.raw[:need]


def _decode(lib, raw):
    counts = (ctypes.c_size_t * 4)()
    elems = (A.Bytes * max(1, len(raw)))()
    assert lib.gen_emu_decode_request(raw, len(raw), counts, elems, len(raw)) == 0
    out, k = [], 0
    for f in range(4):
        out.append([ctypes.string_at(elems[k + j].p, elems[k + j].len) if elems[k + j].len else b""
                    for j in range(counts[f])])
        k += counts[f]
    return out


@pytest.mark.parametrize("fields", [
    [[], [], [], []],
    [[b""], [b"a" * 127, b"b" * 128], [b"c" * 255], [b"d" * 256]],
    [[b"e" * 65535], [b"f" * 65536, b""], [], [b"g"]],
    [[], [bytes(range(200)) * 3], [b"s" * 72, b"t" * 71], []],
])
def test_encode_token_request_is_minimal_der(lib, fields):
    raw = _encode(lib, fields)
    assert raw == R.der_encode_token_request(fields)
    assert _decode(lib, raw) == fields


# ---------------------------------------------------------------- 5. error paths
def test_refusals_name_the_order(lib, ctx, pp_a):
    pp = pp_a[1]
    good = F.transfer_order(pp, 700, 1, 1, ["k"], [b"o"])

    def refused(bad, match, issue=False):
        with pytest.raises(ValueError, match=match):
            generate(lib, ctx, [good, bad] if not issue else [F.issue_order(pp, 1, [b"o"], b"i"), bad], issue=issue,
                     caps=(1 << 16, 1 << 16))
    refused(dict(good, ids=[], inputs=b"", in_values=[], in_bfs=[]), "order 1: no inputs")
    refused(dict(good, out_values=[], owners=[]), "order 1: no outputs")
    refused(dict(good, seed=None), "order 1: null seed")
    refused(dict(good, type=b"\xc3\x28"), "order 1: type is not valid UTF-8")
    refused(dict(good, ids=[b"\xed\xa0\x80"]), "order 1: input id 0 is not valid UTF-8")
    refused(dict(good, out_values=[1 << 63]), "order 1: output value 0 is 2\\^63 or more")
    refused(F.issue_order(pp, 2, [], b"i"), "order 1: no outputs", issue=True)
    refused(F.issue_order(pp, 2, [b"o"], b"i", values=[1 << 63]), "order 1: output value 0 is 2\\^63", issue=True)
    refused(dict(F.issue_order(pp, 2, [b"o"], b"i"), seed=None), "order 1: null seed", issue=True)
    top = pp.base ** pp.exponent
    if top < 1 << 63:  # the prover's refusal; the 1-in/1-out transfer has no range proof
        two = F.transfer_order(pp, 701, 1, 2, ["k"], [b"o", b"p"])
        refused(dict(two, out_values=[top, 0]), "outside authorized range")
        refused(F.issue_order(pp, 3, [b"o"], b"i", values=[top]), "outside authorized range", issue=True)
        a, _, _, codes = generate(lib, ctx, [dict(good, out_values=[top])])
        assert codes == [0] and a[0]


def test_context_without_a_positive_exponent_is_refused(lib, pp_a):
    """a context is not created with exponent 0; it is with a negative one, on
    which no range proof can be made"""
    wrap = json.loads(pp_a[0])
    js = json.loads(base64.b64decode(wrap["Raw"]))
    js["RangeProofParams"]["Exponent"] = -1
    wrap["Raw"] = base64.b64encode(json.dumps(js).encode()).decode()
    raw = json.dumps(wrap).encode()
    h = lib.emu_ctx_create(raw, len(raw), ctypes.create_string_buffer(256), 256)
    assert h
    try:
        with pytest.raises(ValueError, match="order 0: public parameters with exponent <= 0"):
            generate(lib, h, [F.transfer_order(pp_a[1], 702, 1, 1, ["k"], [b"o"])], caps=(1 << 16, 1 << 16))
    finally:
        lib.emu_ctx_destroy(h)


def test_undecodable_input_leaves_its_neighbours_alone(lib, ctx, pp_a):
    pp = pp_a[1]
    a = F.transfer_order(pp, 710, 1, 1, ["k0"], [b"owner-a"])
    b = F.transfer_order(pp, 711, 2, 2, ["k1", "k2"], [b"o", None])
    c = F.transfer_order(pp, 712, 1, 1, ["k3"], [b"owner-c"])
    bad = bytearray(b["inputs"])
    bad[63] ^= 1
    actions, metas, coms, codes = generate(lib, ctx, [a, dict(b, inputs=bytes(bad)), c])
    assert codes == [0, A.FTZ_ERR_PARSE, 0]
    assert actions[1] == b"" and metas[1] == [b"", b""] and coms[1] == [bytes(64)] * 2
    alone = generate(lib, ctx, [a, c])
    assert (actions[0], metas[0], coms[0]) == (alone[0][0], alone[1][0], alone[2][0])
    assert (actions[2], metas[2], coms[2]) == (alone[0][1], alone[1][1], alone[2][1])


def test_short_capacity_reports_the_needed_sizes(lib, ctx, pp_a):
    o = [F.transfer_order(pp_a[1], 720, 1, 1, ["k"], [b"o"])]
    na, nm = sizes(lib, ctx, o)
    for caps in ((na - 1, nm), (na, nm - 1)):
        with pytest.raises(ValueError, match="need %d action bytes and %d metadata bytes" % (na, nm)):
            generate(lib, ctx, o, caps=caps)
    assert generate(lib, ctx, o, caps=(na, nm))[3] == [0]


# ---------------------------------------------------------------- 6. sanitizers, stand-alone
def test_planner_and_encoder_under_asan_ubsan(pp_a, tmp_path):
    exe = _build("gen_main", MAIN_SRCS, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    ppf = tmp_path / "pp.json"
    ppf.write_bytes(pp_a[0])
    r = subprocess.run([exe, str(ppf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gen_main ok" in r.stdout
