"""GPU tier of batched Pointcheval-Sanders verification
(ftz_verify_ps_signatures) and the audit of RangeProofParams.SignedValues
(ftz_pp_audit_signed_values): the fixture's verdicts (tests/ps_ref.py through
tests/golden/ps_golden.json) under both final exponentiations and both line
layouts, the sextet and pass boundaries, the audit, and the known-answer pin
of the pairing stack on the reference-style PP-A."""
import base64
import ctypes
import json
import os
import threading

import pytest

import ps_ref as S
from conftest import case_tuple

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, Z, R, P = S.C, S.Z, S.R, S.P
ERR_PS, ERR_PARSE = 14, 1
SETTINGS = [(f, l) for f in ("exact", "fuentes") for l in ("one_lane", "sextet")]


@pytest.fixture(scope="module")
def zk():
    import zkatdlog
    return zkatdlog


@pytest.fixture(scope="module")
def g():
    with open(os.path.join(ROOT, "tests", "golden", "ps_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pp_raw(g):
    return base64.b64decode(g["pp"])


@pytest.fixture(scope="module")
def ctx(zk, pp_raw):
    """the base-8 parameters, default options (exact, default layouts)"""
    with zk.Context(pp_raw, device=0) as c:
        yield c


@pytest.fixture(scope="module")
def pp_a(golden):
    return Z.PublicParams.from_json(golden["pp_a"]["pp"].encode())


def item(c):
    return (bytes.fromhex(c["m"]), bytes.fromhex(c["h"]), bytes.fromhex(c["r"]), bytes.fromhex(c["s"]))


def tamper(it):
    """the item with its m off by one: never a signature on the new message"""
    m, h, r, s = it
    return ((int.from_bytes(m, "big") ^ 1).to_bytes(32, "big"), h, r, s)


def signed_items(pp, negate_s=False):
    """(i, R_i, S_i) of every signed value; h is left to the binding (HashToZr of i's bytes)"""
    out = []
    for i, (r, s) in enumerate(pp.signed_values):
        out.append((i, C.g1_bytes(r), C.g1_bytes(C.g1_neg(s) if negate_s else s)))
    return out


# 1 ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("fexp,layout", SETTINGS)
def test_golden_cases_every_setting(zk, g, pp_raw, fexp, layout):
    with zk.Context(pp_raw, device=0, fexp=fexp) as c:
        c.set_layout("g2lines", layout)
        got = c.verify_ps_signatures([item(x) for x in g["cases"]])
        want = [x["code"] for x in g["cases"]]
        assert got == want, {x["name"]: (a, b) for x, a, b in zip(g["cases"], got, want) if a != b}
        assert set(want) == {0, ERR_PARSE, ERR_PS}


def test_missing_hash_is_computed(ctx, g):
    """(m, R, S) items: h = HashToZr(m's 32 bytes), ints and bytes alike"""
    sv = [x for x in g["cases"] if x["kind"] == "signed_value"]
    a = ctx.verify_ps_signatures([(i, bytes.fromhex(x["r"]), bytes.fromhex(x["s"])) for i, x in enumerate(sv)])
    b = ctx.verify_ps_signatures([(bytes.fromhex(x["m"]), bytes.fromhex(x["r"]), bytes.fromhex(x["s"])) for x in sv])
    assert a == b == [0] * 8
    assert ctx.verify_ps_signatures([(1, bytes.fromhex(sv[0]["r"]), bytes.fromhex(sv[0]["s"]))]) == [ERR_PS]
    assert ctx.verify_ps_signatures([]) == []
    lib = ctx._lib
    codes = (ctypes.c_int32 * 1)()
    assert lib.ftz_verify_ps_signatures(ctx._h, 0, None, None) == 0
    assert lib.ftz_verify_ps_signatures(ctx._h, 1, None, codes) != 0
    rec = (ctypes.c_uint8 * 192)()
    assert lib.ftz_verify_ps_signatures(ctx._h, 1, ctypes.addressof(rec), None) != 0


# 2 ---------------------------------------------------------------- sextet boundaries
@pytest.mark.parametrize("n", [1, 9, 10, 11, 64, 65])
def test_one_invalid_item_among_valid_ones(ctx, g, n):
    """ten jobs share a wave: the one invalid item at the first, the last and
    the wave-boundary positions, every neighbour unchanged"""
    valid = [item(x) for x in g["cases"] if x["code"] == 0 and x["kind"] != "both_infinity"]
    base = [valid[k % len(valid)] for k in range(n)]
    assert ctx.verify_ps_signatures(base) == [0] * n
    for pos in sorted({0, n - 1, 9, 10} & set(range(n))):
        items = list(base)
        items[pos] = tamper(items[pos])
        want = [0] * n
        want[pos] = ERR_PS
        assert ctx.verify_ps_signatures(items) == want, pos
    # the other way round: one valid item among invalid ones
    for pos in sorted({0, n - 1, 9, 10} & set(range(n))):
        items = [tamper(x) for x in base]
        items[pos] = base[pos]
        want = [ERR_PS] * n
        want[pos] = 0
        assert ctx.verify_ps_signatures(items) == want, pos


# 3 ---------------------------------------------------------------- tiling into passes
@pytest.mark.parametrize("batch", [1, 16])
def test_tiling_across_passes(zk, ctx, g, pp_raw, batch):
    """passes of 4 x batch items: codes position by position across the pass
    boundaries, and the same in one pass on the default context"""
    n = 3 * (4 * batch) + 7
    cases = g["cases"]
    items, want = [], []
    for k in range(n):
        x = cases[k % len(cases)]
        it, code = item(x), x["code"]
        if k % 64 == 0 and code == 0 and x["kind"] != "both_infinity":
            it, code = tamper(it), ERR_PS
        items.append(it)
        want.append(code)
    assert want[0] == ERR_PS
    with zk.Context(pp_raw, device=0, batch=batch) as small:
        assert small.options["batch"] == batch
        assert small.verify_ps_signatures(items) == want
    assert ctx.verify_ps_signatures(items) == want


# 4 ---------------------------------------------------------------- the audit
@pytest.mark.parametrize("name", ["pp_a", "pp_b"])
def test_audit_golden_parameters(zk, golden, name):
    with zk.Context(golden[name]["pp"].encode(), device=0) as c:
        codes = c.audit_signed_values()
        assert len(codes) == c.base == golden[name]["base"]
        assert codes == [0] * c.base


def test_audit_finds_swapped_entries(zk, pp_raw):
    sw = Z.PublicParams.from_json(pp_raw)
    sw.signed_values[3], sw.signed_values[5] = sw.signed_values[5], sw.signed_values[3]
    raw = sw.to_json()
    assert zk.validate_public_params(raw) == ""
    with zk.Context(raw, device=0) as c:   # the file loads: nothing else checks the table
        assert c.audit_signed_values() == [0, 0, 0, ERR_PS, 0, ERR_PS, 0, 0]
        # each of the two is a valid signature on the other index
        r3, s3 = (C.g1_bytes(x) for x in sw.signed_values[3])
        r5, s5 = (C.g1_bytes(x) for x in sw.signed_values[5])
        assert c.verify_ps_signatures([(5, r3, s3), (3, r5, s5), (3, r3, s3)]) == [0, 0, ERR_PS]


def test_audit_refuses_infinity_and_short_buffers(zk, ctx, pp_raw):
    inf = Z.PublicParams.from_json(pp_raw)
    inf.signed_values[2] = (None, None)
    raw = inf.to_json()
    assert zk.validate_public_params(raw) == ""
    with zk.Context(raw, device=0) as c:
        assert c.verify_ps_signatures([(2, bytes(64), bytes(64))]) == [0]   # Verify skips both pairs
        assert c.audit_signed_values() == [0, 0, ERR_PS, 0, 0, 0, 0, 0]
    lib = ctx._lib
    count = ctypes.c_size_t(99)
    codes = (ctypes.c_int32 * 8)(*([7] * 8))
    assert lib.ftz_pp_audit_signed_values(ctx._h, codes, 7, ctypes.byref(count)) == -1   # FTZ_E_INVALID
    assert count.value == 8 and list(codes) == [7] * 8
    assert lib.ftz_pp_audit_signed_values(ctx._h, codes, 8, ctypes.byref(count)) == 0
    assert count.value == 8 and list(codes) == [0] * 8
    assert lib.ftz_pp_audit_signed_values(ctx._h, codes, 8, None) != 0


# 5 ---------------------------------------------------------------- the known-answer pin
@pytest.mark.parametrize("fexp,layout", SETTINGS)
def test_pp_a_signed_values_pair_to_one(zk, golden, pp_a, fexp, layout):
    """FExp(e(-S, Q) e(R, PK0 + m PK1 + h PK2)) is exactly one for every signed
    value of the reference-style PP-A, whatever the line layout and the final
    exponentiation: a known answer for lines, Miller loop and FExp that depends
    on no byte order.  With S negated none of them is."""
    with zk.Context(golden["pp_a"]["pp"].encode(), device=0, fexp=fexp) as c:
        c.set_layout("g2lines", layout)
        n = len(pp_a.signed_values)
        assert n == 100
        assert c.verify_ps_signatures(signed_items(pp_a)) == [0] * n
        assert c.verify_ps_signatures(signed_items(pp_a, negate_s=True)) == [ERR_PS] * n
        assert c.audit_signed_values() == [0] * n


# 6 ---------------------------------------------------------------- next to the engine
def test_concurrent_with_transfers(zk, golden, pp_a):
    cases = [x for x in golden["pp_a"]["cases"] if x["kind"] == "transfer"]
    sel = [k % len(cases) for k in range(256)]
    good, bad = signed_items(pp_a), signed_items(pp_a, negate_s=True)
    items = [(bad if k % 7 == 3 else good)[k % 100] for k in range(2000)]
    want_ps = [ERR_PS if k % 7 == 3 else 0 for k in range(2000)]
    out = {}
    with zk.Context(golden["pp_a"]["pp"].encode(), device=0) as c:
        packed = zk._abi.pack_ps_sigs(items)

        def ps():
            out["ps"] = [list(c.verify_ps_signatures_packed(packed)) for _ in range(2)]

        def tx():
            out["tx"] = [list(c.verify_transfers([case_tuple(cases[k]) for k in sel])) for _ in range(2)]
        th = [threading.Thread(target=ps), threading.Thread(target=tx)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert out["ps"] == [want_ps] * 2
    assert out["tx"] == [[cases[k]["expect"] for k in sel]] * 2
