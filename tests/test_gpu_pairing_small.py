"""GPU: the sextet Miller loop and final exponentiation (dev/sx29.h) at the
smallest batch sizes, with both final-exponentiation variants.

One transfer is 4 pair jobs; three are 12, which cross the one-wave workgroup
of 10 jobs plus 4 ghost lanes, so the second workgroup of every pairing kernel
is mostly empty.  Each batch goes through ftz_verify_transfers (verdicts) and
through a debug batch (ftz_ctx_set_debug FTZ_DEBUG_CHALLENGES), whose
recomputed challenges are compared with the oracle's as test_challenges.py
does: the membership transcript holds the recomputed GT bytes, so equal
challenges mean equal pairing values.  The three-transfer batches hold one
tampered proof.

Reference: exact variant -- the recorded traces of the golden PP-A cases
(tests/golden/challenge_traces.json); Fuentes variant -- the oracle run live
under FE_FUENTES, once per module, on the Fuentes-made golden transfers and on
one exact-variant tampered proof (which a Fuentes context rejects at the
membership check).
"""
import json
import os

import pytest

from conftest import case_tuple
from ftsoracle import bn254 as C
from ftsoracle import zkat as Z

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
EXACT = {1: ["valid_2in_2out"], 3: ["valid_2in_2out_1", "membership_value", "valid_2in_2out"]}
FUENTES = {1: ["fuentes_valid_transfer_0"], 3: ["fuentes_valid_transfer_0", "membership_value", "fuentes_valid_transfer_1"]}


def compare(name, expect, dev, ora):
    """per class the oracle's values are a prefix of the device's (accepted proofs: equal), as
    test_challenges.compare; returns the number of values compared"""
    n = 0
    for kind in (Z.ERR_WF, Z.ERR_MEMBERSHIP, Z.ERR_RANGE):
        d = [v for k, v in dev if k == kind]
        o = [v for k, v in ora if k == kind]
        if expect == Z.OK:
            assert d == o, (name, kind)
        if d:
            assert d[:len(o)] == o, (name, kind, len(d), len(o))
            n += len(o)
    return n


@pytest.fixture(scope="module")
def exact_ref(golden):
    """name -> (case, expected code, oracle challenges), exact variant: the recorded traces"""
    with open(os.path.join(HERE, "golden", "challenge_traces.json")) as f:
        traces = json.load(f)["traces"]["pp_a"]
    by = {c["name"]: c for c in golden["pp_a"]["cases"]}
    return {n: (by[n], by[n]["expect"], [(k, bytes.fromhex(h)) for k, h in traces[n]["challenges"]])
            for n in set(sum(EXACT.values(), []))}


@pytest.fixture(scope="module")
def fuentes_ref(golden):
    """the same under the Fuentes variant: the oracle run live, once"""
    by = {c["name"]: c for c in golden["pp_a"]["cases"] + golden["pp_a_fuentes"]["cases"]}
    pp = Z.PublicParams.from_json(golden["pp_a"]["pp"].encode())
    dec = lambda b: [C.g1_from_bytes(b[i:i + 64]) for i in range(0, len(b), 64)]  # noqa: E731
    out = {}
    old = C.FE_VARIANT
    C.FE_VARIANT = C.FE_FUENTES
    try:
        for n in set(sum(FUENTES.values(), [])):
            ins, outs, proof = case_tuple(by[n])
            Z.CHALLENGE_TRACE = []
            try:
                code = Z.transfer_verify(pp, dec(ins), dec(outs), proof)[1]
                out[n] = (by[n], code, [(k, h.to_bytes(32, "big")) for k, h in Z.CHALLENGE_TRACE])
            finally:
                Z.CHALLENGE_TRACE = None
    finally:
        C.FE_VARIANT = old
    assert out["membership_value"][1] == Z.ERR_MEMBERSHIP and out["fuentes_valid_transfer_0"][1] == Z.OK
    return out


def run(golden, variant, names, ref):
    import zkatdlog
    batch = [case_tuple(ref[n][0]) for n in names]
    want = [ref[n][1] for n in names]
    compared = 0
    with zkatdlog.Context(golden["pp_a"]["pp"].encode(), device=0, fexp=variant) as ctx:
        assert list(ctx.verify_transfers(batch)) == want
        ctx.set_debug(challenges=True)
        b = ctx.load_transfers(batch)
        try:
            b.run()
            assert list(b.codes()) == want
            for i, n in enumerate(names):
                compared += compare(n, want[i], b.challenges(i), ref[n][2])
        finally:
            b.close()
    # the well-formedness transcript and the four membership ones (GT bytes) of every proof at least
    assert compared >= 5 * len(names)


@pytest.mark.parametrize("n", [1, 3])
def test_small_batch_exact(golden, exact_ref, n):
    assert n == 1 or any(exact_ref[x][1] != Z.OK for x in EXACT[n])  # one tampered proof
    run(golden, "exact", EXACT[n], exact_ref)


@pytest.mark.parametrize("n", [1, 3])
def test_small_batch_fuentes(golden, fuentes_ref, n):
    assert n == 1 or any(fuentes_ref[x][1] != Z.OK for x in FUENTES[n])
    run(golden, "fuentes", FUENTES[n], fuentes_ref)
