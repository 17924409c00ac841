"""Cases of tests/test_g1_shared.py and tests/test_gpu_g1_shared.py: golden
PP-A transfers and copies of valid_2in_2out whose two inputs (outputs) are
equal or opposite points, so that the sum of the sibling partials c T_0 + c T_1
of the well-formedness sum job doubles or is the point at infinity
(dev/jobs.h job_g1_sum_parts).  The oracle's verdict and recomputed challenges
of every case are computed live, once per session."""
import functools
import json
import os

from conftest import GOLDEN, case_tuple
from ftsoracle import bn254 as C
from ftsoracle import zkat as Z

BASE = ["valid_2in_2out", "valid_3in_1out", "valid_1in_3out", "valid_ownership_1in_1out"]


def _neg(raw):
    return C.g1_bytes(C.g1_neg(C.g1_from_bytes(raw)))


@functools.lru_cache(maxsize=None)
def pp_a():
    with open(GOLDEN) as f:
        g = json.load(f)["pp_a"]
    return g["pp"].encode(), {c["name"]: c for c in g["cases"]}


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, (inputs, outputs, proof))]"""
    _, by = pp_a()
    out = [(n, case_tuple(by[n])) for n in BASE]
    ins, outs, proof = case_tuple(by["valid_2in_2out"])
    a, b = ins[:64], outs[:64]
    out.append(("inputs_equal", (a + a, outs, proof)))
    out.append(("inputs_opposite", (a + _neg(a), outs, proof)))
    out.append(("outputs_equal", (ins, b + b, proof)))
    out.append(("outputs_opposite", (ins, b + _neg(b), proof)))
    return out


def oracle_run(pp, tx):
    """(code, [(class, 32-byte challenge)]) of the oracle's transfer_verify"""
    ins, outs, proof = tx
    dec = lambda b: [C.g1_from_bytes(b[i:i + 64]) for i in range(0, len(b), 64)]  # noqa: E731
    Z.CHALLENGE_TRACE = []
    try:
        code = Z.transfer_verify(pp, dec(ins), dec(outs), proof)[1]
        return code, [(k, (h % (1 << 256)).to_bytes(32, "big")) for k, h in Z.CHALLENGE_TRACE]
    finally:
        Z.CHALLENGE_TRACE = None


@functools.lru_cache(maxsize=None)
def oracle():
    """{name: (code, challenges)} of every case"""
    pp = Z.PublicParams.from_json(pp_a()[0])
    return {name: oracle_run(pp, tx) for name, tx in cases()}


def compare(name, expect, dev, ora):
    """tests/test_challenges.py compare, and the WF class in full whatever the verdict"""
    n = 0
    for kind in (Z.ERR_WF, Z.ERR_MEMBERSHIP, Z.ERR_RANGE):
        d = [v for k, v in dev if k == kind]
        o = [v for k, v in ora if k == kind]
        if expect == Z.OK or kind == Z.ERR_WF:
            assert d == o, (name, kind)
        if d:
            assert d[:len(o)] == o, (name, kind, len(d), len(o))
            n += len(o)
    return n


def traces():
    with open(os.path.join(os.path.dirname(__file__), "golden", "challenge_traces.json")) as f:
        return json.load(f)["traces"]
