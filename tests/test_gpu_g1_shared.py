"""GPU tier of tests/test_g1_shared.py: the shared variable partials of the
well-formedness sum jobs and the dense work lists of k_g1_part through the C
ABI on the MI355X, debug challenges on.

Batches of 1, 5 and 37 transfers interleave every shape of the cases (so the
list lengths are no multiples of a wave and sharing and non-sharing jobs
alternate): the equal / opposite copies of tests/g1_shared_cases.py against the
live oracle, every accepted golden PP-A transfer and one PP-B transfer (the
16-term Horner variable point) against the oracle's recorded traces
(tests/golden/challenge_traces.json).  A mixed pass of transfer and issue
actions runs through the token-request path, which returns verdicts only; a
small prover pass is re-verified by the verifier, since the prover's launches
read the same lists."""
import base64
import hashlib
import json
import math
import os

import pytest

import g1_shared_cases as S
from conftest import case_tuple
from ftsoracle import zkat as Z
from test_challenges import oracle_list
from test_prover import witness


@pytest.fixture(scope="module")
def pool(golden):
    """[(name, transfer, oracle code, oracle challenges)]: live cases, then the accepted golden ones"""
    ora = S.oracle()
    out = [(n, tx, ora[n][0], ora[n][1]) for n, tx in S.cases()]
    tr = S.traces()["pp_a"]
    for c in golden["pp_a"]["cases"]:
        if c["kind"] == "transfer" and c["expect"] == Z.OK and c["name"] not in S.BASE:
            out.append((c["name"], case_tuple(c), c["expect"], oracle_list(tr[c["name"]])))
    return out


@pytest.fixture(scope="module")
def dctx(golden):
    import zkatdlog
    with zkatdlog.Context(golden["pp_a"]["pp"].encode(), device=0) as c:
        c.set_debug(challenges=True)
        yield c


def run_batch(ctx, items):
    b = ctx.load_transfers([tx for _, tx, _, _ in items])
    try:
        b.run()
        codes = list(b.codes())
        compared = 0
        for i, (name, _, want, ora) in enumerate(items):
            assert codes[i] == want, (i, name)
            compared += S.compare(name, want, b.challenges(i), ora)
        return compared
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,stride", [(1, 1), (5, 5), (37, 7)])
def test_gpu_batches_match_oracle(dctx, pool, n, stride):
    """item k of the batch is case (start + k stride) of the pool: 1-in/1-out
    (no range part), 2/2, 3/1 and 1/3 shapes and rejected copies interleaved"""
    assert math.gcd(len(pool), stride) == 1  # the stride walks the whole pool
    items = [pool[(4 + k * stride) % len(pool)] for k in range(n)]
    assert run_batch(dctx, items) > 0


@pytest.mark.gpu
def test_gpu_every_case_once(dctx, pool):
    names = {name for name, _, _, _ in pool}
    assert names >= {"inputs_equal", "inputs_opposite", "outputs_equal", "outputs_opposite",
                     "wf_response_plus_r_accepts", "g1_compressed_accepts"}
    assert run_batch(dctx, pool) >= len(pool)


@pytest.mark.gpu
def test_gpu_pp_b_horner_point(golden):
    import zkatdlog
    c = next(c for c in golden["pp_b"]["cases"] if c["name"] == "ppb_valid_2in_2out")
    ora = oracle_list(S.traces()["pp_b"][c["name"]])
    with zkatdlog.Context(golden["pp_b"]["pp"].encode(), device=0) as ctx:
        ctx.set_debug(challenges=True)
        assert run_batch(ctx, [(c["name"], case_tuple(c), c["expect"], ora)] * 3) == 3 * len(ora)


@pytest.mark.gpu
def test_gpu_mixed_transfer_and_issue_actions():
    """token requests hold issue and transfer actions side by side: one mixed
    plan (verdicts and failing action as the oracle's fixture)"""
    import zkatdlog
    with open(os.path.join(os.path.dirname(__file__), "golden", "token_requests.json")) as f:
        fx = json.load(f)
    ledger = {k: base64.b64decode(v) for k, v in fx["ledger"].items()}
    with zkatdlog.Context(fx["pp"].encode(), device=0) as ctx:
        codes, failed = ctx.verify_token_requests([base64.b64decode(r["raw"]) for r in fx["requests"]], ledger)
    assert list(zip(codes, failed)) == [(r["expect"], r["failed_action"]) for r in fx["requests"]]
    assert {Z.OK, Z.ERR_WF} <= set(codes)


@pytest.mark.gpu
def test_gpu_prover_pass_reverified(golden):
    import zkatdlog
    js = golden["pp_a"]["pp"].encode()
    pp = Z.PublicParams.from_json(js)
    base = [witness(pp, 700, 2, 2), witness(pp, 701, 1, 1)]
    ws = [base[i % 2] | {"seed": hashlib.sha256(b"g1s%d" % i).digest()} for i in range(8)]
    with zkatdlog.Context(js, device=0) as ctx:
        proofs, codes = ctx.prove_transfers(ws)
        assert codes == [0] * 8
        tx = [(w["inputs"], w["outputs"], p) for w, p in zip(ws, proofs)]
        tx.append((ws[0]["inputs"], ws[0]["outputs"][64:] + ws[0]["outputs"][:64], proofs[0]))
        got = list(ctx.verify_transfers(tx))
    assert got[:8] == [0] * 8 and got[8] != 0
