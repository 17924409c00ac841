"""GPU tier of the generating calls: zkatdlog.Context.generate_transfers /
generate_issues and zkatdlog.encode_token_request on the MI355X -- byte parity
with the oracle's composition (tests/generate_fx.py), a batch across the
prover's pass boundary checked with the library's own verifier and auditor,
PP-B with a 63-bit value, the signed round trip and two threads."""
import base64
import hashlib
import json
import os
import threading

import pytest

import generate_fx as F
import nymsign_ref as S
import signed_requests_fx as SF
from ftsoracle import bn254 as C
from ftsoracle import zkat as Z
from zkatdlog import _abi as A

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pp_a(golden):
    js = golden["pp_a"]["pp"].encode()
    return js, Z.PublicParams.from_json(js)


@pytest.fixture(scope="module")
def gctx(pp_a):
    import zkatdlog
    c = zkatdlog.Context(pp_a[0], device=0)
    yield c
    c.close()


def token_json(owner, raw):
    """json.Marshal(token.Token{Owner, Data}) of a ledger token"""
    return ('{"Owner":%s,"Data":{"curve":1,"element":"%s"}}' % (
        "null" if owner is None else '"%s"' % base64.b64encode(owner).decode(),
        base64.b64encode(raw).decode())).encode()


def opening(meta):
    v = json.loads(meta)
    return (v["Type"], int.from_bytes(base64.b64decode(v["Value"]["element"]), "big"),
            int.from_bytes(base64.b64decode(v["BlindingFactor"]["element"]), "big"))


def check_parity(ctx, pp):
    ts, te, iss, ie = F.parity_expected(pp, "pp_a")
    actions, metas, coms, codes = ctx.generate_transfers(ts)
    assert codes == [0] * len(ts)
    for i, (a, m, c, _) in enumerate(te):
        assert (actions[i], metas[i], coms[i]) == (a, m, c), i
    actions, metas, coms, codes = ctx.generate_issues(iss)
    assert codes == [0] * len(iss)
    for i, (a, m, c, _) in enumerate(ie):
        assert (actions[i], metas[i], coms[i]) == (a, m, c), i


# ---------------------------------------------------------------- 7. parity
def test_gpu_actions_match_the_oracle_composition(gctx, pp_a):
    check_parity(gctx, pp_a[1])


def test_gpu_actions_without_prover_tables(pp_a):
    import zkatdlog
    with zkatdlog.Context(pp_a[0], device=0, prover_tables=0) as c:
        check_parity(c, pp_a[1])


# ---------------------------------------------------------------- 8. across the pass boundary
def test_gpu_batch_of_4099_orders_verifies(gctx, pp_a):
    """4,099 orders: the prover's passes hold min(ftz_options.batch, 4096)
    witnesses (runtime.hip prove_chunked), so the call takes two passes -- two
    launches of every kernel, the second pass with three orders -- and each pass
    is planned in one piece per planning thread."""
    import zkatdlog
    pp = pp_a[1]
    n = 4099
    shapes = [(1, 1), (2, 2), (1, 2), (2, 1), (3, 1), (2, 2), (1, 1), (2, 3)]
    owners = [None, b"", b"a", b"ab", b"abc", F.LONG_OWNER, b"owner-6", b"owner-7"]
    bases = [F.transfer_order(pp, 800 + b, ni, no, ["-"] * ni, [owners[(b + k) % 8] for k in range(no)], ttype="USD")
             for b, (ni, no) in enumerate(shapes)]
    orders, ledger = [], {}
    for i in range(n):
        b = bases[i % 8]
        ids = ["t%05d:%d" % (i, k) for k in range(len(b["ids"]))]
        orders.append(dict(b, ids=ids, seed=hashlib.sha256(b"batch-%d" % i).digest()))
        for k, key in enumerate(ids):
            ledger[key] = token_json(b"in-owner", b["inputs"][64 * k:64 * k + 64])
    orders[n - 1] = dict(orders[0])  # the same order at both ends of the call
    actions, metas, coms, codes = gctx.generate_transfers(orders)
    assert codes == [0] * n
    assert actions[n - 1] == actions[0] and metas[n - 1] == metas[0] and coms[n - 1] == coms[0]
    flat = [c for cs in coms[:n - 1] for c in cs]
    assert len(set(flat)) == len(flat) == sum(len(o["out_values"]) for o in orders[:n - 1])
    reqs = [zkatdlog.encode_token_request([], [a]) for a in actions]
    # order 5's action over order 1's inputs (another witness of the same shape): not what the ledger holds
    swapped = actions[5].replace(b"t00005:", b"t00001:")
    assert swapped != actions[5] and len(orders[5]["ids"]) == len(orders[1]["ids"]) == 2
    assert orders[5]["inputs"] != orders[1]["inputs"]
    reqs.append(zkatdlog.encode_token_request([], [swapped]))
    vcodes, failed = gctx.verify_token_requests(reqs, ledger, batched=True)
    assert vcodes[:n] == [0] * n
    assert vcodes[n] != 0 and failed[n] == 0
    opens = [opening(m) for ms in metas for m in ms]
    assert [v for _, v, _ in opens] == [v for o in orders for v in o["out_values"]]
    assert gctx.audit_openings([c for cs in coms for c in cs], opens) == [0] * len(opens)


# ---------------------------------------------------------------- 9. PP-B
def test_gpu_pp_b_63_bit_value(golden):
    import zkatdlog
    js = golden["pp_b"]["pp"].encode()
    pp = Z.PublicParams.from_json(js)
    assert (pp.base, pp.exponent) == (16, 16)
    top = (1 << 63) - 1
    o = F.transfer_order(pp, 900, 2, 2, ["a:0", "a:1"], [b"o1", None], ttype="EUR", out_values=[top, 5], bound=1 << 40)
    o["in_values"] = [top, 5]  # balanced
    ins = [Z.token_commitment(pp, "EUR", v, b) for v, b in zip(o["in_values"], o["in_bfs"])]
    o["inputs"] = b"".join(C.g1_bytes(p) for p in ins)
    io = F.issue_order(pp, 901, [b"o"], b"issuer", ttype="EUR", values=[top])
    with zkatdlog.Context(js, device=0) as c:
        actions, metas, coms, codes = c.generate_transfers([o])
        assert codes == [0]
        proof = base64.b64decode(json.loads(actions[0])["Proof"])
        assert c.verify_transfers([(o["inputs"], b"".join(coms[0]), proof)]) == [0]
        ia, im, ic, codes = c.generate_issues([io])
        assert codes == [0]
        assert c.verify_issues([(b"".join(ic[0]), base64.b64decode(json.loads(ia[0])["Proof"]), False)]) == [0]
        opens = [opening(m) for m in metas[0] + im[0]]
        assert [v for _, v, _ in opens] == [top, 5, top]
        assert c.audit_openings(coms[0] + ic[0], opens) == [0, 0, 0]
        with pytest.raises(Exception, match="order 0: output value 0 is 2\\^63 or more"):
            c.generate_transfers([dict(o, out_values=[1 << 63, 5])])
        with pytest.raises(Exception, match="order 0: output value 0 is 2\\^63 or more"):
            c.generate_issues([dict(io, values=[1 << 63])])


# ---------------------------------------------------------------- 10. signed round trip
def test_gpu_signed_round_trip():
    """generate -> the message (request without signatures || txID) -> the owners'
    idemix signatures -> the signed request -> ftz_verify_signed_token_requests,
    with the owners of the signed-request fixture: the pseudonym of a ledger key
    is derived from that key as tests/gen_signed_requests.py derives it"""
    import zkatdlog
    fx = SF.load()
    pp = Z.PublicParams.from_json(fx["pp"].encode())
    with open(os.path.join(HERE, "golden", "idemix_bn254_golden.json")) as f:
        ipk = bytes.fromhex(json.load(f)["ipk"])

    def h(tag):
        return int.from_bytes(hashlib.sha256(tag.encode()).digest(), "big")
    keys = sorted(fx["owners"]["bn254"])[:2]
    o = F.transfer_order(pp, 950, 2, 2, keys, [bytes.fromhex(fx["owners"]["bn254"][k]) for k in keys], ttype="ABC")
    ledger = {k: token_json(bytes.fromhex(fx["owners"]["bn254"][k]), o["inputs"][64 * i:64 * i + 64])
              for i, k in enumerate(keys)}
    txid = b"generated-tx-1"
    with zkatdlog.Context(fx["pp"].encode(), device=0) as ctx:
        ix = zkatdlog.Idemix(ctx, ipk, A.FTZ_CURVE_BN254)
        ec = zkatdlog.Ecdsa(ctx)
        try:
            actions, _, _, codes = ctx.generate_transfers([o])
            assert codes == [0]
            msg = zkatdlog.encode_token_request([], actions) + txid
            items = []
            for k in keys:
                sk, rn = 1 + h("sk|bn254|%s" % k) % (S.R - 1), h("rnym|bn254|%s" % k) % S.R
                signer = ix.add_signer(sk.to_bytes(32, "big"))
                nym = ix.make_nyms(signer, [rn.to_bytes(32, "big")])[0]
                items.append((signer, rn.to_bytes(32, "big"), nym, msg))
            sigs, scodes = ix.sign_owner_signatures(items)
            assert scodes == [0, 0]
            req = zkatdlog.encode_token_request([], actions, sigs)
            assert zkatdlog.decode_token_request(req) == [[], actions, sigs, []]
            got = ctx.verify_signed_token_requests([req], [txid], ledger, idemix=ix, ecdsa=ec, auditor=None)
            assert got[0] == [0]
            bad = bytearray(sigs[1])
            bad[40] ^= 1
            req = zkatdlog.encode_token_request([], actions, [sigs[0], bytes(bad)])
            got = ctx.verify_signed_token_requests([req], [txid], ledger, idemix=ix, ecdsa=ec, auditor=None)
            assert got[0] == [A.FTZ_ERR_SIGNATURE]
        finally:
            ix.close()
            ec.close()


# ---------------------------------------------------------------- 11. two threads
def test_gpu_two_threads_equal_serial(gctx, pp_a):
    pp = pp_a[1]
    sets = [[F.transfer_order(pp, 1000 + 10 * t + i, 2, 2, ["x%d" % i, "y%d" % i], [b"o%d" % t, None], ttype="T")
             for i in range(40)] for t in range(2)]
    serial = [gctx.generate_transfers(s) for s in sets]
    got, errs = [None, None], []

    def work(t):
        try:
            got[t] = gctx.generate_transfers(sets[t])
        except Exception as e:  # surfaced below
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs
    assert got == serial
