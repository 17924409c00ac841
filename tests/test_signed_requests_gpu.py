"""GPU tier of the signed request path: ftz_verify_signed_token_requests through
zkatdlog.Context.verify_signed_token_requests against the verdicts of
tests/golden/signed_requests.json (tests/signed_request_ref.py), by name, under
every signer configuration of the fixture (auditor nil / empty / P-384, no
idemix handle, no x509 handle, both idemix curves), across the pipeline's
512 / 513 chunk boundary, and from several threads beside the unsigned call."""
import base64
import json
import os
import threading

import pytest

import signed_requests_fx as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return F.load()


@pytest.fixture(scope="module")
def gpu(fx):
    import zkatdlog
    from zkatdlog import _abi as A

    def ipk(name):
        with open(os.path.join(HERE, "golden", name)) as f:
            return bytes.fromhex(json.load(f)["ipk"])
    ctx = zkatdlog.Context(fx["pp"].encode(), device=0)
    h = {"ctx": ctx, "ec": zkatdlog.Ecdsa(ctx),
         "bn254": zkatdlog.Idemix(ctx, ipk("idemix_bn254_golden.json"), A.FTZ_CURVE_BN254),
         "fp256bn": zkatdlog.Idemix(ctx, ipk("idemix_golden.json"), A.FTZ_CURVE_FP256BN_AMCL)}
    yield h
    for k in ("bn254", "fp256bn", "ec"):
        h[k].close()
    ctx.close()


def run(gpu, fx, name, rs, ledger=None):
    cfg = F.config(fx, name)
    return list(zip(*gpu["ctx"].verify_signed_token_requests(
        [r["raw_b"] for r in rs], [r["binding_b"] for r in rs], ledger or fx["ledgers"][cfg["curve"]],
        idemix=gpu[cfg["curve"]] if cfg["ix"] else None, ecdsa=gpu["ec"] if cfg["ec"] else None,
        auditor=cfg["auditor"], issuers=cfg["issuers"])))


def of_config(fx, name):
    return [r for r in fx["requests"] if r["config"] == name]


def want(rs):
    return [(r["expect"], r["failed_action"]) for r in rs]


def pipeline_chunks(n, ch=4096, ramp=8):
    """chunks of host/request.cpp: ch/8, ch/4, ch/2, then ch"""
    k, c = 0, max(ch // ramp, 1)
    while n > 0:
        n -= c
        k += 1
        c = min(ch, 2 * c)
    return k


def test_gpu_signed_none_and_one(gpu, fx):
    assert run(gpu, fx, "A", []) == []
    r = next(x for x in fx["requests"] if x["name"] == "valid_mixed")
    assert run(gpu, fx, "A", [r]) == [(0, -1)]
    r = next(x for x in fx["requests"] if x["name"] == "no_signature_at_all")
    assert run(gpu, fx, "A", [r]) == [(10, -1)]


def test_gpu_signed_fixture_by_name(gpu, fx):
    got, exp = {}, {}
    for name in fx["configs"]:
        rs = of_config(fx, name)
        for r, o in zip(rs, run(gpu, fx, name, rs)):
            got[r["name"]], exp[r["name"]] = o, (r["expect"], r["failed_action"])
    assert len(exp) == len(fx["requests"])
    assert got == exp


def test_gpu_signed_every_x509_item_unsupported(gpu, fx):
    """the x509 call of the chunk gets items and none of them reaches the device"""
    rs = [r for r in fx["requests"] if r["name"] == "empty_issuer_list_p384_issuer"] * 3
    assert run(gpu, fx, "any_issuer_nil_auditor", rs) == [(11, 0)] * 3


@pytest.mark.parametrize("n", [512, 513, 600])
def test_gpu_signed_tiled_across_chunks(gpu, fx, n):
    """the first pipeline chunk is 512 requests: 513 and 600 cross into a second one, whose
    signature stage reuses the handles' slots; the ledger is asked at most once per chunk"""
    import zkatdlog
    a = of_config(fx, "A")
    rs = (a * (n // len(a) + 1))[:n]
    led = zkatdlog.NativeLedger(fx["ledgers"]["bn254"])
    try:
        got = run(gpu, fx, "A", rs, led)
        calls, _ = led.counts()
    finally:
        led.close()
    assert got == want(rs)
    assert calls <= pipeline_chunks(n)


def test_gpu_signed_threads_beside_unsigned(gpu, fx):
    """two threads in the signed call and one in the unsigned call on one context"""
    base = fx["base"]
    plain = [r for r in base["requests"]]
    a = of_config(fx, "A")
    rs = (a * (600 // len(a) + 1))[:600]
    out = {}

    def signed(k):
        out[k] = run(gpu, fx, "A", rs)

    def unsigned():
        out["u"] = list(zip(*gpu["ctx"].verify_token_requests([base64.b64decode(r["raw"]) for r in plain] * 4,
                                                              base["ledger_b"], batched=True)))
    th = [threading.Thread(target=signed, args=(0,)), threading.Thread(target=signed, args=(1,)),
          threading.Thread(target=unsigned)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert out[0] == want(rs) and out[1] == want(rs)
    assert out["u"] == [(r["expect"], r["failed_action"]) for r in plain] * 4
