"""Loader of tests/golden/signed_requests.json (made by tests/gen_signed_requests.py).

The fixture holds only what the signed request path adds: actions are named by
(request, field, index) in tests/golden/token_requests.json, with byte
substitutions (the Issuer of an issue action, an input key); ledger tokens are
the ones of that file with their Owner replaced per key."""
import base64
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle", "py"))
from ftsoracle import request as R  # noqa: E402

BASE_OWNER = base64.b64encode(b"owner-identity")
BASE_ISSUER = base64.b64encode(b"issuer")


def load_base():
    with open(os.path.join(HERE, "golden", "token_requests.json")) as f:
        d = json.load(f)
    d["fields"] = {r["name"]: None for r in d["requests"]}
    d["raw"] = {r["name"]: base64.b64decode(r["raw"]) for r in d["requests"]}
    d["ledger_b"] = {k: base64.b64decode(v) for k, v in d["ledger"].items()}
    return d


def action(base, spec):
    """the bytes of one action: {"lit": hex} or {"req", "f", "i", "sub": [[old hex, new hex], ...]}"""
    if "lit" in spec:
        return bytes.fromhex(spec["lit"])
    if base["fields"][spec["req"]] is None:
        base["fields"][spec["req"]] = R.der_token_request(base["raw"][spec["req"]])
    a = base["fields"][spec["req"]][spec["f"]][spec["i"]]
    for old, new in spec.get("sub", []):
        old, new = bytes.fromhex(old), bytes.fromhex(new)
        assert a.count(old) == 1, (spec, old)
        a = a.replace(old, new)
    return a


def with_issuer(identity):
    """substitution that puts `identity` into an issue action of the base fixture"""
    return [(b'"Issuer":"' + BASE_ISSUER + b'"').hex(), (b'"Issuer":"' + base64.b64encode(identity) + b'"').hex()]


def with_key(old, new):
    return [json.dumps(old).encode().hex(), json.dumps(new).encode().hex()]


def raw_request(base, r):
    """the request bytes of fixture entry r"""
    if "raw" in r:
        return bytes.fromhex(r["raw"])
    fields = [[action(base, s) for s in r["issues"]], [action(base, s) for s in r["transfers"]],
              [bytes.fromhex(x) for x in r["sigs"]], [bytes.fromhex(x) for x in r["auditor_sigs"]]]
    raw = R.der_encode_token_request(fields)
    if r.get("extra_field"):  # bytes after the fourth field, inside the outer SEQUENCE
        body = R.der_encode_token_request(fields)
        off, n = R._header(body, 0, 0x30)
        inner = body[off:off + n] + bytes.fromhex(r["extra_field"])
        raw = b"\x30" + R._der_len(len(inner)) + inner
    return raw + bytes.fromhex(r.get("trailing", ""))


def ledger(base, fx, curve):
    """key -> token bytes with the fixture's owners on `curve` ("bn254" / "fp256bn")"""
    out = {}
    for k, v in base["ledger_b"].items():
        owner = fx["owners"][curve].get(k)
        out[k] = v.replace(BASE_OWNER, base64.b64encode(bytes.fromhex(owner))) if owner is not None else v
    for k, (src, owner) in fx["extra_ledger"].items():
        out[k] = base["ledger_b"][src].replace(BASE_OWNER, base64.b64encode(bytes.fromhex(owner)))
    return out


def load():
    base = load_base()
    with open(os.path.join(HERE, "golden", "signed_requests.json")) as f:
        fx = json.load(f)
    for r in fx["requests"]:
        r["raw_b"] = raw_request(base, r)
        r["binding_b"] = r["binding"].encode()
    fx["ledgers"] = {c: ledger(base, fx, c) for c in fx["owners"]}
    fx["pp"] = base["pp"]
    fx["base"] = base
    return fx


def config(fx, name):
    """-> dict(curve, ix (bool), ec (bool), auditor (bytes | None), issuers [bytes])"""
    c = fx["configs"][name]
    return {"curve": c["curve"], "ix": c["ix"], "ec": c["ec"],
            "auditor": None if c["auditor"] is None else bytes.fromhex(c["auditor"]),
            "issuers": [bytes.fromhex(x) for x in c["issuers"]]}
