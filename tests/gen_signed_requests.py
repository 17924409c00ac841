#!/usr/bin/env python3
"""Fixture maker for the signed request path (tests/golden/signed_requests.json).

Actions come by name from tests/golden/token_requests.json (the proofs are not
duplicated); this file adds bindings, real idemix owners per ledger key (under
the issuer keys of idemix_bn254_golden.json / idemix_golden.json), x509 auditor
and issuer keys, the signatures (tests/nymsign_ref.py, tests/ecsign_ref.py, the
oracle's nym_sign on FP256BN) and the verdicts of tests/signed_request_ref.py,
with the ZK checks answered by the proof corpus's own verdicts.

    python tests/gen_signed_requests.py
"""
import base64
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ecsign_ref as E  # noqa: E402
import nymsign_ref as S  # noqa: E402
import p256_ref as P  # noqa: E402
import signed_request_ref as V  # noqa: E402
import signed_requests_fx as F  # noqa: E402
from ftsoracle import bn254 as C  # noqa: E402
from ftsoracle import idemix as I  # noqa: E402
from ftsoracle import request as R  # noqa: E402
from ftsoracle import zkat as Z  # noqa: E402


def h(tag):
    return int.from_bytes(hashlib.sha256(tag.encode()).digest(), "big")


def corpus_zk():
    g = json.load(open(os.path.join(HERE, "golden", "zkatdlog_golden.json")))["pp_a"]
    memo = {}

    def split(hx):
        b = bytes.fromhex(hx)
        return tuple(C.g1_from_bytes(b[64 * i:64 * i + 64]) for i in range(len(b) // 64))
    for c in g["cases"]:
        proof = base64.b64decode(c["proof"])
        if c["kind"] == "transfer":
            memo[("transfer", split(c["inputs"]), split(c["outputs"]), proof, False)] = c["expect"]
        else:
            memo[("issue", (), split(c["outputs"]), proof, bool(c["anonymous"]))] = c["expect"]

    def zk(pp, kind, ins, outs, proof, anonymous):
        key = (kind, tuple(ins), tuple(outs), proof, bool(anonymous))
        if key not in memo:
            memo[key] = R._zk(pp, kind, ins, outs, proof, anonymous)
        return memo[key]
    return zk


def main():
    base = F.load_base()
    pp = Z.PublicParams.from_json(base["pp"].encode())
    zk = corpus_zk()
    ipk = {"bn254": I.IssuerPKBn254(bytes.fromhex(json.load(open(os.path.join(HERE, "golden", "idemix_bn254_golden.json")))["ipk"])),
           "fp256bn": I.IssuerPK(bytes.fromhex(json.load(open(os.path.join(HERE, "golden", "idemix_golden.json")))["ipk"]))}
    role = I.pb_field(1, 2, b"idemix") + I.pb_field(2, 0, 2)
    ou = I.pb_field(1, 2, b"idemix") + I.pb_field(2, 2, b"org1.department1") + I.pb_field(3, 2, b"")

    # ---- owners: one pseudonym per ledger key and curve
    def secrets(curve, key):
        n = S.R if curve == "bn254" else I.N
        return 1 + h("sk|%s|%s" % (curve, key)) % (n - 1), h("rnym|%s|%s" % (curve, key)) % n

    def owner_identity(curve, key):
        sk, rn = secrets(curve, key)
        if curve == "bn254":
            return S.owner_of(S.make_nym(ipk[curve], sk, rn))
        return I.raw_owner_encode(b"si", I.serialize_idemix_identity(I.make_nym(ipk[curve], sk, rn), ou=ou, role=role), 0x13)

    def owner_sign(curve, key, msg):
        sk, rn = secrets(curve, key)
        if curve == "bn254":
            return S.sign(ipk[curve], sk, rn, S.make_nym(ipk[curve], sk, rn), msg)
        r = [h("r%d|%s|%s" % (k, key, hashlib.sha256(msg).hexdigest())) % I.N for k in range(3)]
        return I.nym_sign(ipk[curve], sk, rn, I.make_nym(ipk[curve], sk, rn), msg, *r)

    token_keys = [k for k, v in base["ledger_b"].items() if F.BASE_OWNER in v]
    owners = {"bn254": {k: owner_identity("bn254", k).hex() for k in token_keys},
              "fp256bn": {k: owner_identity("fp256bn", k).hex() for k in token_keys if k.startswith("tx000")}}

    # ---- x509 keys
    d = {n: 1 + h("x509|" + n) % (P.N - 1) for n in ("auditor", "iss1", "iss2", "iss3")}
    ident = {n: E.identity_of(v) for n, v in d.items()}
    p384 = P.serialized_identity(P.pem_encode("PUBLIC KEY", P.spki_der(0, 0, bytes.fromhex("2b81040022"),
                                                                         b"\x04" + bytes(range(96)))))
    assert P.identity_code(p384) == P.ERR_UNSUPPORTED
    configs = {
        "A": {"curve": "bn254", "ix": True, "ec": True, "auditor": ident["auditor"].hex(),
              "issuers": [ident["iss1"].hex(), ident["iss2"].hex()]},
        "nil_auditor": {"curve": "bn254", "ix": True, "ec": True, "auditor": None,
                        "issuers": [ident["iss1"].hex(), ident["iss2"].hex()]},
        "empty_auditor": {"curve": "bn254", "ix": True, "ec": True, "auditor": "", "issuers": []},
        "any_issuer": {"curve": "bn254", "ix": True, "ec": True, "auditor": ident["auditor"].hex(), "issuers": []},
        "any_issuer_nil_auditor": {"curve": "bn254", "ix": True, "ec": True, "auditor": None, "issuers": []},
        "p384_auditor": {"curve": "bn254", "ix": True, "ec": True, "auditor": p384.hex(), "issuers": []},
        "p384_issuer_listed": {"curve": "bn254", "ix": True, "ec": True, "auditor": None, "issuers": [p384.hex()]},
        "no_ix": {"curve": "bn254", "ix": False, "ec": True, "auditor": ident["auditor"].hex(), "issuers": []},
        "no_ec": {"curve": "bn254", "ix": True, "ec": False, "auditor": ident["auditor"].hex(),
                  "issuers": [ident["iss1"].hex()]},
        "no_ec_nil_auditor": {"curve": "bn254", "ix": True, "ec": False, "auditor": None, "issuers": []},
        "fp256bn": {"curve": "fp256bn", "ix": True, "ec": True, "auditor": ident["auditor"].hex(), "issuers": []},
    }

    # ---- actions by name
    def tr(req, i, *sub):
        return {"req": req, "f": 1, "i": i, "sub": [list(s) for s in sub]}

    def iss(req, i, who, *sub):
        s = [F.with_issuer(who if isinstance(who, bytes) else ident[who])] if who is not None else []
        return {"req": req, "f": 0, "i": i, "sub": s + [list(x) for x in sub]}

    def keys_of(spec):
        a = F.action(base, spec)
        try:
            return json.loads(a).get("Inputs") or []
        except (ValueError, AttributeError):
            return []
    T2 = tr("valid_mixed", 0)             # 2 in, 2 out
    T3 = tr("valid_mixed", 1)             # 3 in, 1 out
    T1 = tr("valid_transfers_only", 0)    # 1 in, 1 out
    TW = tr("transfer_wf_fails_at_2", 1)  # well-formedness fails
    TM = tr("transfer_membership", 0)
    k1 = keys_of(T1)[0]
    k2 = keys_of(T2)
    # further tokens: the commitment of T1's input under owners that are no idemix identity
    extra_ledger = {
        "script-owner": [k1, I.raw_owner_encode(b"htlc", b"a script", 0x13).hex()],
        "undecodable-owner": [k1, b"owner-identity".hex()],
        "unknown-type-owner": [k1, I.raw_owner_encode(b"zz", b"x", 0x13).hex()],
    }

    reqs = []

    def add(name, cfg, issues, transfers, note="", binding=None, sigs=None, aud=None, sig_binding=None,
            aud_binding=None, **kw):
        """sigs / aud: None = the right ones; else a function of the right lists -> the lists to ship;
        sig_binding / aud_binding: the binding the issuers and owners / the auditor sign instead of the request's"""
        c = configs[cfg]
        binding = binding if binding is not None else "tx-" + name
        r = {"name": name, "config": cfg, "binding": binding, "issues": issues, "transfers": transfers, "note": note}
        r.update(kw)
        body = R.der_encode_token_request([[F.action(base, s) for s in issues], [F.action(base, s) for s in transfers],
                                           [], []])
        msg = body + (sig_binding or binding).encode()
        ctx = {"msg": msg, "curve": c["curve"]}
        right_aud = [E.sign(d["auditor"], body + (aud_binding or binding).encode())] if c["auditor"] else []
        right = []
        for s in issues:
            who = None
            try:
                who = V._issuer_of(F.action(base, s))
            except Exception:
                pass
            name_of = [n for n, v in ident.items() if v == who]
            right.append(E.sign(d[name_of[0]], msg) if name_of else b"\x30\x00")
        for s in transfers:
            for k in keys_of(s):
                key = k if k in owners[c["curve"]] else k1
                right.append(owner_sign(c["curve"], key, msg))
        r["sigs"] = [x.hex() for x in (sigs(right, ctx) if sigs else right)]
        r["auditor_sigs"] = [x.hex() for x in (aud(right_aud, ctx) if aud else right_aud)]
        reqs.append(r)

    def flip(sig):
        b = bytearray(sig)
        b[len(b) // 2] ^= 1
        return bytes(b)

    def high_s(sig):
        r, s = P.parse_signature(sig)
        return P.encode_signature(r, P.N - s)

    add("valid_transfer_with_auditor", "A", [], [T2])
    add("valid_issue_with_issuer", "A", [iss("valid_mixed", 0, "iss1")], [])
    add("valid_mixed", "A", [iss("valid_mixed", 0, "iss1"), iss("valid_mixed", 1, "iss2")], [T2, T3, T1])
    add("valid_no_actions", "A", [], [], "the auditor still signs the empty request")
    add("nil_auditor_ignores_auditor_signatures", "nil_auditor", [], [T2], aud=lambda a, c: [b"not a signature"])
    add("nil_auditor_no_signature_at_all", "nil_auditor", [], [], "no check consumes a signature")
    add("empty_non_nil_auditor", "empty_auditor", [], [T2], "row 2 runs on an empty identity")
    add("issuer_not_in_list", "A", [iss("valid_mixed", 0, "iss3")], [])
    add("issue_action_does_not_unmarshal", "A", [{"lit": b'{"Anonymous":1}'.hex()}], [], "row 3")
    add("empty_issuer_list_admits_any", "any_issuer", [iss("valid_mixed", 0, "iss3")], [])
    add("empty_issuer_list_undecodable_issuer", "any_issuer", [iss("valid_mixed", 0, None)], [],
        "the base fixture's Issuer bytes are no SerializedIdentity")
    add("empty_issuer_list_p384_issuer", "any_issuer_nil_auditor", [iss("valid_mixed", 0, p384)], [],
        "the x509 call gets one item and none reaches the device")
    add("listed_p384_issuer", "p384_issuer_listed", [iss("valid_mixed", 0, p384)], [])
    # the cursor exhausted at each position
    add("no_signature_at_all", "A", [], [T1], sigs=lambda s, c: [], aud=lambda a, c: [])
    add("auditor_signature_missing_owner_consumed", "A", [], [T1], aud=lambda a, c: [],
        note="the owner's signature is taken for the auditor's")
    add("issuer_signature_missing", "A", [iss("valid_mixed", 0, "iss1")], [], sigs=lambda s, c: [])
    add("second_issuer_signature_missing", "A", [iss("valid_mixed", 0, "iss1"), iss("valid_mixed", 1, "iss2")], [],
        sigs=lambda s, c: s[:1])
    add("owner_0_signature_missing", "A", [], [T2], sigs=lambda s, c: [])
    add("owner_1_signature_missing", "A", [], [T2], sigs=lambda s, c: s[:1])
    add("second_transfer_signature_missing", "A", [], [T2, T1], sigs=lambda s, c: s[:2])
    add("owners_swapped", "A", [], [T2], sigs=lambda s, c: [s[1], s[0]])
    add("trailing_extra_signatures", "A", [], [T2], sigs=lambda s, c: s + [b"left over", b""])
    add("two_auditor_signatures_second_taken_by_owner", "A", [], [T2], sigs=lambda s, c: s[1:],
        aud=lambda a, c: a + [owner_sign(c["curve"], k2[0], c["msg"])])
    add("high_s_auditor_signature", "A", [], [T2], aud=lambda a, c: [high_s(a[0])])
    add("bad_owner_signature", "A", [], [T2], sigs=lambda s, c: [s[0], flip(s[1])])
    add("signed_over_another_binding", "A", [], [T2], binding="tx-B", sig_binding="tx-A", aud_binding="tx-A")
    add("owners_signed_over_another_binding", "A", [], [T2], binding="tx-D", sig_binding="tx-C")
    # owners
    add("script_owner", "A", [], [tr("valid_transfers_only", 0, F.with_key(k1, "script-owner"))])
    add("undecodable_owner", "A", [], [tr("valid_transfers_only", 0, F.with_key(k1, "undecodable-owner"))])
    add("unknown_owner_type", "A", [], [tr("valid_transfers_only", 0, F.with_key(k1, "unknown-type-owner"))])
    add("script_owner_after_bad_signature", "A", [], [T2, tr("valid_transfers_only", 0, F.with_key(k1, "script-owner"))],
        sigs=lambda s, c: [flip(s[0])] + s[1:])
    # inputs
    add("missing_input_before_signature", "A", [], [tr("valid_mixed", 0, F.with_key(k2[0], "no-such-key"))],
        sigs=lambda s, c: [b"junk", b"junk"])
    add("missing_input_after_good_signature", "A", [], [tr("valid_mixed", 0, F.with_key(k2[1], "no-such-key"))])
    add("missing_input_after_bad_signature", "A", [], [tr("valid_mixed", 0, F.with_key(k2[1], "no-such-key"))],
        sigs=lambda s, c: [flip(s[0])] + s[1:])
    add("input_not_json_after_good_signature", "A", [], [tr("valid_mixed", 0, F.with_key(k2[1], "bad-json-token"))])
    add("input_off_curve_before_signature", "A", [], [tr("valid_mixed", 0, F.with_key(k2[0], "off-curve-token"))],
        sigs=lambda s, c: [b"", b""])
    add("input_nil_data_panics_after_signature", "A", [], [tr("valid_transfers_only", 0, F.with_key(k1, "nil-data-token"))],
        "the token deserializes, its owner is the base fixture's (no RawOwner)")
    # proofs and signatures
    add("bad_proof_good_signatures", "A", [], [TW])
    add("bad_signature_and_bad_proof", "A", [], [TW], sigs=lambda s, c: [flip(x) for x in s])
    add("membership_fails_good_signatures", "A", [], [TM])
    add("issue_0_bad_proof_issue_1_bad_signature", "A",
        [iss("first_failure_issue_wins", 1, "iss1"), iss("valid_mixed", 1, "iss2")], [], sigs=lambda s, c: [s[0], flip(s[1])])
    add("issue_0_bad_signature_issue_1_bad_proof", "A",
        [iss("valid_mixed", 1, "iss2"), iss("first_failure_issue_wins", 1, "iss1")], [], sigs=lambda s, c: [flip(s[0]), s[1]])
    add("issue_bad_proof_before_unlisted_issuer", "A", [iss("first_failure_issue_wins", 1, "iss3")], [])
    add("issue_nil_output_malformed_before_signature", "A", [iss("issue_nil_output_malformed", 0, "iss1")], [],
        sigs=lambda s, c: [])
    add("issue_fails_before_transfer_signature", "A", [iss("valid_mixed", 0, "iss1")], [T1],
        sigs=lambda s, c: [flip(s[0]), s[1]])
    add("transfer_panics_after_signatures", "A", [], [tr("transfer_panics", 1)])
    # rows 2 and 3
    add("bad_auditor_signature_and_unparsable_action", "A", [], [{"lit": b"{".hex()}], aud=lambda a, c: [flip(a[0])])
    add("good_auditor_signature_and_unparsable_action", "A", [], [{"lit": b"{".hex()}])
    add("p384_auditor", "p384_auditor", [], [T1], aud=lambda a, c: [b"\x30\x00"])
    add("p384_auditor_unparsable_action", "p384_auditor", [], [{"lit": b"{".hex()}])
    # ASN.1
    add("trailing_bytes_after_sequence_not_signed", "A", [], [T1], trailing=b"\x00\x01garbage".hex())
    add("extra_field_inside_sequence_not_signed", "A", [], [T1], extra_field=b"\x04\x03abc".hex())
    reqs.append({"name": "asn1_empty", "config": "A", "binding": "tx-empty", "raw": "", "note": "row 1"})
    reqs.append({"name": "asn1_truncated", "config": "A", "binding": "tx-trunc", "raw": "300630003000", "note": "row 1"})
    # handles left out
    add("no_idemix_handle", "no_ix", [], [T1])
    add("no_idemix_handle_missing_input_first", "no_ix", [], [tr("valid_mixed", 0, F.with_key(k2[0], "no-such-key"))])
    add("no_idemix_handle_issue_only", "no_ix", [iss("valid_mixed", 0, "iss3")], [])
    add("no_x509_handle_auditor", "no_ec", [], [T1])
    add("no_x509_handle_nil_auditor_transfer", "no_ec_nil_auditor", [], [T2])
    add("no_x509_handle_nil_auditor_issue", "no_ec_nil_auditor", [iss("valid_mixed", 0, "iss1")], [])
    # FP256BN owners
    add("fp256bn_valid_transfer", "fp256bn", [], [T2])
    add("fp256bn_owners_swapped", "fp256bn", [], [T2], sigs=lambda s, c: [s[1], s[0]])
    add("fp256bn_valid_mixed", "fp256bn", [iss("valid_mixed", 0, "iss3")], [T3, T2])

    fx = {"generator": "tests/gen_signed_requests.py (tests/signed_request_ref.py; corpus verdicts for the ZK checks)",
          "configs": configs, "owners": owners, "extra_ledger": extra_ledger, "requests": reqs}
    ledgers = {c: F.ledger(base, fx, c) for c in owners}
    for r in reqs:
        c = F.config(fx, r["config"])
        sg = V.Signers(ipk[c["curve"]] if c["ix"] else None, V.CURVE_BN254 if c["curve"] == "bn254" else V.CURVE_FP256BN,
                       c["ec"], c["auditor"], c["issuers"])
        code, at = V.verify_signed_token_request(pp, sg, F.raw_request(base, r), r["binding"].encode(),
                                                 ledgers[c["curve"]].get, zk=zk)
        r["expect"], r["failed_action"] = code, at
        print("%-52s %-24s %2d %2d" % (r["name"], r["config"], code, at))
    path = os.path.join(HERE, "golden", "signed_requests.json")
    with open(path, "w") as f:
        json.dump(fx, f, indent=1)
    print("wrote", path, len(reqs), "requests,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
