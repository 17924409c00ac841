"""TEST INFRASTRUCTURE ONLY -- restatement of Validator.VerifyTokenRequestFromRaw
(crypto/validator/validator.go:45-108) with its signature checks, on top of the
oracle's decoders (ftsoracle.request), its idemix verifiers (ftsoracle.idemix)
and the P-256 restatement (tests/p256_ref.py).  Written from the reference's
control flow, one Go statement at a time; it shares no code with the product's
merge (host/request.cpp).

    signed   = asn1.Marshal(TokenRequest{Issues, Transfers}) || binding  (:57-66)
    sigs     = AuditorSignatures ++ Signatures if len(pp.Auditor) != 0 else Signatures  (:67-73)
    cursor   = common/backend.go:32-40: every HasBeenSignedBy takes the next one
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "py"))
import p256_ref as P  # noqa: E402
from ftsoracle import gojson as J  # noqa: E402
from ftsoracle import idemix as I  # noqa: E402
from ftsoracle import request as R  # noqa: E402
from ftsoracle import zkat as Z  # noqa: E402

OK = 0
ERR_PARSE = Z.ERR_PARSE
ERR_INPUT = R.ERR_INPUT
ERR_OWNER = I.ERR_OWNER
ERR_SIGNATURE = I.ERR_SIGNATURE
ERR_UNSUPPORTED = I.ERR_UNSUPPORTED
ERR_IDENTITY = P.ERR_IDENTITY
ERR_ISSUER = 15
CURVE_FP256BN, CURVE_BN254 = 0, 1


class Signers:
    """what the validator holds: the idemix issuer key and curve (None: no owner
    verifier on this side), whether x509 signatures are verified here, and
    PublicParams.Auditor (None = nil, b"" = empty non-nil) / Issuers"""

    def __init__(self, ipk=None, curve=CURVE_BN254, x509=True, auditor=None, issuers=()):
        self.ipk, self.curve, self.x509, self.auditor, self.issuers = ipk, curve, x509, auditor, list(issuers)


def signed_message(raw, binding):
    f = R.der_token_request(raw)
    return R.der_encode_token_request([f[0], f[1], [], []]) + binding


def _issuer_of(raw):
    """IssueAction.Issuer of an action that deserializes (nil -> b"")"""
    v = R._top(raw)
    if v is None:
        return b""
    v = J.resolve(v, R.ISSUE_SCHEMA)
    return J.dec_bytes(J.field(v, "Issuer")) or b""


def _owner_of(raw):
    """token.Token.Owner of a ledger value that deserializes (nil -> b"")"""
    v = R._top(raw)
    if v is None:
        return b""
    return J.dec_bytes(J.field(v, "Owner")) or b""


class _Backend:
    def __init__(self, message, sigs):
        self.message, self.sigs, self.cursor = message, sigs, 0

    def has_been_signed_by(self, verify):
        """verify(message, sigma) -> code"""
        if self.cursor >= len(self.sigs):
            return ERR_SIGNATURE  # "invalid state, insufficient number of signatures"
        sigma = self.sigs[self.cursor]
        self.cursor += 1
        return verify(self.message, sigma)


def _x509_verifier(sg, identity):
    """(code, verify): DeserializeVerifier on this side"""
    if not sg.x509:
        return ERR_UNSUPPORTED, None
    code = P.identity_code(identity)
    if code != OK:
        return code, None
    q = P.public_key(identity)
    return OK, lambda msg, sig: P.signature_code(q, msg, sig)


def _owner_verifier(sg, owner):
    """(code, verify): Deserializer.GetOwnerVerifier on this side"""
    if sg.ipk is None:
        return ERR_UNSUPPORTED, None
    bn = sg.curve == CURVE_BN254
    try:
        typ, ident = I.raw_owner_decode(owner)
    except R.Asn1Error:
        return ERR_OWNER, None
    if typ == "htlc":
        return ERR_UNSUPPORTED, None
    if typ != "si":
        return ERR_OWNER, None
    nym, err = (I.bn_deserialize_idemix_identity if bn else I.deserialize_idemix_identity)(ident)
    if err:
        return err[0], None
    ver = I.bn_nym_verify if bn else I.nym_verify
    return OK, lambda msg, sig: ver(sg.ipk, nym, sig, msg)[0]


def verify_signed_token_request(pp, sg, raw, binding, get_state, zk=R._zk):
    """-> (code, failed_action)"""
    # VerifyTokenRequestFromRaw
    try:
        f = R.der_token_request(raw)
    except R.Asn1Error:
        return ERR_PARSE, -1
    signed = R.der_encode_token_request([f[0], f[1], [], []]) + binding
    sigs = (f[3] + f[2]) if (sg.auditor is not None and len(sg.auditor) != 0) else f[2]
    be = _Backend(signed, sigs)
    # verifyAuditorSignature
    if sg.auditor is not None:
        # an empty identity holds no PEM block: GetAuditorVerifier fails whoever verifies x509 signatures
        code, ver = _x509_verifier(sg, sg.auditor) if len(sg.auditor) != 0 else (ERR_IDENTITY, None)
        if code == OK:
            code = be.has_been_signed_by(ver)
        if code != OK:
            return code, -1
    # unmarshalIssueActions, unmarshalTransferActions
    try:
        issues = [R.decode_issue_action(x) for x in f[0]]
        transfers = [R.decode_transfer_action(x) for x in f[1]]
    except J.GoJSONError:
        return ERR_PARSE, -1
    # verifyIssues
    for k, a in enumerate(issues):
        if any(o is None for o in a["outputs"]):
            return Z.ERR_MALFORMED, k
        if any(o.kind != "ok" for o in a["outputs"]):
            return Z.ERR_PANIC, k
        code = zk(pp, "issue", [], [o.point for o in a["outputs"]], a["proof"] or b"", a["anonymous"])
        if code != OK:
            return code, k
        issuer = _issuer_of(f[0][k])
        if len(sg.issuers) != 0 and not any(issuer == x for x in sg.issuers):
            return ERR_ISSUER, k
        code, ver = _x509_verifier(sg, issuer)
        if code == OK:
            code = be.has_been_signed_by(ver)
        if code != OK:
            return code, k
    # verifyTransfers: TransferSignatureValidate, then TransferZKProofValidate
    for t, a in enumerate(transfers):
        at = len(issues) + t
        ins = []
        for key in a["inputs"]:
            val = get_state(key)
            if not val:
                return ERR_INPUT, at
            try:
                ins.append(R.decode_token(val))
            except J.GoJSONError:
                return ERR_INPUT, at
            code, ver = _owner_verifier(sg, _owner_of(val))
            if code == OK:
                code = be.has_been_signed_by(ver)
            if code != OK:
                return code, at
        if any(o is None or o.kind != "ok" for o in a["outputs"]) or any(e.kind != "ok" for e in ins):
            return Z.ERR_PANIC, at
        code = zk(pp, "transfer", [e.point for e in ins], [o.point for o in a["outputs"]], a["proof"] or b"", False)
        if code != OK:
            return code, at
    return OK, -1
