"""Orders of the generating calls (ftz_generate_transfers / ftz_generate_issues)
and what the oracle composes for them: blinding factors from the order's seed,
commitments, the oracle's proof, Go's JSON of the action and of one
token.Metadata per output.  Shared by the CPU tier (tests/test_generate.py) and
the GPU tier (tests/test_generate_gpu.py); oracle proofs are slow, so the
expected values of the parity orders are computed once per process."""
import hashlib
import random

from ftsoracle import bn254 as C
from ftsoracle import gojson as J
from ftsoracle import zkat as Z

TYPE = 'tok<&>"x"'
LONG_OWNER = bytes((7 * i + 3) % 251 for i in range(701))


def compressed(pt):
    """gnark's compressed form of a G1 point in a 64-byte input slot"""
    x, y = pt
    flag = 0xC0 if y > C.P - y else 0x80
    b = bytearray(x.to_bytes(32, "big"))
    b[0] |= flag
    return bytes(b) + bytes(32)


def transfer_order(pp, seed_i, n_in, n_out, ids, owners, ttype=TYPE, compress=(), out_values=None, bound=None):
    rng = random.Random(seed_i)
    top = bound or pp.base ** pp.exponent
    ins_v = [rng.randrange(top // (n_in + 1)) for _ in range(n_in)]
    in_bf = [rng.randrange(C.R) for _ in range(n_in)]
    if out_values is None:  # balanced: the outputs split the inputs' sum
        s = sum(ins_v)
        out_values = [s // n_out] * (n_out - 1)
        out_values.append(s - sum(out_values))
    ins = [Z.token_commitment(pp, ttype, v, b) for v, b in zip(ins_v, in_bf)]
    raw = [compressed(p) if i in compress else C.g1_bytes(p) for i, p in enumerate(ins)]
    return {"ids": list(ids), "inputs": b"".join(raw), "in_values": ins_v, "in_bfs": in_bf,
            "out_values": list(out_values), "owners": list(owners), "type": ttype,
            "seed": hashlib.sha256(b"generate-seed-%d" % seed_i).digest(), "_ins": ins}


def issue_order(pp, seed_i, owners, issuer, ttype=TYPE, values=None, bound=None):
    rng = random.Random(seed_i)
    top = bound or pp.base ** pp.exponent
    values = list(values) if values is not None else [rng.randrange(top) for _ in owners]
    return {"issuer": issuer, "values": values, "owners": list(owners), "type": ttype,
            "seed": hashlib.sha256(b"generate-issue-seed-%d" % seed_i).digest()}


def parity_transfers(pp):
    """the shapes, escapes, owner lengths (the three base64 padding classes, both
    empty forms, a long one) and the compressed input of the parity test"""
    return [transfer_order(pp, 11, 1, 1, ['a"b'], [None]),
            transfer_order(pp, 22, 2, 2, ["k\\1", "x<y"], [b"", b"\x01"], compress=(0,)),
            transfer_order(pp, 12, 1, 2, ["u\u2028v"], [b"ab", b"abc"]),
            transfer_order(pp, 31, 3, 1, ["tx0:0", "tx0:1", "tx1:0"], [LONG_OWNER])]


def parity_issues(pp):
    return [issue_order(pp, 41, [LONG_OWNER], b"issuer-identity"),
            issue_order(pp, 42, [None, b""], None),
            issue_order(pp, 43, [b"xy"], b"")]


def _token(owner, point):
    return J.enc_struct([("Owner", J.enc_bytes(owner)), ("Data", J.enc_elem(C.g1_bytes(point)))])


def _metadata(ttype, v, bf, owner, issuer):
    return J.enc_struct([("Type", J.enc_str(ttype)), ("Value", Z.enc_zr(v)), ("BlindingFactor", Z.enc_zr(bf)),
                         ("Owner", J.enc_bytes(owner)), ("Issuer", J.enc_bytes(issuer))]).encode()


def expect_transfer(pp, o):
    """(action, [metadata], [commitment RawBytes], [blinding factors])"""
    rnd = Z.Rand(o["seed"])
    bfs = [rnd.zr("tx/token/bf/%d" % k) for k in range(len(o["out_values"]))]
    outs = [Z.token_commitment(pp, o["type"], v, b) for v, b in zip(o["out_values"], bfs)]
    proof = Z.transfer_prove(pp, Z.Rand(o["seed"]), o["_ins"], outs, list(zip(o["in_values"], o["in_bfs"])),
                             list(zip(o["out_values"], bfs)), o["type"], tag="tx")
    action = J.enc_struct([
        ("Inputs", J.enc_list(o["ids"], J.enc_str)),
        ("InputCommitments", J.enc_list(o["_ins"], lambda p: J.enc_elem(C.g1_bytes(p)))),
        ("OutputTokens", J.enc_list(list(zip(o["owners"], outs)), lambda t: _token(*t))),
        ("Proof", J.enc_bytes(proof)),
        ("Metadata", "{}")]).encode()
    metas = [_metadata(o["type"], v, b, w, None) for v, b, w in zip(o["out_values"], bfs, o["owners"])]
    return action, metas, [C.g1_bytes(p) for p in outs], bfs


def expect_issue(pp, o):
    rnd = Z.Rand(o["seed"])
    bfs = [rnd.zr("issue/token/bf/%d" % k) for k in range(len(o["values"]))]
    outs = [Z.token_commitment(pp, o["type"], v, b) for v, b in zip(o["values"], bfs)]
    proof = Z.issue_prove(pp, Z.Rand(o["seed"]), outs, list(zip(o["values"], bfs)), o["type"], anonymous=False,
                          tag="issue")
    action = J.enc_struct([
        ("Issuer", J.enc_bytes(o["issuer"])),
        ("outputs", J.enc_list(list(zip(o["owners"], outs)), lambda t: _token(*t))),
        ("Proof", J.enc_bytes(proof)),
        ("Anonymous", "false"),
        ("Metadata", "null")]).encode()
    metas = [_metadata(o["type"], v, b, w, o["issuer"]) for v, b, w in zip(o["values"], bfs, o["owners"])]
    return action, metas, [C.g1_bytes(p) for p in outs], bfs


_CACHE = {}


def parity_expected(pp, pp_key):
    """(transfer orders, their expectations, issue orders, their expectations), once per process"""
    if pp_key not in _CACHE:
        ts, iss = parity_transfers(pp), parity_issues(pp)
        _CACHE[pp_key] = (ts, [expect_transfer(pp, o) for o in ts], iss, [expect_issue(pp, o) for o in iss])
    return _CACHE[pp_key]
