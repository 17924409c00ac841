#!/usr/bin/env python3
"""Idemix pseudonym signing rate on BN254 (zkatdlog.Idemix.sign_owner_signatures):
signatures per second of one ftz_sign_owner_signatures call over N signatures
(default 8,192) under one signer, 9,500-byte messages shared by pairs of items
(the two owners of a two-input transfer sign the same request, as in bench.py's
owner_signatures leg), the binding's packing untimed, best of 5, for
  (a) deterministic randomness (the DRBG over sk, SHA-256(msg) and RNym), and
  (b) hedged randomness (32 bytes of entropy per signature).
The pseudonyms come from make_nyms on the same handle.  Every signature of the
warm-up call is verified by the same handle before timing, and the rate of that
verification (verify_owner_signatures, packed, best of 5) is recorded as context.
Writes profiles/nymsign_bench.json.
    python nymsignbench.py [N] [variant.so] [out.json]
"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nymsign_ref as S  # noqa: E402

import zkatdlog  # noqa: E402

if len(sys.argv) > 2:  # A/B: a variant build (build.py --variant)
    zkatdlog._abi.use_library(sys.argv[2])
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "nymsign_bench.json")
REPS = 5
MSG_LEN = 9500
PSEUDONYMS = 16

SK = (0x1234567 << 200) % S.R
msgs = [hashlib.shake_256(b"nymsignbench %d" % i).digest(MSG_LEN) for i in range((n + 1) // 2)]
seeds = [os.urandom(32) for _ in range(n)]

pp = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_a"]["pp"].encode()
ipk_raw = bytes.fromhex(json.load(open(os.path.join(ROOT, "tests", "golden", "idemix_bn254_golden.json")))["ipk"])
ctx = zkatdlog.Context(pp, device=0)
ix = zkatdlog.Idemix(ctx, ipk_raw, curve_id=zkatdlog._abi.FTZ_CURVE_BN254)
signer = ix.add_signer(SK.to_bytes(32, "big"))
r_nyms = [hashlib.sha256(b"rnym %d" % i).digest()[1:].rjust(32, b"\x00") for i in range(PSEUDONYMS)]  # < 2^248 < r
nyms = ix.make_nyms(signer, r_nyms)
ipk = S.I.IssuerPKBn254(ipk_raw)
assert nyms[0] == S.nym_bytes(S.make_nym(ipk, SK, int.from_bytes(r_nyms[0], "big")))
owners = [S.owner_of(S.C.g1_from_bytes(nb)) for nb in nyms]


def best_of(f):
    best = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def rate(hedged):
    items = [(signer, r_nyms[i % PSEUDONYMS], nyms[i % PSEUDONYMS], msgs[i // 2], seeds[i] if hedged else None)
             for i in range(n)]
    arr, keep = zkatdlog._abi.pack_nym_sign_items(items)
    sigs, codes = ix.sign_owner_signatures_packed(arr, n)  # warm-up, and every one verifies
    assert codes == [0] * n
    varr, vkeep = zkatdlog._abi.pack_owner_sigs([(owners[i % PSEUDONYMS], msgs[i // 2], sigs[i]) for i in range(n)])
    assert ix.verify_owner_signatures_packed(varr, n) == [0] * n
    best, out = best_of(lambda: ix.sign_owner_signatures_packed(arr, n))
    assert out[1] == [0] * n and (hedged or out[0] == sigs)
    vbest, vout = best_of(lambda: ix.verify_owner_signatures_packed(varr, n))
    assert vout == [0] * n
    return ({"signatures": n, "best_ms": round(best * 1e3, 3), "per_s": round(n / best)},
            {"signatures": n, "best_ms": round(vbest * 1e3, 3), "per_s": round(n / vbest)})


det, vdet = rate(False)
hed, vhed = rate(True)
out = {"n": n, "reps": REPS, "msg_len": MSG_LEN, "distinct_messages": len(msgs), "pseudonyms": PSEUDONYMS,
       "deterministic": det, "hedged": hed,
       "verify_context": {"what": "verify_owner_signatures on the same handle over the signatures just made "
                                  "(packed, best of %d); context, not a baseline of the signer" % REPS,
                          "deterministic": vdet, "hedged": vhed}}
ix.close()
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(out))
