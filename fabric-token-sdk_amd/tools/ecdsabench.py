#!/usr/bin/env python3
"""x509 ECDSA P-256 verification rate (zkatdlog.Ecdsa): signatures per second of
one ftz_verify_ecdsa_signatures call over N signatures (default 8,192), the
binding's packing untimed, for
  (a) one registered key (the auditor: fixed-base tables for G and Q), and
  (b) all ad-hoc keys (every signature under another identity, decoded per call).
Writes profiles/ecdsa_bench.json.  Where the `openssl` CLI exists the file also
records 16 x the verify rate of `openssl speed -seconds 1 ecdsap256` as CPU
context (one core's rate times 16 cores; context, not a baseline of this code).
    python ecdsabench.py [N] [variant.so]
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import p256_ref as R  # noqa: E402

import zkatdlog  # noqa: E402

if len(sys.argv) > 2:  # A/B: a variant build (build.py --variant)
    zkatdlog._abi.use_library(sys.argv[2])
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
REPS = 5


def identity_of(pt):
    return R.serialized_identity(R.pem_encode("PUBLIC KEY", R.spki_der(*pt)))


def sign_with(d, msg, k, kg):
    """low-S signature with nonce k, kg = k G"""
    e = int.from_bytes(hashlib.sha256(msg).digest(), "big")
    r = kg[0] % R.N
    s = pow(k, -1, R.N) * (e + r * d) % R.N
    assert r and s
    return R.encode_signature(r, min(s, R.N - s))


# keys d = D0 + i and nonces k = K0 + i by repeated addition of G (one affine addition each)
D0, K0 = 0x1234567 << 200, 0x7654321 << 190
msgs = [b"request %d " % i + bytes((i * 7 + j) & 0xff for j in range(i % 200)) for i in range(n)]
dq, kg = R.mul(R.G, D0), R.mul(R.G, K0)
one_key = identity_of(dq)
reg_items, adhoc_items = [], []
for i in range(n):
    reg_items.append((msgs[i], sign_with(D0, msgs[i], K0 + i, kg)))
    adhoc_items.append((identity_of(dq), msgs[i], sign_with(D0 + i, msgs[i], K0 + i, kg)))
    dq, kg = R.add(dq, R.G), R.add(kg, R.G)
assert R.verify(adhoc_items[-1][0], adhoc_items[-1][1], adhoc_items[-1][2]) == 0

pp = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_a"]["pp"].encode()
ctx = zkatdlog.Context(pp, device=0)
ec = zkatdlog.Ecdsa(ctx)
key = ec.add_identity(one_key)


def rate(items):
    arr, keep = zkatdlog._abi.pack_ecdsa_sigs(items)
    assert ec.verify_signatures_packed(arr, len(items)) == [0] * len(items)  # warm-up, and every one verifies
    best = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        codes = ec.verify_signatures_packed(arr, len(items))
        dt = time.perf_counter() - t0
        assert not any(codes)
        best = dt if best is None else min(best, dt)
    return {"signatures": len(items), "best_ms": round(best * 1e3, 3), "per_s": round(len(items) / best)}


out = {"n": n, "reps": REPS, "registered_key": rate([(key, m, s) for m, s in reg_items]),
       "adhoc_keys": rate(adhoc_items)}
if shutil.which("openssl"):
    r = subprocess.run(["openssl", "speed", "-seconds", "1", "ecdsap256"], capture_output=True, text=True)
    m = re.search(r"ecdsa \(nistp256\)\s+\S+\s+\S+\s+([\d.]+)\s+([\d.]+)", r.stdout)
    if m:
        out["cpu_context"] = {"what": "16 x `openssl speed -seconds 1 ecdsap256` verify/s (one core x 16); context only",
                              "openssl_verify_per_s_one_core": float(m.group(2)),
                              "per_s_16_cores": round(16 * float(m.group(2)))}
ec.close()
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ecdsa_bench.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(out))
