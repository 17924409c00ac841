#!/usr/bin/env python3
"""x509 ECDSA P-256 signing rate (zkatdlog.Ecdsa.sign): signatures per second of
one ftz_sign_ecdsa call over N signatures (default 8,192) under one signer, the
binding's packing untimed, best of 5, for
  (a) deterministic nonces (RFC 6979), and
  (b) hedged nonces (32 bytes of entropy per signature).
The messages are the ones of tools/ecdsabench.py.  Every signature of the
warm-up call is verified by the same handle (registered key) before timing.
Writes profiles/ecsign_bench.json.  Where the `openssl` CLI exists the file also
records 16 x the sign rate of `openssl speed -seconds 1 ecdsap256` as CPU
context (one core's rate times 16 cores; context, not a baseline of this code).
    python ecsignbench.py [N] [variant.so] [out.json]
"""
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
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ecsign_bench.json")
REPS = 5

D0 = 0x1234567 << 200
msgs = [b"request %d " % i + bytes((i * 7 + j) & 0xff for j in range(i % 200)) for i in range(n)]
seeds = [os.urandom(32) for _ in range(n)]

pp = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_a"]["pp"].encode()
ctx = zkatdlog.Context(pp, device=0)
ec = zkatdlog.Ecdsa(ctx)
signer, xy = ec.add_signer(D0.to_bytes(32, "big"))
x, y = int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:], "big")
assert (x, y) == R.mul(R.G, D0)
key = ec.add_identity(R.serialized_identity(R.pem_encode("PUBLIC KEY", R.spki_der(x, y))))


def rate(items):
    arr, keep = zkatdlog._abi.pack_ecdsa_sign_items(items)
    sigs = ec.sign_packed(arr, len(items))  # warm-up, and every one verifies
    assert ec.verify_signatures([(key, it[1], s) for it, s in zip(items, sigs)]) == [0] * len(items)
    best = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = ec.sign_packed(arr, len(items))
        dt = time.perf_counter() - t0
        assert len(out) == len(items)
        best = dt if best is None else min(best, dt)
    return {"signatures": len(items), "best_ms": round(best * 1e3, 3), "per_s": round(len(items) / best)}


out = {"n": n, "reps": REPS, "deterministic": rate([(signer, m) for m in msgs]),
       "hedged": rate([(signer, m, s) for m, s in zip(msgs, seeds)])}
if shutil.which("openssl"):
    r = subprocess.run(["openssl", "speed", "-seconds", "1", "ecdsap256"], capture_output=True, text=True)
    m = re.search(r"ecdsa \(nistp256\)\s+\S+\s+\S+\s+([\d.]+)\s+([\d.]+)", r.stdout)
    if m:
        out["cpu_context"] = {"what": "16 x `openssl speed -seconds 1 ecdsap256` sign/s (one core x 16); context only",
                              "openssl_sign_per_s_one_core": float(m.group(1)),
                              "per_s_16_cores": round(16 * float(m.group(1)))}
ec.close()
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(out))
