#!/usr/bin/env python3
"""Pointcheval-Sanders verification rate (zkatdlog.Context.verify_ps_signatures)
and the time of the signed-values audit (Context.audit_signed_values):
  (a) signatures per second of one ftz_verify_ps_signatures call over N items
      (default 8,192): the signed values of the golden PP-A randomized (r R, r S)
      -- valid -- with every 64th item's m off by one, packing untimed, best of 5,
      every code checked;
  (b) the audit of PP-A (base 100) and of a base-4096 parameter set made with
      setup_public_params, best of 5, all codes zero.
There is no target.  For context the membership rate implied by a bench.py
headline on the same box -- transfers/s x 4 at PP-A, a 2-in/2-out transfer
holding four membership proofs that reach the pairings -- can be given with
--headline; a PS item is a membership job without its hashes.
Writes profiles/ps_bench.json.
    python psbench.py [N] [--headline TRANSFERS_PER_S] [--lib variant.so] [--out out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ps_ref as S  # noqa: E402

import zkatdlog  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=8192)
ap.add_argument("--headline", type=float, default=None, help="bench.py transfers/s of the parent commit on this box")
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps_bench.json"))
args = ap.parse_args()
if args.lib:  # A/B: a variant build (build.py --variant)
    zkatdlog._abi.use_library(args.lib)
n, REPS, BIG_BASE = args.n, 5, 4096
C, Z = S.C, S.Z


def best_of(f):
    best = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


pp_raw = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_a"]["pp"].encode()
pp = Z.PublicParams.from_json(pp_raw)
base = len(pp.signed_values)
# 64 randomizations of the table (the Python scalar multiplications are the slow part), tiled to n
pool = []
for k in range(64):
    i, r = (7 * k) % base, 0x9E3779B97F4A7C15 * (k + 1)
    pool.append((i, C.g1_bytes(C.g1_mul(pp.signed_values[i][0], r)), C.g1_bytes(C.g1_mul(pp.signed_values[i][1], r))))
items, want = [], []
for k in range(n):
    m, r, s = pool[k % 64]
    bad = k % 64 == 63
    items.append((m + 1 if bad else m, Z.ps_hash(m), r, s))
    want.append(14 if bad else 0)
packed = zkatdlog._abi.pack_ps_sigs(items)

out = {"n": n, "reps": REPS, "tampered": sum(1 for w in want if w)}
with zkatdlog.Context(pp_raw, device=0) as ctx:
    assert list(ctx.verify_ps_signatures_packed(packed)) == want  # warm-up
    best, codes = best_of(lambda: ctx.verify_ps_signatures_packed(packed))
    assert list(codes) == want
    out["verify"] = {"signatures": n, "best_ms": round(best * 1e3, 3), "per_s": round(n / best)}
    assert ctx.audit_signed_values() == [0] * base
    best, codes = best_of(ctx.audit_signed_values)
    assert codes == [0] * base
    out["audit_pp_a"] = {"base": base, "best_ms": round(best * 1e3, 3)}
big = zkatdlog.setup_public_params(BIG_BASE, 2, b"psbench base 4096")
with zkatdlog.Context(big, device=0) as ctx:
    assert ctx.audit_signed_values() == [0] * BIG_BASE
    best, codes = best_of(ctx.audit_signed_values)
    assert codes == [0] * BIG_BASE
    out["audit_base_4096"] = {"base": BIG_BASE, "best_ms": round(best * 1e3, 3), "per_s": round(BIG_BASE / best)}
if args.headline:
    out["membership_context"] = {
        "what": "membership verifications per second implied by the parent commit's bench.py headline on the same "
                "box (transfers/s x 4 at PP-A); context, not a target",
        "headline_transfers_per_s": round(args.headline), "memberships_per_s": round(4 * args.headline),
        "ps_over_membership": round(out["verify"]["per_s"] / (4 * args.headline), 3)}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(out))
