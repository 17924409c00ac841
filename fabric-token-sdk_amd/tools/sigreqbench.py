#!/usr/bin/env python3
"""The price of the signatures in the request path, on one GPU.

Workload: raw token requests of two 2-in/2-out transfer actions each (GPU-made
proofs, as zkatdlog.workload.RequestSet builds them) whose ledger inputs belong
to real idemix pseudonyms on BN254 and which carry the owners' signatures and
one x509 auditor's, made with the library's own batch signers.  One request in
64 carries a tampered signature; every verdict is checked.

In one process, alternating, best of --reps:
  (a) ftz_verify_token_requests_batched on the raw requests (no signature);
  (b) ftz_verify_signed_token_requests;
  (c) what a caller had before (b): (a), then ftz_verify_owner_signatures, then
      ftz_verify_ecdsa_signatures, one after the other, over messages assembled
      and packed beforehand (untimed);
  and (b) with a nil auditor and no x509 handle: the difference to (b) bounds
      what the x509 stage's own copy and upload of every message can cost.

    python fabric-token-sdk_amd/tools/sigreqbench.py [--requests 20000] [--reps 5] [--out profiles/signed_requests_bench.json]
"""
import argparse
import base64
import ctypes
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=20000)
    ap.add_argument("--per", type=int, default=2)
    ap.add_argument("--distinct", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    import ecsign_ref as E
    import nymsign_ref as S
    import zkatdlog
    from zkatdlog import _abi as A
    from zkatdlog import workload as W

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_a"]
    ipk_raw = bytes.fromhex(json.load(open(os.path.join(ROOT, "tests", "golden", "idemix_bn254_golden.json")))["ipk"])
    ctx = zkatdlog.Context(g["pp"].encode(), device=0)
    ix = zkatdlog.Idemix(ctx, ipk_raw, A.FTZ_CURVE_BN254)
    ec = zkatdlog.Ecdsa(ctx)
    t0 = time.time()
    valid = W.prove_distinct(ctx, args.distinct, tag=b"sigreq")

    # ---- signers: 64 pseudonyms of one user secret, one x509 auditor
    def h32(tag, mod):
        return (int.from_bytes(hashlib.sha256(tag).digest(), "big") % mod).to_bytes(32, "big")
    signer = ix.add_signer(h32(b"sigreq/sk", S.R - 1))
    r_nyms = [h32(b"sigreq/rnym/%d" % k, S.R) for k in range(64)]
    nyms = ix.make_nyms(signer, r_nyms)
    from ftsoracle import bn254 as C
    owners = [S.owner_of(C.g1_from_bytes(n)) for n in nyms]
    owners_b64 = [base64.b64encode(o).decode() for o in owners]
    d_aud = 1 + int.from_bytes(hashlib.sha256(b"sigreq/auditor").digest(), "big") % (E.N - 1)
    aud_signer, _ = ec.add_signer(d_aud.to_bytes(32, "big"))
    auditor = E.identity_of(d_aud)

    # ---- requests without signatures, their ledger and their signed messages
    n, per = args.requests, args.per
    ledger, acts_of, msgs, bindings, who = {}, [], [], [], []
    for r in range(n):
        acts, signers_r = [], []
        for a in range(per):
            ins, outs, proof = valid.item((r * per + a) % valid.n)
            keys = ["sig%07d:%d:%d" % (r, a, i) for i in range(len(ins) // 64)]
            for i, k in enumerate(keys):
                o = (r * 7 + a * 3 + i) % 64
                ledger[k] = ('{"Owner":"%s","Data":%s}' % (owners_b64[o], W._elem(ins[64 * i:64 * i + 64]))).encode()
                signers_r.append(o)
            acts.append(W.transfer_action_json(keys, ins, outs, proof))
        acts_of.append(acts)
        who.append(signers_r)
        bindings.append(b"tx%07d" % r)
        msgs.append(W.token_request(acts) + bindings[-1])

    # ---- signatures, in calls of 1000 requests
    raws, osigs, asigs = [], [], []
    expect = np.zeros(n, dtype=np.int32)
    failed = np.full(n, -1, dtype=np.int32)
    for r0 in range(0, n, 1000):
        rr = range(r0, min(n, r0 + 1000))
        sigs, codes = ix.sign_owner_signatures([(signer, r_nyms[o], nyms[o], msgs[r]) for r in rr for o in who[r]])
        assert not any(codes)
        au = ec.sign([(aud_signer, msgs[r]) for r in rr])
        k = 0
        for j, r in enumerate(rr):
            s = sigs[k:k + len(who[r])]
            k += len(who[r])
            a = au[j]
            if r % 64 == 63:  # tampered: an owner's signature, or the auditor's
                if (r // 64) % 2:
                    a = a[:-1] + bytes([a[-1] ^ 1])
                    expect[r], failed[r] = A.FTZ_ERR_SIGNATURE, -1
                else:
                    at = (r // 128) % len(s)
                    s[at] = s[at][:40] + bytes([s[at][40] ^ 1]) + s[at][41:]
                    expect[r], failed[r] = A.FTZ_ERR_SIGNATURE, at // (len(s) // per)
            osigs.append(s)
            asigs.append(a)
            raws.append(W.token_request(acts_of[r], sigs=s, auditor_sigs=[a]))
    t_setup = time.time() - t0

    led = zkatdlog.NativeLedger(ledger)
    i32 = ctypes.POINTER(ctypes.c_int32)
    plain, keep_a = A.pack_bytes(raws)
    signed, keep_b = A.pack_signed_requests(raws, bindings)
    aud_key = ec.add_identity(auditor)
    o_items = [(owners[o], msgs[r], osigs[r][k]) for r in range(n) for k, o in enumerate(who[r])]
    e_items = [(aud_key, msgs[r], asigs[r]) for r in range(n)]
    o_arr, keep_o = A.pack_owner_sigs(o_items)
    e_arr, keep_e = A.pack_ecdsa_sigs(e_items)
    codes = np.zeros(n, dtype=np.int32)
    fail = np.zeros(n, dtype=np.int32)
    cp, fp = codes.ctypes.data_as(i32), fail.ctypes.data_as(i32)
    # what (c) must find: the proofs alone accept everything, the tampering shows in the signature calls
    o_want = [A.FTZ_ERR_SIGNATURE if (expect[r] and failed[r] >= 0 and k == (r // 128) % len(who[r])) else 0
              for r in range(n) for k in range(len(who[r]))]
    e_want = [A.FTZ_ERR_SIGNATURE if (expect[r] and failed[r] < 0) else 0 for r in range(n)]

    def run_a():
        ctx.verify_token_requests_packed(plain, n, led, cp, fp, batched=True)
        assert not codes.any()

    def run_b():
        ctx.verify_signed_token_requests_packed(signed, n, led, cp, fp, ix, ec, auditor, ())
        assert np.array_equal(codes, expect) and np.array_equal(fail, failed)

    def run_c():
        run_a()
        assert ix.verify_owner_signatures_packed(o_arr, len(o_items)) == o_want
        assert ec.verify_signatures_packed(e_arr, n) == e_want

    # (b) without the x509 stage (auditor nil, no handle): what the second pass over the messages costs
    expect_o = np.where(failed >= 0, expect, 0).astype(np.int32)

    def run_b_owners():
        ctx.verify_signed_token_requests_packed(signed, n, led, cp, fp, ix, None, None, ())
        assert np.array_equal(codes, expect_o) and np.array_equal(fail, failed)

    runs = {"a_unsigned": run_a, "b_signed": run_b, "c_three_calls": run_c, "b_owners_only": run_b_owners}
    for f in runs.values():  # warm-up, untimed
        f()
    times = {k: [] for k in runs}
    stats = {}
    for _ in range(args.reps):
        for k, f in runs.items():
            ctx.request_stats(reset=True)
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
            stats[k] = ctx.request_stats(reset=True)
    led.close()
    msg_bytes = sum(len(m) for m in msgs) / n
    n_owner = len(o_items) / n
    out = {"requests": n, "transfers": n * per, "owner_signatures": len(o_items), "auditor_signatures": n,
           "tampered": int((expect != 0).sum()), "request_bytes_mean": round(sum(len(x) for x in raws) / n, 1),
           "signed_message_bytes_mean": round(msg_bytes, 1), "setup_s": round(t_setup, 1), "reps": args.reps,
           "layout": "two blobs: the owner pass and the x509 pass each upload the request's signed message",
           # dev/idemix.h: job + 240 B of integers + 176 B of transcript prefix per owner item; ecdsa_rt.hip: 16 + 128 + 16
           "signature_stage_upload_bytes_per_request_estimate": round(2 * msg_bytes + n_owner * (32 + 240 + 176) + 160, 1)}
    for k in runs:
        best = min(times[k])
        out[k] = {"best_s": round(best, 4), "runs_s": [round(x, 4) for x in times[k]],
                  "spread_s": round(max(times[k]) - min(times[k]), 4), "requests_per_s": round(n / best, 1),
                  "transfers_per_s": round(n * per / best, 1), "calling_thread_ms": stats[k]}
    out["b_over_a"] = round(min(times["b_signed"]) / min(times["a_unsigned"]), 3)
    out["x509_stage_s"] = round(min(times["b_signed"]) - min(times["b_owners_only"]), 4)
    out["b_over_c"] = round(min(times["b_signed"]) / min(times["c_three_calls"]), 3)
    out["b_not_slower_than_c_within_c_spread"] = bool(
        min(times["b_signed"]) <= min(times["c_three_calls"]) + out["c_three_calls"]["spread_s"])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    ix.close()
    ec.close()
    ctx.close()


if __name__ == "__main__":
    main()
