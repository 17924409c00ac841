#!/usr/bin/env python3
"""ftz_generate_transfers against the two calls it replaces, same process, same
device: 8,192 two-in/two-out PP-A orders with ~700-byte owners in one call, and
the same witnesses through ftz_commit_tokens followed by ftz_prove_transfers
(which returns proofs only: the caller would still write the action and
metadata JSON).  Packing is untimed (the witness array of the second leg points
into the buffer the commit call fills), best of 5; both figures and the
prover's host-side statistics go to profiles/generate_bench.json.
    python fabric-token-sdk_amd/tools/genbench.py
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))

import bench  # noqa: E402,F401  (sets GPU_MAX_HW_QUEUES before HIP starts)

import numpy as np  # noqa: E402

import zkatdlog  # noqa: E402
from zkatdlog import _abi as A  # noqa: E402
from zkatdlog import workload as W  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_bench.json"))
    a = ap.parse_args()
    n = a.n
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_a"]
    bases = [b for b in W.witness_bases() if len(b["in_values"]) == 2 and len(b["out_values"]) == 2]
    sd = W.seeds(n, b"genbench")
    rng = random.Random(7)
    owners = [bytes(rng.randrange(256) for _ in range(700)) for _ in range(16)]
    u8p, szp, i32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)
    with zkatdlog.Context(g["pp"].encode(), device=0) as ctx:
        lib = ctx._lib
        # ---- the new call
        orders = []
        for i in range(n):
            b = bases[i % len(bases)]
            orders.append({"ids": ["tx%07d:0" % i, "tx%07d:1" % i], "inputs": b["inputs"], "in_values": b["in_values"],
                           "in_bfs": b["in_bfs"], "out_values": b["out_values"],
                           "owners": [owners[i % 16], owners[(i + 5) % 16]], "type": b["type"],
                           "seed": sd[32 * i:32 * i + 32]})
        oarr, okeep = A.pack_transfer_orders(orders)
        na, nm = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.ftz_generate_transfers_size(ctx._h, n, oarr, ctypes.byref(na), ctypes.byref(nm)) == 0
        act, meta = np.empty(na.value, dtype=np.uint8), np.empty(nm.value, dtype=np.uint8)
        coms = np.empty(64 * 2 * n, dtype=np.uint8)
        aoff, moff = np.zeros(n + 1, dtype=np.uint64), np.zeros(2 * n + 1, dtype=np.uint64)
        codes = np.zeros(n, dtype=np.int32)

        def generate():
            rc = lib.ftz_generate_transfers(ctx._h, n, oarr, act.ctypes.data_as(u8p), na.value, aoff.ctypes.data_as(szp),
                                            meta.ctypes.data_as(u8p), nm.value, moff.ctypes.data_as(szp),
                                            coms.ctypes.data_as(u8p), codes.ctypes.data_as(i32p))
            assert rc == 0 and not codes.any()
        # ---- the two calls it replaces, on the same witnesses (blinding factors drawn by the caller)
        bfs = [[rng.randrange(1, R) for _ in range(2)] for _ in range(n)]
        opens = [(bases[i % len(bases)]["type"], bases[i % len(bases)]["out_values"][k], bfs[i][k])
                 for i in range(n) for k in range(2)]
        parr, pkeep = A.pack_openings(opens)
        cbuf = np.zeros(64 * 2 * n, dtype=np.uint8)
        ws = [dict(bases[i % len(bases)], out_bfs=bfs[i], seed=sd[32 * i:32 * i + 32]) for i in range(n)]
        warr, wkeep = A.pack_transfer_witnesses(ws)
        for i in range(n):  # the outputs are what the commit call writes
            warr[i].outputs = cbuf.ctypes.data + 128 * i
        cap = n * 12288
        pbuf, poff, pcodes = np.empty(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)

        def two_calls():
            assert lib.ftz_commit_tokens(ctx._h, 2 * n, parr, cbuf.ctypes.data_as(u8p)) == 0
            rc = lib.ftz_prove_transfers(ctx._h, n, warr, pbuf.ctypes.data_as(u8p), cap, poff.ctypes.data_as(szp),
                                         pcodes.ctypes.data_as(i32p))
            assert rc == 0 and not pcodes.any()
        res = {"orders": n, "shape": "2-in/2-out PP-A", "owner_bytes": 700, "reps": a.reps}
        for name, fn in (("generate", generate), ("commit_then_prove", two_calls)):
            fn()  # warm-up: slots, tables
            ctx.prover_stats(reset=True)
            best = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            st = ctx.prover_stats(reset=True)
            res[name] = {"best_ms": round(best * 1e3, 3), "orders_per_s": round(n / best, 1),
                         "host_ms_per_call": {k: round(v / a.reps, 3) for k, v in st.items() if k.endswith("_ms")}}
        res["generate"]["output_bytes"] = int(aoff[n]) + int(moff[2 * n]) + 128 * n
        res["commit_then_prove"]["output_bytes"] = int(poff[n]) + 128 * n
        res["generate_not_slower"] = res["generate"]["best_ms"] <= res["commit_then_prove"]["best_ms"]
        # the generated actions verify (one request per action, ledger from the inputs)
        ab = act.tobytes()
        reqs = [zkatdlog.encode_token_request([], [ab[int(aoff[i]):int(aoff[i + 1])]]) for i in range(0, n, 64)]
        ledger = {}
        for i in range(0, n, 64):
            for k in range(2):
                raw = orders[i]["inputs"][64 * k:64 * k + 64]
                ledger[orders[i]["ids"][k]] = W.token_json(raw)
        vc, _ = ctx.verify_token_requests(reqs, ledger, batched=True)
        res["sampled_requests_verified"] = sum(1 for c in vc if c == 0)
        assert res["sampled_requests_verified"] == len(reqs)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
