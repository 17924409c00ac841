#!/usr/bin/env python3
"""From a rocprofv3 --kernel-trace CSV of a bench run: the last `passes` device
passes (one k_verdict each).  Prints, per stream that runs k_decode, the gap
from the previous k_verdict's end on that stream to the next k_decode's start;
the union-busy fraction of the window; and per-kernel total time.
    python passgaps.py <kernel_trace.csv> <passes>"""
import csv
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
npass = int(sys.argv[2])
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["n"] = r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
rows.sort(key=lambda r: r["s"])
verd = [r for r in rows if "k_verdict" in r["n"]]
dec = [r for r in rows if r["n"].endswith("k_decode")]
print("kernels", len(rows), "k_verdict", len(verd), "k_decode", len(dec))
last_dec = dec[-npass:]
t0 = last_dec[0]["s"]
t1 = verd[-1]["e"]
win = [r for r in rows if r["e"] > t0 and r["s"] < t1]
print("window %.2f ms, %d kernels" % ((t1 - t0) / 1e6, len(win)))
by_stream = defaultdict(list)
for r in win:
    by_stream[r["Stream_Id"]].append(r)
gaps = []
for sid, rs in sorted(by_stream.items()):
    prev_v = None
    out = []
    for r in rs:
        if "k_verdict" in r["n"]:
            prev_v = r
        elif r["n"].endswith("k_decode") and prev_v is not None:
            # first kernel of the pass on this stream after the verdict (k_copy precedes k_decode)
            first = next(x for x in rs if x["s"] >= prev_v["e"])
            out.append(((first["s"] - prev_v["e"]) / 1e3, (r["s"] - prev_v["e"]) / 1e3))
            prev_v = None
    if out:
        print("stream %s: verdict->first kernel / ->k_decode (us):" % sid, " ".join("%.0f/%.0f" % g for g in out))
        gaps += out
if gaps:
    a = sorted(g[0] for g in gaps)
    b = sorted(g[1] for g in gaps)
    print("verdict -> next pass's first kernel: median %.0f us (min %.0f, max %.0f); -> k_decode: median %.0f us (min %.0f, max %.0f); n %d"
          % (a[len(a) // 2], a[0], a[-1], b[len(b) // 2], b[0], b[-1], len(a)))
iv = sorted((max(r["s"], t0), min(r["e"], t1)) for r in win)
busy, cur_s, cur_e = 0, iv[0][0], iv[0][1]
for s, e in iv[1:]:
    if s <= cur_e:
        cur_e = max(cur_e, e)
    else:
        busy += cur_e - cur_s
        cur_s, cur_e = s, e
busy += cur_e - cur_s
print("device busy (union of kernels) %.2f ms = %.1f %% of the window" % (busy / 1e6, 100.0 * busy / (t1 - t0)))
tot = defaultdict(lambda: [0, 0])
for r in win:
    tot[r["n"]][0] += r["e"] - r["s"]
    tot[r["n"]][1] += 1
print("per kernel: total ms (count)")
for n, (t, c) in sorted(tot.items(), key=lambda kv: -kv[1][0])[:16]:
    print("  %-40s %9.2f (%d)" % (n[:40], t / 1e6, c))
print("sum of kernel time %.2f ms" % (sum(t for t, _ in tot.values()) / 1e6))
