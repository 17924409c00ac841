#!/usr/bin/env python3
"""zkatdlog batch-verification benchmark (BASELINE.json configs[1] / [3]).

One step = one pass of the verification path over a batch of `--batch`
(default 4096) synthetic 2-in/2-out zkatdlog transfers (BASELINE configs[1]),
END TO END: proof bytes in host memory -> Go-encoding/json parse + base64 +
structural checks on host threads -> one H2D copy -> the HIP kernel pipeline
-> verdict codes back in host memory.  The timed region is ONE
ftz_verify_transfers call over steps x batch transfers (the job engine cuts it
into device batches and pipelines host planning with device execution), so
`value` includes parsing and upload.  Inputs: distinct proofs made by the GPU
batch prover (a fresh seed per proof; made and checked before timing) with
~1/64 rows replaced by tampered golden-corpus proofs; every verdict is checked
against its expected code.

With N GPUs (torchrun, one process per GPU) the job is N x steps x batch
transfers sharded contiguously by transaction (zkatdlog.dist.verify_shard,
weak scaling: each rank verifies steps x batch); the only collective is the
verdict-bitmap all-gather over RCCL (configs[3]).  Prints ONE JSON line (a
compact summary, < 6 KB).

A plain run does only what the headline needs: set-up, warm-up, the timed
steps, the result line.  --full adds every other leg (device-only rate,
roofline, owner signatures, token requests, standalone MSMs, the batch prover,
PP-B, the n=1 seam, the CPU baselines; each can be switched off with its own
--no-* option) and writes every leg in full to --detail-out.
--dump-outputs DIR writes what the timed call returned for its last step (the
verdict codes of the job's last --batch transfers) to DIR/verdict_codes.npy.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--full] [--dump-outputs DIR]
"""
import os as _os

# Hardware queues per process: the engine keeps 4 batches in flight on 3 streams
# each (9 high- and 4 low-priority streams per context); HIP's default of 4
# queues would serialise them (set before the HIP runtime initialises).  12, not
# more: HIP caps each priority level at this many queues, and with 16 two live
# contexts (the PP-B leg's beside the headline's) mapped more queues than the
# hardware scheduler holds at once -- it then time-slices them and a kernel
# stalls ~10.7 ms every few passes (profiles/r04/hwqueue_stalls.txt).  The
# GPU boxes export HIP's default of 4, which costs the driver's 20-step job
# 3-7 % (profiles/r05/hwq_sweep.txt), so the bench raises it; it is not silent:
# the bench line reports the value it found and the one it ran with, and
# FTS_KEEP_HW_QUEUES=1 keeps an operator's value.
_HWQ_FOUND = _os.environ.get("GPU_MAX_HW_QUEUES")
if not (_os.environ.get("FTS_KEEP_HW_QUEUES") == "1" and _HWQ_FOUND):
    _os.environ["GPU_MAX_HW_QUEUES"] = "12"
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))

METRIC = "zkatdlog transfer proofs verified/sec (node) + BN254 G1 MSM 2^20 latency"
MAD_PER_M = 136  # u32 MADs per 254-bit CIOS Montgomery product (8x8 + 8x8 + 8)


_CPU = {}


def _cpu_lib():
    """oracle/cpu/libftscpu.so (the C++ CPU restatement; a labelled baseline,
    never on the product path)"""
    if "lib" not in _CPU:
        import ctypes

        from zkatdlog import _abi as A
        sys.path.insert(0, os.path.join(ROOT, "oracle", "cpu"))
        import build_cpu
        lib = ctypes.CDLL(build_cpu.build())
        lib.emu_ctx_create.restype = ctypes.c_void_p
        lib.emu_ctx_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        lib.emu_ctx_destroy.argtypes = [ctypes.c_void_p]
        lib.emu_verify_transfers.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(A.Transfer),
                                             ctypes.POINTER(ctypes.c_int32)]
        lib.emu_prove_transfers.restype = ctypes.c_long
        lib.emu_prove_transfers.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(A.TransferWitness),
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_char_p, ctypes.c_size_t]
        lib.emu_set_threads.argtypes = [ctypes.c_int]
        lib.emu_msm_cpu.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32,
                                    ctypes.c_char_p]
        lib.emu_gen_points.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p]
        lib.cpu_msm_pippenger.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                          ctypes.c_uint32, ctypes.c_char_p]
        _CPU["lib"] = lib
    return _CPU["lib"]


def host_cores():
    """(cores this process may run on, the machine's logical CPUs)"""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return aff, os.cpu_count() or aff


def cpu_quota():
    """CPUs the cgroup CPU quota grants (cgroup v2 cpu.max or v1 cfs quota /
    period), or None when unlimited / unknown: on a shared box the affinity
    mask can list every CPU of the machine while the quota allows a few."""
    import math
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else max(1, math.floor(int(q) / int(per)))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else max(1, q // per)
    except (OSError, ValueError):
        return None


def _cpu_ctx(pp_json):
    import ctypes
    lib = _cpu_lib()
    err = ctypes.create_string_buffer(256)
    c = lib.emu_ctx_create(pp_json, len(pp_json), err, 256)
    if not c:
        raise RuntimeError(err.value.decode())
    return lib, c


def cpu_verify(pp_json, job, cores, sample, reps=3):
    """The C++ CPU restatement of the verifier (oracle/cpu: host build of the
    planner + job code, 4 x 64-bit Montgomery) on `cores` threads over the first
    `sample` transfers of `job`: one warm-up, median of `reps` runs.  Returns
    (transfers/s, median seconds, sample)."""
    import ctypes

    import numpy as np
    lib, c = _cpu_ctx(pp_json)
    lib.emu_set_threads(cores)
    try:
        n = min(sample, job.n)
        codes = np.zeros(n, dtype=np.int32)
        cp = codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        lib.emu_verify_transfers(c, min(n, 2 * cores), job.ptr(), cp)  # warm-up
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            lib.emu_verify_transfers(c, n, job.ptr(), cp)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(codes, job.expect[:n]), "CPU restatement disagrees with the expected verdicts"
    finally:
        lib.emu_ctx_destroy(c)
    med = sorted(times)[reps // 2]
    return n / med, med, n


def cpu_prove(pp_json, bases, cores, n, reps=3):
    """The C++ CPU restatement of the batch prover (planner_prove + job code on
    the host) on `cores` threads: n 2-in/2-out transfer proofs, median of reps."""
    import ctypes

    import numpy as np

    from zkatdlog import _abi as A
    from zkatdlog import workload as W
    lib, c = _cpu_ctx(pp_json)
    lib.emu_set_threads(cores)
    try:
        sel = np.arange(n) % len(bases)
        wp, wn, keep = A.pack_transfer_witnesses_tiled(bases, sel, W.seeds(n, b"cpu-prover"))
        cap = n * 16384
        buf = np.empty(cap, dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        codes = np.zeros(n, dtype=np.int32)
        err = ctypes.create_string_buffer(256)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = lib.emu_prove_transfers(c, n, wp, buf.ctypes.data, cap, offs.ctypes.data, codes.ctypes.data, err, 256)
            times.append(time.perf_counter() - t0)
            assert r > 0, err.value
    finally:
        lib.emu_ctx_destroy(c)
    med = sorted(times)[reps // 2]
    return n / med, med


def cpu_msm(lg, cores, seed=7):
    """CPU-tuned Pippenger (oracle/cpu/msm_pippenger.cpp: gnark-crypto's CPU
    MultiExp restated -- XYZZ buckets, signed windows over GLV halves, tasks of
    window x point slice on every core, 4 x 64-bit Montgomery products) of the
    bench's 2^lg known-log MSM (P_i = (i+1) G, the same scalars as the GPU leg).
    Returns (ms of one run, RawBytes result)."""
    import ctypes

    import numpy as np
    lib = _cpu_lib()
    n = 1 << lg
    scal = np.random.default_rng(seed + lg).bytes(32 * n)
    pts = ctypes.create_string_buffer(64 * n)
    lib.emu_gen_points(n, 1, cores, pts)
    out = ctypes.create_string_buffer(64)
    lib.cpu_msm_pippenger(min(n, 4096), pts, scal, cores, 0, out)  # warm-up (threads, allocator)
    t0 = time.perf_counter()
    rc = lib.cpu_msm_pippenger(n, pts, scal, cores, 0, out)
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt * 1e3, out.raw


def cpu_baselines(pp_a, job_a, pp_b, job_b, bases_a, gpu_msm20):
    """CPU reference figures: the C++ restatement on ALL
    cores this process may use -- threads = the affinity mask's CPUs, capped by
    the cgroup CPU quota when one is set (the headline cpu_baseline) -- and on
    the 16-core per-GPU share of the box, for PP-A and PP-B verification, PP-A
    proving and the 2^20 Pippenger; with a quota below the affinity the
    oversubscribed all-affinity-threads run is reported too.  Samples are sized
    for a few seconds of CPU work each."""
    aff, nproc = host_cores()
    quota = cpu_quota()
    usable = min(aff, quota) if quota else aff
    share = min(16, usable)
    out = {"affinity_cores": aff, "nproc": nproc, "cgroup_cpu_quota": quota, "usable_cores": usable,
           "impl": "cpp-restatement (oracle/cpu, 4x64-bit Montgomery)"}
    head = None
    runs = [("all", usable), ("share16", share)]
    if usable < aff:
        runs.append(("affinity_threads", aff))
    for label, cores in runs:
        r, med, n = cpu_verify(pp_a, job_a, cores, max(2048, 48 * min(cores, usable)))
        out["verify_pp_a_" + label] = {"value": round(r, 2), "unit": "transfers/s", "cores": cores,
                                       "sample": "%d transfers, median %.2f s" % (n, med)}
        if label == "affinity_threads":
            continue
        if label == "all":
            head = {"value": round(r, 2), "unit": "transfers/s", "cores": cores, "kind": "port",
                    "impl": "cpp-restatement", "affinity_cores": aff, "nproc": nproc, "cgroup_cpu_quota": quota,
                    "sample": "%d transfers of the bench job (same proofs, same verdicts) verified by the C++ CPU "
                              "restatement of the verifier (oracle/cpu: host build of the planner + job code with the "
                              "GPU path's algorithms -- bilinear membership rewrite, GLV, fixed-base tables -- and "
                              "4x64-bit Montgomery products) on %d threads = every CPU this process may use "
                              "(affinity %d of nproc %d, cgroup CPU quota %s); median of 3 runs after a warm-up: "
                              "%.2f s" % (n, cores, aff, nproc, quota if quota else "none", med)}
        if job_b is not None:
            r, med, n = cpu_verify(pp_b, job_b, cores, max(256, 8 * cores))
            out["verify_pp_b_" + label] = {"value": round(r, 2), "unit": "transfers/s", "cores": cores,
                                           "sample": "%d PP-B transfers, median %.2f s" % (n, med)}
        r, med = cpu_prove(pp_a, bases_a, cores, max(512, 12 * cores))
        out["prove_pp_a_" + label] = {"value": round(r, 2), "unit": "proofs/s", "cores": cores,
                                      "sample": "median %.2f s" % med}
    ms, res = cpu_msm(20, usable)
    out["msm_2^20_all"] = {"ms": round(ms, 1), "cores": usable, "matches_gpu": gpu_msm20 is None or res == gpu_msm20,
                           "impl": "CPU-tuned Pippenger (oracle/cpu/msm_pippenger.cpp: XYZZ buckets, GLV, "
                                   "window x slice tasks on every usable core)"}
    return head, out


_PEAK = {}


def madpeak(device):
    if device in _PEAK:
        return _PEAK[device]
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftsmadpeak.so"))
    lib.ftz_madpeak.restype = ctypes.c_double
    lib.ftz_madpeak.argtypes = [ctypes.c_int, ctypes.c_uint32]
    _PEAK[device] = max(lib.ftz_madpeak(device, 20000) for _ in range(3))
    return _PEAK[device]


def valu_ceiling(device):
    """Highest measured VALU issue rate (wave-instructions/s, chip-wide) of the
    hot kernels' static instruction mixes (csrc/tools/madpeak.hip
    ftz_valu_rate ops 9 and 10) at 2 and 8 waves per SIMD: the issue-rate
    ceiling a kernel of that mix can reach on this GPU."""
    key = ("valu", device)
    if key not in _PEAK:
        import ctypes
        lib = ctypes.CDLL(os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftsmadpeak.so"))
        lib.ftz_valu_rate.restype = ctypes.c_double
        lib.ftz_valu_rate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]
        _PEAK[key] = max(lib.ftz_valu_rate(device, op, w, 20000) for op in (9, 10) for w in (2, 8))
    return _PEAK[key]


def msm_latency(ctx, lg, reps=5, seed=7):
    """BASELINE configs[2]: latency of one BN254 G1 MSM of 2^lg points resident
    in HBM (P_i = (i + 1) G generated on the device, random 256-bit scalars),
    median wall-clock of `reps` synchronous runs after one warm-up; the result
    must be identical on every run (tests/test_msm.py checks it bit-exactly).
    ms: scalars resident in HBM; ms_host_scalars: scalars copied from
    page-locked host memory inside the timed call (ftz_msm_run_scalars).
    With ctx.options["msm_precompute"] the resident-point mode (window multiples
    stored at load, one bucket set, no Horner chain); load_s is the staging
    time including that precomputation."""
    import numpy as np

    import zkatdlog
    n = 1 << lg
    pre = bool(ctx.options.get("msm_precompute"))
    scal = np.random.default_rng(seed + lg).bytes(32 * n)
    t_load = time.perf_counter()
    m = zkatdlog.Msm(ctx, scalars=scal, gen_offset=1)
    t_load = time.perf_counter() - t_load
    hbuf = None
    try:
        first = m.run()
        wall, dev = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = m.run()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(m.info()["last_ms"])
            assert out == first, "MSM result changed between runs"
        info = m.info()
        # the same MSM with the scalars starting in (page-locked) host memory:
        # ftz_msm_run_scalars = chunked H2D copies overlapped with the fused key
        # kernel, then the resident pipeline
        hbuf = zkatdlog.HostBuffer(ctx, len(scal))
        hbuf.write(scal)
        assert m.run_scalars(hbuf) == first, "host-scalar MSM differs"
        hwall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = m.run_scalars(hbuf)
            hwall.append((time.perf_counter() - t0) * 1e3)
            assert out == first, "host-scalar MSM result changed between runs"
    finally:
        m.close()
        if hbuf is not None:
            hbuf.close()
    wall.sort()
    dev.sort()
    hwall.sort()
    # algorithmic work of a GLV Pippenger with c-bit windows: one mixed addition
    # (7M + 4S) per (window, virtual point) and 2 Jacobian additions (12M + 4S)
    # per bucket in the running-sum reduction, in Montgomery products M
    c = info["window_bits"]
    windows, nv, buckets = (129 + c - 1) // c, 2 * n, 1 << (c - 1)
    m_prod = windows * nv * 11 + (1 if pre else windows) * 2 * buckets * 16
    peak = madpeak(ctx.device)
    ach = m_prod * MAD_PER_M / (dev[reps // 2] * 1e-3)
    return {"n": n, "ms": round(wall[reps // 2], 3), "device_ms": round(dev[reps // 2], 3),
            "ms_host_scalars": round(hwall[reps // 2], 3),
            "host_scalars_note": "scalars in page-locked host memory: %d MB H2D inside the time" % (32 * n >> 20),
            "window_bits": c, "mode": "resident-point" if pre else "variable-base", "load_s": round(t_load, 3),
            "result": first.hex(),
            "roofline": {"bound": "valu", "achieved": round(ach / 1e12, 4), "peak": round(peak / 1e12, 4),
                         "unit": "TMAD/s", "frac": round(ach / peak, 4), "m_products": m_prod,
                         "note": "W x 2n mixed adds x 11 M + (W, or 1 resident-point) x 2 x 2^(c-1) Jacobian "
                                 "adds x 16 M, 136 MAD per M, over the device time"}}


def msm_split_latency(ctx, lg, rank, world, dist, reps=5, seed=7):
    """configs[2] over N GPUs: the 2^lg known-log points split
    into contiguous rank slices (each rank stages its slice with its own
    generator offset), every rank runs its partial MSM, the 64-byte partials
    are all-gathered over RCCL and added on the device (zkatdlog.dist.msm_shard).
    Median over reps of the max-over-ranks wall time, barrier to barrier."""
    import numpy as np
    import torch

    import zkatdlog
    from zkatdlog.dist import max_elapsed, msm_shard, shard_range
    n = 1 << lg
    scal = np.random.default_rng(seed + lg).bytes(32 * n)
    a, b = shard_range(n, rank, world)
    m = zkatdlog.Msm(ctx, scalars=scal[32 * a:32 * b], gen_offset=1 + a) if b > a else None
    part = (lambda s, e: m.run()) if m else (lambda s, e: bytes(64))
    try:
        first = msm_shard(ctx, n, rank, world, dist, part)[2]
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            out = msm_shard(ctx, n, rank, world, dist, part)[2]
            times.append(max_elapsed(time.perf_counter() - t0, dist))
            assert out == first, "split MSM result changed between runs"
    finally:
        if m:
            m.close()
    times.sort()
    return {"n": n, "ms": round(times[reps // 2] * 1e3, 3), "ranks": world, "points_per_rank": b - a}


def prover_bench(ctx, batch, steps):
    """BASELINE configs[4] at the configs[1] shape: ONE ftz_prove_transfers call
    of steps x batch 2-in/2-out transfer proofs (witness bases tiled, a fresh
    seed per proof), end to end (witness structs in host memory -> proof JSON
    bytes in host memory).  Every proof is then re-verified by the GPU
    verifier."""
    import ctypes

    import numpy as np

    from zkatdlog import _abi as A
    from zkatdlog import workload as W
    bases = W.witness_bases()
    n = batch * steps
    sel = np.arange(n) % len(bases)
    wp, wn, keep = A.pack_transfer_witnesses_tiled(bases, sel, W.seeds(n, b"bench-prover"))
    ctx.prover_stats(reset=True)
    t0 = time.perf_counter()
    blob, offs, codes = ctx.prove_packed("transfer", wp, wn)
    dt = time.perf_counter() - t0
    host = ctx.prover_stats(reset=True)
    ins = np.frombuffer(b"".join(b["inputs"] for b in bases), dtype=np.uint8)
    outs = np.frombuffer(b"".join(b["outputs"] for b in bases), dtype=np.uint8)
    rows = np.zeros(n, dtype=A.transfer_dtype())
    ia, ik = A.buffer_address(ins)
    oa, ok_ = A.buffer_address(outs)
    pa, pk = A.buffer_address(blob)
    rows["inputs"], rows["n_in"] = ia + 128 * sel, 2
    rows["outputs"], rows["n_out"] = oa + 128 * sel, 2
    rows["proof"], rows["proof_len"] = pa + offs[:-1], offs[1:] - offs[:-1]
    v = ctx.verify_transfers_packed(ctypes.cast(rows.ctypes.data, ctypes.POINTER(A.Transfer)), n)
    return {"proofs_per_s": round(n / dt, 1), "ms_per_batch": round(dt / steps * 1e3, 3), "batch": batch,
            "proofs": n, "bytes_per_proof": round(float(offs[-1]) / n, 1),
            "all_accepted_by_gpu_verifier": bool((codes == 0).all() and (v == 0).all()),
            # host-side time of the call per pass (ftz_ctx_prover_stats): planning +
            # flattening (shape templates), enqueue, wait for the device, proof copy-out
            "host_ms_per_pass": {k[:-3]: round(host[k] / max(1, host["passes"]), 3)
                                 for k in ("plan_ms", "submit_ms", "wait_ms", "copy_ms")}}


def device_only(ctx, job, batch, steps, inflight=4):
    """Device-resident rate (the round-1 headline, kept as a secondary figure):
    `inflight` batches planned + uploaded once (ftz_batch_load_transfers), then
    re-run; no host parsing or upload in the timed region."""
    import numpy as np

    from zkatdlog import workload as W
    batches = []
    for k in range(inflight):
        sub = W.Job(job.rows[k * batch:(k + 1) * batch], job.expect[k * batch:(k + 1) * batch], [job])
        batches.append((ctx.load_packed(sub.ptr(), sub.n), sub))
    for b, _ in batches:
        b.run()
    t0 = time.perf_counter()
    for k in range(steps):
        b, _ = batches[k % len(batches)]
        if k >= len(batches):
            b.wait()
        b.submit()
    for b, _ in batches:
        b.wait()
    dt = time.perf_counter() - t0
    ok = all(np.array_equal(np.asarray(b.codes()), s.expect) for b, s in batches)
    stats = batches[0][0].stats()
    t1 = time.perf_counter()
    batches[0][0].run()
    lat = (time.perf_counter() - t1) * 1e3
    for b, _ in batches:
        b.close()
    return {"transfers_per_s": round(batch * steps / dt, 1), "ms_per_batch": round(dt / steps * 1e3, 3),
            "batches_in_flight": inflight, "batch_latency_ms": round(lat, 3), "verdicts_ok": ok,
            "kernel_ms": {k: round(v[0], 3) for k, v in stats.items()}}


def plan_rate(ctx, job, batch, reps=3):
    """Host planning of one batch (JSON parse, base64, structural checks, job
    layout into the pinned staging blob on the context's planning threads) plus
    its one H2D copy, via the staged load: best of `reps`, seconds."""
    from zkatdlog import workload as W
    sub = W.Job(job.rows[:batch], job.expect[:batch], [job])
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        b = ctx.load_packed(sub.ptr(), sub.n)
        best = min(best, time.perf_counter() - t0)
        b.close()
    return best


def roofline(ctx, job, batch, device, tx_per_s, keep_serial=False, pp_key="pp_a"):
    """Integer-VALU roofline of the dominant kernel.  The timed steps overlap
    three streams, so per-kernel wall times there include shared SIMDs; the
    roofline pass re-runs 3 steps of one batch with every kernel on one stream
    (ftz_ctx_set_serial, same kernels, same inputs) and takes each kernel's
    HIP-event time there.  achieved = counted Montgomery products per job
    (profiles/opcounts.json, the oracle-checked job code run with an op
    counter) x jobs x 136 MAD / time."""
    from zkatdlog import workload as W
    sub = W.Job(job.rows[:batch], job.expect[:batch], [job])
    b = ctx.load_packed(sub.ptr(), sub.n)
    ctx.set_serial(True)
    try:
        b.run()
        acc = None
        for _ in range(3):
            b.run()
            st = b.stats()
            acc = st if acc is None else {k: (acc[k][0] + st[k][0], st[k][1]) for k in st}
    finally:
        ctx.set_serial(keep_serial)
        b.close()
    kern = {k: (v[0] / 3, v[1]) for k, v in acc.items() if k != "total"}
    peak = madpeak(device)
    opc = json.load(open(os.path.join(ROOT, "profiles", "opcounts.json")))[pp_key]
    names = {"g1": "k_g1_part+k_g1_combine (side stream)", "g1p": "k_g1_part+k_g1_combine (pairing inputs)",
             "g2": "k_g2_part+k_g2_sum+k_g2_binv+k_g2lines1 (t' + pair-2 lines)", "miller": "k_miller", "fexp": "k_fexp_easy_a+k_fexp_binv+k_fexp_easy_b+k_fexp_expt x3+k_fexp_hard",
             "hash": "k_hash", "decode": "k_decode"}
    mjob = dict(opc["m_per_job"])
    mjob["g1p"] = mjob["g1"]  # the pairing-input G1 jobs run the same job code
    # device kernel split (tests/native/opcount.py): k_g2lines = t' + pair-2 lines, k_miller = f-chain only
    mk = opc.get("m_per_kernel_job", {})
    mjob["g2"] = mk.get("k_g2lines", mjob["g2"])
    mjob["miller"] = mk.get("k_miller", mjob["miller"])
    dom = max((k for k in kern if k in names and mjob.get(k)), key=lambda k: kern[k][0])
    m_job = mjob[dom]
    achieved = m_job * kern[dom][1] * MAD_PER_M / (kern[dom][0] * 1e-3)
    traffic = issue = None
    pmc = os.path.join(ROOT, "profiles", "pmc_fetch.json")
    if os.path.exists(pmc) and pp_key == "pp_a":
        pdoc = json.load(open(pmc))
        traffic = pdoc.get("per_launch_bytes", {}).get(dom)
        valu = pdoc.get("per_launch_valu", {})
        if valu:
            ceil = valu_ceiling(device)
            rates = {k: valu[k] / (kern[k][0] * 1e-3) for k in valu if k in kern and kern[k][0] > 0}
            issue = {"unit": "wave-inst/ns", "ceiling": round(ceil / 1e9, 1),
                     "per_kernel": {k: {"rate": round(r / 1e9, 1), "frac": round(r / ceil, 4)}
                                    for k, r in rates.items()},
                     "note": "SQ_INSTS_VALU per launch (profiles/pmc_fetch.json, rocprofv3 --pmc) / serial "
                             "kernel time, against the highest measured issue rate of the kernels' "
                             "instruction mixes (ftz_valu_rate, live); counts every issued VALU op, "
                             "including carries and moves the TMAD figure does not price"}
    step_mad = opc["m_per_tx"] * tx_per_s * MAD_PER_M
    return {"bound": "valu", "kernel": names[dom], "achieved": round(achieved / 1e12, 4),
            "peak": round(peak / 1e12, 4), "unit": "TMAD/s", "frac": round(achieved / peak, 4),
            "traffic": traffic, "issue": issue, "kernel_ms_serial": round(kern[dom][0], 3), "jobs": kern[dom][1],
            "m_per_job": round(m_job, 1),
            "serial_ms": {k: round(v[0], 3) for k, v in kern.items()},
            "per_kernel_frac": {k: round(mjob[k] * kern[k][1] * MAD_PER_M / (kern[k][0] * 1e-3) / peak, 4)
                                for k in kern if k in mjob and kern[k][0] > 0},
            "pipeline": {"achieved": round(step_mad / 1e12, 4), "frac": round(step_mad / peak, 4),
                         "note": "whole step, end to end: counted products per transfer x 136 x transfers/s"},
            "note": "integer VALU roofline (v_mad_u64_u32, peak = measured madpeak); per-kernel time from a "
                    "serial pass (ftz_ctx_set_serial) of one batch of the bench job; traffic = HBM bytes per "
                    "launch from rocprofv3 FETCH_SIZE (profiles/pmc_fetch.json)"}


def seam_leg(pp_json, device, valid, bad, seconds=2.0, callers=(64, 256, 1024, 4096), ctx=None, **opts):
    """The drop-in seam (BASELINE configs[1] at the Go shim's granularity): the
    shim calls ftz_verify_transfers with ONE TransferAction per call
    (validator_transfer.go:84-98).  (a) latency of one call of s transfers with
    nothing else in flight; (b) closed loop: C native threads each calling
    ftz_verify_transfers(ctx, 1, ...) back to back for `seconds`
    (csrc/tools/callers.cpp) -- throughput and per-call p50 / p99 latency.
    Verdicts are checked against the expected codes.  ctx: an existing context
    with the wanted options (the bench's own: a second context's 13 streams
    next to the first one's would share the 16 hardware queues), else one is
    made with **opts."""
    import ctypes

    import numpy as np

    import zkatdlog
    from zkatdlog import workload as W
    lib = ctypes.CDLL(os.path.join(ROOT, "fabric-token-sdk_amd", "zkatdlog", "_lib", "libftscallers.so"))
    lib.ftz_callers_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                    ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_size_t]
    pool = W.mixed_job(valid, bad, min(valid.n, 16384), seed=11)
    own = ctx is None
    if own:
        ctx = zkatdlog.Context(pp_json, device=device, **opts)
    try:
        lat = {}
        for s_ in (1, 16, 64, 256, 1024, 4096):
            sub = W.Job(pool.rows[:s_], pool.expect[:s_], [pool])
            ctx.verify_transfers_packed(sub.ptr(), s_)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                codes = ctx.verify_transfers_packed(sub.ptr(), s_)
                ts.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(codes, sub.expect)
            lat[str(s_)] = round(sorted(ts)[1], 3)
        loop = []
        out = (ctypes.c_double * 6)()
        exp = np.ascontiguousarray(pool.expect, dtype=np.int32)
        for c in callers:
            err = ctypes.create_string_buffer(512)
            rc = lib.ftz_callers_run(ctx._h, pool.rows.ctypes.data, exp.ctypes.data, pool.n, c, seconds, out, err, 512)
            if rc != 0:
                raise RuntimeError("ftz_callers_run failed: %d %s" % (rc, err.value.decode(errors="replace")))
            loop.append({"callers": c, "transfers_per_s": round(out[0], 1), "p50_ms": round(out[1], 3),
                         "p99_ms": round(out[2], 3), "max_ms": round(out[5], 3), "calls": int(out[3]),
                         "verdict_mismatches": int(out[4])})
        st = ctx.options
    finally:
        if own:
            ctx.close()
    return {"call_latency_ms_by_size": lat, "closed_loop_n1": loop,
            "options": {k: st[k] for k in ("batch", "slots", "window_us", "hold_inflight", "small_pass")}}


def seam_subprocess(device, seconds):
    """The seam leg in a fresh process (tools/seamsweep.py with the default
    options): measured inside bench.py after the other legs, the same calls ran
    markedly slower (64 callers: 4.7k/s at p50 15 ms against 11.9k/s at 5.4 ms
    alone, profiles/r03p), so the latency curve is taken in isolation, as a
    validator process would run it."""
    import subprocess
    assert device == 0, "the seam leg runs on local device 0 (rank 0)"
    env = dict(os.environ, SEAM_SECONDS=str(seconds))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fabric-token-sdk_amd", "tools", "seamsweep.py"), ""],
                       capture_output=True, text=True, env=env, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("seam leg failed: %s" % r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    out.pop("spec", None)
    out["process"] = "fresh (tools/seamsweep.py)"
    return out


def ppb_leg(device, args, bad_b):
    """BASELINE configs[0]'s 64-bit range proof (PP-B: base 16, exponent 16) on
    the GPU: the batch prover and ONE end-to-end ftz_verify_transfers call over
    the proofs it made (plus tampered PP-B corpus rows), with the verifier's
    roofline at PP-B (serial pass, profiles/opcounts.json pp_b)."""
    import numpy as np

    import zkatdlog
    from zkatdlog import workload as W
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_b"]
    pp = g["pp"].encode()
    ctx = zkatdlog.Context(pp, device=device)
    try:
        bases = W.random_witness_bases(ctx, 16, seed=16)
        n_prove = 4096
        W.prove_distinct(ctx, 512, tag=b"ppb-warm", bases=bases)
        t0 = time.perf_counter()
        valid = W.prove_distinct(ctx, n_prove, tag=b"ppb", bases=bases)
        t_prove = time.perf_counter() - t0
        # the engine sizes passes by pairing jobs: 4 x batch of them, the pairings of a
        # PP-A pass -- 1024 PP-B transfers (2 outputs x 16 digits each) per pass
        pass_n = max(1, 4 * ctx.options["batch"] // (2 * ctx.exponent))
        job = W.mixed_job(valid, bad_b, 64 * pass_n, seed=5)  # 64 device passes
        ctx.verify_transfers_packed(job.ptr(), (ctx.options["slots"] + 1) * pass_n)  # warm the engine slots
        t0 = time.perf_counter()
        codes = ctx.verify_transfers_packed(job.ptr(), job.n)
        dt = time.perf_counter() - t0
        ok = bool(np.array_equal(codes, job.expect))
        rate = job.n / dt
        roof = roofline(ctx, job, min(pass_n, job.n), device, rate, pp_key="pp_b")
    finally:
        ctx.close()
    return {"verify_transfers_per_s": round(rate, 1), "verify_transfers": job.n, "verdicts_bit_exact": ok,
            "prove_proofs_per_s": round(n_prove / t_prove, 1), "proofs": n_prove,
            "pp": "b=16,e=16 (values < 2^64)", "device_pass_transfers": pass_n, "roofline": roof}, (pp, job, bases)


def requests_leg(ctx, valid, n_req=100000, per=2):
    """Block-level binding (the recommended drop-in): ONE
    ftz_verify_token_requests_batched call over n_req raw asn1(TokenRequest)
    requests of `per` transfer actions each (GPU-made proofs, 1/97 of the
    requests spending a key missing from the ledger), end to end from request
    bytes: ASN.1 + action JSON decoding, ledger lookups through a NATIVE
    get_states callback (one call per 8192-request chunk, a hash map --
    tools/callers.cpp), element checks, ZK verification in the job engine,
    verdicts.  Then the same call with the one-key-at-a-time get_state."""
    import numpy as np

    import zkatdlog
    from zkatdlog import workload as W
    t0 = time.perf_counter()
    rs = W.RequestSet(valid, n_req, per=per)
    led = zkatdlog.NativeLedger(rs.ledger)
    t_build = time.perf_counter() - t0
    i32 = ctypes.POINTER(ctypes.c_int32)
    out = {"requests": n_req, "transfers": n_req * per, "request_bytes": rs.nbytes(), "setup_s": round(t_build, 1)}
    codes = np.zeros(n_req, dtype=np.int32)
    failed = np.zeros(n_req, dtype=np.int32)
    # warm-up over the whole set (untimed): the request threads' per-thread parse
    # buffers, the engine slots, and the first touch of the request bytes
    ctx.verify_token_requests_packed(rs.ptr(), n_req, led, codes.ctypes.data_as(i32), failed.ctypes.data_as(i32),
                                     batched=True)
    for batched in (True, False):
        codes[:] = 0
        failed[:] = 0
        c0 = led.counts()
        ctx.request_stats(reset=True)
        est0 = ctx.engine_stats(reset=True)
        t0 = time.perf_counter()
        ctx.verify_token_requests_packed(rs.ptr(), n_req, led, codes.ctypes.data_as(i32), failed.ctypes.data_as(i32),
                                         batched=batched)
        dt = time.perf_counter() - t0
        c1 = led.counts()
        stages = ctx.request_stats(reset=True)
        est = ctx.engine_stats()
        ok = bool(np.array_equal(codes, rs.expect) and np.array_equal(failed, rs.failed))
        out["batched_get_states" if batched else "per_key_get_state"] = {
            "requests_per_s": round(n_req / dt, 1), "transfers_per_s": round(n_req * per / dt, 1),
            "s": round(dt, 3), "verdicts_bit_exact": ok, "callback_calls": c1[0] - c0[0],
            "keys_looked_up": c1[1] - c0[1], "calling_thread_ms": stages,
            "engine": {"batches": est["batches"], "max_in_flight": est["max_in_flight"],
                       "plan_ms_per_batch": round(est["plan_ms"] / max(1, est["batches"]), 3),
                       "device_ms_per_batch": round(est["device_ms"] / max(1, est["batches"]), 3)}}
    led.close()
    return out


def owner_signatures(ctx, n=8192, reps=5):
    """Idemix owner-signature leg on both idemix curves:
    BN254 (the curve cmd/pp/dlog/gen.go:117 and the NWO topologies deploy; the
    reference's tokengen issuer) and FP256BN_AMCL (the unit-test keys)."""
    from zkatdlog import _abi as A
    return {"BN254": owner_signatures_curve(ctx, "idemix_bn254_golden.json", A.FTZ_CURVE_BN254, "BN254", n, reps),
            "FP256BN_AMCL": owner_signatures_curve(ctx, "idemix_golden.json", A.FTZ_CURVE_FP256BN_AMCL,
                                                   "FP256BN_AMCL", n, reps)}


def owner_signatures_curve(ctx, fixture, curve_id, curve_name, n, reps):
    """n NymSignatures (two input owners per ~9.5 KB request, one distinct message
    per request) verified by ONE ftz_verify_owner_signatures call, end to end from
    host bytes (proto / ASN.1 decoding, upload, k_nym_part + k_nym_fin, verdicts);
    best of `reps`.  Signatures: the fixture's "bench" entries (made offline), tiled."""
    import hashlib

    import zkatdlog
    g = json.load(open(os.path.join(ROOT, "tests", "golden", fixture)))
    ent = g["bench"]

    def expand(seed, L):
        out = bytearray()
        k = 0
        while len(out) < L:
            out += hashlib.sha256(seed + k.to_bytes(4, "big")).digest()
            k += 1
        return bytes(out[:L])
    msgs = {}
    for e in ent:
        msgs.setdefault(e["msg_seed"], expand(bytes.fromhex(e["msg_seed"]), e["msg_len"]))
    base = [(bytes.fromhex(e["owner"]), msgs[e["msg_seed"]], bytes.fromhex(e["sig"])) for e in ent]
    items = []
    for r in range(n // 2):  # request r: entries 2(r mod 32), +1 share one message; a fresh copy per request
        a, b = base[(2 * r) % len(base)], base[(2 * r + 1) % len(base)]
        m = bytes(bytearray(a[1]))
        items += [(a[0], m, a[2]), (b[0], m, b[2])]
    from zkatdlog import _abi as A
    ix = zkatdlog.Idemix(ctx, bytes.fromhex(g["ipk"]), curve_id=curve_id)
    arr, keep = A.pack_owner_sigs(items)  # the Go shim hands over its own buffers: packing is not timed
    codes = ix.verify_owner_signatures_packed(arr, n)  # warm-up
    ok = all(c == 0 for c in codes)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        codes = ix.verify_owner_signatures_packed(arr, n)
        dt = time.perf_counter() - t0
        ok = ok and all(c == 0 for c in codes)
        best = dt if best is None else min(best, dt)
    ix.close()
    return {"signatures_per_s": round(n / best, 1), "ms_per_call": round(best * 1e3, 3), "signatures": n,
            "msg_bytes": len(base[0][1]), "all_accepted": ok, "curve": curve_name}


def compact_line(line):
    """The final stdout line: the contract's fields plus every leg's headline
    numbers, without notes, per-kernel tables or MSM result bytes (those stay in
    the detail file).  Kept under 6 KB."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "verdicts_bit_exact", "accepted", "setup_s", "library", "engine",
            "cpu_baseline", "msm_split", "plan_upload_s_per_batch")
    out = {k: line[k] for k in keep if k in line}
    rf = line.get("roofline")
    if rf:
        out["roofline"] = {k: rf.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic",
                                                  "kernel_ms_serial", "jobs", "m_per_job", "serial_ms",
                                                  "per_kernel_frac")}
        iss = rf.get("issue") or {}
        out["roofline"]["issue_frac"] = {k: v.get("frac") for k, v in (iss.get("per_kernel") or {}).items()}
        out["roofline"]["pipeline_frac"] = (rf.get("pipeline") or {}).get("frac")

    def msm_rows(rows):
        if not rows:
            return rows
        return [{"n": r["n"], "ms": r["ms"], "device_ms": r.get("device_ms"), "ms_host_scalars": r.get("ms_host_scalars"),
                 "window_bits": r.get("window_bits"), "frac": (r.get("roofline") or {}).get("frac"),
                 "matches_variable_base": r.get("matches_variable_base")} for r in rows]
    out["msm"] = msm_rows(line.get("msm"))
    out["msm_resident"] = msm_rows(line.get("msm_resident"))
    m20 = next((r for r in (line.get("msm") or []) if r["n"] == 1 << 20), None)
    out["msm_2^20_latency_ms"] = m20["ms"] if m20 else None
    out["msm_2^20_latency_ms_device"] = m20.get("device_ms") if m20 else None
    out["msm_2^20_latency_ms_host_scalars"] = m20.get("ms_host_scalars") if m20 else None
    if line.get("prover"):
        out["prover"] = {k: line["prover"].get(k) for k in ("proofs_per_s", "ms_per_batch", "batch",
                                                            "all_accepted_by_gpu_verifier")}
    if line.get("pp_b"):
        p = line["pp_b"]
        out["pp_b"] = {k: p.get(k) for k in ("verify_transfers_per_s", "verdicts_bit_exact", "prove_proofs_per_s")}
        out["pp_b"]["frac"] = (p.get("roofline") or {}).get("frac")
    if line.get("device_only"):
        d = line["device_only"]
        out["device_only"] = {k: d.get(k) for k in ("transfers_per_s", "ms_per_batch", "batch_latency_ms",
                                                    "verdicts_ok", "kernel_ms")}
    if line.get("owner_signatures"):
        out["owner_signatures"] = {k: v.get("signatures_per_s") for k, v in line["owner_signatures"].items()}
    if line.get("token_requests"):
        t = line["token_requests"]
        out["token_requests"] = {"batched_transfers_per_s": (t.get("batched_get_states") or {}).get("transfers_per_s"),
                                 "per_key_transfers_per_s": (t.get("per_key_get_state") or {}).get("transfers_per_s"),
                                 "verdicts_bit_exact": all((t.get(k) or {}).get("verdicts_bit_exact", True)
                                                           for k in ("batched_get_states", "per_key_get_state")),
                                 "vs_verify_transfers": t.get("vs_verify_transfers")}
    if line.get("seam"):
        s = line["seam"]
        out["seam"] = {"call_latency_ms_by_size": s.get("call_latency_ms_by_size"),
                       "closed_loop_n1": [{k: r.get(k) for k in ("callers", "transfers_per_s", "p99_ms", "max_ms",
                                                                 "verdict_mismatches")}
                                          for r in s.get("closed_loop_n1") or []]}
    if line.get("cpu_baselines"):
        out["cpu_baselines"] = {k: (v.get("value") if isinstance(v, dict) and "value" in v else
                                    v.get("ms") if isinstance(v, dict) else v)
                                for k, v in line["cpu_baselines"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=256,
                    help="steps of --batch transfers per GPU (default: 256 x 4096 = a 1M-transfer job, configs[3])")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096, help="transfers per step (per GPU)")
    ap.add_argument("--distinct", type=int, default=16384, help="distinct GPU-made proofs in the workload")
    ap.add_argument("--full", action="store_true",
                    help="every leg besides the headline (CPU baselines, MSMs, prover, PP-B, seam, device-only, roofline, "
                         "owner signatures, token requests) and the detail file; without it only the timed steps run")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the verdict codes the timed call returned for its last step to DIR/verdict_codes.npy "
                         "(float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--msm", default="16,20,24", help="log2 sizes of the standalone G1 MSM (configs[2]); '' = none")
    ap.add_argument("--no-prover", action="store_true", help="skip the batch-prover leg (configs[4])")
    ap.add_argument("--no-seam", action="store_true", help="skip the n=1 drop-in seam leg (latency curve)")
    ap.add_argument("--no-ppb", action="store_true", help="skip the PP-B (64-bit range proof) verify / prove leg")
    ap.add_argument("--seam-seconds", type=float, default=2.0)
    ap.add_argument("--no-extras", action="store_true", help="only the headline (no device-only / roofline legs)")
    ap.add_argument("--device-batch", type=int, default=None,
                    help="proofs per device pass (ftz_options.batch; default: the library's)")
    ap.add_argument("--slots", type=int, default=None, help="job-engine batch slots (ftz_options.slots)")
    ap.add_argument("--threads", type=int, default=None, help="host planning threads (ftz_options.threads)")
    ap.add_argument("--serial", action="store_true",
                    help="profiling: every kernel on one stream for the whole run (ftz_ctx_set_serial), so that a "
                         "rocprofv3 kernel trace gives per-kernel durations without overlap")
    ap.add_argument("--opt", default="", help="A/B: extra ftz_options fields, e.g. 'pass_shaping=0,small_pass=0'")
    ap.add_argument("--lib", default=None, help="A/B only: a variant build of libftsamd.so (build.py --variant)")
    ap.add_argument("--detail-out", default=os.path.join("gpurun_out", "bench_detail.json"),
                    help="every leg in full (repo-relative path); the last stdout line is the compact summary")
    ap.add_argument("--layout", default=os.environ.get("FTZ_LAYOUT", ""),
                    help="kernel layouts, e.g. 'g2lines=sextet,pairing=one_lane' (ftz_ctx_set_layout)")
    args = ap.parse_args()
    if not args.full:  # a plain run: the headline alone
        args.no_cpu_baseline = args.no_prover = args.no_seam = args.no_ppb = args.no_extras = True
        args.msm = ""

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group("nccl")  # RCCL over xGMI

    import numpy as np

    import zkatdlog
    from zkatdlog import _abi
    from zkatdlog import workload as W
    from zkatdlog.dist import bitmap_of, verify_shard
    if args.lib:
        _abi.use_library(args.lib)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")))["pp_a"]
    pp_json = g["pp"].encode()
    extra_opt = {k: int(v) for k, v in (kv.split("=") for kv in filter(None, args.opt.split(",")))}
    ctx = zkatdlog.Context(pp_json, device=local, batch=args.device_batch, slots=args.slots, threads=args.threads,
                           **extra_opt)
    db = ctx.options["batch"]  # proofs per device pass: the engine cuts the job into passes of db
    if args.serial:
        ctx.set_serial(True)
    for kv in filter(None, (args.layout or "").split(",")):  # profiling A/B: stage=layout
        stage, layout = kv.split("=")
        ctx.set_layout(stage, layout)
    t_setup = time.time()
    valid = W.prove_distinct(ctx, args.distinct, tag=b"bench/%d" % rank)
    bad = W.golden_tampered()
    n_total = world * args.steps * args.batch
    job = W.mixed_job(valid, bad, n_total, seed=2024)  # the whole N-GPU job (rows are cheap)
    # warm-up: at least one device pass per engine slot (+1), so every slot's
    # grow-only pinned / device buffers exist before the timed job
    n_warm = max(args.warmup * args.batch, (ctx.options["slots"] + 1) * db) if args.warmup else 0
    warm = W.mixed_job(valid, bad, n_warm, seed=7, offset=5)
    t_setup = time.time() - t_setup
    if warm.n:
        wc = ctx.verify_transfers_packed(warm.ptr(), warm.n)
        assert np.array_equal(wc, warm.expect), "warm-up verdicts differ from the expected codes"

    def barrier():
        if dist is not None:
            import torch
            torch.cuda.synchronize()
            dist.barrier()

    barrier()
    ctx.engine_stats(reset=True)
    t0 = time.perf_counter()
    start, stop, codes = verify_shard(ctx, job.rows, n_total, rank, world)  # ONE call, end to end
    bits = bitmap_of(codes)
    if dist is not None:  # configs[3]: the RCCL verdict reduce is part of the timed job
        from zkatdlog.dist import gather_verdicts, max_elapsed
        ok_local = bool(np.array_equal(codes, job.expect[start:stop]))
        _, n_accept, verdict_ok = gather_verdicts(bits, stop - start, ok_local, dist)  # RCCL over xGMI
    barrier()
    elapsed = time.perf_counter() - t0
    est = ctx.engine_stats()
    if dist is not None:
        elapsed = max_elapsed(elapsed, dist)
    else:
        ok_local = bool(np.array_equal(codes, job.expect[start:stop]))
        verdict_ok, n_accept = ok_local, int((codes == 0).sum())

    if args.dump_outputs:  # what the caller of the timed path received for the last step of this rank's shard
        os.makedirs(args.dump_outputs, exist_ok=True)
        name = "verdict_codes" if world == 1 else "verdict_codes_rank%d" % rank
        last = np.asarray(codes[-min(args.batch, 1 << 23):], dtype=np.float32)  # at most 32 MB
        np.save(os.path.join(args.dump_outputs, name + ".npy"), last)

    msm_split = None
    if dist is not None and args.msm:
        lg_split = 20 if "20" in args.msm.split(",") else int(args.msm.split(",")[-1])
        msm_split = msm_split_latency(ctx, lg_split, rank, world, dist)

    if rank == 0:
        value = n_total / elapsed
        extras = {}
        if not args.no_extras:
            extras["plan_upload_s_per_batch"] = round(plan_rate(ctx, job, db), 4)
            extras["device_only"] = device_only(ctx, job, db, max(4, args.steps * args.batch // db),
                                                inflight=1 if args.serial else 4)
            extras["roofline"] = roofline(ctx, job, db, local, value, keep_serial=args.serial)
            extras["owner_signatures"] = owner_signatures(ctx)
            extras["token_requests"] = requests_leg(ctx, valid)
            extras["token_requests"]["vs_verify_transfers"] = round(
                extras["token_requests"]["batched_get_states"]["transfers_per_s"] / value, 3)
        msm = [msm_latency(ctx, int(x)) for x in args.msm.split(",") if x]
        msm_res = None
        if args.msm and not args.no_extras:  # resident-point mode, its own context (ftz_options differ)
            import zkatdlog
            with zkatdlog.Context(pp_json, device=local, msm_precompute=1) as cpre:
                msm_res = [msm_latency(cpre, int(x)) for x in args.msm.split(",") if x]
                for r in msm_res:  # same points and scalars: the same sum
                    plain = next((q for q in msm if q["n"] == r["n"]), None)
                    r["matches_variable_base"] = plain is None or plain["result"] == r["result"]
        msm20 = next((r["ms"] for r in msm if r["n"] == 1 << 20), None)
        msm20_bytes = next((bytes.fromhex(r["result"]) for r in msm if r["n"] == 1 << 20), None)
        prover = None if args.no_prover else prover_bench(ctx, args.batch, min(args.steps, 16))
        ppb, ppb_job = None, None
        if not args.no_ppb and not args.no_extras:
            ppb, ppb_job = ppb_leg(local, args, W.golden_tampered("pp_b"))
        if not args.no_seam and not args.no_extras:
            extras["seam"] = seam_subprocess(local, args.seam_seconds)
        cpu = None
        if world == 1 and not args.no_cpu_baseline:
            cpu, extras["cpu_baselines"] = cpu_baselines(pp_json, job, ppb_job[0] if ppb_job else None,
                                                         ppb_job[1] if ppb_job else None, W.witness_bases(),
                                                         msm20_bytes)
        line = {
            "metric": METRIC, "value": round(value, 2), "unit": "transfers/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32 (Fp/Fr Montgomery)",
            "data": "synthetic: %d distinct GPU-prover-made 2-in/2-out transfers (PP-A b=100 e=2, fresh seed per "
                    "proof) tiled over the job, ~1/64 rows tampered golden-corpus proofs; end to end from host "
                    "proof bytes (parse + upload + kernels + verdicts in the timed region)" % args.distinct,
            "config": {"workload": "batch verify %d zkatdlog transfers per GPU per step (BASELINE configs[1]); "
                                   "%d-GPU job of %d transfers sharded by tx (configs[3])"
                                   % (args.batch, world, n_total),
                       "batch_per_gpu": args.batch, "device_pass": db, "pp": "b=100,e=2", "fexp": "exact",
                       "parallelism": "tx-sharded x%d" % world},
            "verdicts_bit_exact": verdict_ok, "accepted": n_accept, "setup_s": round(t_setup, 2),
            "library": os.path.relpath(_abi.loaded_path(), ROOT),
            "engine": {"batches": est["batches"], "max_in_flight": est["max_in_flight"],
                       "host_plan_ms_per_batch": round(est["plan_ms"] / max(1, est["batches"]), 3),
                       "enqueue_ms_per_batch": round(est["submit_ms"] / max(1, est["batches"]), 3),
                       "device_ms_per_batch": round(est["device_ms"] / max(1, est["batches"]), 3),
                       "parse_rate_transfers_per_s": round(est["proofs"] / max(1e-9, est["plan_ms"] * 1e-3), 1),
                       "planning_threads": ctx.options["threads"],
                       "hw_queues": {"GPU_MAX_HW_QUEUES": int(os.environ["GPU_MAX_HW_QUEUES"]),
                                     "found_in_env": _HWQ_FOUND}},
            "roofline": extras.pop("roofline", None), "cpu_baseline": cpu,
            "msm_2^20_latency_ms": msm20, "msm": msm, "msm_resident": msm_res, "msm_split": msm_split, "prover": prover, "pp_b": ppb,
        }
        line.update(extras)
        summary = compact_line(line)
        if args.full:
            # every leg in full -> the detail file; the one stdout line (kept
            # short for callers that read only the tail of the output) is the
            # compact summary of the same numbers
            detail = os.path.join(ROOT, args.detail_out)
            os.makedirs(os.path.dirname(detail), exist_ok=True)
            with open(detail, "w") as f:
                json.dump(line, f, indent=1)
            summary["detail"] = args.detail_out
        print(json.dumps(summary), flush=True)
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()
    if not verdict_ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
