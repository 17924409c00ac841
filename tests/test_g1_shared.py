"""Shared variable partials of the well-formedness sum job and the work lists
of k_g1_part, on the host build of the planner and the device job code.

The sum job of a transfer's well-formedness side, ... - c (sum T_i), takes
c (sum T_i) from the partials c T_i its per-token sibling jobs leave
(dev/jobs.h G1Job.sh_first / sh_count, job_g1_sum_parts).  Every case's verdict
and recomputed challenges must be the oracle's (computed live, CHALLENGE_TRACE)
-- the well-formedness class in full even for the rejected copies whose two
inputs or outputs are equal (the sibling sum doubles) or opposite (it is the
point at infinity).  The structural test checks the flattened plan itself."""
import base64
import ctypes
import json
import os
import subprocess

import pytest

import g1_shared_cases as S
from conftest import ROOT
from ftsoracle import zkat as Z
from zkatdlog import _abi as A

CAP = 128
SHARE_MAX = 8  # dev/jobs.h G1_SHARE_MAX


def emu_run(emu, pp_json, txs):
    """[(code, [(class, value)])] of the host emulation with debug challenges"""
    emu.emu_challenges.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p,
                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p,
                                   ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    ctx = emu.emu_ctx_create(pp_json, len(pp_json), ctypes.create_string_buffer(256), 256)
    assert ctx
    try:
        arr, keep = A.pack_transfers(txs)
        n = len(txs)
        codes = (ctypes.c_int32 * n)()
        kinds = (ctypes.c_int32 * (n * CAP))()
        vals = ctypes.create_string_buffer(32 * n * CAP)
        counts = (ctypes.c_size_t * n)()
        emu.emu_challenges(ctx, 0, n, ctypes.cast(arr, ctypes.c_void_p), codes, kinds, vals, CAP, counts)
        out = []
        for i in range(n):
            assert counts[i] <= CAP
            out.append((codes[i], [(kinds[i * CAP + k], vals.raw[32 * (i * CAP + k):32 * (i * CAP + k + 1)])
                                   for k in range(counts[i])]))
        return out
    finally:
        emu.emu_ctx_destroy(ctx)


@pytest.fixture(scope="module")
def emu_results(emu):
    cs = S.cases()
    return dict(zip([n for n, _ in cs], emu_run(emu, S.pp_a()[0], [tx for _, tx in cs])))


def test_substituted_cases_reach_the_sum_job():
    """the oracle rejects the copies on well-formedness after recomputing its transcript"""
    ora = S.oracle()
    for name in S.BASE:
        assert ora[name][0] == Z.OK, name
    for name in ("inputs_equal", "inputs_opposite", "outputs_equal", "outputs_opposite"):
        code, ch = ora[name]
        assert code == Z.ERR_WF, name
        assert [k for k, _ in ch].count(Z.ERR_WF) == 1, name


@pytest.mark.parametrize("name", [n for n, _ in S.cases()])
def test_emu_matches_oracle(emu_results, name):
    code, dev = emu_results[name]
    want, ora = S.oracle()[name]
    print(name, "code", code, "oracle", want, "challenges", len(dev), len(ora))
    assert code == want
    assert S.compare(name, want, dev, ora) > 0


# ------------------------------------------------------------------ plan structure
LISTS_LIB = os.path.join(ROOT, "tests", "_build", "libftsg1lists.so")


@pytest.fixture(scope="module")
def lists_lib():
    csrc = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "g1_lists.cpp")] + [
        os.path.join(csrc, "host", f) for f in ("planner.cpp", "gojson.cpp")]
    deps = srcs + [os.path.join(csrc, d, f) for d in ("dev", "host") for f in os.listdir(os.path.join(csrc, d))
                   if f.endswith(".h")]
    if not (os.path.exists(LISTS_LIB) and os.path.getmtime(LISTS_LIB) >= max(os.path.getmtime(p) for p in deps)):
        os.makedirs(os.path.dirname(LISTS_LIB), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread",
                        "-Wl,--no-undefined"] + srcs + ["-o", LISTS_LIB], check=True)
    lib = ctypes.CDLL(LISTS_LIB)
    lib.g1l_check.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                              ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t]
    return lib


def wide_transfer(n_in):
    """valid_2in_2out with its input side repeated to n_in tokens (parsed and
    planned like any proof; the verdict does not matter here)"""
    ins, outs, proof = S.cases()[0][1]
    doc = json.loads(proof)
    wf = json.loads(base64.b64decode(doc["WellFormedness"]))
    for key in ("InputBlindingFactors", "InputValues"):
        wf[key] = [wf[key][k % 2] for k in range(n_in)]
    doc["WellFormedness"] = base64.b64encode(json.dumps(wf).encode()).decode()
    return (b"".join(ins[64 * (k % 2):64 * (k % 2) + 64] for k in range(n_in)), outs, json.dumps(doc).encode())


def lists_check(lib, txs, threads):
    arr, keep = A.pack_transfers(txs)
    stats = (ctypes.c_uint32 * 5)()
    err = ctypes.create_string_buffer(256)
    pp = S.pp_a()[0]
    rc = lib.g1l_check(pp, len(pp), len(txs), ctypes.cast(arr, ctypes.c_void_p), threads, stats, err, 256)
    assert rc == 0, err.value.decode()
    return dict(zip(("jobs", "sharing", "fixed", "chains", "wide"), stats))


def test_lists_and_siblings_of_the_flat_plan(lists_lib):
    """every (job, fixed term) and every own chain once in the lists; sharing
    jobs after their siblings, same scalar, unit weights -- over several pieces
    (relocated sibling indices) and interleaved shapes"""
    base = [tx for _, tx in S.cases()]
    one = lists_check(lists_lib, [base[0]], 1)
    # a 2-in/2-out transfer: 14 side jobs, two of them sharing, 36 real fixed terms, 12 chains
    assert (one["sharing"], one["wide"]) == (2, 0)
    side = lists_check(lists_lib, [base[3]], 1)  # 1-in/1-out: well-formedness only, side jobs only
    assert side == {"jobs": 4, "sharing": 2, "fixed": 12, "chains": 2, "wide": 0}
    many = lists_check(lists_lib, [base[k % len(base)] for k in range(150)], 4)  # 4 pieces
    assert many["sharing"] == 2 * 150
    assert many["chains"] < many["jobs"] and many["fixed"] < 3 * many["jobs"]


def test_wide_side_keeps_its_chain(lists_lib):
    at_cap = lists_check(lists_lib, [wide_transfer(SHARE_MAX)], 1)
    over = lists_check(lists_lib, [wide_transfer(SHARE_MAX + 1)], 1)
    assert (at_cap["sharing"], at_cap["wide"]) == (2, 0)
    assert (over["sharing"], over["wide"]) == (1, 1)  # the output side still shares
