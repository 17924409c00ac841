"""GPU: ftz_options.lookahead -- full device passes planned, uploaded and
enqueued behind the pass running on their stream triple (engine.hip,
host/engine_policy.h).  Every test runs batch = 64 and slots = 4 on tiled
golden-corpus transfers (valid and tampered mixed, the oracle's verdicts as
expected codes), with lookahead 1 and, as the control, 0."""
import ctypes
import threading

import numpy as np
import pytest

from conftest import case_tuple

pytestmark = pytest.mark.gpu

N_BIG = 1280  # 20 passes of 64: each of the 8 buffer sets of lookahead = 1 is used at least twice


@pytest.fixture(scope="module")
def zk():
    import zkatdlog
    return zkatdlog


@pytest.fixture(scope="module")
def corpus(golden):
    return [c for c in golden["pp_a"]["cases"] if c["kind"] == "transfer"]


def _job(corpus, n, seed):
    """n corpus transfers in a seeded order: (ftz_transfer array, keepalive, expected codes)"""
    from zkatdlog import _abi as A
    idx = np.random.default_rng(seed).integers(len(corpus), size=n)
    arr, keep = A.pack_transfers([case_tuple(corpus[i]) for i in idx])
    return arr, keep, np.asarray([corpus[i]["expect"] for i in idx], dtype=np.int32)


@pytest.fixture(scope="module")
def big(corpus):
    job = _job(corpus, N_BIG, 9)
    assert (job[2] == 0).sum() > 100 and (job[2] != 0).sum() > 100
    return job


def _row(arr, i):
    """pointer to row i of a packed ftz_transfer array"""
    return ctypes.cast(ctypes.byref(arr, i * ctypes.sizeof(arr._type_)), ctypes.POINTER(arr._type_))


def _ctx(zk, golden, lookahead, **opts):
    return zk.Context(golden["pp_a"]["pp"].encode(), device=0, batch=64, slots=4, lookahead=lookahead, **opts)


def _join(threads, timeout=120):
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a caller is wedged"


@pytest.mark.parametrize("lookahead", [1, 0])
def test_ordering_and_reuse(zk, golden, big, lookahead):
    """one call of 20 passes: codes at their rows, and the counters show passes
    queued behind running ones with lookahead 1 and none with 0"""
    arr, keep, want = big
    with _ctx(zk, golden, lookahead) as c:
        assert c.options["lookahead"] == lookahead
        got = c.verify_transfers_packed(arr, N_BIG)
        st = c.engine_stats()
        sets, partial_ahead = c.engine_sets()
    assert np.array_equal(got, want)
    assert st["batches"] >= N_BIG // 64 and st["proofs"] == N_BIG, st
    assert len(sets) == 4 * (1 + lookahead)
    assert partial_ahead == 0
    if lookahead:
        assert st["queued_ahead"] > 0 and st["max_per_triple"] == 2, st
        assert 4 < st["max_in_flight"] <= 8, st
    else:
        assert st["queued_ahead"] == 0 and st["max_per_triple"] == 1 and st["max_in_flight"] <= 4, st


@pytest.mark.parametrize("lookahead", [1, 0])
@pytest.mark.parametrize("first_pass", [0, 24])
def test_first_pass_and_tail_split(zk, golden, big, lookahead, first_pass):
    """a smaller first pass shifts every later pass off the 64-row grid and the
    tail goes in two halves: same codes"""
    arr, keep, want = big
    with _ctx(zk, golden, lookahead, first_pass=first_pass, tail_split=16) as c:
        got = c.verify_transfers_packed(arr, N_BIG)
        st = c.engine_stats()
        partial_ahead = c.engine_sets()[1]
    assert np.array_equal(got, want)
    assert partial_ahead == 0
    assert (st["queued_ahead"] > 0) == bool(lookahead), st
    if first_pass:
        assert st["batches"] >= N_BIG // 64 + 1, st


@pytest.mark.parametrize("lookahead", [1, 0])
def test_small_calls_beside_a_big_job(zk, golden, corpus, big, lookahead):
    """32 threads of one-transfer calls while a 1,280-transfer call runs: every
    code right, nobody wedged, and no partial pass (the only kind a one-transfer
    call can be in, unless it filled up a pass of the big call) went behind a
    running pass"""
    arr, keep, want = big
    sarr, skeep, swant = _job(corpus, 32 * 4, 10)
    got_small = np.full(32 * 4, -99, dtype=np.int32)
    res, errs = {}, []
    with _ctx(zk, golden, lookahead) as c:
        def big_call():
            try:
                res["big"] = c.verify_transfers_packed(arr, N_BIG)
            except Exception as e:  # pragma: no cover - reported below
                errs.append(repr(e))

        def small_calls(t):
            try:
                for k in range(4):
                    i = 4 * t + k
                    got_small[i] = c.verify_transfers_packed(_row(sarr, i), 1)[0]
            except Exception as e:  # pragma: no cover - reported below
                errs.append(repr(e))

        th = [threading.Thread(target=big_call)] + [threading.Thread(target=small_calls, args=(t,)) for t in range(32)]
        for t in th:
            t.start()
        _join(th)
        st = c.engine_stats()
        partial_ahead = c.engine_sets()[1]
    assert not errs, errs[:3]
    assert np.array_equal(res["big"], want)
    assert np.array_equal(got_small, swant)
    assert st["proofs"] == N_BIG + 32 * 4, st
    assert partial_ahead == 0
    # only full passes queue ahead, and at most proofs // 64 passes can be full
    assert st["queued_ahead"] <= st["proofs"] // 64, st
    if not lookahead:
        assert st["queued_ahead"] == 0, st


def test_poisoned_item_in_a_pass_queued_ahead(zk, golden, corpus, big):
    """planning fails (ftz_ctx_debug_poison) for a pass in the middle of the big
    call, which is planned while the passes before it run: only that call gets
    the error, four callers beside it their codes, and the same call succeeds
    once the poison is cleared"""
    arr, keep, want = big
    others = [_job(corpus, 100, 20 + k) for k in range(4)]
    res = {}
    with _ctx(zk, golden, 1) as c:
        assert c._lib.ftz_ctx_debug_poison(c._h, arr[700].proof) == 0

        def call(key, a, n):
            try:
                res[key] = c.verify_transfers_packed(a, n)
            except zk.DeviceError as e:
                res[key] = e
        th = [threading.Thread(target=call, args=("big", arr, N_BIG))]
        th += [threading.Thread(target=call, args=(k, o[0], 100)) for k, o in enumerate(others)]
        for t in th:
            t.start()
        _join(th)
        assert isinstance(res["big"], zk.DeviceError) and "poisoned item" in str(res["big"]), res["big"]
        for k, o in enumerate(others):
            assert not isinstance(res[k], Exception), res[k]
            assert np.array_equal(res[k], o[2]), k
        assert c._lib.ftz_ctx_debug_poison(c._h, None) == 0
        assert np.array_equal(c.verify_transfers_packed(arr, N_BIG), want)
        assert c.engine_stats()["queued_ahead"] > 0


def test_destroy_after_queued_passes(zk, golden, big):
    """the context goes right after a big call returns, and right after a
    failed one: both destroys come back"""
    arr, keep, want = big
    for poison in (False, True):
        c = _ctx(zk, golden, 1)
        if poison:
            assert c._lib.ftz_ctx_debug_poison(c._h, arr[N_BIG - 100].proof) == 0
            with pytest.raises(zk.DeviceError, match="poisoned item"):
                c.verify_transfers_packed(arr, N_BIG)
        else:
            assert np.array_equal(c.verify_transfers_packed(arr, N_BIG), want)
        t = threading.Thread(target=c.close)
        t.start()
        _join([t], timeout=60)


def test_no_growth_after_warm_up(zk, golden, corpus, big):
    """5 passes warm all 8 buffer sets: each set then has the same capacities,
    and a 20-pass call leaves them as they are"""
    arr, keep, want = big
    warr, wkeep, wwant = _job(corpus, 5 * 64, 11)
    with _ctx(zk, golden, 1) as c:
        assert np.array_equal(c.verify_transfers_packed(warr, 5 * 64), wwant)
        before, _ = c.engine_sets()
        assert len(before) == 8 and all(min(s) > 0 for s in before), before
        assert len(set(before)) == 1, before
        assert np.array_equal(c.verify_transfers_packed(arr, N_BIG), want)
        after, _ = c.engine_sets()
    assert after == before
