"""GPU tier of x509 ECDSA P-256 verification (zkatdlog.Ecdsa -> ftz_verify_ecdsa_signatures
-> k_ecdsa_pre / _part / _fin): exact codes for every case of
tests/golden/ecdsa_golden.json on the registered-key route and on the ad-hoc
route, across wave and chunk boundaries, and from two threads."""
import json
import os
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_SIGS = 4096  # host/sigpipe.h SIG_CHUNK_ITEMS
KEYS_PER_HANDLE = 4


@pytest.fixture(scope="module")
def fx():
    """the fixture, a context and handles holding every registrable identity, at most 4 each"""
    import zkatdlog
    import p256_ref as R
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_golden.json")) as f:
        g = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")) as f:
        pp = json.load(f)["pp_a"]["pp"].encode()
    cases = []
    for c in g["cases"]:
        ident = bytes.fromhex(g["keys"][c["key"]]["identity"] if "key" in c else c["identity"])
        cases.append((c["name"], ident, bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), c["expect"]))
    ctx = zkatdlog.Context(pp, device=0)
    handles, where = [], {}  # identity -> (handle index, key)
    for _, ident, _, _, _ in cases:
        if ident in where or R.identity_code(ident) != 0:
            continue
        if not handles or sum(1 for h, _ in where.values() if h == len(handles) - 1) == KEYS_PER_HANDLE:
            handles.append(zkatdlog.Ecdsa(ctx))
        where[ident] = (len(handles) - 1, handles[-1].add_identity(ident))
    yield {"g": g, "cases": cases, "handles": handles, "where": where, "R": R}
    for h in handles:
        h.close()
    ctx.close()


def routed(fx, hi, i, registered):
    """item i (cycling the cases) for handle hi: by key when `registered` and the handle holds the identity"""
    name, ident, msg, sig, want = fx["cases"][i % len(fx["cases"])]
    h, key = fx["where"].get(ident, (None, None))
    who = key if (registered and h == hi) else ident
    return (who, msg, sig), want


def test_every_case_on_both_routes(fx):
    assert 2 <= len(fx["handles"]) and len(fx["where"]) <= KEYS_PER_HANDLE * len(fx["handles"])
    n = len(fx["cases"])
    want = [c[4] for c in fx["cases"]]
    names = [c[0] for c in fx["cases"]]
    # the ad-hoc route: every identity decoded per call
    got = fx["handles"][0].verify_signatures([(c[1], c[2], c[3]) for c in fx["cases"]])
    assert dict(zip(names, got)) == dict(zip(names, want))
    # the registered route: each handle takes the identities it holds by key (the rest stay ad-hoc)
    by_key = set()
    for hi, h in enumerate(fx["handles"]):
        items = [routed(fx, hi, i, True)[0] for i in range(n)]
        by_key |= {i for i in range(n) if isinstance(items[i][0], int)}
        got = h.verify_signatures(items)
        assert dict(zip(names, got)) == dict(zip(names, want)), hi
    # every case whose identity deserializes went through a table; the others cannot be registered
    R = fx["R"]
    for i, (name, ident, _, _, _) in enumerate(fx["cases"]):
        assert (i in by_key) == (R.identity_code(ident) == 0), name
    accepted = [names[i] for i in range(n) if want[i] == 0]
    assert "doubling" in accepted and "s_half_n" in accepted and len(accepted) >= 30


@pytest.mark.parametrize("size", [1, 63, 64, 65, CHUNK_SIGS + 1, 2 * CHUNK_SIGS + 1])
def test_tiled_batches_mixed_routes(fx, size):
    """valid and invalid cases interleaved, registered and ad-hoc items and all
    message lengths mixed within the waves; every position's code matches.  The
    last size is three chunks: the third goes into the slot the first one used"""
    h = fx["handles"][0]
    for start in ((0, 17) if size < 1000 else (5,)):
        items, want = [], []
        for i in range(size):
            it, w = routed(fx, 0, start + i, (i // 3) % 2 == 0)
            items.append(it)
            want.append(w)
        if size > 64:
            assert any(isinstance(it[0], int) for it in items) and any(not isinstance(it[0], int) for it in items)
            assert len({len(it[1]) for it in items[:64]}) > 4 and len(set(want[:64])) >= 2
        got = h.verify_signatures(items)
        assert got == want, [i for i in range(size) if got[i] != want[i]][:10]


def test_two_threads_on_one_handle(fx):
    h = fx["handles"][0]
    batches = []
    for t in range(2):
        pairs = [routed(fx, 0, 7 * t + i, i % 2 == t) for i in range(150)]
        batches.append(([p[0] for p in pairs], [p[1] for p in pairs]))
    serial = [h.verify_signatures(items) for items, _ in batches]
    assert serial == [want for _, want in batches]
    out = [None, None]

    def run(t):
        for _ in range(3):
            out[t] = h.verify_signatures(batches[t][0])

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert out == serial


def test_verifier_and_registration(fx):
    import zkatdlog
    from zkatdlog import _abi
    g, h = fx["g"], fx["handles"][0]
    good = next(c for c in fx["cases"] if c[0] == "good")
    _, ident, msg, sig, _ = good
    for who in (ident, fx["where"][ident][1]):
        v = h.verifier(who)
        v.verify(msg, sig)
        with pytest.raises(zkatdlog.ZKError) as e:
            v.verify(msg + b"x", sig)
        assert e.value.code == _abi.FTZ_ERR_SIGNATURE
    # the same identity bytes give the same index; the key comes back as the fixture's
    assert h.add_identity(ident) == fx["where"][ident][1]
    assert h.public_key(ident).hex() == g["keys"]["pub"]["xy"]
    # what does not deserialize cannot be registered, and says why
    for name, code in (("id_p384", _abi.FTZ_ERR_UNSUPPORTED), ("id_off_curve", _abi.FTZ_ERR_IDENTITY)):
        bad = next(c for c in fx["cases"] if c[0] == name)[1]
        with pytest.raises(zkatdlog.DeviceError):
            h.add_identity(bad)
        with pytest.raises(zkatdlog.ZKError) as e:
            h.public_key(bad)
        assert e.value.code == code
    # an index that was never handed out is an error of the call
    with pytest.raises(zkatdlog.DeviceError):
        h.verify_signatures([(KEYS_PER_HANDLE, msg, sig)])
    assert h.verify_signatures([]) == []
