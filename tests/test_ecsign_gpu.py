"""GPU tier of batched ECDSA P-256 signing (zkatdlog.Ecdsa.add_signer / sign ->
ftz_sign_ecdsa -> k_ecsign_pre / _part / _fin): byte-exact against
tests/ecsign_ref.py on every case of tests/golden/ecsign_golden.json and across
wave and chunk boundaries, verified again by the same handle on both routes,
and from two threads.

The Python reference costs about 11 ms per signature, so one pool of 80
reference signatures is computed once and larger batches tile it: the
deterministic path (and the hedged one, for a given seed) repeats exactly."""
import json
import os
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_SIGS = 4096  # host/sigpipe.h SIG_CHUNK_ITEMS
RFC_X = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
RFC_U = ("60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6"
         "7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299")
FTZ_ERR_SIGNATURE = 10
POOL = 80


@pytest.fixture(scope="module")
def fx():
    """the fixture; two handles with three of its six signers each; on the first one the signers'
    identities are registered too, and a pool of reference signatures under its signers is made"""
    import zkatdlog
    import ecsign_ref as S
    with open(os.path.join(ROOT, "tests", "golden", "ecsign_golden.json")) as f:
        g = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")) as f:
        pp = json.load(f)["pp_a"]["pp"].encode()
    ctx = zkatdlog.Context(pp, device=0)
    names = sorted(g["keys"])
    assert len(names) == 6
    handles, where, returned = [zkatdlog.Ecdsa(ctx), zkatdlog.Ecdsa(ctx)], {}, {}  # where: name -> (handle, signer)
    for i, name in enumerate(names):
        idx, xy = handles[i // 3].add_signer(bytes.fromhex(g["keys"][name]["d"]))
        assert xy.hex() == g["keys"][name]["xy"], name
        where[name] = (i // 3, idx)
        returned[name] = xy
    h = handles[0]
    ds = [int(g["keys"][n]["d"], 16) for n in names[:3]]
    idents = [S.identity_of(d) for d in ds]
    # the registered identities are built from the public_xy that add_signer returned
    reg = []
    for name in names[:3]:
        xy = returned[name]
        ident = S.R.serialized_identity(S.R.pem_encode(
            "PUBLIC KEY", S.R.spki_der(int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:], "big"))))
        reg.append(h.add_identity(ident))
    rng = random.Random(21)
    lens = [0, 1, 55, 56, 63, 64, 65, 119, 120, 200, 1000, 31]
    pool = []  # (signer, msg, entropy, expected DER)
    for i in range(POOL):
        signer = (i * 7 + i // 5) % 3
        msg = b"%d:" % i + bytes(rng.randrange(256) for _ in range(lens[i % len(lens)]))
        if i == 5:
            msg = b""
        ent = bytes(rng.randrange(256) for _ in range(32)) if i % 3 == 1 else None
        pool.append((signer, msg, ent, S.sign(ds[signer], msg, ent)))
    assert len({p[1] for p in pool}) == POOL
    yield {"g": g, "handles": handles, "where": where, "names": names, "pool": pool, "idents": idents, "reg": reg,
           "S": S}
    for x in handles:
        x.close()
    ctx.close()


def test_every_fixture_case_byte_exact(fx):
    g = fx["g"]
    seen = set()
    for hi, h in enumerate(fx["handles"]):
        cases = [c for c in g["cases"] if fx["where"][c["key"]][0] == hi]
        items = [(fx["where"][c["key"]][1], bytes.fromhex(c["msg"]),
                  bytes.fromhex(c["entropy"]) if c["entropy"] else None) for c in cases]
        assert len({it[0] for it in items}) == 3
        got = h.sign(items)
        assert {c["name"]: s.hex() for c, s in zip(cases, got)} == {c["name"]: c["sig"] for c in cases}
        seen |= {c["name"] for c in cases}
    assert len(seen) == len(g["cases"]) >= 40


@pytest.mark.parametrize("size", [1, 63, 64, 65, CHUNK_SIGS + 1, 2 * CHUNK_SIGS + 1])
def test_batches_sign_then_verify(fx, size):
    """signers, message lengths and entropy / no entropy mixed inside the first wave; every position
    byte-equal to the reference; the same handle accepts every signature by registered key and ad hoc,
    and refuses each one over its neighbour's message.  The last size is three chunks: the third goes
    into the slot the first one used"""
    h, pool = fx["handles"][0], fx["pool"]
    for start in ((0, 23) if size < 1000 else (3,)):
        pick = [pool[(start + i) % POOL] for i in range(size)]
        if size >= 64:
            first = pick[:64]
            assert len({p[0] for p in first}) == 3 and len({len(p[1]) for p in first}) > 8
            assert any(p[2] for p in first) and any(p[2] is None for p in first)
        got = h.sign([p[:3] for p in pick])
        assert got == [p[3] for p in pick], [i for i in range(size) if got[i] != pick[i][3]][:10]
        by_key = h.verify_signatures([(fx["reg"][p[0]], p[1], s) for p, s in zip(pick, got)])
        assert by_key == [0] * size
        ad_hoc = h.verify_signatures([(fx["idents"][p[0]], p[1], s) for p, s in zip(pick, got)])
        assert ad_hoc == [0] * size
        other = [pool[(start + i + 1) % POOL][1] for i in range(size)]
        wrong = h.verify_signatures([(fx["reg"][p[0]], m, s) for p, m, s in zip(pick, other, got)])
        assert wrong == [FTZ_ERR_SIGNATURE] * size


def test_two_signers_over_one_shared_message(fx):
    h, S, g = fx["handles"][0], fx["S"], fx["g"]
    msg = b"one request, endorsed twice" * 9
    a, b = h.sign([(0, msg), (1, msg)])  # the same object: stored once in the blob
    ds = [int(g["keys"][n]["d"], 16) for n in fx["names"][:2]]
    assert a != b and [a, b] == [S.sign(ds[0], msg), S.sign(ds[1], msg)]
    assert h.verify_signatures([(fx["reg"][0], msg, a), (fx["reg"][1], msg, b), (fx["reg"][0], msg, b)]) == \
        [0, 0, FTZ_ERR_SIGNATURE]
    # the Signer / Verifier pair of one identity
    signer, verifier = h.signer(1), h.verifier(fx["reg"][1])
    assert signer.sign(msg) == b
    verifier.verify(msg, signer.sign(msg, entropy=bytes(range(32))))


def test_one_thread_signs_while_one_verifies(fx):
    h, pool = fx["handles"][0], fx["pool"]
    sign_items = [p[:3] for p in pool] * 2
    verify_items = [(fx["reg"][p[0]], pool[(i + i % 2) % POOL][1], p[3]) for i, p in enumerate(pool)] * 2
    serial = [h.sign(sign_items), h.verify_signatures(verify_items)]
    assert serial[0] == [p[3] for p in pool] * 2
    assert serial[1] == [0 if i % 2 == 0 else FTZ_ERR_SIGNATURE for i in range(POOL)] * 2
    out = [None, None]

    def run(t):
        for _ in range(3):
            out[t] = h.sign(sign_items) if t == 0 else h.verify_signatures(verify_items)

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert out == serial


def test_errors_and_registration(fx):
    import zkatdlog
    import p256_ref as R
    ctx = fx["handles"][0].ctx
    h = zkatdlog.Ecdsa(ctx)
    try:
        assert h.sign([]) == []
        for d in (0, R.N, R.N + 5, 2**256 - 1):
            with pytest.raises(zkatdlog.DeviceError):
                h.add_signer(d.to_bytes(32, "big"))
        with pytest.raises(zkatdlog.DeviceError):  # no signer yet: index 0 is unknown
            h.sign([(0, b"m")])
        idx, xy = h.add_signer(RFC_X.to_bytes(32, "big"))
        assert idx == 0 and xy.hex().upper() == RFC_U
        for k in range(1, 8):
            assert h.add_signer((RFC_X + k).to_bytes(32, "big"))[0] == k
        with pytest.raises(zkatdlog.DeviceError):  # the ninth
            h.add_signer((RFC_X + 8).to_bytes(32, "big"))
        for bad in (8, -1):
            with pytest.raises(zkatdlog.DeviceError):
                h.sign([(0, b"m"), (bad, b"m")])
        # RFC 6979 A.2.5 "sample" (s flipped low) and "test" straight from the device
        sample, test = h.sign([(0, b"sample"), (0, b"test")])
        assert R.parse_signature(sample) == (
            0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716,
            R.N - 0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8)
        assert R.parse_signature(test) == (
            0xF1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367,
            0x019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083)
    finally:
        h.close()
