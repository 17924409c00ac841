"""GPU tier of batched idemix pseudonym signing on BN254 (zkatdlog.Idemix.add_signer /
sign_owner_signatures / make_nyms -> ftz_sign_owner_signatures / ftz_idemix_make_nyms ->
k_nymsign_pre / _part / _fin, k_nym_make_pre / _fin): byte-exact against
tests/nymsign_ref.py on every case of tests/golden/nymsign_golden.json and across
wave and chunk boundaries, verified again by the same handle, and from threads.

One reference signature (tests/nymsign_ref.py: two oracle scalar multiplications
and the Python DRBG) costs about 8 ms and a pseudonym about 7 ms, so one pool of
64 reference signatures over 6 pseudonyms is computed once (under a second) and
larger batches tile it: the deterministic path (and the hedged one, for a given
seed) repeats exactly."""
import ctypes
import json
import os
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_SIGS = 4096  # host/sigpipe.h SIG_CHUNK_ITEMS
FTZ_ERR_OWNER, FTZ_ERR_SIGNATURE = 9, 10
POOL = 64


def b32(v):
    return v.to_bytes(32, "big")


@pytest.fixture(scope="module")
def fx():
    """the fixture; one BN254 handle with the fixture's five user secrets registered; a pool of
    reference signatures under three of them"""
    import zkatdlog
    from zkatdlog import _abi
    import nymsign_ref as S
    with open(os.path.join(ROOT, "tests", "golden", "nymsign_golden.json")) as f:
        g = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "idemix_bn254_golden.json")) as f:
        ipk_raw = bytes.fromhex(json.load(f)["ipk"])
    with open(os.path.join(ROOT, "tests", "golden", "zkatdlog_golden.json")) as f:
        pp = json.load(f)["pp_a"]["pp"].encode()
    ipk = S.I.IssuerPKBn254(ipk_raw)
    ctx = zkatdlog.Context(pp, device=0)
    ix = zkatdlog.Idemix(ctx, ipk_raw, curve_id=_abi.FTZ_CURVE_BN254)
    names = sorted(g["keys"])
    where = {name: ix.add_signer(bytes.fromhex(g["keys"][name]["sk"])) for name in names}
    assert sorted(where.values()) == list(range(5))
    rng = random.Random(41)
    # six pseudonyms: two under each of three signers
    pseud = []  # (signer index, sk, r_nym, nym point, nym bytes, owner bytes)
    for name in ("a", "max", "c"):
        sk = int(g["keys"][name]["sk"], 16)
        for _ in range(2):
            rn = rng.randrange(S.R)
            nym = S.make_nym(ipk, sk, rn)
            pseud.append((where[name], sk, rn, nym, S.nym_bytes(nym), S.owner_of(nym)))
    lens = [0, 1, 17, 18, 25, 26, 27, 28, 29, 81, 82, 200, 1000, 63, 64, 65]
    pool = []  # (signer, r_nym bytes, nym bytes, msg, entropy, expected signature, owner)
    for i in range(POOL):
        signer, sk, rn, nym, nb, own = pseud[(i * 5 + i // 7) % 6]
        msg = b"%d:" % i + bytes(rng.randrange(256) for _ in range(lens[i % len(lens)]))
        if i == 5:
            msg = b""
        ent = bytes(rng.randrange(256) for _ in range(32)) if i % 3 == 1 else None
        pool.append((signer, b32(rn), nb, msg, ent, S.sign(ipk, sk, rn, nym, msg, ent), own))
    assert len({p[3] for p in pool}) == POOL
    yield {"g": g, "ix": ix, "ctx": ctx, "where": where, "pool": pool, "pseud": pseud, "S": S, "ipk": ipk,
           "ipk_raw": ipk_raw}
    ix.close()
    ctx.close()


def case_msg(S, c):
    return bytes.fromhex(c["msg"]) if "msg" in c else S.expand(bytes.fromhex(c["msg_seed"]), c["msg_len"])


def test_every_fixture_case_byte_exact(fx):
    g, S, ix = fx["g"], fx["S"], fx["ix"]
    cases = g["cases"]
    items = [(fx["where"][c["key"]], bytes.fromhex(c["r_nym"]), bytes.fromhex(c["nym"]), case_msg(S, c),
              bytes.fromhex(c["entropy"]) if c["entropy"] else None) for c in cases]
    assert len(cases) >= 40 and any(it[4] for it in items) and any(it[4] is None for it in items)
    sigs, codes = ix.sign_owner_signatures(items)
    assert codes == [0] * len(cases)
    assert {c["name"]: s.hex() for c, s in zip(cases, sigs)} == {c["name"]: c["sig"] for c in cases}
    owners = [S.owner_of(S.C.g1_from_bytes(it[2])) for it in items]
    assert ix.verify_owner_signatures([(o, it[3], s) for o, it, s in zip(owners, items, sigs)]) == [0] * len(cases)


@pytest.mark.parametrize("size", [1, 63, 64, 65, CHUNK_SIGS + 1, 2 * CHUNK_SIGS + 1])
def test_batches_sign_then_verify(fx, size):
    """signers, pseudonyms, message lengths and entropy / no entropy mixed inside the first wave; every
    position byte-equal to the reference; the same handle accepts every signature, and refuses one
    over a message with one flipped byte.  The last size is three chunks: the third goes into the
    slot the first one used"""
    ix, pool = fx["ix"], fx["pool"]
    for start in ((0, 23) if size < 1000 else (3,)):
        pick = [pool[(start + i) % POOL] for i in range(size)]
        if size >= 64:
            first = pick[:64]
            assert len({p[0] for p in first}) == 3 and len({p[2] for p in first}) == 6
            assert len({len(p[3]) for p in first}) > 8
            assert any(p[4] for p in first) and any(p[4] is None for p in first)
        sigs, codes = ix.sign_owner_signatures([p[:5] for p in pick])
        assert codes == [0] * size
        assert sigs == [p[5] for p in pick], [i for i in range(size) if sigs[i] != pick[i][5]][:10]
        assert ix.verify_owner_signatures([(p[6], p[3], s) for p, s in zip(pick, sigs)]) == [0] * size
        k = size // 2
        flipped = bytearray(pick[k][3] or b"\x00")
        flipped[-1] ^= 0x10
        assert ix.verify_owner_signatures([(pick[k][6], bytes(flipped), sigs[k])]) == [FTZ_ERR_SIGNATURE]


def test_make_nyms_against_the_oracle_and_sign_with_one(fx):
    """65 pseudonyms in one call; the RNym values carry explicit zero digits into the device's uniform
    walk (0, 1, r - 1, one non-zero byte in each of the 32 positions)"""
    ix, S, ipk, g = fx["ix"], fx["S"], fx["ipk"], fx["g"]
    rng = random.Random(42)
    rns = [0, 1, S.R - 1] + [0xa7 << (8 * j) for j in range(31)] + [0x2f << 248]
    rns += [rng.randrange(S.R) for _ in range(65 - len(rns))]
    assert len(rns) == 65 and all(r < S.R for r in rns)
    name = "b"
    sk = int(g["keys"][name]["sk"], 16)
    got = ix.make_nyms(fx["where"][name], [b32(r) for r in rns])
    base = S.C.g1_mul(ipk.hsk, sk)
    want = [S.C.g1_bytes(S.C.g1_add(base, S.C.g1_mul(ipk.hrand, r) if r else None)) for r in rns]
    assert want[7] == S.nym_bytes(S.make_nym(ipk, sk, rns[7]))
    assert got == want, [i for i in range(65) if got[i] != want[i]][:10]
    assert ix.make_nyms(fx["where"][name], []) == []
    # sk = r - 1 and sk = 1 go through the walk with their own zero and 0xff digits
    for nm in ("max", "one"):
        k = int(g["keys"][nm]["sk"], 16)
        assert ix.make_nyms(fx["where"][nm], [b32(5)]) == [S.nym_bytes(S.make_nym(ipk, k, 5))]
    # a signature made with a returned nym verifies
    msg = b"signed under a derived pseudonym"
    signer = ix.owner_signer(fx["where"][name], b32(rns[40]), got[40])
    sig = signer.sign(msg)
    assert sig == S.sign(ipk, sk, rns[40], S.C.g1_from_bytes(got[40]), msg)
    ix.owner_verifier(S.owner_of(S.C.g1_from_bytes(got[40]))).verify(msg, sig)
    # a nym of another RNym gives a well-formed signature that does not verify
    sigs, codes = ix.sign_owner_signatures([(fx["where"][name], b32(rns[40]), got[41], msg)])
    assert codes == [0]
    assert ix.verify_owner_signatures([(S.owner_of(S.C.g1_from_bytes(got[41])), msg, sigs[0])]) == [FTZ_ERR_SIGNATURE]


def test_two_entropies_give_two_signatures(fx):
    ix, S, ipk = fx["ix"], fx["S"], fx["ipk"]
    signer, sk, rn, nym, nb, own = fx["pseud"][0]
    msg = b"one request, signed twice" * 7
    e1, e2 = bytes(range(32)), bytes(range(1, 33))
    sigs, codes = ix.sign_owner_signatures([(signer, b32(rn), nb, msg, e1), (signer, b32(rn), nb, msg, e2),
                                            (signer, b32(rn), nb, msg)])
    assert codes == [0, 0, 0] and len(set(sigs)) == 3
    assert sigs == [S.sign(ipk, sk, rn, nym, msg, e) for e in (e1, e2, None)]
    assert ix.verify_owner_signatures([(own, msg, s) for s in sigs]) == [0, 0, 0]


def test_refused_nyms_leave_their_neighbours_alone(fx):
    ix, S, pool = fx["ix"], fx["S"], fx["pool"]
    pick = [pool[i] for i in range(8)]
    items = [list(p[:5]) for p in pick]
    x, y = int.from_bytes(pick[1][2][:32], "big"), int.from_bytes(pick[1][2][32:], "big")
    items[1][2] = b32(x) + b32(y ^ 1)         # off the curve
    items[3][2] = b32(x + S.P) + b32(y)       # on the curve once reduced, but not canonical
    items[6][2] = bytes(64)                   # (0, 0): gnark's infinity
    sigs, codes = ix.sign_owner_signatures([tuple(it) for it in items])
    bad = {1, 3, 6}
    assert codes == [FTZ_ERR_OWNER if i in bad else 0 for i in range(8)]
    for i in range(8):
        assert sigs[i] == (bytes(136) if i in bad else pick[i][5]), i
    with pytest.raises(__import__("zkatdlog").ZKError):
        ix.owner_signer(items[6][0], items[6][1], items[6][2]).sign(b"m")


def test_whole_call_errors(fx):
    import zkatdlog
    from zkatdlog import _abi
    S, g = fx["S"], fx["g"]
    ix = zkatdlog.Idemix(fx["ctx"], fx["ipk_raw"], curve_id=_abi.FTZ_CURVE_BN254)
    p = fx["pool"][0]
    good = (0, p[1], p[2], b"m")
    try:
        assert ix.sign_owner_signatures([]) == ([], [])
        for sk in (0, S.R, S.R + 5, 2**256 - 1):
            with pytest.raises(zkatdlog.DeviceError):
                ix.add_signer(b32(sk))
        with pytest.raises(zkatdlog.DeviceError):  # no signer yet: index 0 is unknown
            ix.sign_owner_signatures([(0, p[1], p[2], b"m")])
        with pytest.raises(zkatdlog.DeviceError):
            ix.make_nyms(0, [b32(1)])
        sk = int(g["keys"]["a"]["sk"], 16)
        for k in range(8):
            assert ix.add_signer(b32(sk if k == 0 else 1 + k)) == k
        with pytest.raises(zkatdlog.DeviceError, match="too many signers"):  # the ninth
            ix.add_signer(b32(77))
        for bad in (8, -1):
            with pytest.raises(zkatdlog.DeviceError):
                ix.sign_owner_signatures([good, (bad, p[1], p[2], b"m")])
            with pytest.raises(zkatdlog.DeviceError):
                ix.make_nyms(bad, [b32(1)])
        for rn in (S.R, 2**256 - 1):
            with pytest.raises(zkatdlog.DeviceError):
                ix.sign_owner_signatures([good, (0, b32(rn), p[2], b"m")])
            with pytest.raises(zkatdlog.DeviceError):
                ix.make_nyms(0, [b32(1), b32(rn)])
        # a null buffer with a non-zero length and a message over 512 MiB: refused before anything is read
        arr, keep = _abi.pack_nym_sign_items([good, good])
        sigs, codes = ctypes.create_string_buffer(2 * 136), (ctypes.c_int32 * 2)()
        arr[1].msg, arr[1].msg_len = None, 5
        assert ix._lib.ftz_sign_owner_signatures(ix._h, 2, arr, sigs, codes) < 0
        arr, keep = _abi.pack_nym_sign_items([good, good])
        arr[1].msg_len = (512 << 20) + 1
        assert ix._lib.ftz_sign_owner_signatures(ix._h, 2, arr, sigs, codes) < 0
        assert b"512 MiB" in ix._lib.ftz_last_error()
        arr, keep = _abi.pack_nym_sign_items([good, good])
        arr[0].nym = None
        assert ix._lib.ftz_sign_owner_signatures(ix._h, 2, arr, sigs, codes) < 0
        # after all that the handle still signs
        assert ix.sign_owner_signatures([p[:5]]) == ([p[5]], [0])
    finally:
        ix.close()
    # an FP256BN handle refuses all three calls and says why
    with open(os.path.join(ROOT, "tests", "golden", "idemix_golden.json")) as f:
        fp_ipk = bytes.fromhex(json.load(f)["ipk"])
    fpx = zkatdlog.Idemix(fx["ctx"], fp_ipk)
    try:
        for call in (lambda: fpx.add_signer(b32(5)), lambda: fpx.sign_owner_signatures([good]),
                     lambda: fpx.make_nyms(0, [b32(1)])):
            with pytest.raises(zkatdlog.DeviceError, match="BN254 only"):
                call()
    finally:
        fpx.close()


def test_two_threads_sign_while_one_verifies(fx):
    ix, pool = fx["ix"], fx["pool"]
    sign_items = [p[:5] for p in pool] * 2
    verify_items = [(p[6], pool[(i + i % 2) % POOL][3], p[5]) for i, p in enumerate(pool)] * 2
    serial = [ix.sign_owner_signatures(sign_items), ix.verify_owner_signatures(verify_items)]
    assert serial[0] == ([p[5] for p in pool] * 2, [0] * (2 * POOL))
    assert serial[1] == [0 if i % 2 == 0 else FTZ_ERR_SIGNATURE for i in range(POOL)] * 2
    out = [None, None, None]

    def run(t):
        for _ in range(3):
            out[t] = ix.sign_owner_signatures(sign_items) if t < 2 else ix.verify_owner_signatures(verify_items)

    th = [threading.Thread(target=run, args=(t,)) for t in range(3)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert out == [serial[0], serial[0], serial[1]]
