#!/usr/bin/env python3
"""Write tests/golden/ecsign_golden.json: the fixture of tests/test_ecsign.py and
tests/test_ecsign_gpu.py.  Run once on a CPU and committed; tests never run it.

Every expected signature comes from tests/ecsign_ref.py (RFC 6979 nonce, low-S,
DER), which the two vectors of RFC 6979 A.2.5 pin; each is checked here with
p256_ref.verify under the key's PUBLIC KEY identity.

Layout: keys[name] = {d, xy, identity}; cases[] = {name, key, msg, entropy | null, sig} (hex)."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ecsign_ref as S  # noqa: E402
import p256_ref as R  # noqa: E402

rng = random.Random(20261020)
RFC_X = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721

keys = {"rfc": RFC_X, "one": 1, "n_minus_1": R.N - 1}
for i in range(3):
    keys["rand%d" % i] = rng.randrange(1, R.N)

cases = []


def case(name, key, msg, entropy=None):
    d = keys[key]
    sig = S.sign(d, msg, entropy)
    assert R.verify(S.identity_of(d), msg, sig) == R.OK, name
    cases.append({"name": name, "key": key, "msg": msg.hex(), "entropy": entropy.hex() if entropy else None,
                  "sig": sig.hex()})


def rbytes(n):
    return bytes(rng.randrange(256) for _ in range(n))


case("rfc_sample", "rfc", b"sample")
case("rfc_test", "rfc", b"test")
case("rfc_sample_entropy", "rfc", b"sample", rbytes(32))
for key in ("one", "n_minus_1"):
    case(key + "_short", key, b"endorse " + key.encode())
    case(key + "_entropy", key, rbytes(100), rbytes(32))
names = sorted(keys)
for j, ln in enumerate((0, 55, 56, 63, 64, 65, 9500)):
    msg = rbytes(ln)
    case("len%d" % ln, names[j % len(names)], msg)
    case("len%d_entropy" % ln, names[(j + 1) % len(names)], msg, rbytes(32))
    case("len%d_other_key" % ln, "rand%d" % (j % 3), msg)
for j in range(12):
    case("random%d" % j, "rand%d" % (j % 3), rbytes(rng.randrange(1, 300)), rbytes(32) if j % 2 else None)
# the same seed under two messages: the hedged nonce still differs
seed = rbytes(32)
case("seed_reuse_a", "rand0", b"message a", seed)
case("seed_reuse_b", "rand0", b"message b", seed)

out = {"keys": {}, "cases": cases}
for name, d in keys.items():
    x, y = S.public_key(d)
    out["keys"][name] = {"d": "%064x" % d, "xy": "%064x%064x" % (x, y), "identity": S.identity_of(d).hex()}
path = os.path.join(HERE, "golden", "ecsign_golden.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print("%d cases, %d keys -> %s" % (len(cases), len(keys), path))
