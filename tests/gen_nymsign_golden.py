#!/usr/bin/env python3
"""Fixture maker for batched idemix pseudonym signing on BN254
(tests/golden/nymsign_golden.json), from tests/nymsign_ref.py.

The issuer key is the `ipk` of tests/golden/idemix_bn254_golden.json (the
reference's tokengen issuer).  Every case records the derived r_sk, r_rnym and
nonce beside the 136 signature bytes, so a mismatch can be located.  Messages
over 200 bytes are stored as (msg_seed, msg_len) and expanded by the SHA-256
counter stream of the idemix fixtures' bench entries (nymsign_ref.expand).

    python tests/gen_nymsign_golden.py
"""
import json
import os
import random

import nymsign_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
# the transcript is 166 + len bytes and job_nym_fin / job_nymsign_fin split the message at 28:
# 17 / 18 and 81 / 82 straddle the room for SHA-256's padding in the 3rd and 4th block, 25 / 26 the
# end of the 3rd block, 27 / 28 / 29 the split
LENGTHS = [0, 17, 18, 25, 26, 27, 28, 29, 81, 82, 9500]


def h64(v):
    return "%064x" % v


def main():
    with open(os.path.join(HERE, "golden", "idemix_bn254_golden.json")) as f:
        ipk = S.I.IssuerPKBn254(bytes.fromhex(json.load(f)["ipk"]))
    rng = random.Random(0x4E594D)
    keys = {"one": 1, "max": S.R - 1, "a": rng.randrange(1, S.R), "b": rng.randrange(1, S.R),
            "c": rng.randrange(1, S.R)}
    cases = []

    def add(name, key, r_nym, msg, entropy=None, seed=None):
        sk = keys[key]
        nym = S.make_nym(ipk, sk, r_nym)
        r_sk, r_rnym, nonce = S.randomness(sk, r_nym, msg, entropy)
        c = {"name": name, "key": key, "r_nym": h64(r_nym), "nym": S.nym_bytes(nym).hex(),
             "entropy": entropy.hex() if entropy else "", "r_sk": h64(r_sk), "r_rnym": h64(r_rnym),
             "nonce": h64(nonce), "sig": S.sign(ipk, sk, r_nym, nym, msg, entropy).hex()}
        if seed is None:
            assert len(msg) <= 200
            c["msg"] = msg.hex()
        else:
            assert msg == S.expand(seed, len(msg))
            c["msg_seed"], c["msg_len"] = seed.hex(), len(msg)
        cases.append(c)

    def rb(n):
        return bytes(rng.randrange(256) for _ in range(n))

    def message(L, tag):
        if L <= 200:
            return rb(L), None
        seed = b"nymsign-" + tag
        return S.expand(seed, L), seed

    # every length, deterministic and hedged, keys and RNym values rotating
    names = list(keys)
    for i, L in enumerate(LENGTHS):
        msg, seed = message(L, b"len%d" % L)
        add("len_%d" % L, names[i % 5], rng.randrange(S.R), msg, None, seed)
        add("len_%d_hedged" % L, names[(i + 2) % 5], rng.randrange(S.R), msg, rb(32), seed)
    # the edge RNym values under the edge keys and a random one
    for key in ("one", "max", "a"):
        for nm, rn in (("zero", 0), ("one", 1), ("max", S.R - 1)):
            add("key_%s_rnym_%s" % (key, nm), key, rn, rb(40 + len(cases)))
    for key in ("one", "max", "c"):
        add("key_%s_rnym_random" % key, key, rng.randrange(S.R), rb(40 + len(cases)), rb(32))
    # one entropy value under two messages, and one message under two entropies
    ent = rb(32)
    rn = rng.randrange(S.R)
    add("seed_reuse_a", "b", rn, b"first message", ent)
    add("seed_reuse_b", "b", rn, b"second message", ent)
    add("same_message_other_seed", "b", rn, b"first message", rb(32))
    add("same_message_no_seed", "b", rn, b"first message")
    # two owners of one two-input transfer sign the same request
    msg, seed = message(9500, b"shared")
    add("shared_request_owner_0", "a", rng.randrange(S.R), msg, None, seed)
    add("shared_request_owner_1", "c", rng.randrange(S.R), msg, None, seed)
    out = {"comment": "batched idemix pseudonym signing on BN254 (dev/nymsign.h): NewNymSignature with r_sk, "
                      "r_rnym and nonce from the HMAC-SHA-256 DRBG; made by tests/gen_nymsign_golden.py from "
                      "tests/nymsign_ref.py; issuer key: the ipk of idemix_bn254_golden.json",
           "keys": {k: {"sk": h64(v)} for k, v in keys.items()}, "cases": cases}
    path = os.path.join(HERE, "golden", "nymsign_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
