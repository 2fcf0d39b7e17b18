"""Writes tests/golden/canon_sign_vectors.json from the model tests/canon_sign_ref.py:  python tests/golden/gen_canon_sign.py
Deterministic (a seeded generator).  Per scheme: message lengths on every block / padding boundary of every hash the scheme
runs, the edge keys, and -- ECDSA -- planted digests at and above the order and 64 random signatures per curve with and
without LOW_S."""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import canon_msg_ref as R  # noqa: E402
import canon_sign_ref as S  # noqa: E402

rng = random.Random(0x5167)
SHA256_LENS = [0, 1, 55, 56, 63, 64, 119, 120]                      # bare, and behind whole-block prefixes (BIP-340)
SHA512_LENS = [0, 1, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112]      # behind a 32- and a 64-byte prefix


def msg(n):
    return bytes(rng.randrange(256) for _ in range(n))


def ecdsa(curve):
    C = R.WEIERSTRASS[curve]
    keys = [1, C.N - 1, 0, C.N, 2**256 - 1]
    mc, dc = [], []

    def add_msg(d, m):
        sig, st = S.ecdsa_sign_msg(C, d, m, 0)
        low, _ = S.ecdsa_sign_msg(C, d, m, S.LOW_S)
        pk, _ = S.public_key(R.CURVE_IDS[curve], (d % 2**256).to_bytes(32, "big"), 33)
        mc.append({"msg": m.hex(), "key": "%064x" % d, "sig": sig.hex(), "sig_low": low.hex(), "status": st, "pk": pk.hex()})

    for n in SHA256_LENS:
        add_msg(rng.randrange(1, C.N), msg(n))
    for d in keys:
        add_msg(d, msg(33))
    for _ in range(64):
        add_msg(rng.randrange(1, C.N), msg(rng.randrange(0, 130)))
    ok = [c for c in mc[-64:]]
    high = sum(c["sig"] != c["sig_low"] for c in ok)
    assert 0 < high < 64, high
    for h in [C.N, C.N + 1, 2**256 - 1, 0, C.N - 1] + [rng.randrange(2**256) for _ in range(8)]:
        for d in ([rng.randrange(1, C.N)] if h not in (0, C.N) else [rng.randrange(1, C.N), 0, 2**256 - 1]):
            h1 = h.to_bytes(32, "big")
            sig, st = S.ecdsa_sign_digest(C, d, h1, 0)
            low, _ = S.ecdsa_sign_digest(C, d, h1, S.LOW_S)
            dc.append({"digest": h1.hex(), "key": "%064x" % d, "sig": sig.hex(), "sig_low": low.hex(), "status": st,
                       "k": S.ecdsa_nonce(C, d, h1)[0].hex()})
    return {"msg_cases": mc, "digest_cases": dc}


def bip340():
    n = R.SECP.N
    out = []

    def add(d, m, aux):
        sig, st = S.bip340_sign(d, m, aux)
        pk, _ = S.public_key(S.SCHEME_BIP340, (d % 2**256).to_bytes(32, "big"), 32)
        out.append({"msg": m.hex(), "key": "%064x" % d, "aux": aux.hex(), "sig": sig.hex(), "status": st, "pk": pk.hex(),
                    "parity": list(S.bip340_parities(d, m, aux)) if st == 0 else [0, 0]})

    for ln in SHA256_LENS + [32]:
        add(rng.randrange(1, n), msg(ln), msg(32))
    for d in (1, n - 1, 0, n, 2**256 - 1):
        add(d, msg(32), bytes(32))
    for _ in range(24):
        add(rng.randrange(1, n), msg(rng.randrange(0, 100)), msg(32))
    assert {tuple(c["parity"]) for c in out if c["status"] == 0} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    return out


def ed25519():
    out = []
    for ln in SHA512_LENS + [rng.randrange(113, 300) for _ in range(8)]:
        seed, m = msg(32), msg(ln)
        sig, pk = S.ed25519_sign(seed, m)
        out.append({"msg": m.hex(), "key": seed.hex(), "sig": sig.hex(), "pk": pk.hex(), "status": 0})
    for seed in (bytes(32), b"\xff" * 32):
        sig, pk = S.ed25519_sign(seed, b"edge")
        out.append({"msg": b"edge".hex(), "key": seed.hex(), "sig": sig.hex(), "pk": pk.hex(), "status": 0})
    return out


if __name__ == "__main__":
    doc = {"ecdsa": {c: ecdsa(c) for c in ("secp256k1", "p256")}, "bip340": bip340(), "ed25519": ed25519(),
           "published": {k: {f: (x.hex() if isinstance(x, bytes) else x) for f, x in v.items()} for k, v in S.published().items()}}
    with open(os.path.join(HERE, "canon_sign_vectors.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(hashlib.sha256(open(os.path.join(HERE, "canon_sign_vectors.json"), "rb").read()).hexdigest())
