"""Writes tests/golden/canon_recover_vectors.json from the model tests/canon_recover_ref.py:
    python tests/golden/gen_canon_recover.py
Deterministic (a seeded generator).  A recovery case: curve, digest, sig (r || s), recid, status, a class and a name, and
"key33": the SEC 1 compressed encoding of the recovered key, from which the forms 65 and 64 follow by decoding it, and on
secp256k1 "address": the form 20; both absent where the status is 8 (every form is zeros then).
A signing case (class "sign") adds the key and the flags and is what fec_canon_ecdsa_sign_recoverable_digest must return.
Hex = the bytes in order.
Classes:
  sign      128 random sign-and-recover cases per curve, LOW_S on every other one
  recid     recid 4, 5, 255 on a good signature
  range     r or s = 0, n, n + 1; r = 2^256 - 1
  digest    z from the digest 0, the digest n (u1 = 0 both times) and all-ones
  infinity  R = k G, any s, z = s k mod n: Q = r^-1 (s R - z G) is the point at infinity
  doubling  z = -s k mod n: u1 G = u2 R, the valid key 2 u2 R
  bit1      the smallest t >= 1 with x = n + t on the curve, both parities (recids 2, 3); r = p - n - 1; r = p - n (x = p:
            refused, not reduced to 0); r = n - 1 with recid 2 (the sum passes 2^256); a random r with bit 1 set
  off-curve an x with no point above it
Keccak cases: "keccak_buffer" is one run of random bytes; a case is the message buffer[at : at + len] and its digest, for
every length of canon_recover_ref.KECCAK_LENGTHS at every start at = 0..7 (every byte alignment), and a few random ones.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import canon_msg_ref as R  # noqa: E402
import canon_recover_ref as K  # noqa: E402
import canon_sign_ref as S  # noqa: E402

rng = random.Random(0x416)
cases = []


def rand32():
    return bytes(rng.randrange(256) for _ in range(32))


def b32(v):
    return v.to_bytes(32, "big")


def add(cls, name, curve, digest, sig, recid, want_status=None, **extra):
    C = R.WEIERSTRASS[curve]
    key33, st = K.recover(C, digest, sig, recid, 33)
    assert want_status is None or st == want_status, (cls, name, st)
    c = {"class": cls, "name": name, "curve": curve, "digest": digest.hex(), "sig": sig.hex(), "recid": recid, "status": st}
    if st == 0:
        c["key33"] = key33.hex()
        if curve == "secp256k1":
            c["address"] = K.recover(C, digest, sig, recid, 20)[0].hex()
    c.update(extra)
    cases.append(c)
    return c


def signed(C):
    d, h1 = rng.randrange(1, C.N), rand32()
    sig, recid, st = K.sign_recoverable_digest(C, d, h1, S.LOW_S)
    assert st == 0
    return d, h1, sig, recid


for curve, C in sorted(R.WEIERSTRASS.items()):
    n, p = C.N, C.P
    for i in range(128):
        d, h1, flags = rng.randrange(1, n), rand32(), (i & 1) * S.LOW_S
        sig, recid, st = K.sign_recoverable_digest(C, d, h1, flags)
        c = add("sign", "random %d" % i, curve, h1, sig, recid, 0, key=b32(d).hex(), flags=flags)
        assert c["key33"] == R.sec1_encode(C.mul(d, C.G)).hex()

    d, h1, sig, recid = signed(C)
    for bad in (4, 5, 255):
        add("recid", "recid %d" % bad, curve, h1, sig, bad, 8)

    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    for v, what in ((0, "0"), (n, "n"), (n + 1, "n + 1")):
        add("range", "r = %s" % what, curve, h1, b32(v) + sig[32:], recid, 8)
        add("range", "s = %s" % what, curve, h1, sig[:32] + b32(v), recid, 8)
    add("range", "r = 2^256 - 1", curve, h1, b32(2**256 - 1) + sig[32:], recid, 8)
    add("range", "s = 2^256 - 1", curve, h1, sig[:32] + b32(2**256 - 1), recid, 8)

    for dg, what in ((bytes(32), "0"), (b32(n), "n"), (b"\xff" * 32, "all-ones")):
        for rid in (0, 1):
            c = add("digest", "digest %s, recid %d" % (what, rid), curve, dg, sig, rid, 0)
            assert K.verify_digest(C, dg, sig, R.sec1_decode(C, bytes.fromhex(c["key33"])))

    for i in range(2):
        k, s2 = rng.randrange(1, n), rng.randrange(1, n)
        Rp = C.mul(k, C.G)
        assert Rp[0] < n
        sg = b32(Rp[0]) + b32(s2)
        add("infinity", "z = s k, case %d" % i, curve, b32(s2 * k % n), sg, Rp[1] & 1, 8)
        c = add("doubling", "z = -s k, case %d" % i, curve, b32(-s2 * k % n), sg, Rp[1] & 1, 0)
        assert c["key33"] == R.sec1_encode(C.mul(2 * s2 * k * pow(Rp[0], -1, n) % n, C.G)).hex()

    t = 1
    while R.sqrt_mod(C, ((n + t) ** 3 + C.A * (n + t) + C.B) % p) is None:
        t += 1
    assert n + t < p
    for rid in (2, 3):
        c = add("bit1", "x = n + %d, recid %d" % (t, rid), curve, h1, b32(t) + sig[32:], rid, 0)
        assert K.verify_digest(C, h1, b32(t) + sig[32:], R.sec1_decode(C, bytes.fromhex(c["key33"])))
    for rid in (2, 3):
        add("bit1", "r = p - n - 1, recid %d" % rid, curve, h1, b32(p - n - 1) + sig[32:], rid)
        add("bit1", "r = p - n (x = p), recid %d" % rid, curve, h1, b32(p - n) + sig[32:], rid, 8)
    add("bit1", "r = n - 1, recid 2 (the sum passes 2^256)", curve, h1, b32(n - 1) + sig[32:], 2, 8)
    add("bit1", "r = n - 1, recid 0", curve, h1, b32(n - 1) + sig[32:], 0)
    add("bit1", "a random r with bit 1 set", curve, h1, sig, recid | 2, 8)

    x = rng.randrange(1, n)
    while R.sqrt_mod(C, (x ** 3 + C.A * x + C.B) % p) is not None:
        x = rng.randrange(1, n)
    for rid in (0, 1):
        add("off-curve", "x with no point, recid %d" % rid, curve, h1, b32(x) + sig[32:], rid, 8)

keccak = []
buffer = bytes(rng.randrange(256) for _ in range(max(K.KECCAK_LENGTHS) + 8))
extra = [rng.randrange(2, 700) for _ in range(4)]
for j, length in enumerate(K.KECCAK_LENGTHS + extra):
    for at in range(8) if length in K.KECCAK_LENGTHS else (j & 7,):
        keccak.append({"len": length, "at": at, "digest": K.keccak256(buffer[at:at + length]).hex()})

doc = {
    "comment": "SEC 1 4.1.6 recovery and Keccak-256 by tests/canon_recover_ref.py (tests/golden/gen_canon_recover.py); hex = the bytes in order",
    "cases": cases,
    "keccak": keccak,
    "keccak_buffer": buffer.hex(),
}
with open(os.path.join(HERE, "canon_recover_vectors.json"), "w") as f:
    json.dump(doc, f, indent=0, sort_keys=True)
    f.write("\n")
print("%d recovery cases, %d keccak cases" % (len(cases), len(keccak)))
