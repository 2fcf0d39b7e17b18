"""Writes tests/golden/canon_x25519_vectors.json from the model tests/canon_x25519_ref.py:
    python tests/golden/gen_canon_x25519.py
Deterministic (a seeded generator).  Every case: k, u, out as 64 hex digits (the 32 bytes in order), status, a class and a
name; the RFC's published cases carry "published": true and are compared with the RFC's own digits here.
Classes:
  low-order      u = 0, 1, the two of order 8, p - 1, p, p + 1, each with and without bit 255 where it fits in 256 bits:
                 zeros and status 7
  non-canonical  every u in [2^255 - 19, 2^255 - 1]
  bit255         u = 9 with bit 255 set (the bit is ignored)
  clamp          scalars whose clamping changes every clamped bit, all-zero, all-ones, a single set bit in each word
  published      RFC 7748 section 5.2 (both vectors, the first iteration) and section 6.1 (both keys, both directions)
  random         256 pairs
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import canon_x25519_ref as X  # noqa: E402

rng = random.Random(0x7748)
cases = []


def rand32():
    return bytes(rng.randrange(256) for _ in range(32))


def add(cls, name, k, u, published=False):
    out, st = X.x25519_status(k, u)
    c = {"class": cls, "name": name, "k": k.hex(), "u": u.hex(), "out": out.hex(), "status": st}
    if published:
        c["published"] = True
    cases.append(c)
    return c


for v in X.LOW_ORDER:
    for top in (0, 1):
        w = v | top << 255
        if w >> 256:
            continue
        c = add("low-order", "u = %d%s" % (v, " with bit 255" if top else ""), rand32(), w.to_bytes(32, "little"))
        assert c["status"] == X.ZERO_SHARED and c["out"] == "00" * 32, c
assert sum(c["class"] == "low-order" for c in cases) == 14

for v in range((1 << 255) - 19, 1 << 255):
    c = add("non-canonical", "u = 2^255 - %d" % ((1 << 255) - v), rand32(), v.to_bytes(32, "little"))
    assert (c["status"] == X.ZERO_SHARED) == (v - X.P in (0, 1))
k = rand32()
c = add("bit255", "u = 9 with bit 255", k, (9 | 1 << 255).to_bytes(32, "little"))
assert c["out"] == X.x25519_base(k).hex()

u = rand32()
every = bytearray(32)              # every bit the clamp clears is set, the one it sets is clear
every[0], every[31] = 0x07, 0x80
add("clamp", "the clamp changes every clamped bit", bytes(every), u)
inv = bytearray(b"\xff" * 32)      # ... and the scalar the clamp leaves alone in those bits
inv[0], inv[31] = 0xF8, 0x7F
add("clamp", "already clamped, all other bits set", bytes(inv), u)
add("clamp", "all-zero scalar", bytes(32), u)
add("clamp", "all-ones scalar", b"\xff" * 32, u)
for w in range(8):
    bit = 32 * w + (3 if w == 0 else 30 if w == 7 else rng.randrange(32))
    add("clamp", "single bit %d (word %d)" % (bit, w), (1 << bit).to_bytes(32, "little"), u)
    add("clamp", "single bit %d (word %d), base point" % (bit, w), (1 << bit).to_bytes(32, "little"), X.BASE_U)

for name, v in X.PUBLISHED.items():
    c = add("published", name, bytes.fromhex(v["k"]), bytes.fromhex(v["u"]), True)
    assert c["out"] == v["out"], name
c = add("published", "rfc7748_5_2_iterated_1", X.BASE_U, X.BASE_U, True)
assert c["out"] == X.ITERATED_1
d = X.DH
for name, k, u, want in (("rfc7748_6_1_alice_public", d["a"], X.BASE_U.hex(), d["A"]), ("rfc7748_6_1_bob_public", d["b"], X.BASE_U.hex(), d["B"]),
                         ("rfc7748_6_1_alice_shared", d["a"], d["B"], d["shared"]), ("rfc7748_6_1_bob_shared", d["b"], d["A"], d["shared"])):
    c = add("published", name, bytes.fromhex(k), bytes.fromhex(u), True)
    assert c["out"] == want, name

for i in range(256):
    c = add("random", "random %d" % i, rand32(), rand32())
    assert c["status"] == 0

doc = {
    "comment": "RFC 7748 section 5 X25519 by tests/canon_x25519_ref.py (tests/golden/gen_canon_x25519.py); hex = the 32 bytes in order",
    "iterated_1000": X.iterate(1000)[-1].hex(),
    "cases": cases,
}
assert doc["iterated_1000"] == X.ITERATED_1000
with open(os.path.join(HERE, "canon_x25519_vectors.json"), "w") as f:
    json.dump(doc, f, indent=0, sort_keys=True)
    f.write("\n")
print("%d cases" % len(cases))
