"""Writes tests/golden/canon_bip32_vectors.json from the model tests/canon_bip32_ref.py:
    python tests/golden/gen_canon_bip32.py
Deterministic (a seeded generator).  Hex = the bytes in order.  The file holds rows, one per line, and
canon_bip32_ref.load_fixture() turns them into cases without any curve arithmetic beyond decoding a key:
"pairs": [curve, d, tweak, key33, out33, out33x]: 64 random (key, tweak) pairs per curve.  key33 = d G; each pair is a
  fec_canon_pubkey_tweak_add case in every input form (65 bytes: key33 decoded; 32 bytes: its x, read as the point with even
  y, whose sum is out33x where that differs from out33, else "") and a fec_canon_seckey_tweak_add case (d + tweak mod n).
"tweak": [class, name, curve, key, tweak, status, out33]: the other tweak-add cases; out33 = the SEC 1 compressed sum, from
  which the forms 65 and 32 follow, "" where the status is not 0.  Classes: tweak (t = 0, 1, n - 1, n, n + 1, 2^256 - 1),
  doubling (t = d), infinity (t = n - d), off-curve (an x with no point), range (x or y >= p), tag (0, 4, 5, 6, 7 on 33 bytes;
  2, 6, 7 on 65), wrong-y (65 bytes, y off by one bit).
"seckey": [class, name, curve, key, tweak, status, out]: tweak (as above), key (0, n, n + 1, 2^256 - 1), zero (k + t = 0 mod n).
"triples": [key, cc, index, child, child_cc, pk, pub_child, pub_cc]: 128 random (parent, chain code, index) triples on
  secp256k1, every other index hardened: CKDpriv(key, cc, index) = (child, child_cc), and with pk = key G,
  CKDpub(pk, cc, index mod 2^31) = (pub_child, pub_cc), pub_cc "" where it is child_cc.
"bip32_pub": [class, name, pk, cc, index, status, child, child_cc] and "bip32_priv": [class, name, key, cc, index, flags, status,
  child, child_cc]: the other derivations, outputs "" where the status is not 0.  Classes: vector1 (BIP-32 test vector 1),
  index (0, 1, 2^31 - 1, 2^31, 2^32 - 1), key (a bad parent), no-comb (flags = 1 on a hardened and on a non-hardened index).
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import canon_bip32_ref as B  # noqa: E402

rng = random.Random(0xB1932)
b32 = B.b32


def rand32():
    return bytes(rng.randrange(256) for _ in range(32))


pairs, tweak, seckey, triples, pub, priv = [], [], [], [], [], []


def add_tweak(cls, name, curve, key, t, want=None):
    out, st = B.pubkey_tweak_add(B.CURVES[curve], key, t, 33)
    assert want is None or st == want, (cls, name, st)
    tweak.append([cls, name, curve, key.hex(), t.hex(), st, out.hex() if st == 0 else ""])


def add_seckey(cls, name, curve, key, t, want=None):
    out, st = B.seckey_tweak_add(B.CURVES[curve], key, t)
    assert want is None or st == want, (cls, name, st)
    seckey.append([cls, name, curve, key.hex(), t.hex(), st, out.hex() if st == 0 else ""])


def add_pub(cls, name, pk, cc, index, want=None):
    child, ccc, st = B.ckd_pub(pk, cc, index)
    assert want is None or st == want, (cls, name, st)
    pub.append([cls, name, pk.hex(), cc.hex(), index, st] + ([child.hex(), ccc.hex()] if st == 0 else ["", ""]))
    return child, ccc


def add_priv(cls, name, key, cc, index, flags=0, want=None):
    child, ccc, st = B.ckd_priv(key, cc, index, flags)
    assert want is None or st == want, (cls, name, st)
    priv.append([cls, name, key.hex(), cc.hex(), index, flags, st] + ([child.hex(), ccc.hex()] if st == 0 else ["", ""]))
    return child, ccc


for curve, C in sorted(B.CURVES.items()):
    n, p = C.N, C.P
    forms = (33, 65, 32) if curve == "secp256k1" else (33, 65)
    for i in range(64):
        d, t = rng.randrange(1, n), rng.randrange(n)
        D = C.mul(d, C.G)
        out, st = B.pubkey_tweak_add(C, B.encode(D, 33), b32(t), 33)
        outx, stx = B.pubkey_tweak_add(C, B.encode(D, 32), b32(t), 33)
        assert st == 0 and stx == 0 and B.seckey_tweak_add(C, b32(d), b32(t))[1] == 0
        pairs.append([curve, b32(d).hex(), b32(t).hex(), B.encode(D, 33).hex(), out.hex(), outx.hex() if outx != out and curve == "secp256k1" else ""])
    d = rng.randrange(1, n)
    D = C.mul(d, C.G)
    pk33, pk65 = B.encode(D, 33), B.encode(D, 65)
    for t, what, st in ((0, "0", 0), (1, "1", 0), (n - 1, "n - 1", 0), (n, "n", 3), (n + 1, "n + 1", 3), (2**256 - 1, "2^256 - 1", 3)):
        for form in forms:
            add_tweak("tweak", "t = %s, %d-byte key" % (what, form), curve, B.encode(D, form), b32(t), st)
        add_seckey("tweak", "t = %s" % what, curve, b32(d), b32(t), st)
    for form in forms:
        dd = d if form != 32 or not (D[1] & 1) else n - d   # x-only reads the even y: the key of n - d
        add_tweak("doubling", "t = d, %d-byte key" % form, curve, B.encode(D, form), b32(dd), 0)
        add_tweak("infinity", "t = n - d, %d-byte key" % form, curve, B.encode(D, form), b32(n - dd), 8)
    x = rng.randrange(1, p)
    while B.sqrt_mod(C, (x**3 + C.A * x + C.B) % p) is not None:
        x = rng.randrange(1, p)
    for tag in (2, 3):
        add_tweak("off-curve", "x with no point, tag %d" % tag, curve, bytes([tag]) + b32(x), b32(1), 2)
    add_tweak("off-curve", "x with no point, 65 bytes", curve, b"\x04" + b32(x) + b32(1), b32(1), 2)
    if curve == "secp256k1":
        add_tweak("off-curve", "x with no point, x-only", curve, b32(x), b32(1), 2)
        add_tweak("range", "x = p, x-only", curve, b32(p), b32(1), 2)
    for v, what in ((p, "p"), (p + 1, "p + 1"), (2**256 - 1, "2^256 - 1")):
        add_tweak("range", "x = %s" % what, curve, b"\x02" + b32(v), b32(1), 2)
    add_tweak("range", "y = p, 65 bytes", curve, b"\x04" + b32(D[0]) + b32(p), b32(1), 2)
    for tag in (0, 4, 5, 6, 7):
        add_tweak("tag", "tag %d, 33 bytes" % tag, curve, bytes([tag]) + pk33[1:], b32(1), 2)
    for tag in (2, 6, 7):
        add_tweak("tag", "tag %d, 65 bytes" % tag, curve, bytes([tag]) + pk65[1:], b32(1), 2)
    add_tweak("wrong-y", "y off by one bit", curve, pk65[:64] + bytes([pk65[64] ^ 1]), b32(1), 2)
    add_tweak("wrong-y", "-y with tag 4 is a key", curve, b"\x04" + b32(D[0]) + b32(p - D[1]), b32(1), 0)
    for k, what in ((0, "0"), (n, "n"), (n + 1, "n + 1"), (2**256 - 1, "2^256 - 1")):
        add_seckey("key", "k = %s" % what, curve, b32(k), b32(1), 6)
    add_seckey("key", "k = n - 1", curve, b32(n - 1), b32(2), 0)
    add_seckey("zero", "k + t = n", curve, b32(d), b32(n - d), 8)
    add_seckey("zero", "k = n - 1, t = 1", curve, b32(n - 1), b32(1), 8)

C = B.SECP256K1
n = C.N
# BIP-32 test vector 1 (the published values are pinned in tests/test_canon_bip32_model.py)
mk, mcc = B.master(bytes(range(16)))
k1, cc1 = add_priv("vector1", "m -> m/0'", mk, mcc, B.HARDENED, 0, 0)
k2, cc2 = add_priv("vector1", "m/0' -> m/0'/1", k1, cc1, 1, 0, 0)
add_priv("vector1", "m -> m/0' without the comb", mk, mcc, B.HARDENED, B.NO_COMB, 0)
p2, pcc2 = add_pub("vector1", "M/0' -> M/0'/1", B.public_key(C, k1), cc1, 1, 0)
assert (p2, pcc2) == (B.public_key(C, k2), cc2)
for i in range(128):
    key, cc = b32(rng.randrange(1, n)), rand32()
    index = rng.randrange(B.HARDENED) | (B.HARDENED if i & 1 else 0)
    pk = B.public_key(C, key)
    ck, ccc, st = B.ckd_priv(key, cc, index)
    cp, pcc, st2 = B.ckd_pub(pk, cc, index & (B.HARDENED - 1))
    assert st == 0 and st2 == 0
    if not i & 1:
        assert (cp, pcc) == (B.public_key(C, ck), ccc)
    triples.append([key.hex(), cc.hex(), index, ck.hex(), ccc.hex(), pk.hex(), cp.hex(), pcc.hex() if pcc != ccc else ""])
key, cc = b32(rng.randrange(1, n)), rand32()
pk = B.public_key(C, key)
for index in (0, 1, B.HARDENED - 1, B.HARDENED, 2**32 - 1):
    add_priv("index", "index %d" % index, key, cc, index, 0, 0)
    add_pub("index", "index %d" % index, pk, cc, index, 9 if index >= B.HARDENED else 0)
for k, what in ((0, "0"), (n, "n"), (2**256 - 1, "2^256 - 1")):
    add_priv("key", "parent key %s" % what, b32(k), cc, 7, 0, 6)
    add_priv("key", "parent key %s, hardened" % what, b32(k), cc, B.HARDENED + 7, 0, 6)
add_priv("key", "parent key 0 under NO_COMB, not hardened", bytes(32), cc, 7, B.NO_COMB, 6)
add_pub("key", "tag 5", b"\x05" + pk[1:], cc, 3, 2)
add_pub("key", "tag 4 on 33 bytes", b"\x04" + pk[1:], cc, 3, 2)
add_pub("key", "x = p", b"\x02" + b32(C.P), cc, 3, 2)
x = rng.randrange(1, C.P)
while B.sqrt_mod(C, (x**3 + 7) % C.P) is not None:
    x = rng.randrange(1, C.P)
add_pub("key", "x with no point", b"\x03" + b32(x), cc, 3, 2)
add_pub("key", "x with no point and a hardened index", b"\x03" + b32(x), cc, B.HARDENED, 2)
add_pub("index", "hardened index %d" % (B.HARDENED + 44), pk, cc, B.HARDENED + 44, 9)
add_priv("no-comb", "a hardened index", key, cc, B.HARDENED + 5, B.NO_COMB, 0)
add_priv("no-comb", "a non-hardened index", key, cc, 5, B.NO_COMB, 9)
add_priv("no-comb", "index 2^31 - 1", key, cc, B.HARDENED - 1, B.NO_COMB, 9)

doc = [("comment", "EC tweak-add and BIP-32 derivation by tests/canon_bip32_ref.py; the layout is in tests/golden/gen_canon_bip32.py; hex = the bytes in order"),
       ("pairs", pairs), ("tweak", tweak), ("seckey", seckey), ("triples", triples), ("bip32_pub", pub), ("bip32_priv", priv)]
with open(os.path.join(HERE, "canon_bip32_vectors.json"), "w") as f:
    f.write("{\n")
    for j, (name, val) in enumerate(doc):
        last = "\n" if j == len(doc) - 1 else ",\n"
        if isinstance(val, str):
            f.write(json.dumps(name) + ": " + json.dumps(val) + last)
        else:
            f.write(json.dumps(name) + ": [\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in val) + "\n]" + last)
    f.write("}\n")
print("%d pairs, %d other tweak, %d seckey, %d triples, %d CKDpub, %d CKDpriv rows" % (len(pairs), len(tweak), len(seckey), len(triples), len(pub), len(priv)))
