"""Writes tests/golden/canon_wallet_vectors.json from the model tests/canon_wallet_ref.py:
    python tests/golden/gen_canon_wallet.py
Deterministic (a seeded generator).  Hex = the bytes in order, one row per line.  Kept small: the tests derive their bulk cases
from seeds with the model.
"hashes": [length, msg, ripemd160, hash160]: one random message of every length at which the padding or the block count
  changes (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 200).
"taproot": [class, name, pk, root, status, out, parity]: pk 32 or 33 bytes, root "" for none, out "" where the status is not 0.
  Classes: bip86 (the BIP's first receive key), random (with and without a root; x-only and 33 bytes with both tags, which
  give the same key), range (x = p, x = 2^256 - 1), off-curve (an x on no point), tag (0, 4, 5 on 33 bytes).
"path": [class, name, pk, cc, indices, status, child, child_cc, fingerprint, hash160]: outputs "" where the status is not 0.
  Classes: vector1 (BIP-32 test vector 1, m/0'/1/2' along [2, 1000000000]), random (depths 1, 2, 3, 8), index (a hardened
  index at each level of 3 in turn; at two levels: the first decides), key (a bad parent, alone and before a hardened index).
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import canon_bip32_ref as B  # noqa: E402
import canon_wallet_ref as W  # noqa: E402

rng = random.Random(0x160)
C = B.SECP256K1
LENGTHS = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 200)


def rand(n):
    return bytes(rng.randrange(256) for _ in range(n))


def rand_key(form=33):
    return B.encode(C.mul(rng.randrange(1, C.N), C.G), form)


def off_curve_x():
    while True:
        x = rng.randrange(C.P)
        if B.sqrt_mod(C, (x * x * x + C.B) % C.P) is None:
            return B.b32(x)


hashes, taproot, path = [], [], []
for n in LENGTHS:
    m = rand(n)
    hashes.append([n, m.hex(), W.ripemd160(m).hex(), W.hash160(m).hex()])


def tap(cls, name, pk, root):
    out, par, st = W.taproot_output_key(pk, root)
    taproot.append([cls, name, pk.hex(), root.hex() if root is not None else "", st, "" if st else out.hex(), par])


tap("bip86", "m/86'/0'/0'/0/0", bytes.fromhex("cc8a4bc64d897bddc5fbc2f670f7a8ba0b386779106cf1223c6fc5d7cd6fc115"), None)
for i in range(6):
    x = rand_key(32)
    root = rand(32) if i & 1 else None
    tap("random", "key %d, x-only" % i, x, root)
    tap("random", "key %d, tag 2" % i, b"\x02" + x, root)
    tap("random", "key %d, tag 3" % i, b"\x03" + x, root)
for name, x in (("x = p", B.b32(C.P)), ("x = 2^256 - 1", b"\xff" * 32)):
    tap("range", name, x, None)
    tap("range", name + ", 33 bytes", b"\x02" + x, rand(32))
x = off_curve_x()
tap("off-curve", "x-only", x, None)
tap("off-curve", "33 bytes", b"\x03" + x, rand(32))
for tag in (0, 4, 5):
    tap("tag", "tag %d" % tag, bytes([tag]) + rand_key(32), None)


def walk(cls, name, pk, cc, indices):
    child, ccc, fp, h160, st = W.derive_pub_path(pk, cc, indices)
    path.append([cls, name, pk.hex(), cc.hex(), indices, st] + (["", "", "", ""] if st else [child.hex(), ccc.hex(), fp.hex(), h160.hex()]))


walk("vector1", "m/0'/1/2'/2/1000000000", bytes.fromhex("0357bfe1e341d01c69fe5654309956cbea516822fba8a601743a012a7896ee8dc2"),
     bytes.fromhex("04466b9cc8e161e966409ca52986c584f07e9dc81f735db683c3ff6ec7b1503f"), [2, 1000000000])
for depth in (1, 2, 3, 8):
    for i in range(3):
        walk("random", "depth %d, %d" % (depth, i), rand_key(), rand(32), [rng.randrange(B.HARDENED) for _ in range(depth)])
for level in range(3):
    idx = [rng.randrange(B.HARDENED) for _ in range(3)]
    idx[level] |= B.HARDENED
    walk("index", "hardened at level %d of 3" % (level + 1), rand_key(), rand(32), idx)
walk("index", "hardened at levels 2 and 3", rand_key(), rand(32), [5, B.HARDENED, 0xFFFFFFFF])
walk("key", "tag 4", b"\x04" + rand_key(32), rand(32), [1, 2])
walk("key", "x on no point", b"\x02" + off_curve_x(), rand(32), [1])
walk("key", "x = p, then a hardened index", b"\x03" + B.b32(C.P), rand(32), [B.HARDENED, 2, 3])

doc = [("comment", "RIPEMD-160, HASH160, Taproot output keys and CKDpub paths by tests/canon_wallet_ref.py; the layout is in tests/golden/gen_canon_wallet.py; hex = the bytes in order"),
       ("hashes", hashes), ("taproot", taproot), ("path", path)]
with open(os.path.join(HERE, "canon_wallet_vectors.json"), "w") as f:
    f.write("{\n")
    for j, (name, val) in enumerate(doc):
        last = "\n" if j == len(doc) - 1 else ",\n"
        if isinstance(val, str):
            f.write(json.dumps(name) + ": " + json.dumps(val) + last)
        else:
            f.write(json.dumps(name) + ": [\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in val) + "\n]" + last)
    f.write("}\n")
print("%d hash, %d Taproot, %d path rows" % (len(hashes), len(taproot), len(path)))
