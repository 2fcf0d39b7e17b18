"""
Writes tests/golden/canon_msg_vectors.json from tests/canon_msg_ref.py with a fixed seed:

    python tests/golden/gen_canon_msg.py

One batch per (scheme, curve, key form), the cases in the order a test concatenates their messages.  First the valid
cases: every message length that decides a block or padding boundary of the hash, each at all four start alignments
mod 4 of the concatenated messages (1-byte messages are put in between where the next alignment needs them); then one
negative case per way a signature, a key or a message can be wrong, and ECDSA's malleable twin, which verifies.
Every signature here is signed by the model -- secp256k1 ECDSA has no published from-the-message vector in the tree; the
published vectors of the other three are in tests/canon_msg_ref.py: published() and are copied under "published".
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import canon_msg_ref as R  # noqa: E402

SHA256_LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120]               # ECDSA; BIP-340 (the message starts a block)
SHA512_LENGTHS = [0, 1, 47, 48, 63, 64, 65, 175, 176, 192]          # behind the 64-byte prefix R || A
SEED = 0x16C0DE


def aligned_lengths(lengths):
    """The message lengths of the valid part, in order: every length of `lengths` starts at every alignment mod 4."""
    seq, cur = [], 0
    for L in lengths:
        todo = {0, 1, 2, 3}
        while todo:
            if cur % 4 in todo:
                todo.discard(cur % 4)
                seq.append(L)
                cur += L
            else:
                seq.append(1)
                cur += 1
    return seq


def case(name, msg, sig, pk, want):
    return {"name": name, "msg": msg.hex(), "sig": sig.hex(), "pk": pk.hex(), "want": want}


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def be32(v):
    return v.to_bytes(32, "big")


def ecdsa_batch(name, pk_len, rng):
    C = R.WEIERSTRASS[name]
    comp = pk_len == 33
    keys = [rng.randrange(1, C.N) for _ in range(5)]
    pts = [C.mul(d, C.G) for d in keys]

    def signed(i, msg):
        d = keys[i % 5]
        k = int.from_bytes(hashlib.sha256(b"nonce" + be32(d) + msg).digest(), "big") % C.N or 1
        return R.ecdsa_sign(C, d, msg, k), R.sec1_encode(pts[i % 5], comp)

    cases = []
    for i, L in enumerate(aligned_lengths(SHA256_LENGTHS)):
        msg = rng.randbytes(L)
        sig, pk = signed(i, msg)
        cases.append(case("valid len %d" % L, msg, sig, pk, 1))
    msg = rng.randbytes(37)
    sig, pk = signed(0, msg)
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    neg = [("message byte changed", flip(msg, 100), sig, pk),
           ("bit of r changed", msg, flip(sig, 77), pk),
           ("bit of s changed", msg, flip(sig, 256 + 131), pk),
           ("bit of the key changed", msg, sig, flip(pk, 8 + 200)),
           ("r = 0", msg, be32(0) + sig[32:], pk),
           ("s = 0", msg, sig[:32] + be32(0), pk),
           ("r = n", msg, be32(C.N) + sig[32:], pk),
           ("r >= n: r + n", msg, be32(r + C.N if r + C.N < 2**256 else 2**256 - 1) + sig[32:], pk),
           ("s = n", msg, sig[:32] + be32(C.N), pk),
           ("s >= n: s + n", msg, sig[:32] + be32(s + C.N if s + C.N < 2**256 else 2**256 - 1), pk),
           ("malleable twin n - s", msg, sig[:32] + be32(C.N - s), pk)]
    x = 1   # a small x on the curve: x + p is the same residue and fits in 32 bytes
    while R.sqrt_mod(C, (x**3 + C.A * x + C.B) % C.P) is None:
        x += 1
    y = R.sqrt_mod(C, (x**3 + C.A * x + C.B) % C.P)
    nx = 1  # and one with no root
    while R.sqrt_mod(C, (nx**3 + C.A * nx + C.B) % C.P) is not None:
        nx += 1
    P0 = pts[0]
    if comp:
        assert R.sec1_decode(C, bytes([2 + (y & 1)]) + be32(x)) == (x, y)
        neg += [("key x >= p: x + p", msg, sig, bytes([2 + (y & 1)]) + be32(x + C.P)),
                ("key x = p", msg, sig, b"\x02" + be32(C.P)),
                ("key x has no root", msg, sig, b"\x02" + be32(nx)),
                ("key of the other parity", msg, sig, bytes([pk[0] ^ 1]) + pk[1:])]
        neg += [("key tag %d" % t, msg, sig, bytes([t]) + pk[1:]) for t in (0, 4, 5, 6, 7)]
    else:
        assert R.sec1_decode(C, b"\x04" + be32(x) + be32(y)) == (x, y)
        neg += [("key x >= p: x + p", msg, sig, b"\x04" + be32(x + C.P) + be32(y)),
                ("key y >= p: 2^256 - 1", msg, sig, b"\x04" + be32(P0[0]) + be32(2**256 - 1)),
                ("key y = p", msg, sig, b"\x04" + be32(P0[0]) + be32(C.P)),
                ("key y off the curve", msg, sig, b"\x04" + be32(P0[0]) + be32((P0[1] + 1) % C.P)),
                ("key with -y", msg, sig, b"\x04" + be32(P0[0]) + be32(C.P - P0[1]))]
        neg += [("key tag %d" % t, msg, sig, bytes([t]) + pk[1:]) for t in (0, 2, 3, 6, 7)]
    for nm, m, sg, k in neg:
        cases.append(case(nm, m, sg, k, R.ecdsa_verify(C, m, sg, k)))
    return {"scheme": "ecdsa", "curve": name, "pk_len": pk_len, "cases": cases}


def bip340_batch(rng):
    C = R.SECP
    keys = [rng.randrange(1, C.N) for _ in range(5)]
    cases = []
    for i, L in enumerate(aligned_lengths(SHA256_LENGTHS)):
        msg = rng.randbytes(L)
        d = keys[i % 5]
        cases.append(case("valid len %d" % L, msg, R.bip340_sign(d, msg, rng.randbytes(32)), R.bip340_pubkey(d), 1))
    msg = rng.randbytes(32)
    sig, pk = R.bip340_sign(keys[0], msg), R.bip340_pubkey(keys[0])
    s = int.from_bytes(sig[32:], "big")
    x = 1
    while R.lift_x(x) is None:
        x += 1
    nx = 1
    while R.lift_x(nx) is not None:
        nx += 1
    neg = [("message byte changed", flip(msg, 9), sig, pk),
           ("bit of r changed", msg, flip(sig, 3), pk),
           ("bit of s changed", msg, flip(sig, 256 + 255), pk),
           ("bit of the key changed", msg, sig, flip(pk, 129)),
           ("r = p", msg, be32(C.P) + sig[32:], pk),
           ("r >= p: 2^256 - 1", msg, be32(2**256 - 1) + sig[32:], pk),
           ("s = n", msg, sig[:32] + be32(C.N), pk),
           ("s >= n: s + n", msg, sig[:32] + be32(s + C.N if s + C.N < 2**256 else 2**256 - 1), pk),
           ("key x >= p: x + p", msg, sig, be32(x + C.P)),
           ("key x = p", msg, sig, be32(C.P)),
           ("key x has no root", msg, sig, be32(nx)),
           ("signature of another message", rng.randbytes(32), sig, pk)]
    for nm, m, sg, k in neg:
        cases.append(case(nm, m, sg, k, R.bip340_verify(m, sg, k)))
    return {"scheme": "bip340", "curve": "secp256k1", "pk_len": 32, "cases": cases}


def ed25519_batch(rng):
    E = R.ED
    seeds = [rng.randbytes(32) for _ in range(5)]
    cases = []
    for i, L in enumerate(aligned_lengths(SHA512_LENGTHS)):
        msg = rng.randbytes(L)
        cases.append(case("valid len %d" % L, msg, R.ed25519_sign(seeds[i % 5], msg), R.ed25519_pubkey(seeds[i % 5]), 1))
    msg = rng.randbytes(50)
    sig, pk = R.ed25519_sign(seeds[0], msg), R.ed25519_pubkey(seeds[0])
    S = int.from_bytes(sig[32:], "little")
    le32 = lambda v: v.to_bytes(32, "little")  # noqa: E731
    y0 = next(y for y in range(2, 19) if R.ed_decode(le32(y)) is not None)   # decodable, and y0 + p fits in 255 bits
    ny = next(y for y in range(2, 1000) if R.ed_decode(le32(y)) is None)     # no x for this y
    neg = [("message byte changed", flip(msg, 300), sig, pk),
           ("bit of R changed", msg, flip(sig, 41), pk),
           ("bit of S changed", msg, flip(sig, 256 + 17), pk),
           ("bit of the key changed", msg, sig, flip(pk, 60)),
           ("S >= l: S + l", msg, sig[:32] + le32(S + E.N), pk),
           ("S = l", msg, sig[:32] + le32(E.N), pk),
           ("key y >= p: y + p", msg, sig, le32(y0 + E.P)),
           ("key y = p", msg, sig, le32(E.P)),
           ("key x = 0 with the sign bit", msg, sig, le32(1 | (1 << 255))),
           ("key y has no x", msg, sig, le32(ny)),
           ("R undecodable", msg, le32(ny) + sig[32:], pk),
           ("R y >= p: y + p", msg, le32(y0 + E.P) + sig[32:], pk),
           ("R with the other sign", msg, flip(sig, 255), pk)]
    for nm, m, sg, k in neg:
        cases.append(case(nm, m, sg, k, R.ed25519_verify(m, sg, k)))
    return {"scheme": "ed25519", "curve": "ed25519", "pk_len": 32, "cases": cases}


def build():
    rng = random.Random(SEED)
    batches = [ecdsa_batch(c, k, rng) for c in ("secp256k1", "p256") for k in (33, 65)] + [bip340_batch(rng), ed25519_batch(rng)]
    pub = {name: {"scheme": sc, "curve": cv, "pk_len": len(pk), "msg": m.hex(), "sig": sg.hex(), "pk": pk.hex(), "want": 1}
           for name, (sc, cv, m, sg, pk) in R.published().items()}
    return {"note": "model-signed by tests/canon_msg_ref.py (seed %#x); secp256k1 ECDSA has no published vector in the tree" % SEED,
            "sha256_lengths": SHA256_LENGTHS, "sha512_lengths": SHA512_LENGTHS, "batches": batches, "published": pub}


if __name__ == "__main__":
    out = os.path.join(HERE, "canon_msg_vectors.json")
    with open(out, "w") as f:
        json.dump(build(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(out, sum(len(b["cases"]) for b in build()["batches"]), "cases")
