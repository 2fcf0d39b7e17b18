"""
Writes tests/golden/canon_batch_vectors.json from the model (tests/canon_batch_ref.py): per scheme 80 valid (message,
signature, key) triples signed by the model over the message lengths that sit on the SHA block edges of both hashes, the
elements the batch calls refuse, and for Ed25519 the signatures with a torsion defect.  Run from the repository root:
    python tests/gen_canon_batch.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import canon_adversarial as ADV   # noqa: E402
import canon_batch_ref as B       # noqa: E402
import canon_msg_ref as R         # noqa: E402

SEED = 0xBA7C4
PER_LENGTH = 10
KEYS = 8


def valid(scheme, rng):
    rows = []
    if scheme == "bip340":
        keys = [rng.randrange(1, R.SECP.N) for _ in range(KEYS)]
    else:
        keys = [rng.randbytes(32) for _ in range(KEYS)]
        pubs = [R.ed25519_pubkey(k) for k in keys]
    for j in range(PER_LENGTH):
        for ln in B.MSG_LENGTHS:
            msg, k = rng.randbytes(ln), (j * len(B.MSG_LENGTHS) + B.MSG_LENGTHS.index(ln)) % KEYS
            if scheme == "bip340":
                sig, pk = R.bip340_sign(keys[k], msg, rng.randbytes(32)), R.bip340_pubkey(keys[k])
            else:
                sig, pk = R.ed25519_sign(keys[k], msg), pubs[k]
            assert B.single(scheme, msg, sig, pk) == 1
            rows.append((msg, sig, pk))
    return rows


def refused(scheme, rows):
    """one spoiled copy of a valid triple per rule"""
    out = []

    def add(name, row, status):
        assert B.single(scheme, *row) == 0
        out.append({"name": name, "msg": row[0].hex(), "sig": row[1].hex(), "pk": row[2].hex(), "status": status})

    msg, sig, pk = rows[3]
    if scheme == "bip340":
        add("s = n", (msg, sig[:32] + R.SECP.N.to_bytes(32, "big"), pk), B.BAD_SCALAR)
        add("s = 2^256 - 1", (msg, sig[:32] + b"\xff" * 32, pk), B.BAD_SCALAR)
        add("r = p", (msg, R.SECP.P.to_bytes(32, "big") + sig[32:], pk), B.BAD_POINT)
        x = next(x for x in range(1, 100) if R.lift_x(x) is None)
        add("r with no square root", (msg, x.to_bytes(32, "big") + sig[32:], pk), B.BAD_POINT)
        add("key with no square root", (msg, sig, x.to_bytes(32, "big")), B.BAD_POINT)
        add("key = p", (msg, sig, R.SECP.P.to_bytes(32, "big")), B.BAD_POINT)
    else:
        p = R.ED.P
        add("S = l", (msg, sig[:32] + R.ED.N.to_bytes(32, "little"), pk), B.BAD_SCALAR)
        add("S = 2^256 - 1", (msg, sig[:32] + b"\xff" * 32, pk), B.BAD_SCALAR)
        y = next(y for y in range(2, 100) if R.ed_decode(y.to_bytes(32, "little")) is None)
        add("key off the curve", (msg, sig, y.to_bytes(32, "little")), B.BAD_POINT)
        add("R off the curve", (msg, y.to_bytes(32, "little") + sig[32:], pk), B.BAD_POINT)
        add("key with non-canonical y = p + 1", (msg, sig, (p + 1).to_bytes(32, "little")), B.BAD_POINT)
        add("R with non-canonical y = p", (msg, p.to_bytes(32, "little") + sig[32:], pk), B.BAD_POINT)
        add("key x = 0 with the sign bit", (msg, sig, (1 | 1 << 255).to_bytes(32, "little")), B.BAD_POINT)
    return out


def torsion(rng):
    """R + T and A + T for T of order 2, 4 and 8, S by the signer's rule on the encodings as they are: the defect
    S B - h A - R is -T, or -h T with h odd"""
    E, tors, out = R.ED, ADV.torsion_points(), []
    for j in (4, 2, 1):   # j T8: orders 2, 4, 8
        T = tors[j]
        for where in ("R", "A"):
            for _ in range(ADV.SEARCH_LIMIT):
                a, r, msg = E.secret_scalar(rng.randbytes(32)), rng.randrange(1, E.N), rng.randbytes(32)
                A, Rp = E.mul(a, E.G), E.mul(r, E.G)
                if where == "R":
                    Rp = E.add(Rp, T)
                else:
                    A = E.add(A, T)
                Renc, Aenc = E.encode(Rp), E.encode(A)
                h = R.ed25519_challenge(Renc, Aenc, msg)
                if h & 1:
                    break
            sig = Renc + ((r + h * a) % E.N).to_bytes(32, "little")
            assert R.ed25519_verify(msg, sig, Aenc) == 0
            out.append({"name": "%s + T of order %d" % (where, ADV.order_of(T)), "msg": msg.hex(), "sig": sig.hex(), "pk": Aenc.hex()})
    return out


def build():
    rng = random.Random(SEED)
    doc = {"comment": "tests/gen_canon_batch.py: valid = [msg, sig, pk] hex, signed by the model"}
    for scheme in B.SCHEMES:
        rows = valid(scheme, rng)
        doc[scheme] = {"valid": [[v.hex() for v in row] for row in rows], "refused": refused(scheme, rows)}
    doc["ed25519"]["torsion"] = torsion(rng)
    return doc


if __name__ == "__main__":
    with open(B.FIXTURE, "w") as f:
        json.dump(build(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(B.FIXTURE, os.path.getsize(B.FIXTURE), "bytes")
