"""
Emits tests/golden/eddsa_verify_vectors.json: the reference's Ed25519Signature::verify (eddsa.rs:360-447) and
EdDsa::<Ed25519, Sha512>::verify (156-212) from the message -- inputs and the expected status -- through
tests/eddsa_verify_ref.py over oracle/py_model.py (restatement-derived; not reference-executed).

    python tests/golden/gen_eddsa_verify.py

Byte form: the three message cases and a near miss of each; R None with A Some, A None with R Some, both Some; an x
whose 64-bit limb exceeds the same limb of p while the value is below p (FieldElement::from_bytes, ed25519.rs:346-348),
and an x with bit 255 set; s with all bytes 0xff.  "Both candidate branches of the reference's sqrt" cannot be told apart
by any input found: the Legendre exponent of the reference's sqrt (ed25519.rs:359-402) lacks bit 63 of (p - 1) / 2, so `leg` is 0 or 1 only for
y^2 in {0, 1, -1}; no x among 2 000 random ones decodes, and x = 0 (y^2 = 0, where both candidates are 0 and the second is
returned) is the one decodable x these cases use.  The roots of x^3 + 0x7FFFFFDA x^2 + x = 1 and = -1, which would take
the first and the second candidate, were not searched for.
Generic form: an R flagged as the identity; signatures built as gen_eddsa_ed25519.py builds them (public key at
infinity, R = to_affine(multiply(G, s))), which verify, with messages on both sides of the padding edges of the 66-byte
prefix; the panic construction of that generator carried over to a hashed k (below); false cases.

Whether a byte-form input outside the special cases verifies TRUE is settled by a bounded search over degenerate
points (search_true_byte_case); what it found is recorded in the fixture's provenance and added as a case.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import eddsa_verify_ref as R  # noqa: E402
from oracle import py_model as M  # noqa: E402

OUT = os.path.join(HERE, "eddsa_verify_vectors.json")
P = (1 << 255) - 19
ORDER = (1 << 252) + 27742317777372353535851937790883648493
GENERIC_LENGTHS = [1, 45, 46, 64, 173, 174, 300]   # 66 + len crosses 111/112 and 239/240


def limbs(v):
    return [(v >> (64 * i)) & R.M64 for i in range(4)]


def value(l):
    return sum(int(x) << (64 * i) for i, x in enumerate(l))


def byte_cases(seed=20261017):
    """-> [(public_key, msg, sig, note)]"""
    rnd = random.Random(seed)
    rb = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    rx = lambda: (rnd.getrandbits(255) % P).to_bytes(32, "little")
    z = bytes(32)   # x = 0: y^2 = 0, the one x found to decode (see the module docstring)
    none = [rx() for _ in range(6)]
    assert all(M.decompress(M.ED25519, b"\x02" + x) is None for x in none) and M.decompress(M.ED25519, b"\x02" + z) is not None
    out = [(rb(32), b"test message", rb(64), "test message"), (rb(32), b"", rb(64), "empty message"),
           (rb(32), b"different message", rb(64), "different message"),
           (z, b"test messagf", z + rb(32), "near miss"), (z, b"different messagE", z + rb(32), "near miss"),
           (z, b"\x00", z + rb(32), "one byte"),
           (z, rb(33), none[0] + rb(32), "R None, A Some"), (none[1], rb(47), z + rb(32), "R Some, A None"),
           (none[2], rb(48), none[3] + rb(32), "both None"),
           (z, rb(20), z + rb(32), "both Some"), (z, rb(64), z + rb(32), "both Some"),
           (z, rb(175), z + bytes(32), "both Some, s = 0"), (z, rb(176), z + bytes(32), "both Some, s = 0"),
           (z, rb(10), z + b"\xff" * 32, "s all 0xff")]
    # a limb above p's limb, the value below p: limb 0 = 2^64 - 1 > 2^64 - 19 with limb 3 small (346-348); and bit 255
    over0 = (R.M64 | (rnd.getrandbits(180) << 64)).to_bytes(32, "little")
    over3 = (rnd.getrandbits(255) | (1 << 255)).to_bytes(32, "little")
    out += [(z, rb(12), over0 + rb(32), "R limb 0 above p's"), (over0, rb(12), z + rb(32), "A limb 0 above p's"),
            (z, rb(17), over3 + rb(32), "R bit 255"), (P.to_bytes(32, "little"), rb(5), z + rb(32), "A = p")]
    return out


def search_true_byte_case():
    """A bounded search for a byte-form input outside the special cases that verifies true: R and A from the degenerate
    x in {0, 1, p - 1}, s in {0, 1}, sixteen one-byte messages.  -> (public_key, msg, sig) or None, and the number tried."""
    be, tried = R.PyBackend(), 0
    xs = [v.to_bytes(32, "little") for v in (0, 1, P - 1)]
    for xa in xs:
        for xr in xs:
            for s in (0, 1):
                for msg in (bytes([m]) for m in range(1, 17)):
                    tried += 1
                    sig = xr + s.to_bytes(32, "big")
                    if R.verify_batch([xa], [msg], [sig], be) == [1]:
                        return (xa, msg, sig), tried
    return None, tried


def panic_case(rnd, pk_xy):
    """The panic construction of gen_eddsa_ed25519.py with k hashed: to_bytes(R) holds x and ONE bit of y (ed25519.rs:
    1505-1525), so with R = (1, y) the hash, and with it Q = multiply(from_affine(pk), k), is fixed before y is: y is then
    solved from d * (1 * y) * Q.t = Q.z, which makes the z of R + Q zero (ed25519.rs:1864-1928) while its y is not.  The
    message is drawn until bit 248 of that y is the bit that was hashed and the model reports the panic."""
    d = value(M.Ed.D)
    pkb = M.compress(M.ED25519, pk_xy[:4], pk_xy[4:], False)
    while True:
        msg = bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(1, 80)))
        for bit in (0, 1):
            k = R.from_bytes_be(hashlib.sha512(bytes([2 + bit]) + (1).to_bytes(32, "little") + pkb + msg).digest()[:32])
            q = M.Ed.multiply((pk_xy[:4], pk_xy[4:], [1, 0, 0, 0], M.Ed.mul(pk_xy[:4], pk_xy[4:])), k)
            den = d * value(q[3]) % P
            if den == 0:
                continue
            y = limbs(value(q[2]) * pow(den, -1, P) % P)
            r_xy = [1, 0, 0, 0] + y
            if M.compress(M.ED25519, r_xy[:4], r_xy[4:], False)[0] != 2 + bit:
                continue
            s = limbs(rnd.randrange(1, ORDER))
            if M.ed25519_eddsa_verify(r_xy, False, pk_xy, False, s, k) == 2:
                return msg, r_xy, s


def generic_cases(seed=20261018):
    """-> [(pk_xy, pk_inf, msg, r_xy, r_inf, s, note)]"""
    rnd = random.Random(seed)
    rb = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    rxy = lambda: limbs(rnd.randrange(P)) + limbs(rnd.randrange(P))
    sc = lambda: limbs(rnd.randrange(1, ORDER))
    out = [(rxy(), 0, b"test message", rxy(), 0, sc(), "test message"), (rxy(), 0, b"", rxy(), 1, sc(), "empty message"),
           (rxy(), 1, b"different message", rxy(), 0, sc(), "different message"),
           (rxy(), 0, rb(30), rxy(), 1, sc(), "R flagged identity")]
    for n in GENERIC_LENGTHS:   # verifying: pk at infinity, R = to_affine(multiply(G, s))
        s = sc()
        x, y, inf = M.Ed.to_affine(M.Ed.multiply(M.Ed.generator(), s))
        assert not inf
        out.append((rxy(), 1, rb(n), list(x) + list(y), 0, s, "verifies: pk at infinity"))
    s = sc()
    x, y, _ = M.Ed.to_affine(M.Ed.multiply(M.Ed.generator(), s))
    out.append((rxy(), 1, b"test messagf", list(x) + list(y), 0, [s[0] ^ 1] + s[1:], "pk at infinity, s off by one bit"))
    out.append((rxy(), 0, rb(50), list(x) + list(y), 0, s, "that R and s under a finite pk"))
    out += [(rxy(), 0, rb(n), rxy(), 0, sc(), "random") for n in (7, 100)]
    out.append((rxy(), 0, rb(9), rxy(), 0, [0, 0, 0, 0], "s = 0"))
    out.append((rxy(), 0, rb(9), rxy(), 0, [R.M64] * 4, "s = 2^256 - 1"))
    pk = rxy()
    msg, r_xy, s = panic_case(rnd, pk)
    out.append((pk, 0, msg, r_xy, 0, s, "the reference panics: z of R + k*A is zero"))
    return out


def main():
    be = R.PyBackend()
    byte = byte_cases()
    found, tried = search_true_byte_case()
    note = ("bounded search for a byte-form input outside the special cases that verifies true (R, A from x in {0, 1, p-1}, "
            "s in {0, 1}, 16 one-byte messages): ")
    if found:
        byte.append(found + ("verifies true outside the special cases",))
        note += "found after %d inputs and included as the last byte-form case" % tried
    else:
        note += "none among %d inputs" % tried
    out = {"provenance": "restatement-derived by tests/eddsa_verify_ref.py over oracle/py_model.py; not reference-executed; " + note,
           "bytes": [], "generic": []}
    for (pk, m, sig, what), st in zip(byte, R.verify_batch([c[0] for c in byte], [c[1] for c in byte], [c[2] for c in byte], be)):
        out["bytes"].append({"note": what, "pk": pk.hex(), "msg": m.hex(), "sig": sig.hex(), "status": st})
    g = generic_cases()
    sts = R.eddsa_verify_batch([c[0] for c in g], [c[1] for c in g], [c[2] for c in g], [c[3] for c in g], [c[4] for c in g],
                               [c[5] for c in g], be)
    h = lambda l: [f"{int(v):016x}" for v in l]
    for (pk, pinf, m, r, rinf, s, what), st in zip(g, sts):
        out["generic"].append({"note": what, "pk": h(pk), "pk_inf": pinf, "msg": m.hex(), "r": h(r), "r_inf": rinf, "s": h(s), "status": st})
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(OUT, {k: [c["status"] for c in v] for k, v in out.items() if k != "provenance"})
    print(out["provenance"])


if __name__ == "__main__":
    main()
