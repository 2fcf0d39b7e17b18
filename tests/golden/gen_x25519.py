"""
Writes tests/golden/x25519_vectors.json: cases of the reference's Curve25519 (forge-ec-curves/src/curve25519.rs) with
their expectations from the literal restatement tests/x25519_ref.py.

  field     Add / Sub / Mul / square / Neg on crafted raw operands, among them one per Mul rare leg (the discarded carry
            of 253, the unrippled += 1 of 261, the fold's += 1 at 291/300), each confirmed reached by the restatement
  x25519    the special scalar bytes [2, 0, ...], u = 0, u with its top bit set, u >= p before reduce, random cases,
            and the bounded search for an input whose final z2 is zero (invert(z2) is None -> the result is 0)
  multiply  raw scalars 0, 1, 2 and [0, 0, 0, 2 << 56] (the x25519 special case through Scalar::to_bytes), the
            identity point, unreduced coordinates and random cases

    python tests/golden/gen_x25519.py
"""
import itertools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import x25519_ref as X  # noqa: E402

M = X.M64
PATTERNS = [0, 1, 2, M, M - 1, 1 << 63, (1 << 63) - 1, 0xFFFFFFFF]
SEARCH_U = 64  # bounded search for a zero final z2: u in 0..SEARCH_U-1 and the small-order-looking values below


def mul_legs(a, b):
    X.LEGS.clear()
    X.mul(a, b)
    return sorted(X.LEGS)


def leg_operands():
    """the first operand pair in a fixed enumeration of patterned limbs on which each Mul leg fires"""
    found = {}
    for a in itertools.product(PATTERNS, repeat=4):
        for b in itertools.product([M, M - 1, 1 << 63, 1, 0], repeat=4):
            for leg in mul_legs(list(a), list(b)):
                found.setdefault(leg, (list(a), list(b)))
            if len(found) == 3:
                return found
    return found


def zero_z2_search(rng):
    """inputs (scalar, u) whose final z2 is zero; records how many were tried"""
    hits, tried = [], 0
    orig = X.invert

    def spy(a):
        if X.is_zero(a):
            spy.zero = True
        return orig(a)
    X.invert = spy
    try:
        cands = [bytes([v] + [0] * 31) for v in range(SEARCH_U)] + [X.to_bytes(X.P), X.to_bytes([X.P[0] + 1] + X.P[1:])]
        for u in cands:
            s = bytes(rng.getrandbits(8) for _ in range(32))
            spy.zero = False
            X.x25519(s, u)
            tried += 1
            if spy.zero:
                hits.append((s, u))
    finally:
        X.invert = orig
    return hits, tried


def main():
    rng = random.Random(25519)
    legs = leg_operands()
    assert set(legs) == {"c1", "c3", "f2"}, legs
    field = []
    for leg, (a, b) in sorted(legs.items()):
        field.append({"op": 2, "a": a, "b": b, "legs": [leg], "expect": X.mul(a, b)})
    crafted = [[0] * 4, [1, 0, 0, 0], X.P, [M] * 4, [M - 18, M, M, (1 << 63) - 1], [0, 0, 0, 1 << 63], [M, 0, M, 0]]
    for a in crafted:
        for b in crafted:
            for op in range(5):
                field.append({"op": op, "a": a, "b": b, "legs": [], "expect": X.FIELD_OPS[op](a, b)})
    for _ in range(200):
        a = [rng.getrandbits(64) for _ in range(4)]
        b = [rng.getrandbits(64) for _ in range(4)]
        op = rng.randrange(5)
        field.append({"op": op, "a": a, "b": b, "legs": [], "expect": X.FIELD_OPS[op](a, b)})

    def rb():
        return bytes(rng.getrandbits(8) for _ in range(32))
    xs = [("scalar_two", bytes([2] + [0] * 31), rb()), ("u_zero", rb(), bytes(32)),
          ("u_top_bit", rb(), bytes(31) + b"\x80"), ("u_all_ones", rb(), b"\xff" * 32),
          ("u_is_p", rb(), X.to_bytes(X.P)), ("u_p_plus_5", rb(), X.to_bytes([X.P[0] + 5] + X.P[1:])),
          ("u_nine", rb(), X.to_bytes([9, 0, 0, 0])), ("scalar_zero", bytes(32), X.to_bytes([9, 0, 0, 0])),
          ("scalar_ones", b"\xff" * 32, rb())]
    hits, tried = zero_z2_search(rng)
    for s, u in hits[:2]:
        xs.append(("z2_zero", s, u))
    for i in range(40):
        xs.append(("random", rb(), rb()))
    x25519 = [{"family": f, "scalar": s.hex(), "u": u.hex(), "expect": X.x25519(s, u).hex()} for f, s, u in xs]

    G = ([9, 0, 0, 0], [1, 0, 0, 0])
    ms = [("k_zero", [0] * 4, G), ("k_one", [1, 0, 0, 0], G), ("k_two", [2, 0, 0, 0], G),
          ("k_special_bytes", [0, 0, 0, 2 << 56], G), ("identity", [rng.getrandbits(64) for _ in range(4)], ([5, 0, 0, 0], [0] * 4)),
          ("k_one_unreduced", [1, 0, 0, 0], ([M] * 4, [M] * 4)), ("k_two_unreduced", [2, 0, 0, 0], ([M] * 4, X.P)),
          ("z_is_p", [rng.getrandbits(64) for _ in range(4)], ([7, 0, 0, 0], X.P))]
    for i in range(30):
        ms.append(("random", [rng.getrandbits(64) for _ in range(4)],
                   ([rng.getrandbits(64) for _ in range(4)], [rng.getrandbits(64) for _ in range(4)])))
    multiply = []
    for f, k, (x, z) in ms:
        ox, oz = X.multiply(x, z, k)
        multiply.append({"family": f, "scalar": k, "point": x + z, "expect": ox + oz})
    doc = {"about": "Curve25519 parity vectors (forge-ec-curves/src/curve25519.rs) from tests/x25519_ref.py; "
                    "see tests/golden/gen_x25519.py",
           "field": field, "x25519": x25519, "multiply": multiply,
           "searches": [{"what": "x25519 input with final z2 = 0", "candidates": tried, "hits": len(hits)}]}
    with open(os.path.join(HERE, "x25519_vectors.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
