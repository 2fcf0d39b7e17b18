"""
Generates tests/golden/ecdsa_sign_vectors.json: Ecdsa::<C, D>::sign fixtures for secp256k1 and P-256 with the digest
and the nonce k given, from the independent Python model oracle/py_model.py (restatement-derived; not
reference-executed).

  python tests/golden/gen_ecdsa_sign.py

The point and scalar arithmetic are py_model's (the curve classes, SecpScalar, P256Scalar, to_bytes_field); the glue
of forge-ec-signature/src/ecdsa.rs:45-71 and 98-211 and the scalar Sub / ct_lt the model lacks are restated literally
below (`sign`), with line citations.

Entries: {"curve", "note", "sk", "digest" (hex), "k", "status", "r", "s"}; status 0 Ok, 1 Err(InvalidPrivateKey),
2 Err(InvalidScalar), 3 Err(InvalidSignature); r = s = one() wherever status != 0.
Per curve: sk in {0, 1, n-1, n, 2^256-1}, k in {0, 1, 2, n-1}, an all-0xFF digest (>= n) and a zero digest, and random
elements.  normalize: secp256k1's half is 0 (its Mul takes invert(2) to zero), so only the `n - s` leg is reachable;
P-256's trait-default ct_lt compares top bytes against half's 0x2C, and both legs appear.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import py_model as M  # noqa: E402

W = 1 << 256
M64 = (1 << 64) - 1
ONE = [1, 0, 0, 0]


def limbs(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def val(l):
    return sum(int(x) << (64 * i) for i, x in enumerate(l))


def _is_zero(a):
    return val(a) == 0


def order(curve):
    return list(M.SecpScalar.N) if curve == 0 else limbs(M.P256Scalar.N)


def ct_lt(curve, a, b):
    """secp256k1: the override (secp256k1.rs:2323-2347), limbs MS -> LS; P-256: the trait default
    (forge-ec-core/src/lib.rs:497-531)."""
    if curve == 1:
        return M.P256Scalar.ct_lt_default(a, b)
    result, eq_so_far = False, True
    for i in (3, 2, 1, 0):
        lt, gt = a[i] < b[i], a[i] > b[i]
        result = result or (eq_so_far and lt)
        eq_so_far = eq_so_far and not lt and not gt
    return result


def sub(curve, a, b):
    """Sub for Scalar: secp256k1.rs:2380-2408 (on a borrow N is added, its carry dropped); p256.rs:1377-1408 (where
    self < rhs, `result += n` through AddAssign = Add (1466-1470, 1352-1375), then the difference, borrow dropped)."""
    n = order(curve)
    if curve == 0:
        d = val(a) - val(b)
        if d < 0:
            d = (d + W + val(n)) % W
        return limbs(d)
    r = list(a)
    if val(a) < val(b):
        r = M.P256Scalar.add(a, n)
    return limbs((val(r) - val(b)) % W)


def scalar_ops(curve):
    S = M.SecpScalar if curve == 0 else M.P256Scalar
    return S.mul, S.add, S.inv, S.from_bytes_be


def half(curve):
    """get_order() / Scalar::from(2): Div (secp256k1.rs:2552-2564, p256.rs:1196-1207) = N * invert(2).unwrap()."""
    mul, _, inv, _ = scalar_ops(curve)
    i2 = inv([2, 0, 0, 0])
    assert i2 is not None      # Div's unwrap sees Some
    return mul(order(curve), i2)


def sign(curve, sk, digest, k, legs=None):
    """sign_internal + sign (ecdsa.rs:98-211) with h_bytes = digest and k = the nonce.  -> (status, r, s).  `legs`
    (a set, optional) receives which leg of normalize ran: True where s was kept."""
    F = M.Secp if curve == 0 else M.P256c
    mul, add, inv, from_bytes = scalar_ops(curve)
    n = order(curve)
    if _is_zero(sk) or not ct_lt(curve, sk, n):                       # 101-104
        return 1, ONE, ONE
    x, _, _ = F.to_affine(F.multiply(F.generator(), list(k)))        # 110-112 (identity: x = 0, never unwrapped)
    r, ok = from_bytes(list(M.to_bytes_field(curve, x)))              # 114-124
    if not ok:                                                        # 126-129
        return 2, ONE, ONE
    if _is_zero(r):                                                   # 131-134
        return 3, ONE, ONE
    h, ok = from_bytes(list(digest))                                  # 147
    if not ok:                                                        # 149-154
        return 2, ONE, ONE
    k_inv = inv(list(k))                                              # 157
    if k_inv is None:                                                 # 159-164
        return 3, ONE, ONE
    s = mul(k_inv, add(h, mul(r, list(sk))))                          # 166-169
    if _is_zero(s):                                                   # 172-177
        return 3, ONE, ONE
    keep = ct_lt(curve, s, half(curve))                               # normalize, 45-71
    if legs is not None:
        legs.add(keep)
    if not keep:
        s = sub(curve, n, s)
    return 0, list(r), list(s)


def main():
    rng = random.Random(0x5161)
    out = {"provenance": "restatement-derived by oracle/py_model.py; not reference-executed", "cases": []}
    for curve in (0, 1):
        nv = val(order(curve))
        good_sk, good_k = limbs(rng.randrange(1, nv)), limbs(rng.randrange(1, nv))

        def digest():
            return bytes(rng.randrange(256) for _ in range(32))

        legs = set()

        def emit(sk, d, k, note):
            st, r, s = sign(curve, sk, d, k, legs)
            out["cases"].append({"curve": curve, "note": note, "sk": [int(v) for v in sk], "digest": d.hex(),
                                 "k": [int(v) for v in k], "status": st, "r": [int(v) for v in r], "s": [int(v) for v in s]})
            return st

        for name, v in (("0", 0), ("1", 1), ("n-1", nv - 1), ("n", nv), ("2^256-1", W - 1)):
            emit(limbs(v), digest(), good_k, "sk = " + name)
        for name, v in (("0", 0), ("1", 1), ("2", 2), ("n-1", nv - 1)):
            emit(good_sk, digest(), limbs(v), "k = " + name)
        emit(good_sk, b"\xff" * 32, good_k, "digest all 0xFF (>= n)")
        emit(good_sk, bytes(32), good_k, "zero digest")
        for j in range(24):
            emit(limbs(rng.randrange(1, nv)), digest(), limbs(rng.randrange(1, nv)), "random")
        # secp256k1 always takes n - s (half is 0); P-256 keeps s where top_byte(s) <= 0x2C
        assert legs == ({False} if curve == 0 else {True, False}), (curve, legs)
    with open(os.path.join(HERE, "ecdsa_sign_vectors.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
