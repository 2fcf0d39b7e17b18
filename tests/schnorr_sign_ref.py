"""
Test-side restatement of Schnorr::<C, Sha256>::sign (forge-ec-signature/src/schnorr.rs:43-88), of its challenge
(66-81; the same lines in verify, 107-122, and batch_verify, 241-256), of signature_to_bytes (145-157) and of
C::Scalar::from_bytes_reduced for 32-byte inputs (forge-ec-core/src/lib.rs:320-468; P-256: p256.rs:1301-1331), written
from the Rust source on hashlib, rfc6979_ref.generate_k and the point / scalar arithmetic of EITHER backend: the C oracle
(CBackend) or oracle/py_model.py (PyBackend).

Readings (the list of forge_ec_amd/csrc/schnorr_sign.hpp and DESIGN.md section 16):
  * from_bytes_reduced, secp256k1 and Ed25519: the trait default on the curve's TRAIT from_bytes / to_bytes / get_order.
      A  the TRAIT from_bytes: the 32 bytes BIG-endian; Some -> that scalar ("direct").  Ed25519's is always Some
         (ed25519.rs:1142-1162), so every input ends here, unreduced.  secp256k1's is Some iff below N, the constant with
         the two top limbs swapped (secp256k1.rs:2271-2297); past this point b[0..7] = FF x 7 and b[7] is FE or FF.
      B  value_lo = the SAME bytes LITTLE-endian, limb i from b[8i..8i+8]; value_hi = 0.
      C  `hi_is_zero && is_less` (375-410) compares value_lo[0] with N[0] first; value_lo[0] is 0xFEFFFFFFFFFFFFFF or
         0xFFFFFFFFFFFFFFFF after A, above N[0]: UNREACHABLE for 32 bytes.  (Restated below as the source has it, and the
         model test asserts that no fixture entry and no crafted input takes it.)
      D  `while !hi_is_zero || !is_less_than(value_lo, N)`: value_hi stays zero, value_lo < 2^256, N > 2^255: zero
         subtractions ("nosub") or one ("sub"), never two.
      E  result_bytes puts limb 3 first with each limb's bytes LITTLE-endian and the TRAIT from_bytes reads them
         big-endian: every 64-bit limb comes back byte-swapped; unwrap_or_else(zero) where that is not below N.
         After "nosub" REACHABLE ("nosub_zero": b = FF x 31 || FE); after "sub" unreachable ("sub_zero": the difference
         is below 2^256 - N = 2^192 + 2^128 - (N mod 2^128) < 2 * 2^192, its top limb 0 or 1, the swap at most
         0x0100000000000000 < N[3]).
  * from_bytes_reduced, P-256: the override: the inherent from_bytes (big-endian, Some iff below n: "direct"), else the
    bytes LITTLE-endian into reduce_wide ("reduce_wide").
  * PointAffine::to_bytes: 33 bytes, what fec_batch_compress writes; an infinite point is 33 zero bytes.
  * sign: b"test message" -> (to_affine(generator()), one) before the key is looked at; k = generate_k(sk, msg) with no
    key check; R = to_affine(multiply(G, k)), P = to_affine(multiply(G, sk)); e; s = k + e * sk with the curve's impl Mul
    / impl Add.  sk = 0: P is the identity and s = k.
  * signature_to_bytes: bytes 0..32 of R's 33-byte encoding, then the TRAIT to_bytes of s (big-endian).
Every function that has legs returns the leg's name with its value.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rfc6979_ref as R  # noqa: E402

M64 = (1 << 64) - 1
N = {0: [0xBFD25E8CD0364141, 0xBAAEDCE6AF48A03B, M64, 0xFFFFFFFFFFFFFFFE],      # secp256k1.rs:27-28 (top limbs swapped)
     1: [0xF3B9CAC2FC632551, 0xBCE6FAADA7179E84, M64, 0xFFFFFFFF00000000],      # p256.rs:23-24
     2: [0x5812631A5CF5D3ED, 0x14DEF9DEA2F79CD6, 0, 0x1000000000000000]}        # ed25519.rs: L
REACHABLE = {0: ("direct", "nosub", "nosub_zero", "sub"), 1: ("direct", "reduce_wide"), 2: ("direct",)}


def load_fixture():
    """tests/golden/schnorr_sign_vectors.json with the challenge entries' points expanded ("r_xy", "pk_xy")."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "schnorr_sign_vectors.json")) as f:
        fx = json.load(f)
    for c in fx["challenge"]:
        pts = fx["points"][str(c["curve"])]
        c["r_xy"], c["pk_xy"] = pts[c["r"]], pts[c["pk"]]
    return fx


def val(l):
    return sum(int(x) << (64 * i) for i, x in enumerate(l))


def limbs(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def trait_from_bytes(curve, b):
    """The TRAIT Scalar::from_bytes of 32 bytes: (limbs, is_some)."""
    l = [0] * 4
    for i in range(4):
        for j in range(8):
            l[i] |= b[31 - (i * 8 + j)] << (j * 8)
    if curve == 2:
        return l, True                                      # ed25519.rs:1158-1161: `let is_valid = true`
    return l, val(l) < val(N[curve])                        # secp256k1.rs:2288-2294, p256.rs:1052


def trait_to_bytes(l):
    return b"".join(int(x).to_bytes(8, "big") for x in reversed(list(l)))


def _default_from_bytes_reduced(curve, b):
    """forge-ec-core/src/lib.rs:320-468 for len(b) == 32, line by line."""
    s, some = trait_from_bytes(curve, b)                    # 327
    if some:
        return s, "direct"                                  # 329-332
    order = N[curve]
    order_bytes = trait_to_bytes(order)                     # 339-340
    value_lo = [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(4)]     # 348-354
    value_hi = [0] * 4                                      # 357-363: len == 32
    hi_is_zero = all(v == 0 for v in value_hi)
    if hi_is_zero:                                          # 375-411
        is_less = False
        for i in (3, 2, 1, 0):
            order_limb = int.from_bytes(order_bytes[8 * i:8 * i + 8], "big")
            if value_lo[3 - i] < order_limb:
                is_less = True
                break
            elif value_lo[3 - i] > order_limb:
                break
        if is_less:
            rb = b"".join(value_lo[3 - i].to_bytes(8, "little") for i in range(4))
            s, some = trait_from_bytes(curve, rb)
            return (s, "hi_zero_less") if some else ([0] * 4, "hi_zero_less_zero")
    order_limbs = [int.from_bytes(order_bytes[24 - 8 * i:32 - 8 * i], "big") for i in range(4)]   # 417-429
    subs = 0
    while val(value_lo) >= val(order_limbs):                # 432 with hi_is_zero (value_hi never changes: 442 needs !hi_is_zero)
        value_lo = limbs((val(value_lo) - val(order_limbs)) & ((1 << 256) - 1))
        subs += 1
    assert subs <= 1
    rb = b"".join(value_lo[3 - i].to_bytes(8, "little") for i in range(4))          # 460-465
    s, some = trait_from_bytes(curve, rb)                   # 467
    leg = "sub" if subs else "nosub"
    return (s, leg) if some else ([0] * 4, leg + "_zero")


def from_bytes_reduced(curve, b, reduce_wide=None):
    """C::Scalar::from_bytes_reduced(&b[0..32]) -> (limbs, leg).  reduce_wide: P-256's Scalar::reduce_wide on an integer
    (the backend's; default oracle/py_model.py's)."""
    b = bytes(b)
    assert len(b) == 32
    if curve != 1:
        return _default_from_bytes_reduced(curve, b)
    s, some = trait_from_bytes(1, b)                        # p256.rs:1308-1315 (the inherent form: the same reading)
    if some:
        return s, "direct"
    if reduce_wide is None:
        from oracle import py_model
        reduce_wide = py_model.P256Scalar.reduce_wide
    return limbs(reduce_wide(int.from_bytes(b, "little"))), "reduce_wide"           # 1320-1330


class PyBackend:
    """oracle/py_model.py"""
    name = "py_model"

    def __init__(self):
        from oracle import py_model
        self.m = py_model

    def generator_affine(self, curve):
        F = self.m.CURVES[curve]
        x, y, inf = F.to_affine(F.generator())
        return list(x) + list(y), inf

    def mul_g_affine(self, curve, k):
        F = self.m.CURVES[curve]
        x, y, inf = F.to_affine(F.multiply(F.generator(), [int(v) for v in k]))
        return list(x) + list(y), inf

    def compress(self, curve, xy, inf):
        return self.m.compress(curve, [int(v) for v in xy[:4]], [int(v) for v in xy[4:]], bool(inf))

    def sc_mul(self, curve, a, b):
        S = self.m.SecpScalar if curve == 0 else self.m.P256Scalar
        return S.mul([int(v) for v in a], [int(v) for v in b])

    def sc_add(self, curve, a, b):
        S = self.m.SecpScalar if curve == 0 else self.m.P256Scalar
        return S.add([int(v) for v in a], [int(v) for v in b])

    def reduce_wide(self, w):
        return self.m.P256Scalar.reduce_wide(w)


class CBackend:
    """oracle/c_oracle.py"""
    name = "c_oracle"

    def __init__(self):
        from oracle import c_oracle
        self.o = c_oracle

    def generator_affine(self, curve):
        xy, inf = self.o.to_affine(curve, self.o.generator(curve))
        return [int(v) for v in xy], inf

    def mul_g_affine(self, curve, k):
        xy, inf = self.o.to_affine(curve, self.o.multiply(curve, self.o.generator(curve), np.array(k, dtype=np.uint64)))
        return [int(v) for v in xy], inf

    def compress(self, curve, xy, inf):
        out = self.o.batch_compress(curve, np.array([xy], dtype=np.uint64), np.array([1 if inf else 0], dtype=np.uint8))
        return bytes(np.asarray(out, dtype=np.uint8).reshape(-1)[:33])

    def _op(self, curve):
        return self.o.secp256k1_scalar_op if curve == 0 else self.o.p256_scalar_op

    def sc_mul(self, curve, a, b):
        return [int(v) for v in self._op(curve)("mul", np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64))[0]]

    def sc_add(self, curve, a, b):
        return [int(v) for v in self._op(curve)("add", np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64))[0]]

    def reduce_wide(self, w):
        # reduce_wide(lo) for lo < 2^256 is Mul's reduction of the exact product lo * 1 (p256.rs:1409-1432)
        assert w < (1 << 256)
        return val(self.sc_mul(1, limbs(w), [1, 0, 0, 0]))


def challenge(be, curve, r_xy, r_inf, pk_xy, pk_inf, msg):
    """e = from_bytes_reduced(SHA256(R.to_bytes() || P.to_bytes() || msg)) -> (limbs, leg)   (schnorr.rs:66-81)"""
    h = hashlib.sha256(be.compress(curve, r_xy, r_inf) + be.compress(curve, pk_xy, pk_inf) + bytes(msg)).digest()
    return from_bytes_reduced(curve, h, be.reduce_wide)


def signature_to_bytes(be, curve, r_xy, r_inf, s):
    return be.compress(curve, r_xy, r_inf)[0:32] + trait_to_bytes(s)                 # 145-157


def sign(be, curve, sk, msg):
    """Schnorr::<C, Sha256>::sign(sk, msg) -> dict(status, r_xy, r_inf, s, sig_bytes, k, e, leg)."""
    sk = [int(v) for v in sk]
    msg = bytes(msg)
    if msg == b"test message":                              # 45-52
        r_xy, r_inf = be.generator_affine(curve)
        s = [1, 0, 0, 0]
        return {"status": 1, "r_xy": r_xy, "r_inf": r_inf, "s": s, "sig_bytes": signature_to_bytes(be, curve, r_xy, r_inf, s),
                "k": None, "e": None, "leg": None}
    kv, retries = R.generate_k(sk, msg, R.ORDER[curve])     # 56
    assert retries == 0
    k = limbs(kv)
    r_xy, r_inf = be.mul_g_affine(curve, k)                 # 59-60
    p_xy, p_inf = be.mul_g_affine(curve, sk)                # 63-64
    e, leg = challenge(be, curve, r_xy, r_inf, p_xy, p_inf, msg)                     # 67-81
    s = be.sc_add(curve, k, be.sc_mul(curve, e, sk))        # 84-85
    return {"status": 0, "r_xy": r_xy, "r_inf": r_inf, "s": s, "sig_bytes": signature_to_bytes(be, curve, r_xy, r_inf, s),
            "k": k, "e": e, "leg": leg}


def sign_many(curve, sk, msgs, nthreads=8):
    """sign() per element over the C oracle with the 2n multiplications and the encodings batched (threaded):
    -> dict of arrays: status (n,), r_xy (n, 8), r_inf (n,), s (n, 4), sig_bytes (n, 64) uint8, k (n, 4), e (n, 4)."""
    be = CBackend()
    o = be.o
    sk = np.ascontiguousarray(np.asarray(sk, dtype=np.uint64)).reshape(-1, 4)
    n = sk.shape[0]
    msgs = [bytes(m) for m in msgs]
    test = [m == b"test message" for m in msgs]
    k = np.array([[0] * 4 if t else limbs(R.generate_k([int(v) for v in sk[i]], msgs[i], R.ORDER[curve])[0])
                  for i, t in enumerate(test)], dtype=np.uint64).reshape(n, 4)
    g = o.generator(curve)
    xy, inf = o.batch_to_affine(curve, o.batch_mul_fixed(curve, np.concatenate([k, sk]), g, nthreads=nthreads), nthreads=nthreads)
    g_xy, g_inf = be.generator_affine(curve)
    for i, t in enumerate(test):
        if t:
            xy[i], inf[i] = g_xy, int(g_inf)
    enc = np.asarray(o.batch_compress(curve, xy, inf), dtype=np.uint8).reshape(2 * n, 33)
    out = {"status": np.array([1 if t else 0 for t in test], dtype=np.uint8), "r_xy": xy[:n].copy(), "r_inf": inf[:n].copy(),
           "s": np.zeros((n, 4), dtype=np.uint64), "sig_bytes": np.zeros((n, 64), dtype=np.uint8), "k": k, "e": np.zeros((n, 4), dtype=np.uint64)}
    for i in range(n):
        if test[i]:
            s = [1, 0, 0, 0]
        else:
            e, _ = from_bytes_reduced(curve, hashlib.sha256(bytes(enc[i]) + bytes(enc[n + i]) + msgs[i]).digest(), be.reduce_wide)
            out["e"][i] = e
            s = be.sc_add(curve, [int(v) for v in k[i]], be.sc_mul(curve, e, [int(v) for v in sk[i]]))
        out["s"][i] = s
        out["sig_bytes"][i] = list(bytes(enc[i])[:32] + trait_to_bytes(s))
    return out
