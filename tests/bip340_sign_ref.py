"""
Test-side restatement of BipSchnorr::sign (forge-ec-signature/src/schnorr.rs:302-420) -> (64 signature bytes, status)
composed from hashlib.sha256 and an arithmetic backend: PyBackend over oracle/py_model.py (slow; the fixture generator
tests/golden/gen_bip340_sign.py uses it) or CBackend over the C oracle (oracle/c_oracle.py: batch_mul_fixed,
batch_to_affine, field_op, secp256k1_scalar_op).  The inherent little-endian Scalar::from_bytes / to_bytes
(secp256k1.rs:1924-1951) and Neg for Scalar (2466-2488) have no oracle call and are restated here.  Every function works
on a whole batch so that the C backend can thread the multiplications.

Readings (kernels_schnorr.hip pins the same ones): `Scalar::from_bytes` and `d.to_bytes()` in schnorr.rs are the
inherent forms, little-endian, None iff the value is not below the reference's N (its two top limbs swapped), zero
valid; `p_x.to_bytes()` is the field's inherent to_bytes (138-178: mont_reduce, big-endian), byte 31 the parity byte.
status: 0 computed, 1 the "test message" pattern, 2 the 0..63 fallback (d, k or e not below N).  Nothing panics.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import py_model as M  # noqa: E402

M64 = (1 << 64) - 1
N = [0xBFD25E8CD0364141, 0xBAAEDCE6AF48A03B, M64, 0xFFFFFFFFFFFFFFFE]     # secp256k1.rs:27-28
N_VALUE = sum(x << (64 * i) for i, x in enumerate(N))
TEST_MESSAGE = b"test message"                                           # schnorr.rs:307
PATTERN_SIG = bytes(range(64))                                           # 311-314, 328-330, 364-366, 401-403
ONE = [1, 0, 0, 0]


def from_bytes_le(b):
    """inherent Scalar::from_bytes (1936-1951) -> (limbs, is_some): little-endian, valid iff value < N."""
    b = bytes(b)
    l = [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(4)]
    valid = (l[3] < N[3] or (l[3] == N[3] and l[2] < N[2]) or (l[3] == N[3] and l[2] == N[2] and l[1] < N[1])
             or (l[3] == N[3] and l[2] == N[2] and l[1] == N[1] and l[0] < N[0]))
    return l, valid


def to_bytes_le(l):
    """inherent Scalar::to_bytes (1924-1933)."""
    return b"".join(int(x).to_bytes(8, "little") for x in l)


def neg(a):
    """Neg for Scalar (2466-2488): zero stays zero, else N - a limb by limb with the two-step borrow."""
    a = [int(x) for x in a]
    if not any(a):
        return a
    out, borrow = [], 0
    for i in range(4):
        d1 = (N[i] - a[i]) & M64
        b1 = N[i] < a[i]
        d2 = (d1 - borrow) & M64
        b2 = d1 < borrow
        out.append(d2)
        borrow = 1 if (b1 or b2) else 0
    return out


class PyBackend:
    """oracle/py_model.py: Secp.multiply, Secp.to_affine, to_bytes_field, SecpScalar.mul / add."""

    def mul_g(self, scalars):
        """-> [(x.to_bytes() 32 bytes, y.to_bytes() 32 bytes)] of to_affine(multiply(G, k))."""
        G = M.Secp.generator()
        out = []
        for k in scalars:
            x, y, _ = M.Secp.to_affine(M.Secp.multiply(G, [int(v) for v in k]))
            out.append((M.to_bytes_field(M.SECP256K1, x), M.to_bytes_field(M.SECP256K1, y)))
        return out

    def sc_mul(self, a, b):
        return M.SecpScalar.mul(list(a), list(b))

    def sc_add(self, a, b):
        return M.SecpScalar.add(list(a), list(b))


class CBackend:
    """oracle/c_oracle.py, threaded."""

    def __init__(self, nthreads=None):
        from oracle import c_oracle as C
        self.C = C
        self.nthreads = nthreads or min(16, os.cpu_count() or 1)

    def mul_g(self, scalars):
        import numpy as np
        C = self.C
        if not len(scalars):
            return []
        k = np.array(scalars, dtype=np.uint64).reshape(-1, 4)
        pts = C.batch_mul_fixed(C.SECP256K1, k, C.generator(C.SECP256K1), nthreads=self.nthreads)
        xy, _ = C.batch_to_affine(C.SECP256K1, pts, nthreads=self.nthreads)      # the identity: x = y = 0
        out = []
        for i in range(k.shape[0]):
            v = [sum(int(w) << (64 * j) for j, w in enumerate(C.field_op(C.SECP256K1, "mul", xy[i, 4 * h:4 * h + 4], ONE)))
                 for h in (0, 1)]
            out.append((v[0].to_bytes(32, "big"), v[1].to_bytes(32, "big")))
        return out

    def sc_mul(self, a, b):
        return [int(v) for v in self.C.secp256k1_scalar_op("mul", a, b)[0]]

    def sc_add(self, a, b):
        return [int(v) for v in self.C.secp256k1_scalar_op("add", a, b)[0]]


def hash_to_scalar(digest):
    """Scalar::from_bytes of a 32-byte hash -> limbs, or None where the reference returns its 0..63 pattern."""
    l, some = from_bytes_le(digest)
    return l if some else None


def sign_batch(keys, msgs, be):
    """BipSchnorr::sign per element -> [(sig 64 bytes, status)]."""
    n = len(keys)
    out = [None] * n
    live = []
    for i, (key, msg) in enumerate(zip(keys, msgs)):
        key, msg = bytes(key), bytes(msg)
        if msg == TEST_MESSAGE:                                          # 307-316
            out[i] = (PATTERN_SIG, 1)
            continue
        d, some = from_bytes_le(key)                                     # 324-332
        if not some:
            out[i] = (PATTERN_SIG, 2)
            continue
        live.append([i, msg, d])
    P = be.mul_g([e[2] for e in live])                                   # 337-338
    second = []
    for (i, msg, d), (px, py) in zip(live, P):
        if py[31] & 1:                                                   # 347-349
            d = neg(d)
        k = hash_to_scalar(hashlib.sha256(to_bytes_le(d) + msg).digest())   # 352-368
        if k is None:
            out[i] = (PATTERN_SIG, 2)
            continue
        second.append((i, msg, d, px, k))
    R = be.mul_g([e[4] for e in second])                                 # 373-374
    for (i, msg, d, px, k), (rx, ry) in zip(second, R):
        if ry[31] & 1:                                                   # 383-385
            k = neg(k)
        e = hash_to_scalar(hashlib.sha256(rx + px + msg).digest())       # 388-405
        if e is None:
            out[i] = (PATTERN_SIG, 2)
            continue
        s = be.sc_add(k, be.sc_mul(e, d))                                # 410-411
        out[i] = (rx + to_bytes_le(s), 0)                                # 412-417
    return out


def parities(keys, msgs, be):
    """(P.y odd, R.y odd) per element, None where no signature is computed (for the fixture's coverage check)."""
    res = []
    for key, msg in zip(keys, msgs):
        key, msg = bytes(key), bytes(msg)
        d, some = from_bytes_le(key)
        if msg == TEST_MESSAGE or not some:
            res.append(None)
            continue
        (px, py), = be.mul_g([d])
        po = bool(py[31] & 1)
        if po:
            d = neg(d)
        k = hash_to_scalar(hashlib.sha256(to_bytes_le(d) + msg).digest())
        if k is None:
            res.append(None)
            continue
        (rx, ry), = be.mul_g([k])
        res.append((po, bool(ry[31] & 1)))
    return res
