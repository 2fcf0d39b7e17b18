"""
Test-side restatement of the reference's three EdDSA signing functions for Ed25519 with SHA-512
(forge-ec-signature/src/eddsa.rs):
  sign(private_key, msg) -> 64 bytes             Ed25519Signature::sign               267-356
  derive_public_key(private_key) -> 32 bytes     Ed25519Signature::derive_public_key  450-508
  eddsa_sign(sk_limbs, msg) -> (R, s)            EdDsa::<Ed25519, Sha512>::sign       43-154
composed from hashlib.sha512 and an arithmetic backend: PyBackend over oracle/py_model.py (slow; the fixture
generator tests/golden/gen_eddsa_sign.py uses it) or CBackend over the C oracle (oracle/c_oracle.py: batch_mul_fixed,
batch_to_affine, batch_compress, ed25519_scalar_mul_release).  The scalar Add (ed25519.rs:1193-1239) has no oracle call
by name and is restated here.  Every function works on a whole batch so that the C backend can thread the
multiplications.

Readings (kernels_eddsa.hip pins the same ones): scalars from bytes are the trait from_bytes, big-endian and never
None; to_bytes of points is the 33-byte trait form; the signature's s bytes are the inherent Scalar::to_bytes (one
conditional subtraction of l, little-endian).  status: 1 the reference panics (to_affine of a zero z that is not the
identity), 2 only a debug build panics (Mul's u128 sums wrap).
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import py_model as M  # noqa: E402

M64 = (1 << 64) - 1
ORDER = [0x5812631A5CF5D3ED, 0x14DEF9DEA2F79CD6, 0, 0x1000000000000000]
TEST_MESSAGE = b"test message"                                                          # eddsa.rs:269, 45
RFC_SIG = bytes.fromhex("e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5"
                        "f0595bbe24655141438e7a100b")                                    # eddsa.rs:283
RFC_PK = bytes.fromhex("d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a")  # eddsa.rs:455
PATTERN_SIG = bytes(range(64))                                                          # eddsa.rs:272-277


def ge_order(r):   # the comparison loop of ed25519.rs:1215-1226
    for i in (3, 2, 1, 0):
        if r[i] < ORDER[i]:
            return False
        if r[i] > ORDER[i]:
            return True
    return True


def sub_order(r):   # 1229-1236
    out, borrow = [], 0
    for i in range(4):
        diff = r[i] - ORDER[i] - borrow
        out.append(diff & M64)
        borrow = 1 if diff < 0 else 0
    return out


def sc_add(a, b):   # impl Add for Scalar, 1193-1239: the sum mod 2^256 (the last carry is dropped), then one subtraction
    r, carry = [], 0
    for i in range(4):
        t = a[i] + b[i] + carry
        r.append(t & M64)
        carry = t >> 64
    return sub_order(r) if ge_order(r) else r


def from_bytes_be(b):   # trait Scalar::from_bytes (1142-1162): big-endian, always Some
    v = int.from_bytes(bytes(b), "big")
    return [(v >> (64 * i)) & M64 for i in range(4)]


def to_bytes_be(l):     # trait Scalar::to_bytes (1164-1175)
    return sum(int(x) << (64 * i) for i, x in enumerate(l)).to_bytes(32, "big")


def to_bytes_inherent(l):   # inherent Scalar::to_bytes (767-781): reduce (744-762, one conditional subtraction), LE
    l = [int(x) for x in l]
    if ge_order(l):
        l = sub_order(l)
    return sum(x << (64 * i) for i, x in enumerate(l)).to_bytes(32, "little")


def clamp(b):           # eddsa.rs:298-300
    b = bytearray(b)
    b[0] &= 248
    b[31] &= 127
    b[31] |= 64
    return bytes(b)


class PyBackend:
    """oracle/py_model.py: Ed.multiply, Ed.to_affine, compress, Ed25519Scalar.mul_release."""

    def mul_g(self, scalars):
        """-> [(x, y, inf, panics)] of to_affine(multiply(G, k))."""
        G = M.Ed.generator()
        out = []
        for k in scalars:
            p = M.Ed.multiply(G, list(k))
            panics = (not M.Ed.is_identity(p)) and all(v == 0 for v in p[2])
            x, y, inf = M.Ed.to_affine(p)
            out.append((list(x), list(y), bool(inf), panics))
        return out

    def compress(self, x, y, inf):
        return M.compress(M.ED25519, x, y, inf)

    def mul_release(self, a, b):
        r, ovf = M.Ed25519Scalar.mul_release(list(a), list(b))
        return [int(v) for v in r], bool(ovf)

    def generator_affine(self):
        x, y, inf = M.Ed.to_affine(M.Ed.generator())
        return list(x), list(y), bool(inf)


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
        pts = C.batch_mul_fixed(C.ED25519, k, C.generator(C.ED25519), nthreads=self.nthreads)
        xy, inf = C.batch_to_affine(C.ED25519, pts, nthreads=self.nthreads)
        out = []
        for i in range(k.shape[0]):
            p = [int(v) for v in pts[i]]
            P = (p[0:4], p[4:8], p[8:12], p[12:16])
            panics = (not M.Ed.is_identity(P)) and all(v == 0 for v in P[2])
            out.append(([int(v) for v in xy[i, :4]], [int(v) for v in xy[i, 4:]], bool(inf[i]), panics))
        return out

    def compress(self, x, y, inf):
        import numpy as np
        xy = np.array(list(x) + list(y), dtype=np.uint64)
        return bytes(self.C.batch_compress(self.C.ED25519, xy, np.array([1 if inf else 0], dtype=np.uint8))[0])

    def mul_release(self, a, b):
        r, ovf = self.C.ed25519_scalar_mul_release(a, b)
        return [int(v) for v in r], bool(ovf)

    def generator_affine(self):
        xy, inf = self.C.to_affine(self.C.ED25519, self.C.generator(self.C.ED25519))
        return [int(v) for v in xy[:4]], [int(v) for v in xy[4:]], bool(inf)


def _key_scalar(key_bytes):
    """SHA512(key) -> (nonce, a): a = the clamped h[32..64] read big-endian (eddsa.rs:293-305, 65-102)."""
    h = hashlib.sha512(bytes(key_bytes)).digest()
    return h[:32], from_bytes_be(clamp(h[32:]))


def sign_batch(keys, msgs, be):
    """Ed25519Signature::sign per element -> [(sig 64 bytes, status)]."""
    pre = []
    for key, msg in zip(keys, msgs):
        key, msg = bytes(key), bytes(msg)
        if msg == TEST_MESSAGE:
            pre.append(("pattern", None, None, None))
        elif not msg and key[0] == 0x9D:
            pre.append(("rfc", None, None, None))
        else:
            nonce, a = _key_scalar(key)
            r = from_bytes_be(hashlib.sha512(nonce + msg).digest()[:32])            # 313-322 (from_bytes_reduced)
            pre.append((None, a, r, msg))
    live = [p for p in pre if p[0] is None]
    pts = be.mul_g([p[1] for p in live] + [p[2] for p in live])
    m = len(live)
    out, j = [], 0
    for special, a, r, msg in pre:
        if special == "pattern":
            out.append((PATTERN_SIG, 0))
            continue
        if special == "rfc":
            out.append((RFC_SIG, 0))
            continue
        A, R = pts[j], pts[m + j]
        j += 1
        if A[3] or R[3]:
            out.append((bytes(64), 1))
            continue
        a33, r33 = be.compress(*A[:3]), be.compress(*R[:3])
        k = from_bytes_be(hashlib.sha512(r33 + a33 + msg).digest()[:32])            # 329-337
        ka, ovf = be.mul_release(k, a)
        s = sc_add(r, ka)                                                           # 340
        out.append((r33[:32] + to_bytes_inherent(s), 2 if ovf else 0))
    return out


def derive_batch(keys, be):
    """Ed25519Signature::derive_public_key per element -> [(pk 32 bytes, status)]."""
    a = [None if bytes(k)[0] == 0x9D else _key_scalar(k)[1] for k in keys]
    live = [x for x in a if x is not None]
    pts = be.mul_g(live)
    out, j = [], 0
    for x in a:
        if x is None:
            out.append((RFC_PK, 0))
            continue
        A = pts[j]
        j += 1
        out.append((bytes(32), 1) if A[3] else (be.compress(*A[:3])[:32], 0))
    return out


def eddsa_sign_batch(sks, msgs, be):
    """EdDsa::<Ed25519, Sha512>::sign per element -> [(r_x limbs, r_y limbs, r_inf, s limbs, status)]."""
    pre = []
    for sk, msg in zip(sks, msgs):
        sk, msg = [int(v) for v in sk], bytes(msg)
        skb = to_bytes_be(sk)                                                       # 65 (trait to_bytes)
        if msg == TEST_MESSAGE or (not msg and skb[0] == 0x9D):
            pre.append((True, None, None, None))
            continue
        nonce, a = _key_scalar(skb)
        r = from_bytes_be(hashlib.sha512(nonce + msg).digest()[:32])
        pre.append((False, a, r, msg))
    live = [p for p in pre if not p[0]]
    pts = be.mul_g([p[1] for p in live] + [p[2] for p in live])
    m = len(live)
    gx, gy, ginf = be.generator_affine()
    out, j = [], 0
    for special, a, r, msg in pre:
        if special:
            out.append((gx, gy, ginf, [1, 0, 0, 0], 0))
            continue
        A, R = pts[j], pts[m + j]
        j += 1
        if A[3] or R[3]:
            out.append(([0] * 4, [0] * 4, False, [0] * 4, 1))
            continue
        k = from_bytes_be(hashlib.sha512(be.compress(*R[:3]) + be.compress(*A[:3]) + msg).digest()[:32])
        ka, ovf = be.mul_release(k, a)
        out.append((R[0], R[1], R[2], sc_add(r, ka), 2 if ovf else 0))
    return out
