"""
Test-side restatement of the reference's two Ed25519 EdDSA verifiers from the message
(forge-ec-signature/src/eddsa.rs):
  verify_batch(public_keys, msgs, sigs) -> [status]                  Ed25519Signature::verify               360-447
  eddsa_verify_batch(pk_xy, pk_inf, msgs, r_xy, r_inf, s) -> [status]  EdDsa::<Ed25519, Sha512>::verify       156-212
composed from hashlib.sha512 and an arithmetic backend: PyBackend over oracle/py_model.py (decompress,
ed25519_eddsa_verify, compress; slow -- the fixture generator tests/golden/gen_eddsa_verify.py uses it) or CBackend over
the C oracle (oracle/c_oracle.py: batch_decompress, batch_ed25519_eddsa_verify, batch_compress).  Every function works on
a whole batch so that the C backend can thread the point computation.

Readings (kernels_eddsa.hip pins the same ones):
  * 362-374 / 158-170: msg == "test message" -> true, an empty message -> true, msg == "different message" -> false, in
    that order, before the key or the signature is looked at.
  * 383-394, 404-415: R = from_bytes(0x02 || sig[0..32]), A = from_bytes(0x02 || public_key); None -> false.  Neither has
    a side effect, so the order of the two tests does not show.
  * 398-401: s = the trait Scalar::from_bytes (ed25519.rs:1142-1162): big-endian, always Some.
  * 419-428: k = SHA512(sig[0..32] || public_key || msg)[0..32] -- the 64 bytes as given -- through from_bytes_reduced
    (forge-ec-core/src/lib.rs:320-331), which returns at its first branch: big-endian, unreduced.
  * 174-177: an identity R -> false.  180-193: k = SHA512(to_bytes(R) || to_bytes(pk) || msg)[0..32] with the 33-byte
    trait PointAffine::to_bytes (ed25519.rs:1505-1525; 33 zero bytes for an identity).
  * 196-211 / 431-446: the point computation, which both backends have under the name ed25519_eddsa_verify.
status: 1 true, 0 false, 2 the reference panics (to_affine unwraps the inverse of a zero z, ed25519.rs:1805).
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import py_model as M  # noqa: E402

M64 = (1 << 64) - 1
TEST_MESSAGE = b"test message"            # eddsa.rs:158, 362
DIFFERENT_MESSAGE = b"different message"  # eddsa.rs:168, 372


def from_bytes_be(b):   # trait Scalar::from_bytes (ed25519.rs:1142-1162): big-endian, always Some
    v = int.from_bytes(bytes(b), "big")
    return [(v >> (64 * i)) & M64 for i in range(4)]


def message_case(msg):
    """The three message cases (158-170, 362-374): the status they decide, or None."""
    if msg == TEST_MESSAGE:
        return 1
    if not msg:
        return 1
    if msg == DIFFERENT_MESSAGE:
        return 0
    return None


class PyBackend:
    """oracle/py_model.py: decompress, compress, ed25519_eddsa_verify."""

    def decompress(self, data33):
        """[33 bytes] -> [None, or (x limbs, y limbs, inf)] (PointAffine::from_bytes)."""
        return [M.decompress(M.ED25519, bytes(b)) for b in data33]

    def compress(self, points):
        """[(xy 8 limbs, inf)] -> [33 bytes] (PointAffine::to_bytes)."""
        return [M.compress(M.ED25519, list(xy[:4]), list(xy[4:]), bool(inf)) for xy, inf in points]

    def verify_points(self, items):
        """[(r_xy, r_inf, pk_xy, pk_inf, s, k)] -> [status] from the point computation on."""
        return [M.ed25519_eddsa_verify(list(r), bool(ri), list(p), bool(pi), list(s), list(k)) for r, ri, p, pi, s, k in items]


class CBackend:
    """oracle/c_oracle.py; the point computation threaded."""

    def __init__(self, nthreads=None):
        from oracle import c_oracle as C
        self.C = C
        self.nthreads = nthreads or min(16, os.cpu_count() or 1)

    def decompress(self, data33):
        import numpy as np
        if not len(data33):
            return []
        b = np.frombuffer(b"".join(bytes(x) for x in data33), dtype=np.uint8).reshape(-1, 33)
        xy, inf, ok = self.C.batch_decompress(self.C.ED25519, b)
        return [([int(v) for v in xy[i, :4]], [int(v) for v in xy[i, 4:]], bool(inf[i])) if ok[i] else None
                for i in range(b.shape[0])]

    def compress(self, points):
        import numpy as np
        if not len(points):
            return []
        xy = np.array([[int(v) for v in p[0]] for p in points], dtype=np.uint64).reshape(-1, 8)
        inf = np.array([1 if p[1] else 0 for p in points], dtype=np.uint8)
        return [bytes(r) for r in self.C.batch_compress(self.C.ED25519, xy, inf)]

    def verify_points(self, items):
        import numpy as np
        if not len(items):
            return []
        col = lambda j, w: np.array([[int(v) for v in it[j]] for it in items], dtype=np.uint64).reshape(-1, w)
        flag = lambda j: np.array([1 if it[j] else 0 for it in items], dtype=np.uint8)
        out = self.C.batch_ed25519_eddsa_verify(col(0, 8), flag(1), col(2, 8), flag(3), col(4, 4), col(5, 4), nthreads=self.nthreads)
        return [int(v) for v in out]


def verify_batch(public_keys, msgs, sigs, be):
    """Ed25519Signature::verify per element -> [status]."""
    n = len(msgs)
    out = [message_case(bytes(m)) for m in msgs]
    live = [i for i in range(n) if out[i] is None]
    dec = be.decompress([b"\x02" + bytes(sigs[i])[:32] for i in live] + [b"\x02" + bytes(public_keys[i]) for i in live])   # 383-391, 404-412
    items, where = [], []
    for j, i in enumerate(live):
        R, A = dec[j], dec[len(live) + j]
        if R is None or A is None:                                                       # 392-394, 413-415
            out[i] = 0
            continue
        sig, pk = bytes(sigs[i]), bytes(public_keys[i])
        s = from_bytes_be(sig[32:])                                                      # 398
        k = from_bytes_be(hashlib.sha512(sig[:32] + pk + bytes(msgs[i])).digest()[:32])  # 419-428
        items.append((R[0] + R[1], R[2], A[0] + A[1], A[2], s, k))
        where.append(i)
    for i, st in zip(where, be.verify_points(items)):                                    # 431-446
        out[i] = st
    return out


def eddsa_verify_batch(pk_xy, pk_inf, msgs, r_xy, r_inf, s, be):
    """EdDsa::<Ed25519, Sha512>::verify per element -> [status].  pk_inf / r_inf: sequences of flags, or None."""
    n = len(msgs)
    out = [message_case(bytes(m)) for m in msgs]
    for i in range(n):
        if out[i] is None and r_inf is not None and r_inf[i]:                            # 174-177
            out[i] = 0
    live = [i for i in range(n) if out[i] is None]
    pinf = lambda i: bool(pk_inf is not None and pk_inf[i])
    enc = be.compress([([int(v) for v in r_xy[i]], False) for i in live] + [([int(v) for v in pk_xy[i]], pinf(i)) for i in live])
    items = []
    for j, i in enumerate(live):
        k = from_bytes_be(hashlib.sha512(enc[j] + enc[len(live) + j] + bytes(msgs[i])).digest()[:32])   # 179-193
        items.append(([int(v) for v in r_xy[i]], False, [int(v) for v in pk_xy[i]], pinf(i), [int(v) for v in s[i]], k))
    for i, st in zip(live, be.verify_points(items)):                                     # 196-211
        out[i] = st
    return out
