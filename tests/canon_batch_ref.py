"""
Batch (random linear combination) verification of BIP-340 and Ed25519 signatures as a model: what
fec_canon_bip340_batch_verify_msg and fec_canon_ed25519_batch_verify_msg compute (include/fecgpu_canon.h),
on hashlib, the big-integer curves of oracle/canon_model.py and the per-signature model of tests/canon_msg_ref.py.  The sum is
formed directly with the model's point arithmetic.  Test infrastructure: tests/gen_canon_batch.py writes
tests/golden/canon_batch_vectors.json from it, tests/test_canon_batch_model.py pins it.

  a_i      = the first 16 bytes, big-endian, of SHA-256(T || T || seed || le64(i)), T = SHA-256("fecgpu/batch-coefficient");
             0 is replaced by 1
  status_i = 3 where s >= the order; else 2 where the key or R does not decode (BIP-340: lift_x fails, r >= p among it;
             Ed25519: RFC 8032 5.1.3); else 0.  (4, a bad message range, is the *_dev forms' alone.)
  BIP-340:   sum a_i R_i + sum (a_i e_i mod n) P_i + (-sum a_i s_i mod n) G == infinity           over the admitted elements
  Ed25519:   8 (sum a_i (-R_i) + sum (a_i h_i mod l) (-A_i) + (sum a_i S_i mod l) B) == (0, 1)     over the admitted elements
"""
import hashlib
import json
import os
import struct

import canon_msg_ref as R
from oracle import canon_model as M

SECP, ED = M.SECP256K1, M.ED25519
TAG = b"fecgpu/batch-coefficient"
SCHEMES = ("bip340", "ed25519")
BAD_POINT, BAD_SCALAR, BAD_RANGE = 2, 3, 4
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canon_batch_vectors.json")
MSG_LENGTHS = (0, 1, 55, 56, 64, 119, 120, 300)   # the SHA-256 and SHA-512 block edges behind a 64-byte prefix, and a long one

_K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_H0 = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def sha256_compress(state, block):
    """FIPS 180-4 section 6.2.2 on one 64-byte block: hashlib shows no midstate, the header's constant needs one"""
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & 0xFFFFFFFF   # noqa: E731
    w = list(struct.unpack(">16I", block))
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & 0xFFFFFFFF)
    a, b, c, d, e, f, g, h = state
    for t in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + _K[t] + w[t]) & 0xFFFFFFFF
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & 0xFFFFFFFF
        a, b, c, d, e, f, g, h = (t1 + t2) & 0xFFFFFFFF, a, b, c, (d + t1) & 0xFFFFFFFF, e, f, g
    return [(x + y) & 0xFFFFFFFF for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def tag_midstate():
    """the SHA-256 state after the block T || T: canon_batch.hpp's after_coefficient_tag"""
    t = hashlib.sha256(TAG).digest()
    return sha256_compress(_H0, t + t)


def coefficient_from_digest(d):
    return int.from_bytes(d[:16], "big") or 1


def coefficient(seed, i):
    t = hashlib.sha256(TAG).digest()
    return coefficient_from_digest(hashlib.sha256(t + t + seed + struct.pack("<Q", i)).digest())


def ones(seed, i):
    """every coefficient 1: the sum without coefficients, for the tests that show what the coefficients are for"""
    return 1


# ---- the two calls ---------------------------------------------------------------------------------
def bip340_batch(msgs, sigs, pks, seed, coeff=coefficient):
    n, C = SECP.N, SECP
    status, acc, gs = [], M.INF, 0
    for i, (msg, sig, pk) in enumerate(zip(msgs, sigs, pks)):
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        P, Rp = R.lift_x(int.from_bytes(pk, "big")), R.lift_x(r)
        st = BAD_SCALAR if s >= n else (BAD_POINT if P is None or Rp is None else 0)
        status.append(st)
        if st:
            continue
        a = coeff(seed, i)
        e = R.bip340_challenge(sig[:32], pk, msg)
        acc = C.add(acc, C.add(C.mul(a, Rp), C.mul(a * e % n, P)))
        gs = (gs + a * s) % n
    acc = C.add(acc, C.mul((-gs) % n, C.G))
    verdict = 1 if acc is M.INF else 0
    return bool(verdict and not any(status)), status, verdict


def ed25519_batch(msgs, sigs, pks, seed, coeff=coefficient, cofactor=8):
    l, E = ED.N, ED
    status, acc, gs = [], E.IDENTITY, 0
    for i, (msg, sig, pk) in enumerate(zip(msgs, sigs, pks)):
        A, Rp = R.ed_decode(pk), R.ed_decode(sig[:32])
        S = int.from_bytes(sig[32:], "little")
        st = BAD_SCALAR if S >= l else (BAD_POINT if A is None or Rp is None else 0)
        status.append(st)
        if st:
            continue
        a = coeff(seed, i)
        h = R.ed25519_challenge(sig[:32], pk, msg)
        acc = E.add(acc, E.add(E.mul(a, E.neg(Rp)), E.mul(a * h % l, E.neg(A))))
        gs = (gs + a * S) % l
    acc = E.mul(cofactor, E.add(acc, E.mul(gs, E.G)))
    verdict = 1 if acc == E.IDENTITY else 0
    return bool(verdict and not any(status)), status, verdict


def batch(scheme, msgs, sigs, pks, seed, **kw):
    return (bip340_batch if scheme == "bip340" else ed25519_batch)(msgs, sigs, pks, seed, **kw)


def single(scheme, msg, sig, pk):
    return R.bip340_verify(msg, sig, pk) if scheme == "bip340" else R.ed25519_verify(msg, sig, pk)


def order(scheme):
    return SECP.N if scheme == "bip340" else ED.N


def s_of(scheme, sig):
    return int.from_bytes(sig[32:], "big" if scheme == "bip340" else "little")


def with_s(scheme, sig, s):
    return sig[:32] + s.to_bytes(32, "big" if scheme == "bip340" else "little")


def cancelling_pair(scheme, sig1, sig2, delta):
    """(s1 + delta, s2 - delta): the sum of the two equations still holds, neither equation does"""
    n = order(scheme)
    return with_s(scheme, sig1, (s_of(scheme, sig1) + delta) % n), with_s(scheme, sig2, (s_of(scheme, sig2) - delta) % n)


def seed_with_odd(label, indices):
    """a seed, found by search from `label`, under which the coefficient of every index in `indices` is odd: a_i T != 0 for a
    torsion point T of any order, so a cofactorless sum refuses such an element for certain and not 7 times in 8"""
    for c in range(1 << 16):
        seed = hashlib.sha256(b"canon-batch-test-seed/" + label.encode() + struct.pack("<I", c)).digest()
        if all(coefficient(seed, i) & 1 for i in indices):
            return seed
    raise AssertionError("no seed found")


def fixed_seed(k):
    return hashlib.sha256(b"canon-batch-fixed-seed/%d" % k).digest()


# ---- the fixture -----------------------------------------------------------------------------------
class Fixture:
    def __init__(self, path=FIXTURE):
        self.doc = json.load(open(path))

    def triples(self, scheme):
        """[(msg, sig, pk)]: valid signatures, by the model"""
        return [tuple(bytes.fromhex(v) for v in row) for row in self.doc[scheme]["valid"]]

    def refused(self, scheme):
        """[(name, msg, sig, pk, status)]: elements the call refuses"""
        return [(c["name"], bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"]), c["status"]) for c in self.doc[scheme]["refused"]]

    def torsion(self):
        """[(name, msg, sig, pk)]: Ed25519 signatures whose defect S B - h A - R is a non-zero torsion point"""
        return [(c["name"], bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"])) for c in self.doc["ed25519"]["torsion"]]

    def tiled(self, scheme, n):
        """n triples: the valid ones over and over (duplicates are legal in a batch; the coefficients differ by index)"""
        t = self.triples(scheme)
        rows = [t[i % len(t)] for i in range(n)]
        return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def load_fixture(path=FIXTURE):
    return Fixture(path)
