"""
RIPEMD-160, HASH160, Taproot output keys and CKDpub along a path as a model (include/fecgpu_canon.h: fec_canon_ripemd160,
fec_canon_hash160, fec_canon_pubkey_hash160, fec_canon_taproot_output_key, fec_canon_bip32_derive_pub_path).  hashlib has no
ripemd160 everywhere, so the model carries a pure-Python one, written from the paper's pseudocode; everything else is hashlib
over tests/canon_bip32_ref.py and oracle/canon_model.py.  Each function returns what the library returns: the bytes and a
status, zeros wherever the status is not 0.  Test infrastructure: tests/golden/gen_canon_wallet.py writes the fixture from it,
tests/test_canon_wallet_model.py pins it by published vectors.
"""
import hashlib

import canon_bip32_ref as B
from oracle.canon_model import SECP256K1

OK, BAD_POINT, BAD_SCALAR, NO_KEY, BAD_INDEX, BIP32_INVALID, BAD_RANGE = 0, 2, 3, 8, 9, 10, 4
M32 = 0xFFFFFFFF

# RIPEMD-160, appendix A of the paper: message words r / r', rotations s / s', constants K / K' by round
_R = [list(range(16)),
      [7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8],
      [3, 10, 14, 4, 9, 15, 8, 1, 2, 7, 0, 6, 13, 11, 5, 12],
      [1, 9, 11, 10, 0, 8, 12, 4, 13, 3, 7, 15, 14, 5, 6, 2],
      [4, 0, 5, 9, 7, 12, 2, 10, 14, 1, 3, 8, 11, 6, 15, 13]]
_RP = [[5, 14, 7, 0, 9, 2, 11, 4, 13, 6, 15, 8, 1, 10, 3, 12],
       [6, 11, 3, 7, 0, 13, 5, 10, 14, 15, 8, 12, 4, 9, 1, 2],
       [15, 5, 1, 3, 7, 14, 6, 9, 11, 8, 12, 2, 10, 0, 4, 13],
       [8, 6, 4, 1, 3, 11, 15, 0, 5, 12, 2, 13, 9, 7, 10, 14],
       [12, 15, 10, 4, 1, 5, 8, 7, 6, 2, 13, 14, 0, 3, 9, 11]]
_S = [[11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8],
      [7, 6, 8, 13, 11, 9, 7, 15, 7, 12, 15, 9, 11, 7, 13, 12],
      [11, 13, 6, 7, 14, 9, 13, 15, 14, 8, 13, 6, 5, 12, 7, 5],
      [11, 12, 14, 15, 14, 15, 9, 8, 9, 14, 5, 6, 8, 6, 5, 12],
      [9, 15, 5, 11, 6, 8, 13, 12, 5, 12, 13, 14, 11, 8, 5, 6]]
_SP = [[8, 9, 9, 11, 13, 15, 15, 5, 7, 7, 8, 11, 14, 14, 12, 6],
       [9, 13, 15, 7, 12, 8, 9, 11, 7, 7, 12, 7, 6, 15, 13, 11],
       [9, 7, 15, 11, 8, 6, 6, 14, 12, 13, 5, 14, 13, 13, 7, 5],
       [15, 5, 8, 11, 14, 14, 6, 14, 6, 9, 12, 9, 12, 5, 15, 8],
       [8, 5, 12, 9, 12, 5, 14, 6, 8, 13, 6, 5, 15, 13, 11, 11]]
_K = [0x00000000, 0x5A827999, 0x6ED9EBA1, 0x8F1BBCDC, 0xA953FD4E]
_KP = [0x50A28BE6, 0x5C4DD124, 0x6D703EF3, 0x7A6D76E9, 0x00000000]
_F = [lambda x, y, z: x ^ y ^ z,
      lambda x, y, z: (x & y) | (~x & M32 & z),
      lambda x, y, z: (x | (~y & M32)) ^ z,
      lambda x, y, z: (x & z) | (y & ~z & M32),
      lambda x, y, z: x ^ (y | (~z & M32))]


def _rol(x, n):
    return ((x << n) | (x >> (32 - n))) & M32


def _line(h, X, r, s, k, fs):
    a, b, c, d, e = h
    for rnd in range(5):
        for j in range(16):
            t = (_rol((a + fs[rnd](b, c, d) + X[r[rnd][j]] + k[rnd]) & M32, s[rnd][j]) + e) & M32
            a, e, d, c, b = e, d, _rol(c, 10), b, t
    return a, b, c, d, e


def ripemd160(msg):
    """the 20 digest bytes"""
    msg = bytes(msg)
    data = msg + b"\x80" + bytes((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "little")
    h = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
    for o in range(0, len(data), 64):
        X = [int.from_bytes(data[o + 4 * i:o + 4 * i + 4], "little") for i in range(16)]
        a, b, c, d, e = _line(h, X, _R, _S, _K, _F)
        ap, bp, cp, dp, ep = _line(h, X, _RP, _SP, _KP, _F[::-1])
        h = [(h[1] + c + dp) & M32, (h[2] + d + ep) & M32, (h[3] + e + ap) & M32, (h[4] + a + bp) & M32, (h[0] + b + cp) & M32]
    return b"".join(v.to_bytes(4, "little") for v in h)


def hash160(msg):
    return ripemd160(hashlib.sha256(bytes(msg)).digest())


# ---- Taproot (BIP-341) ---------------------------------------------------------------------------------------------------
TAPTWEAK_TAG = hashlib.sha256(b"TapTweak").digest()


def taptweak(x32, root=None):
    """H_TapTweak(x || root) as 32 bytes; root None: the key-path-only tweak of BIP-86"""
    return hashlib.sha256(TAPTWEAK_TAG + TAPTWEAK_TAG + bytes(x32) + (bytes(root) if root is not None else b"")).digest()


def taproot_output_key(pk, root=None):
    """pk: 32 bytes x-only, or 33 with tag 2 / 3 (then ignored).  (output key x 32 bytes, parity of y, status)"""
    pk = bytes(pk)
    if len(pk) == 33:
        if pk[0] not in (2, 3):
            return bytes(32), 0, BAD_POINT
        pk = pk[1:]
    out, st = B.pubkey_tweak_add(SECP256K1, pk, taptweak(pk, root), 33)
    if st:
        return bytes(32), 0, st
    return out[1:], out[0] & 1, OK


# ---- CKDpub along a path -------------------------------------------------------------------------------------------------
def derive_pub_path(pk33, cc, path):
    """`path` (1..255 indices) from (pk33, cc): (child key 33, chain code 32, fingerprint 4, child HASH160 20, status); the
    status is the first that is not 0 along the chain, everything is zero then.  The fingerprint is that of the last level's
    parent, the four bytes an xpub record of the child carries."""
    assert 1 <= len(path) <= 255
    k, c = bytes(pk33), bytes(cc)
    parent = k
    for index in path:
        parent = k
        k, c, st = B.ckd_pub(k, c, index)
        if st:
            return bytes(33), bytes(32), bytes(4), bytes(20), st
    return k, c, hash160(parent)[:4], hash160(k), OK


def load_fixture(path):
    """tests/golden/canon_wallet_vectors.json (hex throughout; the layout is in tests/golden/gen_canon_wallet.py)"""
    import json
    doc = json.load(open(path))
    hashes = [dict(zip(("len", "msg", "ripemd160", "hash160"), r)) for r in doc["hashes"]]
    taproot = [dict(zip(("class", "name", "pk", "root", "status", "out", "parity"), r)) for r in doc["taproot"]]
    for c in taproot:
        c["root"] = c["root"] or None
        c["out"] = c["out"] or bytes(32).hex()
    path = [dict(zip(("class", "name", "pk", "cc", "indices", "status", "child", "child_cc", "fingerprint", "hash160"), r)) for r in doc["path"]]
    for c in path:
        for k, n in (("child", 33), ("child_cc", 32), ("fingerprint", 4), ("hash160", 20)):
            c[k] = c[k] or bytes(n).hex()
    return {"hashes": hashes, "taproot": taproot, "path": path}
