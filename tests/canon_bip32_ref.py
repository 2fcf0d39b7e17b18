"""
EC tweak-add and BIP-32 child key derivation as a model (include/fecgpu_canon.h: fec_canon_pubkey_tweak_add,
fec_canon_seckey_tweak_add, fec_canon_bip32_derive_pub, fec_canon_bip32_derive_priv): hmac / hashlib.sha512 and the
big-integer curves SECP256K1 / P256 of oracle/canon_model.py, nothing else.  Each function returns what the library returns:
the bytes and a status, zeros wherever the status is not 0.  Test infrastructure: tests/golden/gen_canon_bip32.py writes the
fixture from it, tests/test_canon_bip32_model.py pins it by BIP-32 test vector 1 and by properties.
"""
import hashlib
import hmac

from oracle.canon_model import INF, P256, SECP256K1

CURVES = {"secp256k1": SECP256K1, "p256": P256}
CURVE_IDS = {"secp256k1": 0, "p256": 1, "ed25519": 2}
OK, BAD_POINT, BAD_SCALAR, BAD_KEY, NO_KEY, BAD_INDEX, BIP32_INVALID = 0, 2, 3, 6, 8, 9, 10
NO_COMB = 1
HARDENED = 1 << 31


def b32(v):
    return v.to_bytes(32, "big")


def sqrt_mod(C, a):
    """a root of a modulo p (both primes are 3 mod 4), or None"""
    r = pow(a, (C.P + 1) // 4, C.P)
    return r if r * r % C.P == a % C.P else None


def encode(pt, form):
    """a finite point as 33 / 65 bytes of SEC 1, or 32: x alone"""
    x, y = pt
    if form == 32:
        return b32(x)
    if form == 33:
        return bytes([2 + (y & 1)]) + b32(x)
    return b"\x04" + b32(x) + b32(y)


def decode(C, b):
    """SEC 1 section 2.3.4 by the length: 33 (tag 2 / 3), 65 (tag 4, on the curve), 32 (x-only: the even y); None when refused"""
    if len(b) == 65:
        pt = (int.from_bytes(b[1:33], "big"), int.from_bytes(b[33:], "big"))
        return pt if b[0] == 4 and C.on_curve(pt) else None
    tag, xb = (2, b) if len(b) == 32 else (b[0], b[1:])
    x = int.from_bytes(xb, "big")
    if tag not in (2, 3) or x >= C.P:
        return None
    y = sqrt_mod(C, (x * x * x + C.A * x + C.B) % C.P)
    if y is None:
        return None
    return (x, y if (y & 1) == (tag & 1) else (C.P - y) % C.P)


def pubkey_tweak_add(C, pk, tweak, out_len):
    """pk + tweak G: (record of out_len bytes, status)"""
    zeros = bytes(out_len)
    P = decode(C, pk)
    if P is None:
        return zeros, BAD_POINT
    t = int.from_bytes(tweak, "big")
    if t >= C.N:
        return zeros, BAD_SCALAR
    Q = C.add(P, C.mul(t, C.G))
    if Q is INF:
        return zeros, NO_KEY
    return encode(Q, out_len), OK


def seckey_tweak_add(C, key, tweak):
    """(key + tweak) mod n: (32 bytes, status)"""
    k, t = int.from_bytes(key, "big"), int.from_bytes(tweak, "big")
    if not 0 < k < C.N:
        return bytes(32), BAD_KEY
    if t >= C.N:
        return bytes(32), BAD_SCALAR
    r = (k + t) % C.N
    return (b32(r), OK) if r else (bytes(32), NO_KEY)


def hmac512(key, data):
    return hmac.new(key, data, hashlib.sha512).digest()


def ckd_pub_from_il(K, il):
    """the end of CKDpub, IL given: the child point or None"""
    C = SECP256K1
    if il >= C.N:
        return None
    Q = C.add(C.mul(il, C.G), K)
    return None if Q is INF else Q


def ckd_pub(pk33, cc, index):
    """BIP-32 CKDpub on secp256k1: (child key 33 bytes, child chain code, status)"""
    zeros = (bytes(33), bytes(32))
    K = decode(SECP256K1, pk33)
    if K is None:
        return zeros + (BAD_POINT,)
    if index >= HARDENED:
        return zeros + (BAD_INDEX,)
    I = hmac512(cc, encode(K, 33) + index.to_bytes(4, "big"))
    Q = ckd_pub_from_il(K, int.from_bytes(I[:32], "big"))
    if Q is None:
        return zeros + (BIP32_INVALID,)
    return encode(Q, 33), I[32:], OK


def ckd_priv_from_il(k, il):
    """the end of CKDpriv, IL given: the child key or None"""
    n = SECP256K1.N
    if il >= n or (il + k) % n == 0:
        return None
    return (il + k) % n


def ckd_priv(key, cc, index, flags=0):
    """BIP-32 CKDpriv on secp256k1: (child key 32 bytes, child chain code, status)"""
    C = SECP256K1
    zeros = (bytes(32), bytes(32))
    k = int.from_bytes(key, "big")
    if not 0 < k < C.N:
        return zeros + (BAD_KEY,)
    if index >= HARDENED:
        data = b"\x00" + key
    elif flags & NO_COMB:
        return zeros + (BAD_INDEX,)
    else:
        data = encode(C.mul(k, C.G), 33)
    I = hmac512(cc, data + index.to_bytes(4, "big"))
    child = ckd_priv_from_il(k, int.from_bytes(I[:32], "big"))
    if child is None:
        return zeros + (BIP32_INVALID,)
    return b32(child), I[32:], OK


def load_fixture(path):
    """tests/golden/canon_bip32_vectors.json (rows; the layout is in tests/golden/gen_canon_bip32.py) as lists of cases:
    "tweak": class, name, curve, key, tweak, status and, where the status is 0, out33; "seckey": ... key, tweak, status, out;
    "bip32_pub": ... pk, cc, index, status, child, child_cc; "bip32_priv": ... key, cc, index, flags, status, child, child_cc.
    Hex throughout, zeros where the status is not 0.  The random pairs and triples become cases of class "random"."""
    import json
    doc = json.load(open(path))
    z32, z33 = bytes(32).hex(), bytes(33).hex()
    tweak = [dict(zip(("class", "name", "curve", "key", "tweak", "status", "out33"), r)) for r in doc["tweak"]]
    for c in tweak:
        if c["status"]:
            del c["out33"]
    seckey = [dict(zip(("class", "name", "curve", "key", "tweak", "status", "out"), r)) for r in doc["seckey"]]
    for i, (curve, d, t, key33, out33, out33x) in enumerate(doc["pairs"]):
        pt = decode(CURVES[curve], bytes.fromhex(key33))
        for form in (33, 65, 32) if curve == "secp256k1" else (33, 65):
            tweak.append({"class": "random", "name": "pair %d, %d-byte key" % (i, form), "curve": curve, "key": encode(pt, form).hex(),
                          "tweak": t, "status": 0, "out33": out33x if form == 32 and out33x else out33})
        out, st = seckey_tweak_add(CURVES[curve], bytes.fromhex(d), bytes.fromhex(t))
        seckey.append({"class": "random", "name": "pair %d" % i, "curve": curve, "key": d, "tweak": t, "status": st, "out": out.hex()})
    for c in seckey:
        c["out"] = c["out"] or z32
    pub = [dict(zip(("class", "name", "pk", "cc", "index", "status", "child", "child_cc"), r)) for r in doc["bip32_pub"]]
    priv = [dict(zip(("class", "name", "key", "cc", "index", "flags", "status", "child", "child_cc"), r)) for r in doc["bip32_priv"]]
    for i, (key, cc, index, child, ccc, pk, pchild, pcc) in enumerate(doc["triples"]):
        priv.append({"class": "random", "name": "triple %d" % i, "key": key, "cc": cc, "index": index, "flags": 0, "status": 0,
                     "child": child, "child_cc": ccc})
        pub.append({"class": "random", "name": "triple %d" % i, "pk": pk, "cc": cc, "index": index & (HARDENED - 1), "status": 0,
                    "child": pchild, "child_cc": pcc or ccc})
    for c in pub:
        c["child"], c["child_cc"] = c["child"] or z33, c["child_cc"] or z32
    for c in priv:
        c["child"], c["child_cc"] = c["child"] or z32, c["child_cc"] or z32
    return {"tweak": tweak, "seckey": seckey, "bip32_pub": pub, "bip32_priv": priv}


def master(seed):
    """BIP-32 master key generation (the model's own: the library leaves it to the caller): (key, chain code)"""
    I = hmac512(b"Bitcoin seed", seed)
    return I[:32], I[32:]


def public_key(C, key, form=33):
    return encode(C.mul(int.from_bytes(key, "big"), C.G), form)
