"""
The canonical-mode SIGNERS as a model (include/fecgpu_canon.h, the signing side): standard RFC 6979 nonces with hmac / hashlib
and the order as a parameter, ECDSA with SHA-256 on secp256k1 and P-256 over the big-integer curves of oracle/canon_model.py,
and the BIP-340 / Ed25519 signers of tests/canon_msg_ref.py, imported.  Each returns what the library returns: the bytes
and a status.  Test infrastructure: tests/golden/gen_canon_sign.py writes the fixture from it, tests/test_canon_sign_model.py
pins it by published values.
"""
import hashlib
import hmac

import canon_msg_ref as R
from oracle import canon_model as M

OK, BAD_SCALAR, BAD_RANGE, RETRY, BAD_KEY = 0, 3, 4, 5, 6
LOW_S = 1
MAX_RETRIES = 128          # rfc6979.hpp: the chain tests 1 + MAX_RETRIES candidates, then reports RETRY
SCHEME_BIP340 = 3


RETRIED = {"count": 0}      # candidates the chain has rejected so far (the tests look at it to know that leg ran)


def rfc6979_chain(x, hz, order, max_retries=MAX_RETRIES):
    """RFC 6979 section 3.2 steps b-h with HMAC-SHA-256 on the 32 octets x = int2octets(d) and hz = bits2octets(h1): the
    first 256-bit candidate in [1, order), or None when 1 + max_retries candidates in a row were outside."""
    mac = lambda k, m: hmac.new(k, m, hashlib.sha256).digest()    # noqa: E731
    V, K = b"\x01" * 32, b"\x00" * 32
    K = mac(K, V + b"\x00" + x + hz)
    V = mac(K, V)
    K = mac(K, V + b"\x01" + x + hz)
    V = mac(K, V)
    for _ in range(1 + max_retries):
        V = mac(K, V)
        k = int.from_bytes(V, "big")
        if 1 <= k < order:
            return k
        RETRIED["count"] += 1
        K = mac(K, V + b"\x00")
        V = mac(K, V)
    return None


def rfc6979_k(n, d, h1, max_retries=MAX_RETRIES):
    """The nonce for a 256-bit order n (qlen = 256, so bits2int is the identity on a 32-byte hash): int2octets(d),
    bits2octets(h1) = h1 mod n."""
    assert n.bit_length() == 256 and len(h1) == 32
    return rfc6979_chain(d.to_bytes(32, "big"), (int.from_bytes(h1, "big") % n).to_bytes(32, "big"), n, max_retries)


def ecdsa_nonce(C, d, h1):
    """(k as 32 big-endian bytes, status) of fec_canon_rfc6979_k."""
    if not 1 <= d < C.N:
        return bytes(32), BAD_KEY
    k = rfc6979_k(C.N, d, h1)
    return (bytes(32), RETRY) if k is None else (k.to_bytes(32, "big"), OK)


def ecdsa_sign_digest(C, d, h1, flags=0):
    """(r || s, status): z = h1 mod n, the RFC 6979 nonce, s = k^-1 (z + r d); LOW_S: s > n/2 becomes n - s."""
    kb, st = ecdsa_nonce(C, d, h1)
    if st:
        return bytes(64), st
    k, n = int.from_bytes(kb, "big"), C.N
    r = C.mul(k, C.G)[0] % n
    s = pow(k, -1, n) * (int.from_bytes(h1, "big") % n + r * d) % n
    if r == 0 or s == 0:
        return bytes(64), RETRY
    if (flags & LOW_S) and s > n // 2:
        s = n - s
    return r.to_bytes(32, "big") + s.to_bytes(32, "big"), OK


def ecdsa_sign_msg(C, d, msg, flags=0):
    return ecdsa_sign_digest(C, d, hashlib.sha256(msg).digest(), flags)


def bip340_sign(d, msg, aux):
    if not 1 <= d < R.SECP.N:
        return bytes(64), BAD_KEY
    return R.bip340_sign(d, msg, aux), OK


def bip340_parities(d, msg, aux):
    """(P.y odd, R.y odd) for the signature bip340_sign makes: which legs of the two negations it takes."""
    n = R.SECP.N
    P = R.SECP.mul(d, R.SECP.G)
    dd = d if P[1] % 2 == 0 else n - d
    t = (dd ^ int.from_bytes(R.tagged("BIP0340/aux", aux), "big")).to_bytes(32, "big")
    k = int.from_bytes(R.tagged("BIP0340/nonce", t + P[0].to_bytes(32, "big") + msg), "big") % n
    return P[1] & 1, R.SECP.mul(k, R.SECP.G)[1] & 1


def ed25519_sign(seed, msg):
    return R.ed25519_sign(seed, msg), R.ed25519_pubkey(seed)


def public_key(scheme, key, out_len):
    """(out_len bytes, status) of fec_canon_public_key; scheme: a curve id or SCHEME_BIP340."""
    if scheme == R.CURVE_IDS["ed25519"]:
        return R.ed25519_pubkey(key), OK
    C = R.SECP if scheme in (0, SCHEME_BIP340) else R.P256
    d = int.from_bytes(key, "big")
    if not 1 <= d < C.N:
        return bytes(out_len), BAD_KEY
    pt = C.mul(d, C.G)
    return (pt[0].to_bytes(32, "big") if scheme == SCHEME_BIP340 else R.sec1_encode(pt, out_len == 33)), OK


# ---- published values ------------------------------------------------------------------------------
A25_KEY = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721


def published():
    """RFC 6979 A.2.5 (P-256, SHA-256): the nonces and signatures of "sample" and "test"; BIP-340 vector 0 (secret key 3,
    zero aux); RFC 8032 section 7.1 tests 1 and 2 from their seeds.  secp256k1 ECDSA has no published vector in the tree:
    its cases are model-signed and checked by the verifier."""
    pub = R.published()
    return {
        "rfc6979_a25_sample": {"scheme": "ecdsa", "curve": "p256", "msg": b"sample", "key": A25_KEY.to_bytes(32, "big"),
                               "k": bytes.fromhex("A6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60"),
                               "sig": pub["rfc6979_a25_sample"][3], "pk": pub["rfc6979_a25_sample"][4]},
        "rfc6979_a25_test": {"scheme": "ecdsa", "curve": "p256", "msg": b"test", "key": A25_KEY.to_bytes(32, "big"),
                             "k": bytes.fromhex("D16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0"),
                             "sig": bytes.fromhex("F1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367"
                                                  "019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083"),
                             "pk": pub["rfc6979_a25_sample"][4]},
        "bip340_vector0": {"scheme": "bip340", "curve": "secp256k1", "msg": pub["bip340_vector0"][2], "key": (3).to_bytes(32, "big"),
                           "aux": bytes(32), "sig": pub["bip340_vector0"][3], "pk": pub["bip340_vector0"][4]},
        "rfc8032_test1": {"scheme": "ed25519", "curve": "ed25519", "msg": pub["rfc8032_test1"][2], "key": M.ED25519_RFC8032_TEST1[0],
                          "sig": pub["rfc8032_test1"][3], "pk": pub["rfc8032_test1"][4]},
        "rfc8032_test2": {"scheme": "ed25519", "curve": "ed25519", "msg": pub["rfc8032_test2"][2], "key": M.ED25519_RFC8032_TEST2[0],
                          "sig": pub["rfc8032_test2"][3], "pk": pub["rfc8032_test2"][4]},
    }
