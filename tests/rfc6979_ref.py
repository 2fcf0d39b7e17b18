"""
Test-side restatement of Rfc6979::<C, Sha256>::generate_k (forge-ec-rng/src/rfc6979.rs:58-181, empty extra_data) with
hashlib / hmac, and of Ecdsa::<C, Sha256>::sign from the message on top of it.

Readings (the list of forge_ec_amd/csrc/rfc6979.hpp and DESIGN.md section 15):
  * private_key_bytes is the TRAIT Scalar::to_bytes: the four limbs big-endian, most significant limb first, NOT reduced
    (secp256k1.rs:2300-2312, p256.rs:1026-1038).
  * h1 = SHA-256(msg) whole: no bits2octets reduction; the same 32 bytes sign_internal uses as h_bytes.
  * SimpleHmac<Sha256> with a 32-byte key is standard HMAC-SHA-256; V = 01.., K = 00..; the two K / V updates with the
    separators 00 and 01; then V = HMAC_K(V), T = V (rlen = 32).
  * a candidate is accepted iff the TRAIT from_bytes is Some -- big-endian value below the reference's order constant
    (secp256k1: the one with the two top limbs swapped, not the true n) -- and it is not zero; otherwise
    K = HMAC_K(V || 00), V = HMAC_K(V) and the loop goes on.
  * no message is special: rfc6979.rs and ecdsa.rs:98-211 do not look for "test message".
`order` is a parameter so that the retry leg, which neither real constant reaches, can be driven with a smaller one
(fec_debug_rfc6979_k, the host build of tests/cpp/rfc6979_host.cpp).
"""
import hashlib
import hmac

import numpy as np

import ecdsa_sign_ref as E

MAX_RETRIES = 128                                    # rfc6979.hpp: a lane that needs more writes k = 0, status 5
ORDER = {c: E._val(E.N[c]) for c in (0, 1)}          # what Scalar::from_bytes compares with (ecdsa_sign_ref.N)


def key_bytes(sk_limbs):
    """Scalar::to_bytes of the raw limbs (least significant limb first in sk_limbs)."""
    return b"".join(int(l).to_bytes(8, "big") for l in reversed(list(sk_limbs)))


def generate_k(sk_limbs, msg, order):
    """-> (k, retries); (0, MAX_RETRIES + 1) where the device code gives up."""
    mac = lambda key, data: hmac.new(key, data, hashlib.sha256).digest()
    x, h1 = key_bytes(sk_limbs), hashlib.sha256(msg).digest()
    v, k = b"\x01" * 32, b"\x00" * 32
    for sep in (b"\x00", b"\x01"):
        k = mac(k, v + sep + x + h1)
        v = mac(k, v)
    for retries in range(MAX_RETRIES + 1):
        v = mac(k, v)
        t = int.from_bytes(v, "big")
        if 0 < t < order:
            return t, retries
        k = mac(k, v + b"\x00")
        v = mac(k, v)
    return 0, MAX_RETRIES + 1


def nonces(curve, sk, msgs, order=None):
    """(n, 4) uint64 limbs of generate_k per element, and the retry counts."""
    order = ORDER[curve] if order is None else order
    out = [generate_k([int(v) for v in s], m, order) for s, m in zip(np.asarray(sk, dtype=np.uint64).reshape(-1, 4), msgs)]
    return np.array([E._limbs(k) for k, _ in out], dtype=np.uint64).reshape(-1, 4), [r for _, r in out]


def sign_msg(oracle, curve, sk, msgs, nthreads=8):
    """Ecdsa::<C, Sha256>::sign(sk, msg) per element: SHA-256, generate_k, then sign with that digest and nonce --
    ecdsa_sign_ref.sign over the C oracle, or, with oracle = None, tests/golden/gen_ecdsa_sign.sign over
    oracle/py_model.py.  A key that sign's check rejects (ecdsa.rs:101-104) draws no nonce: its k is 0 here and the
    signer reports status 1.  -> (r (n,4), s (n,4), status (n,), k (n,4))."""
    sk = np.ascontiguousarray(np.asarray(sk, dtype=np.uint64)).reshape(-1, 4)
    digests = np.array([list(hashlib.sha256(m).digest()) for m in msgs], dtype=np.uint8).reshape(-1, 32)
    k = np.zeros_like(sk)
    for i, m in enumerate(msgs):
        s = [int(v) for v in sk[i]]
        if E._val(s) != 0 and E.ct_lt(curve, s, E.N[curve]):
            k[i] = E._limbs(generate_k(s, m, ORDER[curve])[0])
    if oracle is not None:
        r, s, st = E.sign(oracle, curve, sk, digests, k, nthreads=nthreads)
        return r, s, st, k
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_ecdsa_sign as G
    rows = [G.sign(curve, [int(v) for v in sk[i]], bytes(digests[i]), [int(v) for v in k[i]]) for i in range(len(msgs))]
    return (np.array([x[1] for x in rows], dtype=np.uint64).reshape(-1, 4), np.array([x[2] for x in rows], dtype=np.uint64).reshape(-1, 4),
            np.array([x[0] for x in rows], dtype=np.uint8), k)
