"""
Test-side reference for Ecdsa::<C, D>::sign (forge-ec-signature/src/ecdsa.rs:98-211) with the digest and the nonce
given: a composition over the C oracle (oracle/c_oracle.py) fast enough for thousands of elements --
  R = multiply(G, k), to_affine     threaded fo_batch_mul_fixed / fo_batch_to_affine
  x.to_bytes()                      secp256k1: field_op "mul" by raw 1 (mont_reduce, secp256k1.rs:138-178);
                                    P-256: the raw limbs (p256.rs:288-300)
  Mul / invert / Add of Scalar      secp256k1_scalar_op / p256_scalar_op
and, restated here (the oracle has no call for them): Scalar::from_bytes, Sub, ct_lt, the constant half and
normalize (45-71).  tests/golden/gen_ecdsa_sign.py composes the same glue over oracle/py_model.py; the two are
compared in tests/test_ecdsa_sign_model.py.
"""
import numpy as np

W = 1 << 256
M64 = (1 << 64) - 1
N = {0: [0xBFD25E8CD0364141, 0xBAAEDCE6AF48A03B, M64, 0xFFFFFFFFFFFFFFFE],                       # secp256k1.rs:27-28
     1: [0xF3B9CAC2FC632551, 0xBCE6FAADA7179E84, M64, 0xFFFFFFFF00000000]}                       # p256.rs:23-24
ONE = [1, 0, 0, 0]


def _val(l):
    return sum(int(x) << (64 * i) for i, x in enumerate(l))


def _limbs(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def _scalar_op(oracle, curve):
    f = oracle.secp256k1_scalar_op if curve == 0 else oracle.p256_scalar_op

    def op(name, a, b=None):
        r, ok = f(name, a, b)
        return [int(v) for v in r], ok
    return op


def ct_lt(curve, a, b):
    """secp256k1: the override (secp256k1.rs:2323-2347), a true comparison; P-256: the trait default
    (forge-ec-core/src/lib.rs:497-531), which comes down to top_byte(a) <= top_byte(b)."""
    if curve == 0:
        return _val(a) < _val(b)
    return (int(a[3]) >> 56) <= (int(b[3]) >> 56)


def sub(curve, op, a, b):
    """Sub for Scalar: secp256k1.rs:2380-2408; p256.rs:1377-1408 (`result += n` through Add where self < rhs)."""
    if curve == 0:
        d = _val(a) - _val(b)
        return _limbs(d + _val(N[0]) if d < 0 else d)   # (_limbs takes the result modulo 2^256)
    r = list(a)
    if _val(a) < _val(b):
        r, _ = op("add", a, N[1])
    return _limbs((_val(r) - _val(b)) % W)


def half(oracle, curve):
    """get_order() / Scalar::from(2) = N * invert(2) (Div, secp256k1.rs:2552-2564, p256.rs:1196-1207)."""
    op = _scalar_op(oracle, curve)
    i2, ok = op("inv", [2, 0, 0, 0])
    assert ok
    return op("mul", N[curve], i2)[0]


def sign(oracle, curve, sk, digests, k, nthreads=8):
    """sk, k (n,4) uint64; digests (n,32) uint8.  -> (r (n,4), s (n,4), status (n,) uint8), as fec_ecdsa_sign."""
    sk = np.ascontiguousarray(np.asarray(sk, dtype=np.uint64)).reshape(-1, 4)
    k = np.ascontiguousarray(np.asarray(k, dtype=np.uint64)).reshape(-1, 4)
    digests = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8)).reshape(-1, 32)
    n = sk.shape[0]
    op = _scalar_op(oracle, curve)
    hv = half(oracle, curve)
    nv = _val(N[curve])
    rp = oracle.batch_mul_fixed(curve, k, oracle.generator(curve), nthreads=nthreads)
    xy, _ = oracle.batch_to_affine(curve, rp, nthreads=nthreads)        # the identity: x = 0
    r_out = np.tile(np.array(ONE, dtype=np.uint64), (n, 1))
    s_out = r_out.copy()
    status = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        ski, ki = [int(v) for v in sk[i]], [int(v) for v in k[i]]
        if _val(ski) == 0 or not ct_lt(curve, ski, N[curve]):          # 101-104
            status[i] = 1
            continue
        x = xy[i, :4]
        r = [int(v) for v in oracle.field_op(0, "mul", x, ONE)] if curve == 0 else [int(v) for v in x]
        if _val(r) >= nv:                                               # Scalar::from_bytes: 126-129
            status[i] = 2
            continue
        if _val(r) == 0:                                                # 131-134
            status[i] = 3
            continue
        h = _limbs(int.from_bytes(bytes(digests[i]), "big"))
        if _val(h) >= nv:                                               # 149-154
            status[i] = 2
            continue
        k_inv, ok = op("inv", ki)
        if not ok:                                                      # 159-164
            status[i] = 3
            continue
        s = op("mul", k_inv, op("add", h, op("mul", r, ski)[0])[0])[0]  # 166-169
        if _val(s) == 0:                                                # 172-177
            status[i] = 3
            continue
        if not ct_lt(curve, s, hv):                                     # normalize 45-71
            s = sub(curve, op, N[curve], s)
        r_out[i], s_out[i] = r, s
    return r_out, s_out, status
