"""
RFC 7748 section 5 X25519 over Python integers: the model of canonical mode's fec_canon_x25519 / fec_canon_x25519_base
(include/fecgpu_canon.h).  Decoding, clamping, the ladder and the encoding are the RFC's own pseudocode; nothing is shared
with x25519_ref.py, which models the reference's curve25519.rs (another function altogether).  Pinned by the RFC's published
vectors in test_canon_x25519_model.py.
"""
P = (1 << 255) - 19
A24 = 121665
ZERO_SHARED = 7          # FEC_CANON_ZERO_SHARED
BASE_U = (9).to_bytes(32, "little")


def decode_scalar(k):
    """decodeScalar25519: 32 bytes -> the clamped integer"""
    b = bytearray(k)
    assert len(b) == 32
    b[0] &= 248
    b[31] &= 127
    b[31] |= 64
    return int.from_bytes(b, "little")


def clamp_bytes(k):
    return decode_scalar(k).to_bytes(32, "little")


def decode_u(u):
    """decodeUCoordinate: bit 255 is masked off; a value in [p, 2^255) is accepted and reduced"""
    assert len(u) == 32
    return (int.from_bytes(u, "little") & ((1 << 255) - 1)) % P


def ladder(k, u):
    """the RFC's Montgomery ladder on integers: k the clamped scalar, u < p"""
    x1, x2, z2, x3, z3, swap = u, 1, 0, u, 1, 0
    for t in range(254, -1, -1):
        kt = (k >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return x2 * pow(z2, P - 2, P) % P


def x25519(k, u):
    """32 bytes, 32 bytes -> 32 bytes"""
    return ladder(decode_scalar(k), decode_u(u)).to_bytes(32, "little")


def x25519_status(k, u):
    """(out, status): status ZERO_SHARED when the output is all zero (RFC 7748 section 6.1), else 0"""
    out = x25519(k, u)
    return out, (ZERO_SHARED if out == bytes(32) else 0)


def x25519_base(k):
    return x25519(k, BASE_U)


# u-coordinates of the points of low order (RFC 7748 section 6.1; the list of section 7's reference [cr.yp.to/ecdh.html]):
# 0 and 1, the two of order 8, p - 1, and the non-canonical p, p + 1.
LOW_ORDER = [
    0, 1,
    325606250916557431795983626356110631294008115727848805560023387167927233504,
    39382357235489614581723060781553021112529911719440698176882885853963445705823,
    P - 1, P, P + 1,
]

PUBLISHED = {
    "rfc7748_5_2_vector1": dict(
        k="a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
        u="e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
        out="c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
    "rfc7748_5_2_vector2": dict(
        k="4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
        u="e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
        out="95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"),
}
ITERATED_1 = "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
ITERATED_1000 = "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"
DH = dict(
    a="77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a",
    A="8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a",
    b="5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb",
    B="de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f",
    shared="4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742")


def iterate(steps):
    """RFC 7748 section 5.2's chain from k = u = 9: k, u = X25519(k, u), k.  Returns the list of k after each step."""
    k = u = BASE_U
    out = []
    for _ in range(steps):
        k, u = x25519(k, u), k
        out.append(k)
    return out
