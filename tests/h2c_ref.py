"""
Test-side restatement of the reference's HashToCurve surface for secp256k1 and P-256 (D = Sha256), on hashlib and
oracle/py_model.py: expand_message_xmd, hash_to_field with os2ip_mod_p, map_to_curve, hash_to_curve / encode_to_curve
with SimplifiedSwu, and the trait method C::hash_to_curve.

Readings (the list of forge_ec_amd/csrc/h2c.hpp and DESIGN.md section 18; h2c = forge-ec-hash/src/hash_to_curve.rs):
  * expand_message_xmd (h2c:380-448; the copy at secp256k1.rs:1774-1840 is identical) is RFC 9380's.  The block counter is
    `i as u8` (out_len <= 8160) and dst_prime ends in `dst.len() as u8` (dst_len <= 255).
  * hash_to_field (316-348) asks for 32 * count bytes; os2ip_mod_p (355-377) is the TRAIT from_bytes -- which forwards to
    the inherent one: big-endian, None iff not below p; secp256k1's returns the Montgomery form, P-256's the limbs as read
    -- and None gives one(), the raw limb 1.
  * Secp256k1::map_to_curve (secp256k1.rs:1587-1705): inherent `sqrt` (112-131) and `to_bytes` (138-178), the trait's
    `invert`, `square`, `is_zero`.  P256::map_to_curve (p256.rs:2215-2265): inherent `invert`, `sqrt`, `to_bytes`;
    `square` is the trait's s * s.
  * Both inherent sqrt functions have wrong exponents: None for every input tried.  secp256k1 therefore returns its
    default_point, P-256 (x, +-1).  `cand` (x, y^2 as computed) and `legs` report what the computation did all the same.
  * hash (292-312): two elements, two maps, from_affine (z = one), the curve's Add, clear_cofactor = identity function.
    encode_to_curve (1030-1056): count = 1.  The trait method: secp256k1's override (1712-1769: 96 bytes, the first 32 of
    each 48-byte half, fallback from_raw([i + 1, 0, 0, 0]), to_affine) and the default for P-256 (core lib.rs:1550-1581:
    one SHA-256 of msg || dst, unwrap_or(zero), one map, to_affine).
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import py_model as M  # noqa: E402

SECP, P256 = 0, 1
MAX_DST, MAX_OUT, MAX_COUNT = 255, 255 * 32, 255
LEG_U_ZERO, LEG_INV_ZERO, LEG_SQRT_NONE, LEG_NEGATE, LEG_OS2IP = 1, 2, 4, 8, 16
ONE, ZERO = [1, 0, 0, 0], [0, 0, 0, 0]

# RFC 9380 K.1 (expand_message_xmd, SHA-256), DST and two of its 32-byte vectors
K1_DST = b"QUUX-V01-CS02-with-expander-SHA256-128"
K1 = ((b"", "68a985b87eb6b46952128911f2a4412bbc302a9d759667f87f7a21d803f07235"),
      (b"abc", "d8ccab23b5985ccea865c6c97b6e5b8350e794e603b4b97902f53a8a0d605615"))

SECP_R2 = [0x000E9F61, 0x07A20000, 0x00000100, 0]                       # to_montgomery's constant (219-235)
SECP_Z = [0xFFFFFFFFFFFFFFF5, M.M64, M.M64, M.M64]                      # 1597-1602: raw, not in Montgomery form
SECP_DEFAULT = ([0x79BE667EF9DCBBAC, 0x55A06295CE870B07, 0x029BFCDB2DCE28D9, 0x59F2815B16F81798],
                [0x483ADA7726A3C465, 0x5DA4FBFC0E1108A8, 0xFD17B448A6855419, 0x9C47D08FFB10D4B8])   # 1681-1695, literally
SECP_SQRT_E = [0xFF0C, 0xFFFF, 0xFFFE, 0x3FFF]                          # 112-131
P256_A = [0xFFFFFFFC, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF]               # 2220
P256_Z = [0xFFFFFFF6, M.M64, 0, 0xFFFFFFFF00000001]                     # 2224-2229
P256_SQRT_E = [0xC0000000, 0x40000000, 0x4000000000000000, 0x40000000C0000000]   # 320-339


def expand_message_xmd(msg, dst, out_len):
    """h2c:380-448 with dst_prime built as hash_to_field builds it (324-326)."""
    assert len(dst) <= MAX_DST and out_len <= MAX_OUT
    dst_prime = dst + bytes([len(dst)])
    ell = (out_len + 31) // 32
    b0 = hashlib.sha256(bytes(64) + msg + bytes([out_len >> 8, out_len & 0xFF, 0]) + dst_prime).digest()
    b = hashlib.sha256(b0 + b"\x01" + dst_prime).digest()
    out = b
    for i in range(2, ell + 1):
        b = hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b)) + bytes([i]) + dst_prime).digest()
        out += b
    return out[:out_len]


def os2ip_mod_p(curve, e):
    """355-377 -> (limbs, fell back)."""
    v, ok = M.field_from_bytes(curve, e)
    return (list(v), False) if ok else (list(ONE), True)


def hash_to_field(curve, msg, dst, count):
    """316-348 -> ([limbs] * count, [fell back] * count)."""
    assert 1 <= count <= MAX_COUNT
    ub = expand_message_xmd(msg, dst, 32 * count)
    r = [os2ip_mod_p(curve, ub[32 * i:32 * i + 32]) for i in range(count)]
    return [x[0] for x in r], [x[1] for x in r]


def _odd(curve, a):
    return M.to_bytes_field(curve, a)[31] & 1


def secp_map_parts(u):
    """secp256k1.rs:1592-1654: (effective_u, legs so far, w, x, y2)."""
    F = M.Secp
    b = F.mul([7, 0, 0, 0], SECP_R2)
    legs = LEG_U_ZERO if M._is_zero(u) else 0
    eu = list(ONE) if M._is_zero(u) else list(u)
    u2 = F.sqr(eu)
    u4 = F.sqr(u2)
    u8 = F.sqr(u4)
    z2 = F.sqr(SECP_Z)
    z4 = F.sqr(z2)
    z6 = F.mul(z4, z2)
    v = F.add(F.mul(z2, u4), F.mul(SECP_Z, u2))
    v3 = F.mul(F.sqr(v), v)
    w = F.add(v3, F.mul(F.mul(b, z6), u8))
    x_num = F.mul(v, F.mul(z2, u2))
    if M._is_zero(w):
        legs |= LEG_INV_ZERO
    x = F.mul(x_num, F.inv(w))                      # invert of zero: None -> unwrap_or(zero); Secp.inv returns zero
    y2 = F.add(F.mul(F.sqr(x), x), b)
    return eu, legs, w, x, y2


def secp_map_finish(eu, legs, x, y2, s, some):
    """1657-1704 from the root on: s the inherent sqrt's candidate, some whether it is Some."""
    F = M.Secp
    yv = list(s) if some else list(ZERO)
    if not some:
        legs |= LEG_SQRT_NONE
    negate = _odd(SECP, eu) != _odd(SECP, yv)
    if negate:
        legs |= LEG_NEGATE
    y = F.neg(yv) if negate else yv
    valid = not (legs & LEG_INV_ZERO) and some
    return ((list(x), y) if valid else (list(SECP_DEFAULT[0]), list(SECP_DEFAULT[1]))), legs


def p256_map_parts(u):
    """p256.rs:2220-2254: (legs so far, x, y2)."""
    F = M.P256c
    b = M.P256_B
    z_u2 = F.mul(P256_Z, F.sqr(u))
    tv2 = F.add(F.add(F.sqr(z_u2), z_u2), ONE)
    tz = M._is_zero(tv2)
    tv3 = F.mul(b, list(ONE) if tz else F.inv(tv2))
    tv5 = F.neg(F.mul(P256_A, z_u2))
    tv8 = F.add(F.add(F.sqr(tv5), tv5), b)
    tv9 = F.mul(tv8, tv3)
    x = F.add(tv5, tv9) if tz else F.sub(tv5, tv9)
    y2 = F.add(F.add(F.mul(F.sqr(x), x), F.mul(P256_A, x)), b)
    return (LEG_INV_ZERO if tz else 0), x, y2


def p256_map_finish(u, legs, x, s, some):
    F = M.P256c
    y = list(s) if some else list(ONE)
    if not some:
        legs |= LEG_SQRT_NONE
    negate = (y[0] & 1) != (u[0] & 1)
    if negate:
        legs |= LEG_NEGATE
    return (list(x), F.neg(y) if negate else y), legs


def map_to_curve(curve, u):
    """C::map_to_curve(&from_raw(u)) -> ((x, y), (cand x, cand y2), legs)."""
    u = [int(v) for v in u]
    if curve == SECP:
        eu, legs, _, x, y2 = secp_map_parts(u)
        s = M._secp_pow(y2, SECP_SQRT_E)
        pt, legs = secp_map_finish(eu, legs, x, y2, s, M.Secp.sqr(s) == y2)
    else:
        legs, x, y2 = p256_map_parts(u)
        s = M.P256c.pow(y2, P256_SQRT_E)
        pt, legs = p256_map_finish(u, legs, x, s, M.P256c.sqr(s) == y2)
    return pt, (x, y2), legs


def _field(curve):
    return M.Secp if curve == SECP else M.P256c


def hash_to_curve(curve, msg, dst, encode=False):
    """hash (292-312) or encode_to_curve (1030-1056) -> (projective (x, y, z), [cand] per map, [legs] per map)."""
    assert len(dst) > 0, "Err(DomainSeparationFailure)"
    us, fell = hash_to_field(curve, msg, dst, 1 if encode else 2)
    maps = [map_to_curve(curve, u) for u in us]
    legs = [m[2] | (LEG_OS2IP if f else 0) for m, f in zip(maps, fell)]
    pts = [(m[0][0], m[0][1], list(ONE)) for m in maps]
    r = pts[0] if encode else _field(curve).padd(pts[0], pts[1])
    return r, [m[1] for m in maps], legs


def curve_hash_to_curve(curve, msg, dst):
    """The trait method -> (x, y, infinity)."""
    F = _field(curve)
    if curve == SECP:                                                 # secp256k1.rs:1712-1769
        ub = expand_message_xmd(msg, dst, 96)
        us = []
        for i in range(2):
            v, ok = M.field_from_bytes(SECP, ub[48 * i:48 * i + 32])
            us.append(list(v) if ok else [i + 1, 0, 0, 0])
        pts = [map_to_curve(SECP, u)[0] for u in us]
        return F.to_affine(F.padd((pts[0][0], pts[0][1], list(ONE)), (pts[1][0], pts[1][1], list(ONE))))
    v, ok = M.field_from_bytes(P256, hashlib.sha256(msg + dst).digest())   # core lib.rs:1558-1570
    pt = map_to_curve(P256, list(v) if ok else list(ZERO))[0]
    return F.to_affine((pt[0], pt[1], list(ONE)))


def flat_proj(p):
    return [int(v) for c in p for v in c]


# ---- the message sets the fixture and the GPU tests share ----
def messages(n, seed, dst_len):
    """n messages of mixed lengths: an empty one, and lengths that put the padding of b_0's input
    (64 + len + 3 + dst_len + 1 bytes) at 55, 56, 63 and 64 bytes modulo 64; the rest seeded, 1..150 bytes."""
    import random
    rng = random.Random(seed)
    special = [0] + [(r - (68 + dst_len)) % 64 + 64 * k for k, r in enumerate((55, 56, 63, 64))]
    lens = [special[i] if i < len(special) else rng.randrange(1, 151) for i in range(n)]
    return [bytes(rng.getrandbits(8) for _ in range(l)) for l in lens]


def dst_of(dst_len):
    return bytes((37 * i + 11) & 0xFF for i in range(dst_len))
