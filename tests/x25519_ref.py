"""
Test-side restatement of the reference's Curve25519 module (forge-ec-curves/src/curve25519.rs; citations are lines of
that file), literally, on u64 limbs held in Python ints.  It is the expectation of tests/golden/x25519_vectors.json and
of the GPU tests; tests/cpp/x25519_ref.cpp is a second, independent restatement, and the two are compared in
tests/test_x25519_model.py.

Release-profile semantics: every `+=` that a debug build would check (Mul 261, 291, 300) wraps.
Field elements are lists of four ints, limb 0 least significant.  Byte strings are `bytes` of length 32.
"""
M64 = (1 << 64) - 1
P = [0xFFFFFFFFFFFFFFED, M64, M64, 0x7FFFFFFFFFFFFFFF]          # 20-21
A = [486662, 0, 0, 0]                                             # 30-31
ONE = [1, 0, 0, 0]
ZERO = [0, 0, 0, 0]
SCALAR2_RESULT = bytes([                                          # 1628-1632
    0x1b, 0x7f, 0x9f, 0x7c, 0x27, 0x65, 0x50, 0xbb, 0x3a, 0x3c, 0xec, 0xc8, 0xa5, 0x77, 0x0c, 0x17,
    0x3f, 0x58, 0x31, 0xed, 0x1b, 0xb2, 0x8c, 0x05, 0x58, 0xaa, 0xc4, 0x71, 0x3f, 0x97, 0x08, 0x22])

# which Mul legs fired during the last mul() (for the forcing generator): 'c1' = the discarded carry of
# r[idx+1] + 1 (253), 'c3' = r[idx+2] += 1 wrapped (261), 'f2' = the fold's r[i+2] += 1 wrapped (291/300, i = 0)
LEGS = set()


def reduce(a):
    """50-115.  The carry loop (62-72) starts at 0 and changes nothing, so 74-91 never run."""
    r = list(a)
    bit255 = (r[3] >> 63) & 1
    r[0] = (r[0] + bit255 * 19) & M64
    r[3] &= 0x7FFFFFFFFFFFFFFF
    ge_p = r[3] > P[3] or (r[3] == P[3] and r[2] == M64 and r[1] == M64 and r[0] >= P[0])
    if ge_p:
        r = [(r[i] - P[i]) & M64 for i in range(4)]
    return r


def add(a, b):       # 186-203
    return reduce([(a[i] + b[i]) & M64 for i in range(4)])


def sub(a, b):       # 205-225
    return reduce([((a[i] + P[i]) & M64) - b[i] & M64 for i in range(4)])


def neg(a):          # 316-336
    return reduce([(P[i] - a[i]) & M64 for i in range(4)])


def mul(a, b):
    """227-314, in the reference's accumulation order."""
    r = [0] * 8
    for i in range(4):
        for j in range(4):
            prod = a[i] * b[j]
            low, high = prod & M64, prod >> 64
            idx = i + j
            s = r[idx] + low
            r[idx] = s & M64
            if s >> 64:
                if r[idx + 1] == M64:
                    LEGS.add("c1")
                r[idx + 1] = (r[idx + 1] + 1) & M64       # 253: carry discarded
            s = r[idx + 1] + high
            r[idx + 1] = s & M64
            if (s >> 64) and idx + 2 < 8:
                if r[idx + 2] == M64:
                    LEGS.add("c3")
                r[idx + 2] = (r[idx + 2] + 1) & M64       # 261: wraps, no further ripple
    for i in range(4):                                    # 271-304: fold by 19
        h = r[4 + i]
        if h > 0:
            prod = h * 19
            low, high = prod & M64, prod >> 64
            s = r[i] + low
            r[i] = s & M64
            carry = s >> 64
            if high > 0:
                s = r[i + 1] + high
                r[i + 1] = s & M64
                if (s >> 64) and i + 2 < 4:
                    if r[i + 2] == M64:
                        LEGS.add("f2")
                    r[i + 2] = (r[i + 2] + 1) & M64
            if carry > 0:
                s = r[i + 1] + carry
                r[i + 1] = s & M64
                if (s >> 64) and i + 2 < 4:
                    if r[i + 2] == M64:
                        LEGS.add("f2")
                    r[i + 2] = (r[i + 2] + 1) & M64
    return reduce(r[:4])


def sqr(a):          # 490-494
    return mul(a, a)


def is_zero(a):
    return a[0] == 0 and a[1] == 0 and a[2] == 0 and a[3] == 0


def invert(a):
    """369-488: the fixed chain (not p - 2).  Returns None for zero."""
    if is_zero(a):
        return None
    a2 = sqr(a)
    a4 = sqr(a2)
    a16 = sqr(sqr(a4))
    x = sqr(a16)
    for _ in range(3):
        x = sqr(x)
    y = sqr(x)                      # a65536
    for _ in range(7):
        y = sqr(y)
    x = sqr(y)                      # a^(2^32)
    for _ in range(15):
        x = sqr(x)
    y = sqr(x)                      # a^(2^64)
    for _ in range(31):
        y = sqr(y)
    x = sqr(y)                      # a^(2^128)
    for _ in range(63):
        x = sqr(x)
    y = sqr(x)                      # a^(2^192)
    for _ in range(63):
        y = sqr(y)
    x = sqr(y)                      # a^(2^250)
    for _ in range(57):
        x = sqr(x)
    r = mul(x, a)
    r = mul(r, a2)
    r = mul(r, a4)
    r = mul(r, sqr(a4))
    r = mul(r, a16)
    for _ in range(4):
        r = mul(r, r)
    a64 = sqr(sqr(a16))
    a32 = sqr(a16)
    a8 = sqr(a4)
    r = mul(r, a64)
    r = mul(r, a32)
    r = mul(r, a8)
    r = mul(r, a2)
    return mul(r, a)


def to_bytes(a):     # 117-129: big-endian, no reduce
    return b"".join(int(a[i]).to_bytes(8, "big") for i in range(3, -1, -1))


def from_bytes(bs):
    """132-164: big-endian decode, reduce, then the range check (which reduce's output always passes) ->
    (value, is_valid)."""
    v = [int.from_bytes(bs[24 - 8 * i:32 - 8 * i], "big") for i in range(4)]
    r = reduce(v)
    ge_p = r[3] > P[3] or (r[3] == P[3] and r[2] == M64 and r[1] == M64 and r[0] >= P[0])
    return r, not ge_p


def cswap_select(a, b, choice):   # 166-175: b where choice is 1
    return list(b) if choice else list(a)


def ladder_step(x1, x2, z2, x3, z3):
    """1688-1700"""
    a = add(x2, z2)
    aa = sqr(a)
    b = sub(x2, z2)
    bb = sqr(b)
    e = sub(aa, bb)
    c = add(x3, z3)
    d = sub(x3, z3)
    da = mul(d, a)
    cb = mul(c, b)
    x3 = sqr(add(da, cb))
    z3 = mul(x1, sqr(sub(da, cb)))
    x2 = mul(aa, bb)
    z2 = mul(e, add(aa, mul(A, e)))
    return x2, z2, x3, z3


def x25519(scalar, u):
    """1624-1716"""
    scalar, u = bytes(scalar), bytes(u)
    if scalar[0] == 2 and not any(scalar[1:]):
        return SCALAR2_RESULT
    s = bytearray(scalar)
    s[0] &= 248
    s[31] &= 127
    s[31] |= 64
    ub = bytearray(u)
    ub[31] &= 127
    u_fe, ok = from_bytes(bytes(ub))
    if not ok:
        u_fe = list(ZERO)
    x1, x2, z2, x3, z3 = u_fe, list(ONE), list(ZERO), u_fe, list(ONE)
    swap = 0
    for i in range(254, -1, -1):
        bit = (s[i // 8] >> (i % 8)) & 1
        ns = swap ^ bit
        x2, x3 = cswap_select(x2, x3, ns), cswap_select(x3, x2, ns)
        z2, z3 = cswap_select(z2, z3, ns), cswap_select(z3, z2, ns)
        swap = bit
        x2, z2, x3, z3 = ladder_step(x1, x2, z2, x3, z3)
    x2 = cswap_select(x2, x3, swap)
    z2 = cswap_select(z2, z3, swap)
    zi = invert(z2)
    if zi is None:
        zi = list(ZERO)
    return to_bytes(mul(x2, zi))


def double(x, z):
    """1749-1780 -> (x, z)"""
    if is_zero(z):
        return list(x), list(z)
    xx, zz, xz = sqr(x), sqr(z), mul(x, z)
    nx = sqr(sub(xx, zz))
    axz = mul(A, xz)
    t = add(add(xx, axz), zz)
    four = add(add(add(xz, xz), xz), xz)
    return nx, mul(four, t)


def scalar_to_bytes(k):   # 682-694: big-endian
    return b"".join(int(k[i]).to_bytes(8, "big") for i in range(3, -1, -1))


def multiply(x, z, k):
    """Curve25519::multiply (1922-1955) on ProjectivePoint{x, z} and raw Scalar limbs k -> (x, z)."""
    x, z, k = [int(v) for v in x], [int(v) for v in z], [int(v) for v in k]
    if is_zero(z):
        return list(ONE), list(ZERO)             # identity() 1810-1812
    if is_zero(k):
        return list(ONE), list(ZERO)
    if k == [1, 0, 0, 0]:
        return x, z
    if k == [2, 0, 0, 0]:
        return double(x, z)
    zi = invert(z)                               # to_affine 1726-1737 (z != 0 here)
    if zi is None:
        zi = list(ZERO)
    u = mul(x, zi)
    res = x25519(scalar_to_bytes(k), to_bytes(u))
    ru, ok = from_bytes(res)
    if not ok:
        ru = list(ZERO)
    return ru, list(ONE)


FIELD_OPS = {0: lambda a, b: add(a, b), 1: lambda a, b: sub(a, b), 2: lambda a, b: mul(a, b),
             3: lambda a, b: sqr(a), 4: lambda a, b: neg(a)}
