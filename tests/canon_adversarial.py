"""
Adversarial signatures for the canonical-mode verifiers, built from the model alone (oracle/canon_model.py,
tests/canon_msg_ref.py): inputs made to steer the verification arithmetic into its corners, which neither random nor
bit-flipped signatures reach.  tests/golden/gen_canon_adversarial.py writes the fixture from build().

ECDSA needs no private key for a valid signature with a prescribed R and a prescribed u2 (z is the hash's):
    r = R.x mod n,  s = r / u2,  u1 = z / s,  Q = (R - u1 G) / u2                                   (forge_u2)
or with a prescribed u1:  s = z / u1,  u2 = r / s,  same Q                                           (forge_u1)
and after the hash, where z is free, Q = q G, u1 and u2 are all prescribed:  R = u1 G + u2 Q,  s = r / u2,  z = u1 s.

Every case records `want`, the model's verdict, and `want_parent`, what the verifier answered while it multiplied A by
l - h instead of multiplying -A by h (Ed25519 keys with a torsion component); the two differ
only there, and build() asserts that they do.
"""
import random

import canon_msg_ref as R
from oracle import canon_model as M

SEED = 0xAD7E25A
GLV_LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
SEARCH_LIMIT = 200


def inv(a, n):
    return pow(a, -1, n)


def be32(v):
    return v.to_bytes(32, "big")


def le32(v):
    return v.to_bytes(32, "little")


def hx(v):
    """a 256-bit integer as 64 hex digits; the tests split it into 64-bit limbs"""
    return "%064x" % v


def hxy(pt):
    """x then y, 128 hex digits; None for infinity"""
    return None if pt is M.INF else hx(pt[0]) + hx(pt[1])


# ---- ECDSA ---------------------------------------------------------------------------------------
def prescribed_u2(C):
    n = C.N
    v = [("1", 1), ("2", 2), ("15", 15), ("16", 16), ("17", 17), ("n-1", n - 1), ("(n-1)/2", (n - 1) // 2), ("(n+1)/2", (n + 1) // 2),
         ("2^128", 2**128), ("2^128-1", 2**128 - 1), ("2^128+1", 2**128 + 1), ("2^129", 2**129)]
    if C is R.SECP:   # the GLV eigenvalue: k2 = +-1 with k1 = 0 / 1
        v += [("lambda", GLV_LAMBDA), ("lambda+1", GLV_LAMBDA + 1), ("n-lambda", n - GLV_LAMBDA)]
    return v


def forge_u2(C, z, Rpt, u2):
    """(r, s, Q): a signature of the hash z that verifies under Q with this R and this u2."""
    n = C.N
    r = Rpt[0] % n
    s = r * inv(u2, n) % n
    u1 = z * inv(s, n) % n
    return r, s, C.mul(inv(u2, n), C.add(Rpt, C.neg(C.mul(u1, C.G))))


def forge_u1(C, z, Rpt, u1):
    n = C.N
    r = Rpt[0] % n
    s = z * inv(u1, n) % n
    u2 = r * inv(s, n) % n
    return r, s, C.mul(inv(u2, n), C.add(Rpt, C.neg(C.mul(u1, C.G))))


def first_point_from(C, x):
    """the first curve point with x' >= x, by search"""
    while True:
        y = R.sqrt_mod(C, (x**3 + C.A * x + C.B) % C.P)
        if y is not None:
            return (x, y)
        x += 1


def ecdsa_point(C, z, r, s, Q):
    """(u1, u2, u1 G + u2 Q) for an in-range signature and a key on the curve, else None"""
    n = C.N
    if Q is None or Q is M.INF or not C.on_curve(Q) or not (1 <= r < n and 1 <= s < n):
        return None
    w = inv(s, n)
    u1, u2 = z * w % n, r * w % n
    return u1, u2, C.add(C.mul(u1, C.G), C.mul(u2, Q))


def ecdsa_verify_hash(C, z, r, s, Q):
    t = ecdsa_point(C, z, r, s, Q)
    return 1 if t is not None and t[2] is not M.INF and t[2][0] % C.N == r else 0


def ecdsa_msg_classes(C, rng):
    """(class, name, msg, r, s, Q) per case; every Q is a curve point"""
    n, G = C.N, C.G
    out = []
    z_of = lambda m: R.ecdsa_z(m) % n    # noqa: E731

    def rand_R():
        return C.mul(rng.randrange(1, n), G)

    # R.x in [n, p)
    Rhi = first_point_from(C, n + 1)   # x = n itself would give r = 0
    assert n < Rhi[0] < C.P
    msg = rng.randbytes(40)
    r, s, Q = forge_u2(C, z_of(msg), Rhi, rng.randrange(1, n))
    assert r == Rhi[0] - n
    out.append(("R.x in [n, p)", "r = x - n", msg, r, s, Q))
    out.append(("R.x in [n, p)", "r = x, refused for r >= n", msg, Rhi[0], s, Q))
    # R.x small enough that r + n fits 256 bits: the same key and s with r and with r + n
    Rlo = first_point_from(C, 1)
    msg = rng.randbytes(41)
    r, s, Q = forge_u2(C, z_of(msg), Rlo, rng.randrange(1, n))
    assert r == Rlo[0] and r + n < 2**256
    out.append(("r + n", "R.x < n sent as r", msg, r, s, Q))
    out.append(("r + n", "R.x < n sent as r + n", msg, r + n, s, Q))
    # the final addition
    msg, u1 = rng.randbytes(33), rng.randrange(1, n)
    r, s, Q = forge_u1(C, z_of(msg), C.mul(2 * u1 % n, G), u1)
    assert C.mul(r * inv(s, n) % n, Q) == C.mul(u1, G)
    out.append(("final addition", "u1 G = u2 Q: a doubling", msg, r, s, Q))
    msg, u1, r = rng.randbytes(34), rng.randrange(1, n), rng.randrange(1, n)
    s = z_of(msg) * inv(u1, n) % n
    Q = C.mul(inv(r * inv(s, n) % n, n), C.neg(C.mul(u1, G)))
    assert C.add(C.mul(u1, G), C.mul(r * inv(s, n) % n, Q)) is M.INF
    out.append(("final addition", "u1 G = -u2 Q: infinity", msg, r, s, Q))
    for label, d in (("Q = G", 1), ("Q = -G", n - 1)):
        msg, k = rng.randbytes(35), rng.randrange(1, n)
        r = C.mul(k, G)[0] % n
        out.append(("final addition", label, msg, r, inv(k, n) * (z_of(msg) + r * d) % n, C.mul(d, G)))
    # prescribed u1, prescribed u2
    for label, u1 in (("1", 1), ("2", 2), ("n-1", n - 1)):
        msg = rng.randbytes(20)
        out.append(("prescribed u1", "u1 = " + label, msg) + forge_u1(C, z_of(msg), rand_R(), u1))
    for label, u2 in prescribed_u2(C):
        msg = rng.randbytes(21)
        out.append(("prescribed u2", "u2 = " + label, msg) + forge_u2(C, z_of(msg), rand_R(), u2))
    if C is R.P256:   # the key with x = 0: nobody knows its logarithm, so from the message only a refused signature
        y = R.sqrt_mod(C, C.B)
        assert y is not None
        for label, yy in (("+", y), ("-", C.P - y)):
            out.append(("key x = 0", "key (0, %ssqrt b), another key's signature" % label, rng.randbytes(22),
                        rng.randrange(1, n), rng.randrange(1, n), (0, yy)))
    return out


def ecdsa_msg_cases(name, rng):
    C = R.WEIERSTRASS[name]
    cases = []
    for cls, label, msg, r, s, Q in ecdsa_msg_classes(C, rng):
        assert C.on_curve(Q) and Q is not M.INF
        z = R.ecdsa_z(msg)
        t = ecdsa_point(C, z, r, s, Q)
        for pk_len in (33, 65):
            pk, sig = R.sec1_encode(Q, pk_len == 33), be32(r) + be32(s)
            want = R.ecdsa_verify(C, msg, sig, pk)
            assert want == ecdsa_verify_hash(C, z, r, s, Q)
            c = {"scheme": "ecdsa", "curve": name, "pk_len": pk_len, "class": cls, "name": label, "msg": msg.hex(), "sig": sig.hex(),
                 "pk": pk.hex(), "want": want, "want_parent": want, "ossl": None}
            if t is not None and pk_len == 33:   # the 65-byte twin has the same one
                c["dm"] = {"u1": hx(t[0]), "u2": hx(t[1]), "q": hxy(Q), "point": hxy(t[2])}
            cases.append(c)
    return cases


def ecdsa_hash_cases(name, rng):
    """after the hash, z free: prescribed (u2, Q = q G) pairs, edge z, and for P-256 the key with x = 0"""
    C = R.WEIERSTRASS[name]
    n, G = C.N, C.G
    rows = []
    qs = [("G", 1), ("2G", 2), ("15G", 15), ("16G", 16), ("17G", 17)] + ([("lambda G", GLV_LAMBDA)] if C is R.SECP else [])

    def from_u(cls, label, u1, u2, Q):
        Rpt = C.add(C.mul(u1, G), C.mul(u2, Q))
        r = Rpt[0] % n
        s = r * inv(u2, n) % n
        rows.append((cls, label, u1 * s % n, r, s, Q))

    for ql, q in qs:
        for ul, u2 in prescribed_u2(C):
            from_u("prescribed u2 and Q", "u2 = %s, Q = %s" % (ul, ql), rng.randrange(1, n), u2, C.mul(q, G))
    for label, z in (("0", 0), ("n", n), ("n+1", n + 1), ("2^256-1", 2**256 - 1)):
        d, k = rng.randrange(1, n), rng.randrange(1, n)
        r = C.mul(k, G)[0] % n
        rows.append(("edge z", "z = " + label, z, r, inv(k, n) * (z + r * d) % n, C.mul(d, G)))
    if C is R.P256:
        y = R.sqrt_mod(C, C.B)
        for label, yy in (("+", y), ("-", C.P - y)):
            from_u("key x = 0", "key (0, %ssqrt b)" % label, rng.randrange(1, n), rng.randrange(1, n), (0, yy))
    cases = []
    for cls, label, z, r, s, Q in rows:
        u1, u2, pt = ecdsa_point(C, z, r, s, Q)
        want = ecdsa_verify_hash(C, z, r, s, Q)
        assert want == 1
        assert (u1, u2) == (z * inv(s, n) % n, r * inv(s, n) % n)   # what a test that wants u1 and u2 computes
        cases.append({"curve": name, "class": cls, "name": label, "z": hx(z), "r": hx(r), "s": hx(s), "q": hxy(Q), "point": hxy(pt),
                      "want": want, "ossl": None})
    return cases


# ---- BIP-340 -------------------------------------------------------------------------------------
def bip340_sign_raw(d, msg, k, negate_k=True):
    """BIP-340 signing with the nonce k given; negate_k=False leaves out the negation of k for an odd R.y"""
    C, n = R.SECP, R.SECP.N
    P = C.mul(d, C.G)
    d = d if P[1] % 2 == 0 else n - d
    Rpt = C.mul(k, C.G)
    if negate_k and Rpt[1] % 2:
        k = n - k
    r32, pk32 = be32(Rpt[0]), be32(P[0])
    return r32 + be32((k + R.bip340_challenge(r32, pk32, msg) * d) % n), pk32


def bip340_cases(rng):
    C, n = R.SECP, R.SECP.N
    rows = []
    d = rng.randrange(1, n)
    k = next(k for k in (rng.randrange(1, n) for _ in range(SEARCH_LIMIT)) if C.mul(k, C.G)[1] % 2)
    msg = rng.randbytes(32)
    sig, pk = bip340_sign_raw(d, msg, k, negate_k=False)
    rows.append(("R.y odd", "k not negated: s G - e P has this x and an odd y", msg, sig, pk))
    rows.append(("R.y odd", "the same R.x with the proper s", msg, bip340_sign_raw(d, msg, k)[0], pk))
    msg, r32 = rng.randbytes(32), be32(C.mul(rng.randrange(1, n), C.G)[0])
    P = R.lift_x(int.from_bytes(pk, "big"))
    de = d if C.mul(d, C.G) == P else n - d
    s = R.bip340_challenge(r32, pk, msg) * de % n
    assert C.add(C.mul(s, C.G), C.mul(n - R.bip340_challenge(r32, pk, msg), P)) is M.INF
    rows.append(("R infinity", "s G = e P", msg, r32 + be32(s), pk))
    msg = rng.randbytes(32)
    sig, _ = bip340_sign_raw(d, msg, rng.randrange(1, n))
    rows.append(("s = 0", "s = 0 under an honest R.x", msg, sig[:32] + be32(0), pk))
    for odd in (1, 0):   # the signer's negation of d, seen from the verifier: lift_x(pk) is -d G or d G
        dd = next(v for v in (rng.randrange(1, n) for _ in range(SEARCH_LIMIT)) if C.mul(v, C.G)[1] % 2 == odd)
        msg = rng.randbytes(32)
        sig2, pk2 = bip340_sign_raw(dd, msg, rng.randrange(1, n))
        assert (R.lift_x(int.from_bytes(pk2, "big")) == C.neg(C.mul(dd, C.G))) == bool(odd)
        rows.append(("key -d G", "lift_x(pk) = %sd G" % ("-" if odd else ""), msg, sig2, pk2))
    rows.append(("another key's R.x", "r of a valid signature under another key", msg, sig2[:32] + sig[32:], pk))
    rows.append(("another key's R.x", "a whole valid signature under another key", msg, sig2, pk))
    cases = []
    for cls, label, msg, sig, pk in rows:
        want = R.bip340_verify(msg, sig, pk)
        c = {"scheme": "bip340", "curve": "secp256k1", "pk_len": 32, "class": cls, "name": label, "msg": msg.hex(), "sig": sig.hex(),
             "pk": pk.hex(), "want": want, "want_parent": want, "ossl": None}
        P = R.lift_x(int.from_bytes(pk, "big"))
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        if P is not None and r < C.P and s < n:
            u2 = (n - R.bip340_challenge(sig[:32], pk, msg)) % n
            c["dm"] = {"u1": hx(s), "u2": hx(u2), "q": hxy(P), "point": hxy(C.add(C.mul(s, C.G), C.mul(u2, P)))}
        cases.append(c)
    assert [c["want"] for c in cases] == [0, 1, 0, 0, 1, 1, 0, 0]
    return cases


# ---- Ed25519 -------------------------------------------------------------------------------------
E = R.ED


def torsion_points():
    """[j T8 for j in 0..7]: T8 = l P for the first decodable y whose point has a component of order 8"""
    for y in range(2, SEARCH_LIMIT):
        P = R.ed_decode(le32(y))
        if P is None:
            continue
        T = E.mul(E.N, P)
        if E.mul(4, T) != E.IDENTITY:
            pts = [E.mul(j, T) for j in range(8)]
            assert len(set(pts)) == 8 and E.mul(8, T) == E.IDENTITY and all(E.on_curve(p) for p in pts)
            return pts
    raise AssertionError("no point of order 8 found")


def order_of(T):
    return next(o for o in (1, 2, 4, 8) if E.mul(o, T) == E.IDENTITY)


def ed25519_verify_parent(msg, sig, pk):
    """what the verifier computed before the fix: S B + (l - h) A == R"""
    A, Rp = R.ed_decode(pk), R.ed_decode(sig[:32])
    S = int.from_bytes(sig[32:], "little")
    if A is None or Rp is None or S >= E.N:
        return 0
    h = R.ed25519_challenge(sig[:32], pk, msg)
    return 1 if E.add(E.mul(S, E.G), E.mul((E.N - h) % E.N, A)) == Rp else 0


def ed25519_cases(rng):
    N, B = E.N, E.G
    tors = torsion_points()
    rows = []   # (class, name, msg, sig, pk)

    def honest(a, A, Rpt, r, msg):
        """S = r + h a for the encoded A and R: what a signer with the scalar a answers"""
        Renc, Aenc = E.encode(Rpt), E.encode(A)
        return Renc + le32((r + R.ed25519_challenge(Renc, Aenc, msg) * a) % N), Aenc

    def search(make, accept):
        """the first of make(0), make(1), ... that accept()s; the generator fails after SEARCH_LIMIT tries"""
        for t in range(SEARCH_LIMIT):
            row = make(t)
            if row is not None and accept(*row):
                return row
        raise AssertionError("no case within %d tries" % SEARCH_LIMIT)

    # A = a B + T, honest scalar, prime-order R: accepted exactly when h T is the identity
    a = rng.randrange(1, N)
    for j, T in enumerate(tors):
        A = E.add(E.mul(a, B), T)
        r = rng.randrange(1, N)
        make = lambda t: (b"mixed-order key %d try %d" % (j, t),) + honest(a, A, E.mul(r, B), r, b"mixed-order key %d try %d" % (j, t))  # noqa: E731
        verdicts = (1,) if j == 0 else (1, 0)
        for want in verdicts:
            msg, sig, pk = search(make, lambda m, s, k: R.ed25519_verify(m, s, k) == want)
            h = R.ed25519_challenge(sig[:32], pk, msg)
            assert (E.mul(h, T) == E.IDENTITY) == bool(want)
            rows.append(("mixed-order key", "A = a B + %d T8 (order %d), h T %s identity" % (j, order_of(T), "=" if want else "!="), msg, sig, pk))
        if order_of(T) == 8:   # and what only the parent's equation accepts: (l - h) T = (5 - h) T
            msg, sig, pk = search(make, lambda m, s, k: ed25519_verify_parent(m, s, k) == 1)
            rows.append(("mixed-order key", "A = a B + %d T8 (order 8), h = 5 mod 8" % j, msg, sig, pk))
    # R = r B + T, prime-order key
    A = E.mul(a, B)
    for j, T in enumerate(tors):
        r, msg = rng.randrange(1, N), rng.randbytes(30 + j)
        sig, pk = honest(a, A, E.add(E.mul(r, B), T), r, msg)
        rows.append(("mixed-order R", "R = r B + %d T8" % j, msg, sig, pk))
    # small-order keys, S = 0: R = -h A among the torsion points, and a neighbouring torsion point
    for j, A in enumerate(tors):
        pk = E.encode(A)

        def make(t, pk=pk, j=j):
            msg = b"small-order key %d try %d" % (j, t)
            for Rpt in tors:
                if R.ed25519_verify(msg, E.encode(Rpt) + bytes(32), pk):
                    return msg, E.encode(Rpt) + bytes(32), pk
            return None

        msg, sig, pk = search(make, lambda m, s, k: True)
        h = R.ed25519_challenge(sig[:32], pk, msg)
        assert R.ed_decode(sig[:32]) == E.mul(h, E.neg(A))
        rows.append(("small-order key", "A = %d T8 (order %d), S = 0, R = -h A" % (j, order_of(A)), msg, sig, pk))
        near = search(lambda t: (msg, E.encode(E.add(R.ed_decode(sig[:32]), tors[1 + t % 7])) + bytes(32), pk),
                      lambda m, s, k: R.ed25519_verify(m, s, k) == 0)
        rows.append(("small-order key", "A = %d T8 (order %d), S = 0, a neighbouring torsion R" % (j, order_of(A)),) + near)
    # R = A;  S = 0 with R the identity under a prime-order key
    A = E.mul(a, B)
    msg, Aenc = rng.randbytes(44), E.encode(A)
    rows.append(("R = A", "S = (h + 1) a", msg, Aenc + le32((R.ed25519_challenge(Aenc, Aenc, msg) + 1) * a % N), Aenc))
    rows.append(("R = A", "S = h a", msg, Aenc + le32(R.ed25519_challenge(Aenc, Aenc, msg) * a % N), Aenc))
    rows.append(("S = 0", "S = 0, R = identity, prime-order key", rng.randbytes(45), E.encode(E.IDENTITY) + bytes(32), Aenc))
    # encodings that are not canonical: the identity as y = p + 1, and as y = 1 with the sign bit of x = 0
    ident = E.encode(E.IDENTITY)
    rows.append(("non-canonical A", "A = identity sent as y = p + 1, S = 0, R = identity", rng.randbytes(46), ident + bytes(32), le32(E.P + 1)))
    rows.append(("non-canonical A", "A = identity sent with the sign bit, S = 0, R = identity", rng.randbytes(47), ident + bytes(32), le32(1 | 1 << 255)))
    rows.append(("non-canonical R", "R = identity sent as y = p + 1, S = 0, A = identity", rng.randbytes(48), le32(E.P + 1) + bytes(32), ident))
    cases = []
    for cls, label, msg, sig, pk in rows:
        want, parent = R.ed25519_verify(msg, sig, pk), ed25519_verify_parent(msg, sig, pk)
        c = {"scheme": "ed25519", "curve": "ed25519", "pk_len": 32, "class": cls, "name": label, "msg": msg.hex(), "sig": sig.hex(),
             "pk": pk.hex(), "want": want, "want_parent": parent, "ossl": None}
        A, Rp, S = R.ed_decode(pk), R.ed_decode(sig[:32]), int.from_bytes(sig[32:], "little")
        if A is not None and Rp is not None and S < N:   # the double multiplication of the verifier: S B + h (-A)
            h = R.ed25519_challenge(sig[:32], pk, msg)
            c["dm"] = {"u1": hx(S), "u2": hx(h), "q": hxy(E.neg(A)), "point": hxy(E.add(E.mul(S, B), E.mul(h, E.neg(A))))}
        cases.append(c)
    for cls in ("mixed-order key", "small-order key"):   # without these the fixture would no longer see the -h A bug
        assert any(c["want"] != c["want_parent"] for c in cases if c["class"] == cls), cls
    assert all(c["want"] == c["want_parent"] for c in cases if c["class"] not in ("mixed-order key", "small-order key"))
    for o in (2, 4, 8):
        for verdict in (0, 1):
            assert any(c["class"] == "mixed-order key" and "(order %d)" % o in c["name"] and c["want"] == verdict for c in cases), (o, verdict)
    return cases


def double_mul_cases(name, rng):
    """u1 G + u2 Q where the sum is a doubling or infinity, for the first prescribed u2 (the prescribed (u2, Q) pairs of
    ecdsa_hash_cases carry their u1, u2 and point too: a test sends them through double_mul as well)"""
    C = R.WEIERSTRASS[name]
    n, G = C.N, C.G
    rows = []
    q = rng.randrange(1, n)
    Q = C.mul(q, G)
    for ul, u2 in prescribed_u2(C)[:6]:
        rows.append(("final addition", "u1 G = u2 Q, u2 = " + ul, u2 * q % n, u2, Q))
        rows.append(("final addition", "u1 G = -u2 Q, u2 = " + ul, (n - u2 * q) % n, u2, Q))
    return [{"curve": name, "class": cls, "name": label, "u1": hx(u1), "u2": hx(u2), "q": hxy(Q),
             "point": hxy(C.add(C.mul(u1, G), C.mul(u2, Q))), "ossl": None} for cls, label, u1, u2, Q in rows]


def build():
    rng = random.Random(SEED)
    msg = ecdsa_msg_cases("secp256k1", rng) + ecdsa_msg_cases("p256", rng) + bip340_cases(rng) + ed25519_cases(rng)
    after = ecdsa_hash_cases("secp256k1", rng) + ecdsa_hash_cases("p256", rng)
    dm = double_mul_cases("secp256k1", rng) + double_mul_cases("p256", rng)
    return {"note": "built by tests/canon_adversarial.py (seed %#x) from the model alone; want_parent = the verdict of S B + (l - h) A == R" % SEED,
            "msg": msg, "hash": after, "double_mul": dm}
