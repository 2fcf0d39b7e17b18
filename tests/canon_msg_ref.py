"""
The canonical-mode verifiers FROM THE MESSAGE as a model: hashlib plus the big-integer curves of oracle/canon_model.py.
Standard ECDSA with SHA-256 (FIPS 186-4 section 6.4 / SEC 1) on secp256k1 and P-256, BIP-340 and RFC 8032 Ed25519, each
with `sign` and `verify` on bytes, and the SEC 1 key encodings.  Test infrastructure: tests/golden/gen_canon_msg.py writes
the fixture from it, tests/test_canon_msg_model.py pins it by the published vectors.
"""
import hashlib

from oracle import canon_model as M

SECP, P256, ED = M.SECP256K1, M.P256, M.ED25519
WEIERSTRASS = {"secp256k1": SECP, "p256": P256}
CURVE_IDS = {"secp256k1": 0, "p256": 1, "ed25519": 2}


# ---- SEC 1 section 2.3.3 / 2.3.4 -------------------------------------------------------------------
def sqrt_mod(C, a):
    """A square root of a modulo C.P (both primes are 3 mod 4), or None."""
    r = pow(a, (C.P + 1) // 4, C.P)
    return r if r * r % C.P == a % C.P else None


def sec1_encode(pt, compressed=True):
    x, y = pt
    if compressed:
        return bytes([2 + (y & 1)]) + x.to_bytes(32, "big")
    return b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")


def sec1_decode(C, b):
    """33 bytes: tag 2 or 3, x < p, a root exists, the root with the tag's parity.  65 bytes: tag 4, x, y < p, on the
    curve.  Anything else: None."""
    if len(b) == 33:
        x = int.from_bytes(b[1:], "big")
        if b[0] not in (2, 3) or x >= C.P:
            return None
        y = sqrt_mod(C, (x * x * x + C.A * x + C.B) % C.P)
        if y is None:
            return None
        return (x, y if (y & 1) == (b[0] & 1) else (C.P - y) % C.P)
    if len(b) == 65:
        pt = (int.from_bytes(b[1:33], "big"), int.from_bytes(b[33:], "big"))
        return pt if b[0] == 4 and C.on_curve(pt) else None
    return None


# ---- ECDSA with SHA-256 ----------------------------------------------------------------------------
def ecdsa_z(msg):
    return int.from_bytes(hashlib.sha256(msg).digest(), "big")


def ecdsa_sign(C, d, msg, k):
    """r || s for the nonce k (the caller's; any k in [1, n) that gives r, s != 0)."""
    R = C.mul(k, C.G)
    r = R[0] % C.N
    s = pow(k, -1, C.N) * (ecdsa_z(msg) + r * d) % C.N
    assert r and s
    return r.to_bytes(32, "big") + s.to_bytes(32, "big")


def ecdsa_verify(C, msg, sig, pk):
    Q = sec1_decode(C, pk)
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if Q is None or not (1 <= r < C.N and 1 <= s < C.N):
        return 0
    w = pow(s, -1, C.N)
    R = C.add(C.mul(ecdsa_z(msg) * w % C.N, C.G), C.mul(r * w % C.N, Q))
    return 1 if R is not M.INF and R[0] % C.N == r else 0


# ---- BIP-340 ---------------------------------------------------------------------------------------
def tagged(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + data).digest()


def lift_x(x):
    if x >= SECP.P:
        return None
    y = sqrt_mod(SECP, (pow(x, 3, SECP.P) + 7) % SECP.P)
    if y is None:
        return None
    return (x, y if y % 2 == 0 else SECP.P - y)


def bip340_pubkey(d):
    return SECP.mul(d, SECP.G)[0].to_bytes(32, "big")


def bip340_challenge(r32, pk32, msg):
    return int.from_bytes(tagged("BIP0340/challenge", r32 + pk32 + msg), "big") % SECP.N


def bip340_sign(d, msg, aux=bytes(32)):
    """BIP-340 default signing."""
    n = SECP.N
    P = SECP.mul(d, SECP.G)
    d = d if P[1] % 2 == 0 else n - d
    t = (d ^ int.from_bytes(tagged("BIP0340/aux", aux), "big")).to_bytes(32, "big")
    k = int.from_bytes(tagged("BIP0340/nonce", t + P[0].to_bytes(32, "big") + msg), "big") % n
    assert k
    R = SECP.mul(k, SECP.G)
    k = k if R[1] % 2 == 0 else n - k
    r32, pk32 = R[0].to_bytes(32, "big"), P[0].to_bytes(32, "big")
    return r32 + ((k + bip340_challenge(r32, pk32, msg) * d) % n).to_bytes(32, "big")


def bip340_verify(msg, sig, pk):
    P = lift_x(int.from_bytes(pk, "big"))
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if P is None or r >= SECP.P or s >= SECP.N:
        return 0
    e = bip340_challenge(sig[:32], pk, msg)
    R = SECP.add(SECP.mul(s, SECP.G), SECP.mul((SECP.N - e) % SECP.N, P))
    return 1 if R is not M.INF and R[1] % 2 == 0 and R[0] == r else 0


# ---- Ed25519 (RFC 8032 section 5.1) ----------------------------------------------------------------
def ed_decode(b):
    """Section 5.1.3: None for y >= p, no x, or x = 0 with the sign bit set."""
    v = int.from_bytes(b, "little")
    sign, y = v >> 255, v & ((1 << 255) - 1)
    p = ED.P
    if y >= p:
        return None
    x2 = (y * y - 1) * pow(ED.D * y * y + 1, -1, p) % p
    x = pow(x2, (p + 3) // 8, p)
    if (x * x - x2) % p:
        x = x * pow(2, (p - 1) // 4, p) % p
    if (x * x - x2) % p or (x == 0 and sign):
        return None
    return (p - x if (x & 1) != sign else x, y)


def ed25519_challenge(r32, pk32, msg):
    return int.from_bytes(hashlib.sha512(r32 + pk32 + msg).digest(), "little") % ED.N


def ed25519_pubkey(seed):
    return ED.encode(ED.mul(ED.secret_scalar(seed), ED.G))


def ed25519_sign(seed, msg):
    a = ED.secret_scalar(seed)
    A = ED.encode(ED.mul(a, ED.G))
    r = int.from_bytes(hashlib.sha512(hashlib.sha512(seed).digest()[32:] + msg).digest(), "little") % ED.N
    R = ED.encode(ED.mul(r, ED.G))
    return R + ((r + ed25519_challenge(R, A, msg) * a) % ED.N).to_bytes(32, "little")


def ed25519_verify(msg, sig, pk):
    """Canonical encodings only, S < l, the cofactorless equation S B - h A == R.  -h A is h (-A): A may have a torsion
    component, and (l - h) A is -h A only for A of prime order."""
    A, R = ed_decode(pk), ed_decode(sig[:32])
    S = int.from_bytes(sig[32:], "little")
    if A is None or R is None or S >= ED.N:
        return 0
    h = ed25519_challenge(sig[:32], pk, msg)
    return 1 if ED.add(ED.mul(S, ED.G), ED.mul(h, ED.neg(A))) == R else 0


# ---- the published from-the-message vectors --------------------------------------------------------
def published():
    """name -> (scheme, curve, msg, sig, pk): RFC 6979 A.2.5 (P-256, SHA-256, "sample"; the key compressed here),
    BIP-340 vector 0, RFC 8032 section 7.1 tests 1 and 2."""
    d = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
    out = {"rfc6979_a25_sample": ("ecdsa", "p256", b"sample", bytes.fromhex(
        "EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716"
        "F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8"), sec1_encode(P256.KNOWN_MULTIPLES[d]))}
    out["bip340_vector0"] = ("bip340", "secp256k1", bytes(32), bytes.fromhex(
        "E907831F80848D1069A5371B402410364BDF1C5F8307B0084C55F1CE2DCA8215"
        "25F66A4A85EA8B71E482A74F382D2CE5EBEEE8FDB2172F477DF4900D310536C0"),
        bytes.fromhex("F9308A019258C31049344F85F89D5229B531C845836F99B08601F113BCE036F9"))
    out["rfc8032_test1"] = ("ed25519", "ed25519", b"", bytes.fromhex(
        "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e06522490155"
        "5fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"), M.ED25519_RFC8032_TEST1[1])
    out["rfc8032_test2"] = ("ed25519", "ed25519", bytes([0x72]), bytes.fromhex(
        "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da"
        "085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"), M.ED25519_RFC8032_TEST2[1])
    return out


def verify(scheme, curve, msg, sig, pk):
    if scheme == "ecdsa":
        return ecdsa_verify(WEIERSTRASS[curve], msg, sig, pk)
    return bip340_verify(msg, sig, pk) if scheme == "bip340" else ed25519_verify(msg, sig, pk)
