"""
Keccak-256 and ECDSA public-key recovery as a model (include/fecgpu_canon.h: fec_canon_keccak256, fec_canon_ecdsa_recover,
fec_canon_ecdsa_sign_recoverable_digest): Keccak-f[1600] and the sponge over Python integers with the domain byte as a
parameter, and SEC 1 v2 section 4.1.6 over the big-integer curves of oracle/canon_model.py.  Each function returns what the
library returns: the bytes and a status.  Test infrastructure: tests/golden/gen_canon_recover.py writes the fixture from it,
tests/test_canon_recover_model.py pins it -- the permutation and the sponge by hashlib.sha3_256 (domain byte 0x06), the 0x01
variant by published digests, recovery by sign-and-recover properties and the OpenSSL CLI.
"""
import canon_msg_ref as R
import canon_sign_ref as S
from oracle import canon_model as M

OK, NO_KEY = 0, 8
RATE = 136
MASK = (1 << 64) - 1

# ---- Keccak-f[1600] (the Keccak reference, section 1.2; lanes A[x + 5 y]) ---------------------------
RHO = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]


def _round_constants():
    """rc(t) of the reference: an LFSR over x^8 + x^6 + x^5 + x^4 + 1; bit 2^j - 1 of RC[i] is rc(j + 7 i)"""
    out, r = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            if r & 1:
                c |= 1 << ((1 << j) - 1)
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        out.append(c)
    return out


RC = _round_constants()


def rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f(a):
    """25 lanes in, 25 lanes out"""
    a = list(a)
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
        b = [0] * 25
        for y in range(5):
            for x in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y] ^ d[x], RHO[x + 5 * y])
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & MASK & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
        a[0] ^= RC[rnd]
    return a


def sponge256(msg, domain):
    """32 bytes squeezed at rate 136 after the padding  domain ... 0x80  (0x01: Keccak-256, 0x06: SHA3-256)"""
    padded = bytearray(msg) + bytes([domain]) + bytes(-(len(msg) + 1) % RATE)
    padded[-1] |= 0x80
    a = [0] * 25
    for off in range(0, len(padded), RATE):
        for i in range(RATE // 8):
            a[i] ^= int.from_bytes(padded[off + 8 * i:off + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


def keccak256(msg):
    return sponge256(msg, 0x01)


# the lengths at which the absorbing changes its path: empty, one byte, either side of a SHA-256 block's padding, either side
# of one and two rates, and a long message
KECCAK_LENGTHS = [0, 1, 55, 56, 134, 135, 136, 137, 271, 272, 273, 1000]


# ---- recovery (SEC 1 v2 section 4.1.6) ---------------------------------------------------------------
def recover_point(C, digest, sig, recid):
    """The key as a point, or None: recid > 3, r or s outside [1, n), x = r + (recid >> 1) n >= p, x not on the curve, or
    Q = r^-1 (s R - z G) at infinity."""
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if recid > 3 or not (1 <= r < C.N and 1 <= s < C.N):
        return None
    x = r + (recid >> 1) * C.N
    if x >= C.P:
        return None
    y = R.sqrt_mod(C, (x * x * x + C.A * x + C.B) % C.P)
    if y is None:
        return None
    if (y & 1) != (recid & 1):
        y = (C.P - y) % C.P
    z = int.from_bytes(digest, "big") % C.N
    w = pow(r, -1, C.N)
    Q = C.add(C.mul((-z * w) % C.N, C.G), C.mul(s * w % C.N, (x, y)))
    return None if Q is M.INF else Q


def eth_address(pt):
    return keccak256(pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"))[12:]


def encode(pt, out_len):
    if out_len in (33, 65):
        return R.sec1_encode(pt, out_len == 33)
    raw = pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")
    return raw if out_len == 64 else keccak256(raw)[12:]


def recover(C, digest, sig, recid, out_len):
    """(out_len bytes, status) of fec_canon_ecdsa_recover"""
    Q = recover_point(C, digest, sig, recid)
    return (bytes(out_len), NO_KEY) if Q is None else (encode(Q, out_len), OK)


def verify_digest(C, digest, sig, Q):
    """the verifier of FIPS 186-4 section 6.4 on a given digest and a key given as a point"""
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if not (1 <= r < C.N and 1 <= s < C.N) or not C.on_curve(Q) or Q is M.INF:
        return False
    w = pow(s, -1, C.N)
    Rp = C.add(C.mul(int.from_bytes(digest, "big") * w % C.N, C.G), C.mul(r * w % C.N, Q))
    return Rp is not M.INF and Rp[0] % C.N == r


def recid_of(y_odd, flipped, x_ge_n):
    """the id from its three ingredients, as the signing pass forms it"""
    return ((y_odd & 1) ^ (flipped & 1)) | ((x_ge_n & 1) << 1)


def sign_recoverable_digest(C, d, h1, flags=0):
    """(r || s, recid, status) of fec_canon_ecdsa_sign_recoverable_digest: canon_sign_ref.ecdsa_sign_digest and the id"""
    sig, st = S.ecdsa_sign_digest(C, d, h1, flags)
    if st:
        return sig, 0, st
    k = S.rfc6979_k(C.N, d, h1)
    x, y = C.mul(k, C.G)
    plain, _ = S.ecdsa_sign_digest(C, d, h1, 0)
    return sig, recid_of(y & 1, int(plain != sig), int(x >= C.N)), OK
