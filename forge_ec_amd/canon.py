"""
Canonical-math mode over include/fecgpu_canon.h -- NOT reference parity.

The real secp256k1 / P-256 / Ed25519 groups (standard public keys / ECDH points), for callers who want results
other libraries agree with; forge-ec's own arithmetic does not produce them.
Arrays are numpy uint64 little-endian limbs of the plain integers: scalars (n,4); affine points
(n,8) = x then y; status (n,) uint8: 0 finite, 1 infinity (xy = 0), 2 input point rejected.
The *_verify_msg calls take what arrives on a wire instead: a list of message byte strings, signatures (n,64) uint8
and encoded keys (n,32 / 33 / 65) uint8 (or bytes objects); the hash and the decoding run on the GPU.
GPU only, like the rest of the package.
"""
import numpy as np

from . import _lib as L
from .curves import Context, _check, _ptr, _u64

FINITE, INFINITY, BAD_POINT = 0, 1, 2


def _bytes_rows(a, width, what):
    """bytes, a list of byte strings or an array -> contiguous (n, width) uint8."""
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], (bytes, bytearray)):
        a = np.frombuffer(b"".join(a), dtype=np.uint8)
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
    if a.size % width:
        raise ValueError("%s: not a whole number of %d-byte records" % (what, width))
    return a.reshape(-1, width)


def _verify_msg(lib_fn, h, msgs, sigs, pks, pk_len, what, lead=()):
    sg, pk = _bytes_rows(sigs, 64, "sigs"), _bytes_rows(pks, pk_len, "pks")
    buf, off, total = Context._messages(msgs)
    n = sg.shape[0]
    if not (pk.shape[0] == n and len(off) == n + 1):
        raise ValueError("inputs differ in length")
    out = np.zeros(n, dtype=np.uint8)
    tail = (pk_len,) if lead else ()
    _check(lib_fn(h, *lead, _ptr(buf), _ptr(off), total, _ptr(sg), _ptr(pk), *tail, _ptr(out), n), what)
    return out


def _batch_verify_msg(lib_fn, h, msgs, sigs, pks, seed, what):
    """the *_batch_verify_msg calls: (ok, status (n,), verdict); seed: 32 bytes or None (drawn by the library)"""
    sg, pk = _bytes_rows(sigs, 64, "sigs"), _bytes_rows(pks, 32, "pks")
    buf, off, total = Context._messages(msgs)
    n = sg.shape[0]
    if not (pk.shape[0] == n and len(off) == n + 1):
        raise ValueError("inputs differ in length")
    sd = None if seed is None else _bytes_rows(seed, 32, "seed")
    if sd is not None and sd.shape[0] != 1:
        raise ValueError("seed: 32 bytes")
    st, verdict = np.zeros(n, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    _check(lib_fn(h, _ptr(buf), _ptr(off), total, _ptr(sg), _ptr(pk), None if sd is None else _ptr(sd), _ptr(st), _ptr(verdict), n), what)
    return bool(verdict[0] == 1 and not st.any()), st, int(verdict[0])


def _batch_seed(seed):
    """(pointer or None, the array that keeps it alive)"""
    if seed is None:
        return None, None
    sd = _bytes_rows(seed, 32, "seed")
    if sd.shape[0] != 1:
        raise ValueError("seed: 32 bytes")
    return _ptr(sd), sd


def _sign_msg(lib_fn, h, msgs, secrets, what, lead=(), mid=(), after=()):
    """the *_sign_msg calls: (sigs (n,64), status (n,)); secrets = the 32-byte record arrays, in order."""
    buf, off, total = Context._messages(msgs)
    n = len(off) - 1
    recs = [_bytes_rows(x, 32, "keys") for x in secrets]
    if any(r.shape[0] != n for r in recs):
        raise ValueError("inputs differ in length")
    sigs = np.zeros((n, 64), dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    _check(lib_fn(h, *lead, _ptr(buf), _ptr(off), total, *[_ptr(r) for r in recs], *mid, _ptr(sigs), *after, _ptr(st), n), what)
    return sigs, st


class CanonCurve:
    CURVE = None
    SCHEME = None

    def __init__(self, ctx=None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self._lib = self.ctx._lib
        self._h = self.ctx._h

    def mul_base(self, scalars):
        """(xy, status) with xy[i] = scalars[i] * G."""
        k = _u64(scalars, 4)
        n = k.shape[0]
        xy = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_mul_base(self._h, self.CURVE, _ptr(k), _ptr(xy), _ptr(st), n), "fec_canon_mul_base")
        return xy, st

    def mul_base_secret(self, scalars):
        """mul_base for secret scalars: no table lookup indexed by a digit, no branch on one (include/fecgpu_canon.h, the
        signing side).  Weierstrass: k outside [1, n) gets status 3 and zeros."""
        k = _u64(scalars, 4)
        n = k.shape[0]
        xy = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_mul_base_secret(self._h, self.CURVE, _ptr(k), _ptr(xy), _ptr(st), n), "fec_canon_mul_base_secret")
        return xy, st

    def mul_base_secret_dev(self, d_scalars, d_out_xy, d_status, n, stream=None):
        _check(self._lib.fec_canon_mul_base_secret_dev(self._h, self.CURVE, d_scalars, d_out_xy, d_status, n, stream),
               "fec_canon_mul_base_secret_dev")

    def public_key(self, keys, out_len=None, scheme=None):
        """(keys (n,out_len) uint8, status): ECDSA curves SEC 1 with out_len 33 (default) or 65; Ed25519 32 bytes from the
        seed; scheme=L.CANON_SCHEME_BIP340 (secp256k1): 32 bytes x-only.  status 6: key 0 or >= n, zeros."""
        scheme = self.SCHEME if scheme is None else scheme
        out_len = (33 if scheme in (L.SECP256K1, L.P256) else 32) if out_len is None else out_len
        k = _bytes_rows(keys, 32, "keys")
        n = k.shape[0]
        out = np.zeros((n, out_len), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_public_key(self._h, scheme, _ptr(k), _ptr(out), out_len, _ptr(st), n), "fec_canon_public_key")
        return out, st

    def public_key_dev(self, d_keys, d_out, out_len, d_status, n, stream=None, scheme=None):
        _check(self._lib.fec_canon_public_key_dev(self._h, self.SCHEME if scheme is None else scheme, d_keys, d_out, out_len,
                                                  d_status, n, stream), "fec_canon_public_key_dev")

    def ecdsa_sign_digest(self, digests, keys, flags=0):
        """ECDSA with RFC 6979 nonces over given 32-byte digests (secp256k1, P-256): (sigs (n,64) r || s big-endian, status).
        keys (n,32) big-endian.  flags: L.CANON_SIGN_LOW_S.  status: 0, 6 (key 0 or >= n), 5 (unobservable)."""
        dg, k = _bytes_rows(digests, 32, "digests"), _bytes_rows(keys, 32, "keys")
        n = dg.shape[0]
        if k.shape[0] != n:
            raise ValueError("inputs differ in length")
        sigs = np.zeros((n, 64), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_ecdsa_sign_digest(self._h, self.CURVE, _ptr(dg), _ptr(k), flags, _ptr(sigs), _ptr(st), n),
               "fec_canon_ecdsa_sign_digest")
        return sigs, st

    def ecdsa_sign_digest_dev(self, d_digests, d_keys, flags, d_sigs, d_status, n, stream=None):
        _check(self._lib.fec_canon_ecdsa_sign_digest_dev(self._h, self.CURVE, d_digests, d_keys, flags, d_sigs, d_status, n, stream),
               "fec_canon_ecdsa_sign_digest_dev")

    def ecdsa_sign_recoverable_digest(self, digests, keys, flags=0):
        """ecdsa_sign_digest with the recovery ids: (sigs, recids (n,) uint8 in 0..3, status).  sigs and status are those of
        ecdsa_sign_digest; recids[i] is what ecdsa_recover needs to find the key again, 0 where status is not 0."""
        dg, k = _bytes_rows(digests, 32, "digests"), _bytes_rows(keys, 32, "keys")
        n = dg.shape[0]
        if k.shape[0] != n:
            raise ValueError("inputs differ in length")
        sigs = np.zeros((n, 64), dtype=np.uint8)
        rec = np.zeros(n, dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_ecdsa_sign_recoverable_digest(self._h, self.CURVE, _ptr(dg), _ptr(k), flags, _ptr(sigs), _ptr(rec),
                                                                 _ptr(st), n), "fec_canon_ecdsa_sign_recoverable_digest")
        return sigs, rec, st

    def ecdsa_sign_recoverable_digest_dev(self, d_digests, d_keys, flags, d_sigs, d_recids, d_status, n, stream=None):
        _check(self._lib.fec_canon_ecdsa_sign_recoverable_digest_dev(self._h, self.CURVE, d_digests, d_keys, flags, d_sigs, d_recids,
                                                                     d_status, n, stream), "fec_canon_ecdsa_sign_recoverable_digest_dev")

    def ecdsa_recover(self, digests, sigs, recids, out_len=33):
        """Public-key recovery (SEC 1 section 4.1.6; secp256k1, P-256): digests (n,32), sigs (n,64) r || s big-endian, recids
        (n,) in 0..3 -> (out (n,out_len) uint8, status).  out_len 33 / 65: SEC 1; 64: x || y big-endian; 20 (secp256k1): the
        Ethereum address.  status 8 (L.CANON_NO_KEY): no key, zeros."""
        dg, sg = _bytes_rows(digests, 32, "digests"), _bytes_rows(sigs, 64, "sigs")
        rc = np.ascontiguousarray(np.asarray(recids, dtype=np.uint8)).reshape(-1)
        n = dg.shape[0]
        if not (sg.shape[0] == rc.shape[0] == n):
            raise ValueError("inputs differ in length")
        out = np.zeros((n, out_len), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_ecdsa_recover(self._h, self.CURVE, _ptr(dg), _ptr(sg), _ptr(rc), _ptr(out), out_len, _ptr(st), n),
               "fec_canon_ecdsa_recover")
        return out, st

    def ecdsa_recover_dev(self, d_digests, d_sigs, d_recids, d_out, out_len, d_status, n, stream=None):
        _check(self._lib.fec_canon_ecdsa_recover_dev(self._h, self.CURVE, d_digests, d_sigs, d_recids, d_out, out_len, d_status, n,
                                                     stream), "fec_canon_ecdsa_recover_dev")

    def pubkey_tweak_add(self, pks, tweaks, pk_len=33, out_len=33):
        """pks[i] + tweaks[i] * G on encoded keys (secp256k1, P-256): pks (n,pk_len) with pk_len 33 / 65 (SEC 1) or 32 (x-only,
        even y; secp256k1), tweaks (n,32) big-endian -> (out (n,out_len) uint8, status); out_len 33, 65 or 32 (x alone;
        secp256k1).  status: 0, 2 (the key does not decode), 3 (tweak >= n), 8 (the sum is the point at infinity), zeros then.
        A tweak of 0 returns the key."""
        pk, t = _bytes_rows(pks, pk_len, "pks"), _bytes_rows(tweaks, 32, "tweaks")
        n = pk.shape[0]
        if t.shape[0] != n:
            raise ValueError("inputs differ in length")
        out = np.zeros((n, out_len), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_pubkey_tweak_add(self._h, self.CURVE, _ptr(pk), pk_len, _ptr(t), _ptr(out), out_len, _ptr(st), n),
               "fec_canon_pubkey_tweak_add")
        return out, st

    def pubkey_tweak_add_dev(self, d_pks, pk_len, d_tweaks, d_out, out_len, d_status, n, stream=None):
        _check(self._lib.fec_canon_pubkey_tweak_add_dev(self._h, self.CURVE, d_pks, pk_len, d_tweaks, d_out, out_len, d_status, n,
                                                        stream), "fec_canon_pubkey_tweak_add_dev")

    def seckey_tweak_add(self, keys, tweaks):
        """(keys[i] + tweaks[i]) mod n (secp256k1, P-256), (n,32) big-endian each -> (out (n,32), status).  status: 0, 6 (key 0
        or >= n), 3 (tweak >= n), 8 (the result is 0), zeros then."""
        k, t = _bytes_rows(keys, 32, "keys"), _bytes_rows(tweaks, 32, "tweaks")
        n = k.shape[0]
        if t.shape[0] != n:
            raise ValueError("inputs differ in length")
        out = np.zeros((n, 32), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_seckey_tweak_add(self._h, self.CURVE, _ptr(k), _ptr(t), _ptr(out), _ptr(st), n),
               "fec_canon_seckey_tweak_add")
        return out, st

    def seckey_tweak_add_dev(self, d_keys, d_tweaks, d_out, d_status, n, stream=None):
        _check(self._lib.fec_canon_seckey_tweak_add_dev(self._h, self.CURVE, d_keys, d_tweaks, d_out, d_status, n, stream),
               "fec_canon_seckey_tweak_add_dev")

    def ecdsa_sign_msg(self, msgs, keys, flags=0):
        """ECDSA with SHA-256 and RFC 6979 nonces from the message: msgs a list of n byte strings -> (sigs, status)."""
        return _sign_msg(self._lib.fec_canon_ecdsa_sign_msg, self._h, msgs, [keys], "fec_canon_ecdsa_sign_msg", lead=(self.CURVE,),
                         mid=(flags,))

    def ecdsa_sign_msg_dev(self, d_msgs, d_msg_off, msg_len, d_keys, flags, d_sigs, d_status, n, stream=None):
        _check(self._lib.fec_canon_ecdsa_sign_msg_dev(self._h, self.CURVE, d_msgs, d_msg_off, msg_len, d_keys, flags, d_sigs,
                                                      d_status, n, stream), "fec_canon_ecdsa_sign_msg_dev")

    def rfc6979_k(self, digests, keys):
        """The RFC 6979 nonces alone: (k (n,32) big-endian, status)."""
        dg, k = _bytes_rows(digests, 32, "digests"), _bytes_rows(keys, 32, "keys")
        n = dg.shape[0]
        if k.shape[0] != n:
            raise ValueError("inputs differ in length")
        out = np.zeros((n, 32), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_rfc6979_k(self._h, self.CURVE, _ptr(dg), _ptr(k), _ptr(out), _ptr(st), n), "fec_canon_rfc6979_k")
        return out, st

    def rfc6979_k_dev(self, d_digests, d_keys, d_k_out, d_status, n, stream=None):
        _check(self._lib.fec_canon_rfc6979_k_dev(self._h, self.CURVE, d_digests, d_keys, d_k_out, d_status, n, stream),
               "fec_canon_rfc6979_k_dev")

    def mul(self, scalars, points_xy):
        """(xy, status) with xy[i] = scalars[i] * points_xy[i]; off-curve inputs get status 2."""
        k = _u64(scalars, 4)
        p = _u64(points_xy, 8)
        if p.shape[0] != k.shape[0]:
            raise ValueError("scalars and points differ in length")
        n = k.shape[0]
        xy = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_mul(self._h, self.CURVE, _ptr(k), _ptr(p), _ptr(xy), _ptr(st), n), "fec_canon_mul")
        return xy, st

    def msm(self, scalars, points_xy):
        """(xy, status): the ONE point xy (8 limbs) = sum of scalars[i] * points_xy[i] by the bucket method.  status 0; 1: the sum
        is the point at infinity (Weierstrass; n = 0 included), 2: some input point is off the curve -- zeros then."""
        k = _u64(scalars, 4)
        p = _u64(points_xy, 8)
        if p.shape[0] != k.shape[0]:
            raise ValueError("scalars and points differ in length")
        xy = np.zeros(8, dtype=np.uint64)
        st = np.zeros(1, dtype=np.uint8)
        _check(self._lib.fec_canon_msm(self._h, self.CURVE, _ptr(k), _ptr(p), k.shape[0], _ptr(xy), _ptr(st)), "fec_canon_msm")
        return xy, int(st[0])

    def msm_dev(self, d_scalars, d_points_xy, n, d_out_xy, d_status, stream=None):
        """Enqueue-only form of msm on device pointers: d_scalars (n*32 bytes), d_points_xy (n*64) and d_out_xy (64 bytes: the
        one sum) 16-byte aligned, d_status one byte; d_out_xy and d_status are written whatever n is (n = 0: the identity).
        Nothing is read back or synchronised; single-device ctx only."""
        _check(self._lib.fec_canon_msm_dev(self._h, self.CURVE, d_scalars, d_points_xy, n, d_out_xy, d_status, stream),
               "fec_canon_msm_dev")

    def double_mul(self, u1, u2, points_xy):
        """(xy, status) with xy[i] = u1[i] * G + u2[i] * points_xy[i]  (signature-verification point)."""
        a, b = _u64(u1, 4), _u64(u2, 4)
        p = _u64(points_xy, 8)
        if not (a.shape[0] == b.shape[0] == p.shape[0]):
            raise ValueError("inputs differ in length")
        n = a.shape[0]
        xy = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_double_mul(self._h, self.CURVE, _ptr(a), _ptr(b), _ptr(p), _ptr(xy), _ptr(st), n),
               "fec_canon_double_mul")
        return xy, st

    def double_mul_dev(self, d_u1, d_u2, d_points_xy, d_out_xy, d_status, n, stream=None):
        _check(self._lib.fec_canon_double_mul_dev(self._h, self.CURVE, d_u1, d_u2, d_points_xy, d_out_xy, d_status, n,
                                                  stream), "fec_canon_double_mul_dev")

    def ecdsa_verify(self, z, r, s, pk_xy):
        """Standard ECDSA verification (secp256k1, P-256): (n,) uint8, 1 = valid.  z = digest as an integer."""
        zz, rr, ss = _u64(z, 4), _u64(r, 4), _u64(s, 4)
        pk = _u64(pk_xy, 8)
        n = zz.shape[0]
        if not (rr.shape[0] == ss.shape[0] == pk.shape[0] == n):
            raise ValueError("inputs differ in length")
        out = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_ecdsa_verify(self._h, self.CURVE, _ptr(zz), _ptr(rr), _ptr(ss), _ptr(pk), _ptr(out), n),
               "fec_canon_ecdsa_verify")
        return out

    def ecdsa_verify_dev(self, d_z, d_r, d_s, d_pk_xy, d_result, n, stream=None):
        _check(self._lib.fec_canon_ecdsa_verify_dev(self._h, self.CURVE, d_z, d_r, d_s, d_pk_xy, d_result, n, stream),
               "fec_canon_ecdsa_verify_dev")

    def ecdsa_verify_msg(self, msgs, sigs, pks, pk_len=33):
        """ECDSA with SHA-256 from the message (secp256k1, P-256): msgs a list of n byte strings, sigs (n,64) r || s
        big-endian, pks (n,pk_len) SEC 1 keys, pk_len 33 (compressed) or 65.  (n,) uint8, 1 = valid."""
        return _verify_msg(self._lib.fec_canon_ecdsa_verify_msg, self._h, msgs, sigs, pks, pk_len,
                           "fec_canon_ecdsa_verify_msg", lead=(self.CURVE,))

    def ecdsa_verify_msg_dev(self, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, pk_len, d_result, n, stream=None):
        _check(self._lib.fec_canon_ecdsa_verify_msg_dev(self._h, self.CURVE, d_msgs, d_msg_off, msg_len, d_sigs, d_pks,
                                                        pk_len, d_result, n, stream), "fec_canon_ecdsa_verify_msg_dev")

    def decompress(self, keys, pk_len=33):
        """SEC 1 decoding (secp256k1, P-256): keys (n,pk_len) uint8 -> (xy (n,8), status (n,): 0, or 2 with zeros)."""
        k = _bytes_rows(keys, pk_len, "keys")
        n = k.shape[0]
        xy = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_decompress(self._h, self.CURVE, _ptr(k), pk_len, _ptr(xy), _ptr(st), n), "fec_canon_decompress")
        return xy, st

    def decompress_dev(self, d_in, pk_len, d_xy, d_status, n, stream=None):
        _check(self._lib.fec_canon_decompress_dev(self._h, self.CURVE, d_in, pk_len, d_xy, d_status, n, stream),
               "fec_canon_decompress_dev")

    def scalar_muladd(self, a, b, c):
        """a * b + c modulo the group order, element-wise, any 256-bit inputs."""
        aa, bb, cc = _u64(a, 4), _u64(b, 4), _u64(c, 4)
        if not (aa.shape == bb.shape == cc.shape):
            raise ValueError("operands differ in shape")
        out = np.empty_like(aa)
        _check(self._lib.fec_canon_scalar_op(self._h, self.CURVE, 0, _ptr(aa), _ptr(bb), _ptr(cc), _ptr(out), aa.shape[0]),
               "fec_canon_scalar_op")
        return out

    def scalar_inv(self, a):
        """a^-1 modulo the group order (0 for a = 0)."""
        aa = _u64(a, 4)
        out = np.empty_like(aa)
        _check(self._lib.fec_canon_scalar_op(self._h, self.CURVE, 1, _ptr(aa), None, None, _ptr(out), aa.shape[0]),
               "fec_canon_scalar_op")
        return out

    def ecdsa_sign(self, z, d, k):
        """ECDSA signing with caller-supplied nonces k (e.g. RFC 6979): r = x(k G) mod n, s = k^-1 (z + r d).
        -> (r, s, ok) with ok[i] = 0 where r or s came out 0 (the caller picks another nonce).  All arithmetic
        on the GPU: one comb pass and three scalar-field passes.

        NOT FOR PRODUCTION SECRETS: the comb indexes its table by digits of k, skips zero digits and takes
        wave-level branches on exceptional cases (include/fecgpu_canon.h) -- the nonce and the key are not
        handled in constant time.  This helper exists to check the arithmetic against RFC 6979 / FIPS
        vectors (test keys).  The ctx staging that held k and d is zeroed before returning."""
        kk = _u64(k, 4)
        one = np.zeros_like(kk)
        one[:, 0] = 1
        zero = np.zeros_like(kk)
        xy, st = self.mul_base(kk)
        r = self.scalar_muladd(xy[:, :4], one, zero)                       # x mod n
        s = self.scalar_muladd(self.scalar_inv(kk), self.scalar_muladd(r, d, z), zero)
        ok = ((st == 0) & r.any(axis=1) & s.any(axis=1)).astype(np.uint8)
        self._lib.fec_ctx_wipe(self._h)
        return r, s, ok

    def mul_base_dev(self, d_scalars, d_out_xy, d_status, n, stream=None):
        _check(self._lib.fec_canon_mul_base_dev(self._h, self.CURVE, d_scalars, d_out_xy, d_status, n, stream),
               "fec_canon_mul_base_dev")

    def mul_dev(self, d_scalars, d_points_xy, d_out_xy, d_status, n, stream=None):
        _check(self._lib.fec_canon_mul_dev(self._h, self.CURVE, d_scalars, d_points_xy, d_out_xy, d_status, n, stream),
               "fec_canon_mul_dev")

    def field_op(self, op, a, b=None):
        x = _u64(a, 4)
        y = _u64(b, 4) if b is not None else None
        if y is not None and y.shape != x.shape:
            raise ValueError("operands differ in shape")
        out = np.empty_like(x)
        _check(self._lib.fec_canon_field_op(self._h, self.CURVE, op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]),
               "fec_canon_field_op")
        return out


def _four(lib_fn, h, a, b, c, d, what):
    aa, bb, cc, dd = _u64(a, 4), _u64(b, 4), _u64(c, 4), _u64(d, 4)
    n = aa.shape[0]
    if not (bb.shape[0] == cc.shape[0] == dd.shape[0] == n):
        raise ValueError("inputs differ in length")
    out = np.zeros(n, dtype=np.uint8)
    _check(lib_fn(h, _ptr(aa), _ptr(bb), _ptr(cc), _ptr(dd), _ptr(out), n), what)
    return out


class CanonSecp256k1(CanonCurve):
    CURVE = L.SECP256K1
    SCHEME = L.SECP256K1

    def bip340_sign_msg(self, msgs, keys, aux):
        """BIP-340 default signing: msgs a list of n byte strings (any length), keys (n,32), aux (n,32) -> (sigs, status)."""
        return _sign_msg(self._lib.fec_canon_bip340_sign_msg, self._h, msgs, [keys, aux], "fec_canon_bip340_sign_msg")

    def bip340_sign_msg_dev(self, d_msgs, d_msg_off, msg_len, d_keys, d_aux, d_sigs, d_status, n, stream=None):
        _check(self._lib.fec_canon_bip340_sign_msg_dev(self._h, d_msgs, d_msg_off, msg_len, d_keys, d_aux, d_sigs, d_status, n,
                                                       stream), "fec_canon_bip340_sign_msg_dev")

    def bip340_verify(self, pk_x, r, s, e):
        """BIP-340 Schnorr verification; e = int(tagged_hash("BIP0340/challenge", r || pk || m)).  (n,) uint8."""
        return _four(self._lib.fec_canon_bip340_verify, self._h, pk_x, r, s, e, "fec_canon_bip340_verify")

    def bip340_verify_dev(self, d_pk_x, d_r, d_s, d_e, d_result, n, stream=None):
        _check(self._lib.fec_canon_bip340_verify_dev(self._h, d_pk_x, d_r, d_s, d_e, d_result, n, stream),
               "fec_canon_bip340_verify_dev")

    def bip340_verify_msg(self, msgs, sigs, pks):
        """BIP-340 verification from the message: msgs a list of n byte strings (any length), sigs (n,64), pks (n,32)
        x-only keys.  (n,) uint8, 1 = valid."""
        return _verify_msg(self._lib.fec_canon_bip340_verify_msg, self._h, msgs, sigs, pks, 32, "fec_canon_bip340_verify_msg")

    def bip340_verify_msg_dev(self, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, d_result, n, stream=None):
        _check(self._lib.fec_canon_bip340_verify_msg_dev(self._h, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, d_result, n,
                                                         stream), "fec_canon_bip340_verify_msg_dev")

    def bip340_batch_verify_msg(self, msgs, sigs, pks, seed=None):
        """BIP-340 batch verification (one random linear combination over the batch): -> (ok, status (n,) uint8, verdict).
        status[i]: 0 admitted, 2 the key or R does not decode, 3 s >= n; verdict: 1 iff the equation holds over the admitted
        elements; ok = verdict == 1 and no status set = every signature is valid.  verdict 0 does not say which signature
        is bad: bip340_verify_msg does.  seed: 32 bytes, unpredictable to whoever chose the signatures and fresh per call;
        None draws them from the operating system.  A fixed seed is for tests."""
        return _batch_verify_msg(self._lib.fec_canon_bip340_batch_verify_msg, self._h, msgs, sigs, pks, seed, "fec_canon_bip340_batch_verify_msg")

    def bip340_batch_verify_msg_dev(self, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, seed, d_status, d_verdict, n, stream=None):
        """seed: 32 bytes in host memory (bytes or an array) or None; only enqueues."""
        p, _keep = _batch_seed(seed)
        _check(self._lib.fec_canon_bip340_batch_verify_msg_dev(self._h, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, p, d_status, d_verdict, n,
                                                               stream), "fec_canon_bip340_batch_verify_msg_dev")

    def taproot_output_key(self, pks, roots=None, pk_len=32):
        """Taproot output keys (BIP-341): pks (n,pk_len), pk_len 32 (x-only) or 33 (tag 2 / 3, ignored); roots (n,32) Merkle
        roots or None (no script tree, BIP-86) -> (output keys (n,32) x-only, parity of y (n,), status).  status: 0, 2 (the key
        is refused), 3 / 8 (unobservable), zeros then."""
        pk = _bytes_rows(pks, pk_len, "pks")
        n = pk.shape[0]
        rt = None if roots is None else _bytes_rows(roots, 32, "roots")
        if rt is not None and rt.shape[0] != n:
            raise ValueError("inputs differ in length")
        out = np.zeros((n, 32), dtype=np.uint8)
        par, st = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_taproot_output_key(self._h, _ptr(pk), pk_len, None if rt is None else _ptr(rt), _ptr(out), _ptr(par),
                                                      _ptr(st), n), "fec_canon_taproot_output_key")
        return out, par, st

    def taproot_output_key_dev(self, d_pks, pk_len, d_roots, d_out_keys, d_out_parity, d_status, n, stream=None):
        """d_roots: None for no script tree."""
        _check(self._lib.fec_canon_taproot_output_key_dev(self._h, d_pks, pk_len, d_roots, d_out_keys, d_out_parity, d_status, n,
                                                          stream), "fec_canon_taproot_output_key_dev")


class CanonP256(CanonCurve):
    CURVE = L.P256
    SCHEME = L.P256


class CanonEd25519(CanonCurve):
    """Ed25519 (RFC 8032): affine (x, y) of k*B / k*P; there is no point at infinity, status is 0 or 2."""
    CURVE = L.ED25519
    SCHEME = L.ED25519

    def ed25519_sign_msg(self, msgs, seeds, with_keys=True):
        """RFC 8032 Ed25519 signing: msgs a list of n byte strings, seeds (n,32) -> (sigs (n,64), pks (n,32) or None, status)."""
        n = len(msgs)
        pks = np.zeros((n, 32), dtype=np.uint8) if with_keys else None
        sigs, st = _sign_msg(self._lib.fec_canon_ed25519_sign_msg, self._h, msgs, [seeds], "fec_canon_ed25519_sign_msg",
                             after=(_ptr(pks) if with_keys else None,))
        return sigs, pks, st

    def ed25519_sign_msg_dev(self, d_msgs, d_msg_off, msg_len, d_seeds, d_sigs, d_pks_out, d_status, n, stream=None):
        _check(self._lib.fec_canon_ed25519_sign_msg_dev(self._h, d_msgs, d_msg_off, msg_len, d_seeds, d_sigs, d_pks_out, d_status,
                                                        n, stream), "fec_canon_ed25519_sign_msg_dev")

    def eddsa_verify(self, a_enc, r_enc, s, h):
        """RFC 8032 verification; encodings as little-endian 256-bit integers, h = SHA-512(R||A||M) mod l."""
        return _four(self._lib.fec_canon_eddsa_verify, self._h, a_enc, r_enc, s, h, "fec_canon_eddsa_verify")

    def ed25519_verify_msg(self, msgs, sigs, pks):
        """RFC 8032 Ed25519 verification from the message: msgs a list of n byte strings, sigs (n,64) R || S, pks (n,32).
        (n,) uint8, 1 = valid."""
        return _verify_msg(self._lib.fec_canon_ed25519_verify_msg, self._h, msgs, sigs, pks, 32, "fec_canon_ed25519_verify_msg")

    def ed25519_batch_verify_msg(self, msgs, sigs, pks, seed=None):
        """Ed25519 batch verification by the COFACTORED equation: -> (ok, status (n,) uint8, verdict), as
        CanonSecp256k1.bip340_batch_verify_msg (status 3: S >= l).  Everything ed25519_verify_msg accepts is accepted here; a
        signature whose defect S B - h A - R is a non-zero torsion point is accepted here and refused there."""
        return _batch_verify_msg(self._lib.fec_canon_ed25519_batch_verify_msg, self._h, msgs, sigs, pks, seed, "fec_canon_ed25519_batch_verify_msg")

    def ed25519_batch_verify_msg_dev(self, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, seed, d_status, d_verdict, n, stream=None):
        """seed: 32 bytes in host memory (bytes or an array) or None; only enqueues."""
        p, _keep = _batch_seed(seed)
        _check(self._lib.fec_canon_ed25519_batch_verify_msg_dev(self._h, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, p, d_status, d_verdict, n,
                                                                stream), "fec_canon_ed25519_batch_verify_msg_dev")

    def ed25519_verify_msg_dev(self, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, d_result, n, stream=None):
        _check(self._lib.fec_canon_ed25519_verify_msg_dev(self._h, d_msgs, d_msg_off, msg_len, d_sigs, d_pks, d_result, n,
                                                          stream), "fec_canon_ed25519_verify_msg_dev")

    def eddsa_sign_finish(self, h, a, r):
        """second half of RFC 8032 signing: S = h * a + r (mod l); the first half is R = mul_base(r).
        NOT FOR PRODUCTION SECRETS (see ecdsa_sign): vector-checking only; the ctx staging is zeroed after."""
        out = self.scalar_muladd(h, a, r)
        self._lib.fec_ctx_wipe(self._h)
        return out

    def eddsa_verify_dev(self, d_a_enc, d_r_enc, d_s, d_h, d_result, n, stream=None):
        _check(self._lib.fec_canon_eddsa_verify_dev(self._h, d_a_enc, d_r_enc, d_s, d_h, d_result, n, stream),
               "fec_canon_eddsa_verify_dev")


class CanonX25519:
    """X25519 (RFC 7748 section 5): byte strings in, byte strings out -- scalars, u-coordinates and results are (n,32) uint8,
    little-endian, exactly what other libraries exchange.  Not a CanonCurve: there are no points here, only u."""

    def __init__(self, ctx=None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self._lib = self.ctx._lib
        self._h = self.ctx._h

    def x25519(self, scalars, us):
        """(out (n,32), status): out[i] = X25519(scalars[i], us[i]); status 7 (L.CANON_ZERO_SHARED): the output is all zero
        (a low-order u), which RFC 7748 section 6.1 lets a caller refuse."""
        k, u = _bytes_rows(scalars, 32, "scalars"), _bytes_rows(us, 32, "us")
        n = k.shape[0]
        if u.shape[0] != n:
            raise ValueError("inputs differ in length")
        out = np.zeros((n, 32), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_x25519(self._h, _ptr(k), _ptr(u), _ptr(out), _ptr(st), n), "fec_canon_x25519")
        return out, st

    def x25519_dev(self, d_scalars, d_us, d_out, d_status, n, stream=None):
        _check(self._lib.fec_canon_x25519_dev(self._h, d_scalars, d_us, d_out, d_status, n, stream), "fec_canon_x25519_dev")

    def x25519_base(self, scalars):
        """(n,32): the public keys X25519(scalars[i], 9), through the Ed25519 secret comb and the birational map."""
        k = _bytes_rows(scalars, 32, "scalars")
        n = k.shape[0]
        out = np.zeros((n, 32), dtype=np.uint8)
        _check(self._lib.fec_canon_x25519_base(self._h, _ptr(k), _ptr(out), n), "fec_canon_x25519_base")
        return out

    def x25519_base_dev(self, d_scalars, d_out, n, stream=None):
        _check(self._lib.fec_canon_x25519_base_dev(self._h, d_scalars, d_out, n, stream), "fec_canon_x25519_base_dev")


class CanonKeccak:
    """The curve-less hashes.  Keccak-256 as Ethereum uses it (padding 0x01, not SHA3-256's 0x06): a list of n byte strings ->
    (n,32) uint8.  RIPEMD-160 and HASH160 = RIPEMD-160(SHA-256(.)), Bitcoin's key hash: -> (n,20) uint8."""

    def __init__(self, ctx=None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self._lib = self.ctx._lib
        self._h = self.ctx._h

    def keccak256(self, msgs):
        buf, off, total = Context._messages(msgs)
        n = len(off) - 1
        out = np.zeros((n, 32), dtype=np.uint8)
        _check(self._lib.fec_canon_keccak256(self._h, _ptr(buf), _ptr(off), total, _ptr(out), n), "fec_canon_keccak256")
        return out

    def keccak256_dev(self, d_msgs, d_msg_off, msg_len, d_out, d_status, n, stream=None):
        """d_status may be None; else 4 marks a bad range (zero digest)."""
        _check(self._lib.fec_canon_keccak256_dev(self._h, d_msgs, d_msg_off, msg_len, d_out, d_status, n, stream),
               "fec_canon_keccak256_dev")

    def _digest20(self, fn, what, msgs):
        buf, off, total = Context._messages(msgs)
        n = len(off) - 1
        out = np.zeros((n, 20), dtype=np.uint8)
        _check(fn(self._h, _ptr(buf), _ptr(off), total, _ptr(out), n), what)
        return out

    def ripemd160(self, msgs):
        """RIPEMD-160: a list of n byte strings -> (n,20) uint8."""
        return self._digest20(self._lib.fec_canon_ripemd160, "fec_canon_ripemd160", msgs)

    def ripemd160_dev(self, d_msgs, d_msg_off, msg_len, d_out, d_status, n, stream=None):
        """d_out 4-byte aligned; d_status may be None; else 4 marks a bad range (zero digest)."""
        _check(self._lib.fec_canon_ripemd160_dev(self._h, d_msgs, d_msg_off, msg_len, d_out, d_status, n, stream),
               "fec_canon_ripemd160_dev")

    def hash160(self, msgs):
        """HASH160 = RIPEMD-160(SHA-256(.)): a list of n byte strings -> (n,20) uint8."""
        return self._digest20(self._lib.fec_canon_hash160, "fec_canon_hash160", msgs)

    def hash160_dev(self, d_msgs, d_msg_off, msg_len, d_out, d_status, n, stream=None):
        _check(self._lib.fec_canon_hash160_dev(self._h, d_msgs, d_msg_off, msg_len, d_out, d_status, n, stream),
               "fec_canon_hash160_dev")

    def pubkey_hash160(self, pks, pk_len=33):
        """HASH160 of (n,pk_len) records as their bytes lie, pk_len 33 or 65 -> (n,20) uint8: P2PKH / P2WPKH programs."""
        pk = _bytes_rows(pks, pk_len, "pks")
        n = pk.shape[0]
        out = np.zeros((n, 20), dtype=np.uint8)
        _check(self._lib.fec_canon_pubkey_hash160(self._h, _ptr(pk), pk_len, _ptr(out), n), "fec_canon_pubkey_hash160")
        return out

    def pubkey_hash160_dev(self, d_pks, pk_len, d_out, n, stream=None):
        _check(self._lib.fec_canon_pubkey_hash160_dev(self._h, d_pks, pk_len, d_out, n, stream), "fec_canon_pubkey_hash160_dev")


class CanonBip32:
    """BIP-32 child key derivation on secp256k1: CKDpub and CKDpriv over batches of (parent, chain code, index).  Parents and
    chain codes are (n,33) / (n,32) uint8 arrays, lists of byte strings or bytes; ONE parent -- given as bytes or as a (1,33) /
    (1,32) array -- with n > 1 indices is the shared-parent case (one xpub, many children).  status: 0, 2 / 6 (bad parent
    public / secret key), 9 (L.CANON_BAD_INDEX), 10 (L.CANON_BIP32_INVALID: take the next index; unobservable); zeros then."""

    def __init__(self, ctx=None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self._lib = self.ctx._lib
        self._h = self.ctx._h

    @staticmethod
    def _parents(keys, width, ccs, n):
        k, c = _bytes_rows(keys, width, "parents"), _bytes_rows(ccs, 32, "chain codes")
        if k.shape[0] != c.shape[0] or k.shape[0] not in (n, 1):
            raise ValueError("parents and chain codes must number the indices, or one")
        return k, c

    def derive_pub(self, parent_pks, parent_ccs, indices):
        """CKDpub: (child keys (n,33), child chain codes (n,32), status); an index >= 2^31 gets status 9."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32)).reshape(-1)
        n = idx.shape[0]
        pk, cc = self._parents(parent_pks, 33, parent_ccs, n)
        out, occ = np.zeros((n, 33), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_bip32_derive_pub(self._h, _ptr(pk), _ptr(cc), pk.shape[0], _ptr(idx), _ptr(out), _ptr(occ), _ptr(st), n),
               "fec_canon_bip32_derive_pub")
        return out, occ, st

    def derive_pub_dev(self, d_parent_pks, d_parent_ccs, n_par, d_indices, d_out_pks, d_out_ccs, d_status, n, stream=None):
        _check(self._lib.fec_canon_bip32_derive_pub_dev(self._h, d_parent_pks, d_parent_ccs, n_par, d_indices, d_out_pks, d_out_ccs,
                                                        d_status, n, stream), "fec_canon_bip32_derive_pub_dev")

    def derive_pub_path(self, parent_pks, parent_ccs, indices, fingerprints=True, hash160=True):
        """CKDpub along a path: indices (n,depth), depth 1..255 -> (child keys (n,33), chain codes (n,32), fingerprints (n,4) or
        None, HASH160 of the child keys (n,20) or None, status); the status is the first of the chain that is not 0.  The
        fingerprint is that of the last level's parent, as the child's xpub record carries it."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
        if idx.ndim != 2:
            raise ValueError("indices: one row of the path's indices per element")
        n, depth = idx.shape
        pk, cc = self._parents(parent_pks, 33, parent_ccs, n)
        out, occ = np.zeros((n, 33), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
        fp = np.zeros((n, 4), dtype=np.uint8) if fingerprints else None
        h160 = np.zeros((n, 20), dtype=np.uint8) if hash160 else None
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_bip32_derive_pub_path(self._h, _ptr(pk), _ptr(cc), pk.shape[0], _ptr(idx), depth, _ptr(out), _ptr(occ),
                                                         _ptr(fp) if fingerprints else None, _ptr(h160) if hash160 else None,
                                                         _ptr(st), n), "fec_canon_bip32_derive_pub_path")
        return out, occ, fp, h160, st

    def derive_pub_path_dev(self, d_parent_pks, d_parent_ccs, n_par, d_indices, depth, d_out_pks, d_out_ccs, d_out_fingerprints,
                            d_out_hash160, d_status, n, stream=None):
        """d_out_fingerprints, d_out_hash160: None where not wanted."""
        _check(self._lib.fec_canon_bip32_derive_pub_path_dev(self._h, d_parent_pks, d_parent_ccs, n_par, d_indices, depth, d_out_pks,
                                                             d_out_ccs, d_out_fingerprints, d_out_hash160, d_status, n, stream),
               "fec_canon_bip32_derive_pub_path_dev")

    def derive_priv(self, parent_keys, parent_ccs, indices, flags=0):
        """CKDpriv, hardened and non-hardened indices mixed: (child keys (n,32), child chain codes (n,32), status).
        flags = L.CANON_BIP32_NO_COMB: every index is hardened, the comb pass is skipped (a non-hardened one gets status 9)."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32)).reshape(-1)
        n = idx.shape[0]
        k, cc = self._parents(parent_keys, 32, parent_ccs, n)
        out, occ = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_canon_bip32_derive_priv(self._h, _ptr(k), _ptr(cc), k.shape[0], _ptr(idx), flags, _ptr(out), _ptr(occ),
                                                     _ptr(st), n), "fec_canon_bip32_derive_priv")
        return out, occ, st

    def derive_priv_dev(self, d_parent_keys, d_parent_ccs, n_par, d_indices, flags, d_out_keys, d_out_ccs, d_status, n, stream=None):
        _check(self._lib.fec_canon_bip32_derive_priv_dev(self._h, d_parent_keys, d_parent_ccs, n_par, d_indices, flags, d_out_keys,
                                                         d_out_ccs, d_status, n, stream), "fec_canon_bip32_derive_priv_dev")


CANON_CURVES = {"secp256k1": CanonSecp256k1, "p256": CanonP256, "ed25519": CanonEd25519}
