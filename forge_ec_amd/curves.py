"""
Host-side mirror of the forge-ec-core trait surface for the batched scalar-multiplication path.

Names follow the reference (forge-ec-core/src/lib.rs): `Curve::multiply` (832), `Curve::generator`
/ `identity` (784-830), `PointProjective::{add,double,negate,is_identity}` (699-748),
`FieldElement::{add,sub,mul,square,neg}` (173-241).  The batched forms (`batch_multiply*`) are what
this backend adds: each replaces a caller-side loop over `Curve::multiply` (ecdsa.rs:313-361,
schnorr.rs:268-284, core lib.rs:944-948).

Everything runs on the GPU through libfecgpu.so (include/fecgpu.h); there is no CPU path here.
Arrays are numpy uint64, little-endian limbs: scalars/field elements (n,4); points (n,12) for
secp256k1/P-256 (X,Y,Z) and (n,16) for Ed25519 (X,Y,Z,T) -- the reference's `to_raw()` layout.
"""
import ctypes

import numpy as np

from . import _lib as L
from ._lib import ED25519, P256, SECP256K1, FecError


def _u64(a, cols=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _check(rc, what=""):
    if rc != 0:
        raise FecError(rc, what)


class Context:
    """One fec_ctx.  Context(device) = one GPU, one stream pair (use one per process per GPU).
    Context(devices=[...]) = the multi-device ctx of fec_ctx_create_multi: the element-wise host-pointer
    calls shard the batch contiguously over the listed devices (an ordinal may repeat: several shard
    workers on one GPU) and write straight into the caller's output; the *_dev calls are not available."""

    def __init__(self, device=0, devices=None):
        self._lib = L.lib()
        h = ctypes.c_void_p()
        if devices is not None:
            devs = [int(d) for d in devices]
            arr = (ctypes.c_int * len(devs))(*devs)
            _check(self._lib.fec_ctx_create_multi(ctypes.byref(h), arr, len(devs)), "fec_ctx_create_multi")
            self.device = devs[0] if devs else 0
        else:
            _check(self._lib.fec_ctx_create(ctypes.byref(h), int(device)), "fec_ctx_create")
            self.device = int(device)
        self._h = h

    def wipe(self):
        """fec_ctx_wipe: zero every ctx-owned device buffer that can hold copies of caller data."""
        _check(self._lib.fec_ctx_wipe(self._h), "fec_ctx_wipe")

    def debug_work_areas(self):
        """fec_debug_work_area_count / _read: test hook, not part of the reference's surface -- the device buffers that
        wipe() clears, read back: a list of (name, uint8 array of the buffer's whole capacity), every child of a
        multi-device ctx in order; an unallocated buffer gives an empty array.  Synchronises; reads only."""
        count = self._lib.fec_debug_work_area_count(self._h)
        _check(min(count, 0), "fec_debug_work_area_count")
        out = []
        for i in range(count):
            size, name = ctypes.c_size_t(0), ctypes.c_char_p()
            rc = self._lib.fec_debug_work_area_read(self._h, i, None, 0, ctypes.byref(size), ctypes.byref(name))
            buf = np.zeros(size.value, dtype=np.uint8)
            if size.value:   # (the first call only asked for the size)
                rc = self._lib.fec_debug_work_area_read(self._h, i, _ptr(buf), buf.size, ctypes.byref(size), ctypes.byref(name))
            _check(rc, "fec_debug_work_area_read")
            out.append((name.value.decode(), buf))
        return out

    def check(self):
        """fec_ctx_check: synchronise, then raise FecError(FEC_E_LAUNCH) if a kernel launched through this ctx since
        the last check reported a fault (the outputs of those launches must not be used).  For the *_dev callers;
        the host-pointer calls check by themselves."""
        _check(self._lib.fec_ctx_check(self._h), "fec_ctx_check")

    def debug_force_fault(self, enabled):
        """fec_ctx_debug_force_fault: test hook -- scheduler kernels raise their fault word at once."""
        _check(self._lib.fec_ctx_debug_force_fault(self._h, 1 if enabled else 0), "fec_ctx_debug_force_fault")

    def debug_set_cus(self, cus):
        """fec_ctx_debug_set_cus: test hook -- scheduler launches are sized as for a device of `cus` compute units
        (0 = the device's own count; larger values are clamped to it)."""
        _check(self._lib.fec_ctx_debug_set_cus(self._h, int(cus)), "fec_ctx_debug_set_cus")

    def set_fixed_prefix_bits(self, bits):
        """fec_ctx_set_fixed_prefix_bits: size of the generator's fixed-base prefix tables (0 = off, default 24)."""
        _check(self._lib.fec_ctx_set_fixed_prefix_bits(self._h, int(bits)), "fec_ctx_set_fixed_prefix_bits")

    def build_fixed_prefix(self, curve):
        """fec_ctx_build_fixed_prefix: attach or build the generator's prefix table of `curve` now (synchronous)."""
        _check(self._lib.fec_ctx_build_fixed_prefix(self._h, int(curve)), "fec_ctx_build_fixed_prefix")

    def set_fixed_prefix_after(self, elements):
        """fec_ctx_set_fixed_prefix_after: a ctx left to its defaults builds a table after this many multiplications by G."""
        _check(self._lib.fec_ctx_set_fixed_prefix_after(self._h, int(elements)), "fec_ctx_set_fixed_prefix_after")

    def set_fixed_prefix_budget(self, percent_of_free_memory):
        """fec_ctx_set_fixed_prefix_budget: share of the device's FREE memory a table may take (default 25 %)."""
        _check(self._lib.fec_ctx_set_fixed_prefix_budget(self._h, int(percent_of_free_memory)), "fec_ctx_set_fixed_prefix_budget")

    def set_side_stream_max(self, elements):
        """fec_ctx_set_side_stream_max: u1*G runs beside u2*Q on the second stream up to this many elements."""
        _check(self._lib.fec_ctx_set_side_stream_max(self._h, int(elements)), "fec_ctx_set_side_stream_max")

    def fixed_prefix_bits(self, curve):
        """fec_ctx_fixed_prefix_bits: bits of the prefix table `curve` has now (0 = none)."""
        r = self._lib.fec_ctx_fixed_prefix_bits(self._h, int(curve))
        _check(min(r, 0), "fec_ctx_fixed_prefix_bits")
        return r

    def device_count(self):
        return int(self._lib.fec_ctx_device_count(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fec_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- host-pointer entry points ----
    def batch_mul(self, curve, scalars, points):
        pl = L.POINT_LIMBS[curve]
        s, p = _u64(scalars, 4), _u64(points, pl)
        if s.shape[0] != p.shape[0]:
            raise ValueError("scalars and points differ in length")
        out = np.empty_like(p)
        _check(self._lib.fec_batch_mul(self._h, curve, _ptr(s), _ptr(p), _ptr(out), s.shape[0]), "fec_batch_mul")
        return out

    def batch_mul_fixed(self, curve, scalars, base):
        pl = L.POINT_LIMBS[curve]
        s, b = _u64(scalars, 4), _u64(base).reshape(pl)
        out = np.empty((s.shape[0], pl), dtype=np.uint64)
        _check(self._lib.fec_batch_mul_fixed(self._h, curve, _ptr(s), _ptr(b), _ptr(out), s.shape[0]),
               "fec_batch_mul_fixed")
        return out

    def batch_double_mul(self, curve, u1, u2, q):
        pl = L.POINT_LIMBS[curve]
        a, b, p = _u64(u1, 4), _u64(u2, 4), _u64(q, pl)
        if not (a.shape[0] == b.shape[0] == p.shape[0]):
            raise ValueError("u1, u2 and q differ in length")
        out = np.empty_like(p)
        _check(self._lib.fec_batch_double_mul(self._h, curve, _ptr(a), _ptr(b), _ptr(p), _ptr(out), a.shape[0]),
               "fec_batch_double_mul")
        return out

    def batch_to_affine(self, curve, points):
        """(xy, inf): xy (n,8) affine limbs, inf (n,) uint8 -- Curve::to_affine per element."""
        pl = L.POINT_LIMBS[curve]
        p = _u64(points, pl)
        xy = np.empty((p.shape[0], 8), dtype=np.uint64)
        inf = np.empty(p.shape[0], dtype=np.uint8)
        _check(self._lib.fec_batch_to_affine(self._h, curve, _ptr(p), _ptr(xy), _ptr(inf), p.shape[0]),
               "fec_batch_to_affine")
        return xy, inf

    def multi_scalar_mul(self, curve, scalars, points):
        """Curve::multi_scalar_multiply: sum_i multiply(points[i], scalars[i]) in the reference's order."""
        pl = L.POINT_LIMBS[curve]
        s, p = _u64(scalars, 4), _u64(points, pl)
        if s.shape[0] != p.shape[0]:
            raise ValueError("scalars and points differ in length")
        out = np.empty(pl, dtype=np.uint64)
        _check(self._lib.fec_multi_scalar_mul(self._h, curve, _ptr(s), _ptr(p), _ptr(out), s.shape[0]),
               "fec_multi_scalar_mul")
        return out

    def debug_fold_terms(self, curve, terms):
        """fec_debug_fold_terms: test hook, not part of the reference's surface -- multi_scalar_mul's ordered fold
        (identity + terms[0] + terms[1] + ..., the reference's Add) on raw points the caller supplies."""
        pl = L.POINT_LIMBS[curve]
        t = _u64(terms, pl)
        out = np.empty(pl, dtype=np.uint64)
        _check(self._lib.fec_debug_fold_terms(self._h, curve, _ptr(t) if t.shape[0] else None, _ptr(out), t.shape[0]),
               "fec_debug_fold_terms")
        return out

    def _ecdsa_verify(self, fn, what, digests, r, s, pk_xy, pk_inf):
        d = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8)).reshape(-1, 32)
        rr, ss, pk = _u64(r, 4), _u64(s, 4), _u64(pk_xy, 8)
        n = d.shape[0]
        if not (rr.shape[0] == ss.shape[0] == pk.shape[0] == n):
            raise ValueError("inputs differ in length")
        inf = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        if inf is not None and inf.shape[0] != n:
            raise ValueError("pk_inf and the signatures differ in length")  # the C side reads n bytes
        out = np.empty(n, dtype=np.uint8)
        _check(fn(self._h, _ptr(d), _ptr(rr), _ptr(ss), _ptr(pk), _ptr(inf), _ptr(out), n), what)
        return out

    def ecdsa_verify_secp256k1(self, digests, r, s, pk_xy, pk_inf=None):
        """Ecdsa::<Secp256k1, D>::verify per signature with the digests supplied (ecdsa.rs:213-281).
        digests (n,32) uint8; r, s (n,4); pk_xy (n,8) raw limbs; pk_inf (n,) uint8 or None.
        Returns (n,) uint8: 1 valid, 0 invalid, 2 = the reference panics."""
        return self._ecdsa_verify(self._lib.fec_ecdsa_verify_secp256k1, "fec_ecdsa_verify_secp256k1", digests, r, s,
                                  pk_xy, pk_inf)

    def ecdsa_verify_p256(self, digests, r, s, pk_xy, pk_inf=None):
        """Ecdsa::<P256, D>::verify per signature, same conventions, in the reference's P-256 scalar
        arithmetic (p256.rs:924-1020, 1409-1432) -- not standard ECDSA: see include/fecgpu.h."""
        return self._ecdsa_verify(self._lib.fec_ecdsa_verify_p256, "fec_ecdsa_verify_p256", digests, r, s, pk_xy,
                                  pk_inf)

    def batch_validate_point(self, curve, xy, inf=None):
        """Curve::validate_point per affine point (x, y, infinity): (n,) uint8, 1 valid / 0 not."""
        p = _u64(xy, 8)
        n = p.shape[0]
        fl = np.ascontiguousarray(np.asarray(inf, dtype=np.uint8)).reshape(-1) if inf is not None else None
        if fl is not None and fl.shape[0] != n:
            raise ValueError("flags and points differ in length")  # the C side reads n bytes
        ok = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_batch_validate_point(self._h, curve, _ptr(p), _ptr(fl), _ptr(ok), n), "fec_batch_validate_point")
        return ok

    def batch_ecdh(self, curve, private_keys, pk_xy, pk_inf=None):
        """KeyExchange::derive_shared_secret per element (secp256k1.rs:1884-1904, p256.rs:2281-2312).  Returns
        (secrets (n,32) uint8, status (n,) uint8): 0 Ok, 1 Err(InvalidPublicKey) (P-256), 2 Err (identity).
        NOT FOR PRODUCTION SECRETS: parity mode reproduces reference behaviour; see include/fecgpu.h."""
        kk, pk = _u64(private_keys, 4), _u64(pk_xy, 8)
        n = kk.shape[0]
        if pk.shape[0] != n:
            raise ValueError("inputs differ in length")
        inf = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        if inf is not None and inf.shape[0] != n:
            raise ValueError("pk_inf and the keys differ in length")  # the C side reads n bytes
        out = np.zeros((n, 32), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_batch_ecdh(self._h, curve, _ptr(kk), _ptr(pk), _ptr(inf), _ptr(out), _ptr(st), n), "fec_batch_ecdh")
        return out, st

    @staticmethod
    def _info(info):
        b = bytes(info) if info is not None else b""
        return (ctypes.c_char_p(b) if b else None), len(b)

    def derive_key(self, curve, secrets, info, out_len):
        """KeyExchange::derive_key per element: curve 0 (secp256k1) HKDF-SHA-256 with a zero salt (secp256k1.rs:1846-1883),
        curve 1 (P-256) the reference's XOR placeholder (p256.rs:2314-2344).  secrets (n, secret_len) uint8 with
        secret_len <= 64, or a list of n equally long byte strings; info one byte string (<= 1024 bytes) or None;
        out_len <= 8128.  Returns (n, out_len) uint8.  See include/fecgpu.h."""
        if isinstance(secrets, (list, tuple)):
            secrets = np.array([list(x) for x in secrets], dtype=np.uint8).reshape(len(secrets), -1)
        sec = np.ascontiguousarray(np.asarray(secrets, dtype=np.uint8))
        if sec.ndim != 2:
            raise ValueError("secrets must be (n, secret_len)")
        n, secret_len = sec.shape
        ip, il = self._info(info)
        keys = np.zeros((n, int(out_len)), dtype=np.uint8)
        _check(self._lib.fec_derive_key(self._h, curve, _ptr(sec) if secret_len else None, secret_len, ip, il, int(out_len),
                                        _ptr(keys) if out_len else None, n), "fec_derive_key")
        return keys

    def _ecdh_inputs(self, private_keys, pk_xy, pk_inf):
        kk, pk = _u64(private_keys, 4), _u64(pk_xy, 8)
        n = kk.shape[0]
        if pk.shape[0] != n:
            raise ValueError("inputs differ in length")
        inf = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        if inf is not None and inf.shape[0] != n:
            raise ValueError("pk_inf and the keys differ in length")  # the C side reads n bytes
        return kk, pk, inf, n

    def ecdh_derive_key(self, curve, private_keys, pk_xy, pk_inf, info, out_len):
        """derive_shared_secret followed by derive_key per element; the x coordinate never leaves the device.  Inputs as
        batch_ecdh and derive_key.  Returns (keys (n, out_len) uint8, status (n,) uint8 as batch_ecdh); a key row is zero
        where its status is not 0.  NOT FOR PRODUCTION SECRETS: see include/fecgpu.h."""
        kk, pk, inf, n = self._ecdh_inputs(private_keys, pk_xy, pk_inf)
        ip, il = self._info(info)
        keys = np.zeros((n, int(out_len)), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_ecdh_derive_key(self._h, curve, _ptr(kk), _ptr(pk), _ptr(inf), ip, il, int(out_len),
                                             _ptr(keys) if out_len else None, _ptr(st), n), "fec_ecdh_derive_key")
        return keys, st

    def ecdh_exchange(self, curve, private_keys, peer_xy, peer_inf, info, out_len):
        """KeyExchange::exchange per element with the caller's private keys (forge-ec-core/src/lib.rs:1154-1174; draw them
        with the reference's Scalar::random): the public key to_affine(multiply(generator(), sk)), then
        derive_shared_secret and derive_key.  Returns (public_xy (n, 8), public_inf (n,), keys (n, out_len) uint8,
        status (n,) uint8 as batch_ecdh); everything is zero where the status is not 0."""
        kk, pk, inf, n = self._ecdh_inputs(private_keys, peer_xy, peer_inf)
        ip, il = self._info(info)
        pub = np.zeros((n, 8), dtype=np.uint64)
        pinf = np.zeros(n, dtype=np.uint8)
        keys = np.zeros((n, int(out_len)), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_ecdh_exchange(self._h, curve, _ptr(kk), _ptr(pk), _ptr(inf), ip, il, int(out_len), _ptr(pub), _ptr(pinf),
                                           _ptr(keys) if out_len else None, _ptr(st), n), "fec_ecdh_exchange")
        return pub, pinf, keys, st

    # ---- HashToCurve (include/fecgpu.h: the readings, and the two facts about the reference's sqrt) ----
    H2C_HASH, H2C_ENCODE = 0, 1
    H2C_SWU, H2C_ICART, H2C_ELLIGATOR2 = 0, 1, 2

    def expand_message_xmd(self, msgs, dst, out_len):
        """expand_message_xmd::<Sha256>(msg, dst || len(dst), out_len) per message (hash_to_curve.rs:380-448; RFC 9380's):
        msgs a list of n byte strings, dst one byte string (<= 255 bytes), out_len <= 8160.  Returns (n, out_len) uint8."""
        buf, off, total = self._messages(msgs)
        n = len(off) - 1
        dp, dl = self._info(dst)
        out = np.zeros((n, int(out_len)), dtype=np.uint8)
        _check(self._lib.fec_expand_message_xmd(self._h, _ptr(buf), _ptr(off), total, dp, dl, int(out_len), _ptr(out) if out_len else None, n),
               "fec_expand_message_xmd")
        return out

    def hash_to_field(self, curve, msgs, dst, count):
        """HashToCurveSwu::hash_to_field(msg, dst, count) per message (hash_to_curve.rs:316-377): (n, count, 4) raw limbs."""
        buf, off, total = self._messages(msgs)
        n = len(off) - 1
        dp, dl = self._info(dst)
        u = np.zeros((n, max(int(count), 0), 4), dtype=np.uint64)
        _check(self._lib.fec_hash_to_field(self._h, curve, _ptr(buf), _ptr(off), total, dp, dl, int(count), _ptr(u), n), "fec_hash_to_field")
        return u

    def map_to_curve(self, curve, u, with_cand=True, with_legs=True):
        """C::map_to_curve on n x 4 raw limbs (secp256k1.rs:1587-1705, p256.rs:2215-2265).  Returns (xy (n, 8), cand (n, 8):
        x then y^2 as computed, or None, legs (n,) uint8 or None)."""
        uu = _u64(u, 4)
        n = uu.shape[0]
        xy = np.zeros((n, 8), dtype=np.uint64)
        cand = np.zeros((n, 8), dtype=np.uint64) if with_cand else None
        legs = np.zeros(n, dtype=np.uint8) if with_legs else None
        _check(self._lib.fec_map_to_curve(self._h, curve, _ptr(uu), _ptr(xy), _ptr(cand), _ptr(legs), n), "fec_map_to_curve")
        return xy, cand, legs

    def _h2c(self, curve, mode, msgs, dst, with_cand, with_legs, method):
        buf, off, total = self._messages(msgs)
        n = len(off) - 1
        maps = 2 if mode == self.H2C_HASH else 1
        dp, dl = self._info(dst)
        out = np.zeros((n, 12), dtype=np.uint64)
        cand = np.zeros((n, maps, 8), dtype=np.uint64) if with_cand else None
        legs = np.zeros((n, maps), dtype=np.uint8) if with_legs else None
        _check(self._lib.fec_hash_to_curve(self._h, curve, mode, method, _ptr(buf), _ptr(off), total, dp, dl, _ptr(out), _ptr(cand),
                                           _ptr(legs), n), "fec_hash_to_curve")
        return out, cand, legs

    def hash_to_curve(self, curve, msgs, dst, with_cand=True, with_legs=True, method=0):
        """hash_to_curve::<C, Sha256>(msg, dst, SimplifiedSwu) per message (hash_to_curve.rs:254-312).  Returns (points
        (n, 12) projective raw limbs, cand (n, 2, 8) or None, legs (n, 2) uint8 or None)."""
        return self._h2c(curve, self.H2C_HASH, msgs, dst, with_cand, with_legs, method)

    def encode_to_curve(self, curve, msgs, dst, with_cand=True, with_legs=True, method=0):
        """encode_to_curve::<C, Sha256>(msg, dst, SimplifiedSwu) per message (hash_to_curve.rs:1030-1056).  Returns (points
        (n, 12), cand (n, 1, 8) or None, legs (n, 1) uint8 or None)."""
        return self._h2c(curve, self.H2C_ENCODE, msgs, dst, with_cand, with_legs, method)

    def curve_hash_to_curve(self, curve, msgs, dst):
        """The trait method C::hash_to_curve::<Sha256>(msg, &tag), dst = tag.as_bytes() = suite_id || dst
        (secp256k1.rs:1712-1769; the default forge-ec-core/src/lib.rs:1550-1581 for P-256).  Returns (xy (n, 8), inf (n,))."""
        buf, off, total = self._messages(msgs)
        n = len(off) - 1
        dp, dl = self._info(dst)
        xy = np.zeros((n, 8), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_curve_hash_to_curve(self._h, curve, _ptr(buf), _ptr(off), total, dp, dl, _ptr(xy), _ptr(inf), n),
               "fec_curve_hash_to_curve")
        return xy, inf

    def ecdsa_sign(self, curve, sk, digests, k):
        """Ecdsa::<C, D>::sign per element (ecdsa.rs:98-211) for secp256k1 / P-256 after the hash and the nonce:
        sk (n,4), digests (n,32) uint8 (h_bytes), k (n,4) from Rfc6979::<C, D>::generate_k.  Returns (r (n,4),
        s (n,4), status (n,) uint8): 0 Ok, 1 Err(InvalidPrivateKey), 2 Err(InvalidScalar), 3 Err(InvalidSignature);
        r = s = one() wherever status != 0.  The reference's signatures, not standard ECDSA; not constant-time --
        see include/fecgpu.h."""
        kk, nn = _u64(sk, 4), _u64(k, 4)
        d = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8)).reshape(-1, 32)
        n = kk.shape[0]
        if not (d.shape[0] == nn.shape[0] == n):
            raise ValueError("inputs differ in length")
        sig = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_ecdsa_sign(self._h, curve, _ptr(kk), _ptr(d), _ptr(nn), _ptr(sig), _ptr(st), n), "fec_ecdsa_sign")
        return sig[:, :4].copy(), sig[:, 4:].copy(), st

    def ecdsa_batch_verify(self, curve, digests, r, s, pk_xy, pk_inf, a):
        """Ecdsa::<C, D>::batch_verify (ecdsa.rs:287-391) for secp256k1 / P-256 with the digests and the weights
        a (n,4) supplied.  Returns (result, detail): result 1 true, 0 false, 2 = the reference panics; detail
        (16,) uint64 = r_sum (12 limbs) and r_scalar_sum (4), zero when the loop returned early."""
        d = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8)).reshape(-1, 32)
        rr, ss, pk, aa = _u64(r, 4), _u64(s, 4), _u64(pk_xy, 8), _u64(a, 4)
        n = d.shape[0]
        if not (rr.shape[0] == ss.shape[0] == pk.shape[0] == aa.shape[0] == n):
            raise ValueError("inputs differ in length")
        inf = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        if inf is not None and inf.shape[0] != n:
            raise ValueError("pk_inf and the signatures differ in length")  # the C side reads n bytes
        res = np.zeros(1, dtype=np.uint8)
        detail = np.zeros(16, dtype=np.uint64)
        _check(self._lib.fec_ecdsa_batch_verify(self._h, curve, _ptr(d), _ptr(rr), _ptr(ss), _ptr(pk), _ptr(inf), _ptr(aa),
                                                n, _ptr(res), _ptr(detail)), "fec_ecdsa_batch_verify")
        return int(res[0]), detail

    def eddsa_verify_ed25519(self, r_xy, r_inf, pk_xy, pk_inf, s, k):
        """Eddsa::<Ed25519, D>::verify / Ed25519::verify from the point computation on (eddsa.rs:174-211,
        430-447): r_xy, pk_xy (n,8) raw limbs; r_inf, pk_inf (n,) uint8 or None; s, k (n,4) scalars
        (k = from_bytes_reduced(hash)).  Returns (n,) uint8: 1 true, 0 false, 2 = the reference panics."""
        rr, pk, ss, kk = _u64(r_xy, 8), _u64(pk_xy, 8), _u64(s, 4), _u64(k, 4)
        n = ss.shape[0]
        if not (rr.shape[0] == pk.shape[0] == kk.shape[0] == n):
            raise ValueError("inputs differ in length")
        flags = []
        for f in (r_inf, pk_inf):
            a = np.ascontiguousarray(np.asarray(f, dtype=np.uint8)).reshape(-1) if f is not None else None
            if a is not None and a.shape[0] != n:
                raise ValueError("flags and signatures differ in length")  # the C side reads n bytes
            flags.append(a)
        out = np.empty(n, dtype=np.uint8)
        _check(self._lib.fec_eddsa_verify_ed25519(self._h, _ptr(rr), _ptr(flags[0]), _ptr(pk), _ptr(flags[1]), _ptr(ss),
                                                  _ptr(kk), _ptr(out), n), "fec_eddsa_verify_ed25519")
        return out

    def batch_compress(self, curve, xy, inf=None):
        """PointAffine::to_bytes of each affine point (x, y, infinity) -> (n, 33) uint8."""
        p = _u64(xy, 8)
        n = p.shape[0]
        fl = np.ascontiguousarray(np.asarray(inf, dtype=np.uint8)) if inf is not None else None
        if fl is not None and fl.shape[0] != n:
            raise ValueError("flags and points differ in length")
        out = np.zeros((n, 33), dtype=np.uint8)
        _check(self._lib.fec_batch_compress(self._h, curve, _ptr(p), _ptr(fl), _ptr(out), n), "fec_batch_compress")
        return out

    def _decode(self, fn, what, curve, data, width):
        b = np.ascontiguousarray(np.asarray(data, dtype=np.uint8)).reshape(-1, width)
        n = b.shape[0]
        xy = np.zeros((n, 8), dtype=np.uint64)
        inf, ok = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _check(fn(self._h, curve, _ptr(b), _ptr(xy), _ptr(inf), _ptr(ok), n), what)
        return xy, inf, ok

    def batch_decompress(self, curve, data33):
        """PointAffine::from_bytes of each 33-byte encoding -> (xy (n,8), infinity (n,), ok (n,)); ok = 0 where
        the reference returns None."""
        return self._decode(self._lib.fec_batch_decompress, "fec_batch_decompress", curve, data33, 33)

    def batch_decode_uncompressed(self, curve, data65):
        """forge-ec-encoding UncompressedPoint::to_affine of each 65-byte encoding."""
        return self._decode(self._lib.fec_batch_decode_uncompressed, "fec_batch_decode_uncompressed", curve, data65, 65)

    def batch_encode_uncompressed(self, curve, xy, inf=None):
        """UncompressedPoint::from_affine -> (n, 65) uint8."""
        p = _u64(xy, 8)
        n = p.shape[0]
        fl = np.ascontiguousarray(np.asarray(inf, dtype=np.uint8)).reshape(-1) if inf is not None else None
        if fl is not None and fl.shape[0] != n:
            raise ValueError("flags and points differ in length")
        out = np.zeros((n, 65), dtype=np.uint8)
        _check(self._lib.fec_batch_encode_uncompressed(self._h, curve, _ptr(p), _ptr(fl), _ptr(out), n),
               "fec_batch_encode_uncompressed")
        return out

    def schnorr_batch_verify_secp256k1(self, pk_xy, r_xy, s, a, e, pk_inf=None, r_inf=None):
        """schnorr::batch_verify::<Secp256k1, D> (schnorr.rs:194-290), challenges e and weights a supplied.
        -> (result bool, sides (16,) uint64 = x,y of both affine sums, sides_inf (2,) uint8)."""
        pk, rr = _u64(pk_xy, 8), _u64(r_xy, 8)
        ss, aa, ee = _u64(s, 4), _u64(a, 4), _u64(e, 4)
        n = ss.shape[0]
        if not (pk.shape[0] == rr.shape[0] == aa.shape[0] == ee.shape[0] == n):
            raise ValueError("inputs differ in length")
        pi = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        ri = np.ascontiguousarray(np.asarray(r_inf, dtype=np.uint8)).reshape(-1) if r_inf is not None else None
        for flags in (pi, ri):
            if flags is not None and flags.shape[0] != n:
                raise ValueError("infinity flags and the signatures differ in length")  # the C side reads n bytes
        res = np.zeros(1, dtype=np.uint8)
        sides = np.zeros(16, dtype=np.uint64)
        sinf = np.zeros(2, dtype=np.uint8)
        _check(self._lib.fec_schnorr_batch_verify_secp256k1(self._h, _ptr(pk), _ptr(pi), _ptr(rr), _ptr(ri), _ptr(ss),
                                                            _ptr(aa), _ptr(ee), n, _ptr(res), _ptr(sides), _ptr(sinf)),
               "fec_schnorr_batch_verify_secp256k1")
        return bool(res[0] == 1), sides, sinf

    def schnorr_batch_verify(self, curve, pk_xy, r_xy, s, a, e, pk_inf=None, r_inf=None):
        """schnorr::batch_verify::<C, D> (schnorr.rs:194-290) for any curve; as the secp256k1 form.  (ED25519: the release
        profile's behaviour; schnorr_batch_verify_ed25519 also says whether a debug build would have panicked.)"""
        pk, rr = _u64(pk_xy, 8), _u64(r_xy, 8)
        ss, aa, ee = _u64(s, 4), _u64(a, 4), _u64(e, 4)
        n = ss.shape[0]
        if not (pk.shape[0] == rr.shape[0] == aa.shape[0] == ee.shape[0] == n):
            raise ValueError("inputs differ in length")
        pi = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        ri = np.ascontiguousarray(np.asarray(r_inf, dtype=np.uint8)).reshape(-1) if r_inf is not None else None
        for flags in (pi, ri):
            if flags is not None and flags.shape[0] != n:
                raise ValueError("infinity flags and the signatures differ in length")
        res = np.zeros(1, dtype=np.uint8)
        sides = np.zeros(16, dtype=np.uint64)
        sinf = np.zeros(2, dtype=np.uint8)
        _check(self._lib.fec_schnorr_batch_verify(self._h, curve, _ptr(pk), _ptr(pi), _ptr(rr), _ptr(ri), _ptr(ss), _ptr(aa),
                                                  _ptr(ee), n, _ptr(res), _ptr(sides), _ptr(sinf)), "fec_schnorr_batch_verify")
        # (ED25519: 2 means the reference panics in to_affine -- not a verified batch)
        return bool(res[0] == 1), sides, sinf

    def schnorr_batch_verify_ed25519(self, pk_xy, r_xy, s, a, e, pk_inf=None, r_inf=None):
        """fec_schnorr_batch_verify_ed25519: schnorr::batch_verify::<Ed25519, D> with the scalar Mul as the reference's
        RELEASE profile runs it (u128 sums wrap).  -> (result 0 / 1 / 2 = the reference panics in to_affine, sides (16,),
        sides_inf (2,), debug_build_panics: a debug build panics on these inputs instead)."""
        pk, rr = _u64(pk_xy, 8), _u64(r_xy, 8)
        ss, aa, ee = _u64(s, 4), _u64(a, 4), _u64(e, 4)
        n = ss.shape[0]
        if not (pk.shape[0] == rr.shape[0] == aa.shape[0] == ee.shape[0] == n):
            raise ValueError("inputs differ in length")
        pi = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        ri = np.ascontiguousarray(np.asarray(r_inf, dtype=np.uint8)).reshape(-1) if r_inf is not None else None
        for flags in (pi, ri):
            if flags is not None and flags.shape[0] != n:
                raise ValueError("infinity flags and the signatures differ in length")
        res = np.zeros(1, dtype=np.uint8)
        sides = np.zeros(16, dtype=np.uint64)
        sinf = np.zeros(2, dtype=np.uint8)
        dbg = np.zeros(1, dtype=np.uint8)
        _check(self._lib.fec_schnorr_batch_verify_ed25519(self._h, _ptr(pk), _ptr(pi), _ptr(rr), _ptr(ri), _ptr(ss), _ptr(aa),
                                                          _ptr(ee), n, _ptr(res), _ptr(sides), _ptr(sinf), _ptr(dbg)),
               "fec_schnorr_batch_verify_ed25519")
        return int(res[0]), sides, sinf, bool(dbg[0])

    def schnorr_verify(self, curve, pk_xy, r_xy, s, e, pk_inf=None, r_inf=None):
        """Schnorr::<C, D>::verify per signature (schnorr.rs:90-140) from the point computation on, the challenges
        e = from_bytes_reduced(hash) supplied: (n,) uint8 -- 1 true, 0 false, 2 = the reference panics."""
        pk, rr, ss, ee = _u64(pk_xy, 8), _u64(r_xy, 8), _u64(s, 4), _u64(e, 4)
        n = ss.shape[0]
        if not (pk.shape[0] == rr.shape[0] == ee.shape[0] == n):
            raise ValueError("inputs differ in length")
        pi = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        ri = np.ascontiguousarray(np.asarray(r_inf, dtype=np.uint8)).reshape(-1) if r_inf is not None else None
        for flags in (pi, ri):
            if flags is not None and flags.shape[0] != n:
                raise ValueError("infinity flags and the signatures differ in length")
        out = np.empty(n, dtype=np.uint8)
        _check(self._lib.fec_schnorr_verify(self._h, curve, _ptr(pk), _ptr(pi), _ptr(rr), _ptr(ri), _ptr(ss), _ptr(ee),
                                            _ptr(out), n), "fec_schnorr_verify")
        return out

    def schnorr_verify_dev(self, curve, d_pk_xy, d_pk_inf, d_r_xy, d_r_inf, d_s, d_e, d_status, n, stream=None):
        _check(self._lib.fec_schnorr_verify_dev(self._h, curve, d_pk_xy, d_pk_inf, d_r_xy, d_r_inf, d_s, d_e, d_status, n,
                                                stream), "fec_schnorr_verify_dev")

    def field_op(self, curve, op, a, b=None):
        x = _u64(a, 4)
        y = _u64(b, 4) if b is not None else None
        if y is not None and y.shape != x.shape:
            raise ValueError("operands differ in shape")
        out = np.empty_like(x)
        _check(self._lib.fec_field_op(self._h, curve, op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]), "fec_field_op")
        return out

    def x25519(self, scalars, u):
        """The reference's x25519(scalar, u) per element (curve25519.rs:1624-1716): scalars and u (n, 32) uint8 byte
        strings; returns (n, 32) uint8.  Parity mode, not RFC 7748 -- see include/fecgpu.h."""
        s = np.ascontiguousarray(np.asarray(scalars, dtype=np.uint8)).reshape(-1, 32)
        q = np.ascontiguousarray(np.asarray(u, dtype=np.uint8)).reshape(-1, 32)
        if s.shape != q.shape:
            raise ValueError("inputs differ in length")
        out = np.zeros_like(s)
        _check(self._lib.fec_x25519(self._h, _ptr(s), _ptr(q), _ptr(out), s.shape[0]), "fec_x25519")
        return out

    @staticmethod
    def _messages(msgs):
        """A list of byte strings -> (the concatenated bytes, the n + 1 offsets) of include/fecgpu.h's message layout."""
        msgs = [bytes(m) for m in msgs]
        off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in msgs], out=off[1:])
        buf = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
        return buf, off, int(off[-1])

    def ed25519_sign(self, private_keys, msgs):
        """Ed25519Signature::sign per element (eddsa.rs:267-356), SHA-512 included: private_keys (n, 32) uint8, msgs a
        list of n byte strings.  Returns (sig (n, 64) uint8, status (n,) uint8: 0, 1 the reference panics, 2 a debug
        build panics).  The reference's signatures, not RFC 8032 -- see include/fecgpu.h."""
        k = np.ascontiguousarray(np.asarray(private_keys, dtype=np.uint8)).reshape(-1, 32)
        buf, off, total = self._messages(msgs)
        n = k.shape[0]
        if len(off) != n + 1:
            raise ValueError("inputs differ in length")
        sig = np.zeros((n, 64), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_ed25519_sign(self._h, _ptr(k), _ptr(buf), _ptr(off), total, _ptr(sig), _ptr(st), n), "fec_ed25519_sign")
        return sig, st

    def ed25519_derive_public_key(self, private_keys):
        """Ed25519Signature::derive_public_key per element (eddsa.rs:450-508): (n, 32) uint8 -> (pk (n, 32) uint8,
        status (n,) uint8)."""
        k = np.ascontiguousarray(np.asarray(private_keys, dtype=np.uint8)).reshape(-1, 32)
        pk = np.zeros_like(k)
        st = np.zeros(k.shape[0], dtype=np.uint8)
        _check(self._lib.fec_ed25519_derive_public_key(self._h, _ptr(k), _ptr(pk), _ptr(st), k.shape[0]),
               "fec_ed25519_derive_public_key")
        return pk, st

    def eddsa_sign_ed25519(self, sk, msgs):
        """EdDsa::<Ed25519, Sha512>::sign per element (eddsa.rs:43-154): sk (n, 4) raw Scalar limbs, msgs a list of n
        byte strings.  Returns (r_xy (n, 8), r_inf (n,), s (n, 4), status (n,))."""
        k = _u64(sk, 4)
        buf, off, total = self._messages(msgs)
        n = k.shape[0]
        if len(off) != n + 1:
            raise ValueError("inputs differ in length")
        r_xy = np.zeros((n, 8), dtype=np.uint64)
        r_inf = np.zeros(n, dtype=np.uint8)
        s = np.zeros((n, 4), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_eddsa_sign_ed25519(self._h, _ptr(k), _ptr(buf), _ptr(off), total, _ptr(r_xy), _ptr(r_inf), _ptr(s),
                                                _ptr(st), n), "fec_eddsa_sign_ed25519")
        return r_xy, r_inf, s, st

    def ed25519_verify(self, public_keys, msgs, sigs):
        """Ed25519Signature::verify per element (eddsa.rs:360-447), decoding and SHA-512 included: public_keys (n, 32)
        uint8, msgs a list of n byte strings, sigs (n, 64) uint8.  Returns (n,) uint8: 1 true, 0 false, 2 the reference
        panics.  The reference's verifier, not RFC 8032 -- see include/fecgpu.h."""
        pk = np.ascontiguousarray(np.asarray(public_keys, dtype=np.uint8)).reshape(-1, 32)
        sg = np.ascontiguousarray(np.asarray(sigs, dtype=np.uint8)).reshape(-1, 64)
        buf, off, total = self._messages(msgs)
        n = pk.shape[0]
        if len(off) != n + 1 or sg.shape[0] != n:
            raise ValueError("inputs differ in length")
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_ed25519_verify(self._h, _ptr(pk), _ptr(buf), _ptr(off), total, _ptr(sg), _ptr(st), n), "fec_ed25519_verify")
        return st

    def eddsa_verify_ed25519_msg(self, pk_xy, pk_inf, msgs, r_xy, r_inf, s):
        """EdDsa::<Ed25519, Sha512>::verify per element (eddsa.rs:156-212), SHA-512 included: pk_xy, r_xy (n, 8) raw
        limbs; pk_inf, r_inf (n,) uint8 or None; msgs a list of n byte strings; s (n, 4) raw Scalar limbs.  Returns
        (n,) uint8: 1 true, 0 false, 2 the reference panics."""
        pk, rr, ss = _u64(pk_xy, 8), _u64(r_xy, 8), _u64(s, 4)
        buf, off, total = self._messages(msgs)
        n = ss.shape[0]
        if not (pk.shape[0] == rr.shape[0] == n) or len(off) != n + 1:
            raise ValueError("inputs differ in length")
        flags = []
        for f in (pk_inf, r_inf):
            a = np.ascontiguousarray(np.asarray(f, dtype=np.uint8)).reshape(-1) if f is not None else None
            if a is not None and a.shape[0] != n:
                raise ValueError("flags and signatures differ in length")  # the C side reads n bytes
            flags.append(a)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_eddsa_verify_ed25519_msg(self._h, _ptr(pk), _ptr(flags[0]), _ptr(buf), _ptr(off), total, _ptr(rr),
                                                      _ptr(flags[1]), _ptr(ss), _ptr(st), n), "fec_eddsa_verify_ed25519_msg")
        return st

    def sha512(self, msgs):
        """SHA-512 of each byte string in msgs on the GPU: (n, 64) uint8."""
        buf, off, total = self._messages(msgs)
        n = len(off) - 1
        out = np.zeros((n, 64), dtype=np.uint8)
        _check(self._lib.fec_sha512(self._h, _ptr(buf), _ptr(off), total, _ptr(out), n), "fec_sha512")
        return out

    def sha256(self, msgs):
        """SHA-256 of each byte string in msgs on the GPU: (n, 32) uint8."""
        buf, off, total = self._messages(msgs)
        n = len(off) - 1
        out = np.zeros((n, 32), dtype=np.uint8)
        _check(self._lib.fec_sha256(self._h, _ptr(buf), _ptr(off), total, _ptr(out), n), "fec_sha256")
        return out

    def ecdsa_verify_msg(self, curve, msgs, r, s, pk_xy, pk_inf=None):
        """Ecdsa::<C, Sha256>::verify per signature FROM THE MESSAGE (ecdsa.rs:213-281), SHA-256 included: curve 0
        (secp256k1) or 1 (P-256); msgs a list of n byte strings; r, s (n, 4); pk_xy (n, 8) raw limbs; pk_inf (n,) uint8 or
        None.  Returns (n,) uint8: 1 valid, 0 invalid, 2 = the reference panics."""
        rr, ss, pk = _u64(r, 4), _u64(s, 4), _u64(pk_xy, 8)
        buf, off, total = self._messages(msgs)
        n = rr.shape[0]
        if not (ss.shape[0] == pk.shape[0] == n) or len(off) != n + 1:
            raise ValueError("inputs differ in length")
        inf = np.ascontiguousarray(np.asarray(pk_inf, dtype=np.uint8)).reshape(-1) if pk_inf is not None else None
        if inf is not None and inf.shape[0] != n:
            raise ValueError("flags and signatures differ in length")  # the C side reads n bytes
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_ecdsa_verify_msg(self._h, curve, _ptr(buf), _ptr(off), total, _ptr(rr), _ptr(ss), _ptr(pk), _ptr(inf),
                                              _ptr(st), n), "fec_ecdsa_verify_msg")
        return st

    def bip340_sign(self, private_keys, msgs):
        """BipSchnorr::sign per element (schnorr.rs:302-420), both SHA-256 passes included: private_keys (n, 32) uint8,
        msgs a list of n byte strings.  Returns (sig (n, 64) uint8, status (n,) uint8: 0 computed, 1 the "test message"
        pattern, 2 the 0..63 fallback).  The reference's signatures, not BIP-340 -- see include/fecgpu.h."""
        k = np.ascontiguousarray(np.asarray(private_keys, dtype=np.uint8)).reshape(-1, 32)
        buf, off, total = self._messages(msgs)
        n = k.shape[0]
        if len(off) != n + 1:
            raise ValueError("inputs differ in length")
        sig = np.zeros((n, 64), dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_bip340_sign(self._h, _ptr(k), _ptr(buf), _ptr(off), total, _ptr(sig), _ptr(st), n), "fec_bip340_sign")
        return sig, st

    def ecdsa_sign_msg(self, curve, sk, msgs):
        """Ecdsa::<C, Sha256>::sign per element FROM THE MESSAGE (ecdsa.rs:98-211), SHA-256 and the RFC 6979 nonce
        (forge-ec-rng/src/rfc6979.rs:58-181) included: curve 0 (secp256k1) or 1 (P-256); sk (n, 4) raw limbs; msgs a list
        of n byte strings.  Returns (r (n,4), s (n,4), status (n,) uint8) as ecdsa_sign: 0 Ok, 1 Err(InvalidPrivateKey),
        2 Err(InvalidScalar), 3 Err(InvalidSignature), 5 the nonce loop gave up (never seen); r = s = one() wherever
        status != 0.  The reference's signatures, not standard ECDSA; not constant-time -- see include/fecgpu.h."""
        kk = _u64(sk, 4)
        buf, off, total = self._messages(msgs)
        n = kk.shape[0]
        if len(off) != n + 1:
            raise ValueError("inputs differ in length")
        sig = np.zeros((n, 8), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_ecdsa_sign_msg(self._h, curve, _ptr(kk), _ptr(buf), _ptr(off), total, _ptr(sig), _ptr(st), n),
               "fec_ecdsa_sign_msg")
        return sig[:, :4].copy(), sig[:, 4:].copy(), st

    def rfc6979_k(self, curve, sk, msgs):
        """Rfc6979::<C, Sha256>::generate_k per element (forge-ec-rng/src/rfc6979.rs:40-181): sk (n, 4) raw limbs, hashed
        as they are (no key check); msgs a list of n byte strings.  Returns (k (n,4), status (n,) uint8: 0, or 5 where
        the loop gave up -- never seen).  The reference's nonces, not RFC 6979 to the letter -- see include/fecgpu.h."""
        return self._rfc6979(curve, None, sk, msgs)

    def debug_rfc6979_k(self, curve, order_override, sk, msgs):
        """fec_debug_rfc6979_k: test hook, not part of the reference's surface -- rfc6979_k with candidates compared
        against order_override (4 limbs, at least 2^254) instead of the curve's order constant."""
        return self._rfc6979(curve, _u64(order_override, 4), sk, msgs)

    def _rfc6979(self, curve, order, sk, msgs):
        kk = _u64(sk, 4)
        buf, off, total = self._messages(msgs)
        n = kk.shape[0]
        if len(off) != n + 1:
            raise ValueError("inputs differ in length")
        k = np.zeros((n, 4), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        if order is None:
            _check(self._lib.fec_rfc6979_k(self._h, curve, _ptr(kk), _ptr(buf), _ptr(off), total, _ptr(k), _ptr(st), n), "fec_rfc6979_k")
        else:
            _check(self._lib.fec_debug_rfc6979_k(self._h, curve, _ptr(order), _ptr(kk), _ptr(buf), _ptr(off), total, _ptr(k), _ptr(st), n),
                   "fec_debug_rfc6979_k")
        return k, st

    def scalar_from_bytes_reduced(self, curve, data):
        """C::Scalar::from_bytes_reduced of 32-byte strings (forge-ec-core/src/lib.rs:320-468; P-256: p256.rs:1301-1331):
        data (n, 32) uint8.  Returns (n, 4) raw limbs.  The reference's function, not a reduction mod n -- see
        include/fecgpu.h."""
        b = np.ascontiguousarray(np.asarray(data, dtype=np.uint8)).reshape(-1, 32)
        out = np.zeros((b.shape[0], 4), dtype=np.uint64)
        _check(self._lib.fec_scalar_from_bytes_reduced(self._h, curve, _ptr(b), _ptr(out), b.shape[0]), "fec_scalar_from_bytes_reduced")
        return out

    def schnorr_challenge(self, curve, r_xy, r_inf, pk_xy, pk_inf, msgs):
        """e = from_bytes_reduced(SHA256(R.to_bytes() || P.to_bytes() || msg)) per element (schnorr.rs:66-81), the e that
        schnorr_verify and the batch verifiers take: r_xy, pk_xy (n, 8) affine raw limbs; r_inf, pk_inf (n,) uint8 or
        None; msgs a list of n byte strings.  Returns (n, 4) raw limbs."""
        r, pk = _u64(r_xy, 8), _u64(pk_xy, 8)
        buf, off, total = self._messages(msgs)
        n = r.shape[0]
        if pk.shape[0] != n or len(off) != n + 1:
            raise ValueError("inputs differ in length")
        flags = []
        for f in (r_inf, pk_inf):
            f = np.ascontiguousarray(np.asarray(f, dtype=np.uint8)).reshape(-1) if f is not None else None
            if f is not None and f.shape[0] != n:
                raise ValueError("flags and points differ in length")  # the C side reads n bytes
            flags.append(f)
        e = np.zeros((n, 4), dtype=np.uint64)
        _check(self._lib.fec_schnorr_challenge(self._h, curve, _ptr(r), _ptr(flags[0]), _ptr(pk), _ptr(flags[1]), _ptr(buf), _ptr(off),
                                               total, _ptr(e), n), "fec_schnorr_challenge")
        return e

    def schnorr_sign_msg(self, curve, sk, msgs, with_bytes=True):
        """Schnorr::<C, Sha256>::sign per element FROM THE MESSAGE (schnorr.rs:43-88), the RFC 6979 nonce and the
        challenge hash included: curve 0 (secp256k1) or 1 (P-256); sk (n, 4) raw limbs, signed as they are (no key check);
        msgs a list of n byte strings.  Returns (r_xy (n, 8), r_inf (n,), s (n, 4), sig_bytes (n, 64) uint8 -- the
        reference's signature_to_bytes -- or None, status (n,) uint8: 0 computed, 1 the "test message" pattern, 5 the
        nonce loop gave up (never seen)).  Not constant-time -- see include/fecgpu.h."""
        kk = _u64(sk, 4)
        buf, off, total = self._messages(msgs)
        n = kk.shape[0]
        if len(off) != n + 1:
            raise ValueError("inputs differ in length")
        r = np.zeros((n, 8), dtype=np.uint64)
        rinf = np.zeros(n, dtype=np.uint8)
        s = np.zeros((n, 4), dtype=np.uint64)
        sb = np.zeros((n, 64), dtype=np.uint8) if with_bytes else None
        st = np.zeros(n, dtype=np.uint8)
        _check(self._lib.fec_schnorr_sign_msg(self._h, curve, _ptr(kk), _ptr(buf), _ptr(off), total, _ptr(r), _ptr(rinf), _ptr(s),
                                              _ptr(sb), _ptr(st), n), "fec_schnorr_sign_msg")
        return r, rinf, s, sb, st

    def curve25519_mul(self, scalars, points):
        """Curve25519::multiply per element (curve25519.rs:1922-1955): scalars (n, 4) raw Scalar limbs, points (n, 8)
        ProjectivePoint X limbs then Z limbs; returns (n, 8) likewise."""
        k, p = _u64(scalars, 4), _u64(points, 8)
        if k.shape[0] != p.shape[0]:
            raise ValueError("inputs differ in length")
        out = np.zeros_like(p)
        _check(self._lib.fec_curve25519_mul(self._h, _ptr(k), _ptr(p), _ptr(out), k.shape[0]), "fec_curve25519_mul")
        return out

    def curve25519_field_op(self, op, a, b=None):
        """Add / Sub / Mul / square / Neg of the reference's Curve25519 field (curve25519.rs:186-336, 490-494) on raw
        limbs (n, 4)."""
        x = _u64(a, 4)
        y = _u64(b, 4) if b is not None else None
        if y is not None and y.shape != x.shape:
            raise ValueError("operands differ in shape")
        if y is None and op in (L.F_ADD, L.F_SUB, L.F_MUL):
            raise ValueError("binary op needs b")
        out = np.empty_like(x)
        _check(self._lib.fec_curve25519_field_op(self._h, op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]),
               "fec_curve25519_field_op")
        return out

    def point_op(self, curve, op, p, q=None):
        pl = L.POINT_LIMBS[curve]
        x = _u64(p, pl)
        y = _u64(q, pl) if q is not None else None
        if y is not None and y.shape != x.shape:
            raise ValueError("operands differ in shape")
        out = np.empty_like(x)
        _check(self._lib.fec_point_op(self._h, curve, op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]), "fec_point_op")
        return out

    # ---- device-pointer entry points (raw addresses, e.g. torch.Tensor.data_ptr()) ----
    def batch_mul_dev(self, curve, d_scalars, d_points, d_out, n, stream=None):
        _check(self._lib.fec_batch_mul_dev(self._h, curve, d_scalars, d_points, d_out, n, stream), "fec_batch_mul_dev")

    def batch_mul_fixed_dev(self, curve, d_scalars, d_base, d_out, n, stream=None):
        _check(self._lib.fec_batch_mul_fixed_dev(self._h, curve, d_scalars, d_base, d_out, n, stream),
               "fec_batch_mul_fixed_dev")

    def batch_double_mul_dev(self, curve, d_u1, d_u2, d_q, d_out, n, stream=None):
        _check(self._lib.fec_batch_double_mul_dev(self._h, curve, d_u1, d_u2, d_q, d_out, n, stream),
               "fec_batch_double_mul_dev")

    # ---- device-resident shards of a multi-device ctx (fec_multi_batch_*_dev): lists with one raw device pointer /
    # count per shard worker; `gathered` a raw device pointer on the consumer-th device or None ----
    @staticmethod
    def _ptr_array(ptrs, n):
        if ptrs is None:
            return None
        if len(ptrs) != n:
            raise ValueError("one entry per device of the ctx")
        return (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(p) if p else 0) for p in ptrs])

    def _multi_dev(self, fn, what, curve, inputs, d_out, counts, gathered, consumer, streams):
        n = self.device_count()
        if len(counts) != n:
            raise ValueError("one count per device of the ctx")
        cnt = (ctypes.c_size_t * n)(*[int(c) for c in counts])
        args = [self._ptr_array(a, n) for a in inputs] + [self._ptr_array(d_out, n), cnt,
                                                          ctypes.c_void_p(int(gathered)) if gathered else None, int(consumer),
                                                          self._ptr_array(streams, n)]
        _check(fn(self._h, int(curve), *args), what)

    def multi_batch_mul_dev(self, curve, d_scalars, d_points, d_out, counts, gathered=None, consumer=0, streams=None):
        self._multi_dev(self._lib.fec_multi_batch_mul_dev, "fec_multi_batch_mul_dev", curve, [d_scalars, d_points], d_out,
                        counts, gathered, consumer, streams)

    def multi_batch_mul_fixed_dev(self, curve, d_scalars, d_bases, d_out, counts, gathered=None, consumer=0, streams=None):
        self._multi_dev(self._lib.fec_multi_batch_mul_fixed_dev, "fec_multi_batch_mul_fixed_dev", curve, [d_scalars, d_bases],
                        d_out, counts, gathered, consumer, streams)

    def multi_batch_double_mul_dev(self, curve, d_u1, d_u2, d_q, d_out, counts, gathered=None, consumer=0, streams=None):
        self._multi_dev(self._lib.fec_multi_batch_double_mul_dev, "fec_multi_batch_double_mul_dev", curve, [d_u1, d_u2, d_q],
                        d_out, counts, gathered, consumer, streams)

    def batch_to_affine_dev(self, curve, d_points, d_xy, d_inf, n, stream=None):
        _check(self._lib.fec_batch_to_affine_dev(self._h, curve, d_points, d_xy, d_inf, n, stream),
               "fec_batch_to_affine_dev")

    def batch_compress_dev(self, curve, d_xy, d_inf, d_out, n, stream=None):
        _check(self._lib.fec_batch_compress_dev(self._h, curve, d_xy, d_inf, d_out, n, stream), "fec_batch_compress_dev")

    def ecdsa_verify_secp256k1_dev(self, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n, stream=None):
        _check(self._lib.fec_ecdsa_verify_secp256k1_dev(self._h, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n,
                                                        stream), "fec_ecdsa_verify_secp256k1_dev")

    def batch_validate_point_dev(self, curve, d_xy, d_inf, d_ok, n, stream=None):
        _check(self._lib.fec_batch_validate_point_dev(self._h, curve, d_xy, d_inf, d_ok, n, stream), "fec_batch_validate_point_dev")

    def batch_ecdh_dev(self, curve, d_private_keys, d_pk_xy, d_pk_inf, d_secrets, d_status, n, stream=None):
        _check(self._lib.fec_batch_ecdh_dev(self._h, curve, d_private_keys, d_pk_xy, d_pk_inf, d_secrets, d_status, n, stream),
               "fec_batch_ecdh_dev")

    def derive_key_dev(self, curve, d_secrets, secret_len, info, out_len, d_keys, n, stream=None):
        """fec_derive_key_dev: `info` is a host byte string (or None), everything else raw device addresses."""
        ip, il = self._info(info)
        _check(self._lib.fec_derive_key_dev(self._h, curve, d_secrets, secret_len, ip, il, out_len, d_keys, n, stream), "fec_derive_key_dev")

    def ecdh_derive_key_dev(self, curve, d_private_keys, d_pk_xy, d_pk_inf, info, out_len, d_keys, d_status, n, stream=None):
        ip, il = self._info(info)
        _check(self._lib.fec_ecdh_derive_key_dev(self._h, curve, d_private_keys, d_pk_xy, d_pk_inf, ip, il, out_len, d_keys, d_status, n,
                                                 stream), "fec_ecdh_derive_key_dev")

    def ecdh_exchange_dev(self, curve, d_private_keys, d_peer_xy, d_peer_inf, info, out_len, d_public_xy, d_public_inf, d_keys, d_status, n,
                          stream=None):
        ip, il = self._info(info)
        _check(self._lib.fec_ecdh_exchange_dev(self._h, curve, d_private_keys, d_peer_xy, d_peer_inf, ip, il, out_len, d_public_xy,
                                               d_public_inf, d_keys, d_status, n, stream), "fec_ecdh_exchange_dev")

    def expand_message_xmd_dev(self, d_msgs, d_msg_off, msg_len, dst, out_len, d_out, d_status, n, stream=None):
        """fec_expand_message_xmd_dev: `dst` is a host byte string (or None), everything else raw device addresses."""
        dp, dl = self._info(dst)
        _check(self._lib.fec_expand_message_xmd_dev(self._h, d_msgs, d_msg_off, msg_len, dp, dl, out_len, d_out, d_status, n, stream),
               "fec_expand_message_xmd_dev")

    def hash_to_field_dev(self, curve, d_msgs, d_msg_off, msg_len, dst, count, d_u, d_status, n, stream=None):
        dp, dl = self._info(dst)
        _check(self._lib.fec_hash_to_field_dev(self._h, curve, d_msgs, d_msg_off, msg_len, dp, dl, count, d_u, d_status, n, stream),
               "fec_hash_to_field_dev")

    def map_to_curve_dev(self, curve, d_u, d_xy, d_cand, d_legs, n, stream=None):
        _check(self._lib.fec_map_to_curve_dev(self._h, curve, d_u, d_xy, d_cand, d_legs, n, stream), "fec_map_to_curve_dev")

    def hash_to_curve_dev(self, curve, d_msgs, d_msg_off, msg_len, dst, d_out, d_cand, d_legs, d_status, n, stream=None, mode=0, method=0):
        dp, dl = self._info(dst)
        _check(self._lib.fec_hash_to_curve_dev(self._h, curve, mode, method, d_msgs, d_msg_off, msg_len, dp, dl, d_out, d_cand, d_legs,
                                               d_status, n, stream), "fec_hash_to_curve_dev")

    def encode_to_curve_dev(self, curve, d_msgs, d_msg_off, msg_len, dst, d_out, d_cand, d_legs, d_status, n, stream=None, method=0):
        self.hash_to_curve_dev(curve, d_msgs, d_msg_off, msg_len, dst, d_out, d_cand, d_legs, d_status, n, stream, self.H2C_ENCODE, method)

    def curve_hash_to_curve_dev(self, curve, d_msgs, d_msg_off, msg_len, dst, d_xy, d_inf, d_status, n, stream=None):
        dp, dl = self._info(dst)
        _check(self._lib.fec_curve_hash_to_curve_dev(self._h, curve, d_msgs, d_msg_off, msg_len, dp, dl, d_xy, d_inf, d_status, n, stream),
               "fec_curve_hash_to_curve_dev")

    def x25519_dev(self, d_scalars, d_u, d_out, n, stream=None):
        _check(self._lib.fec_x25519_dev(self._h, d_scalars, d_u, d_out, n, stream), "fec_x25519_dev")

    def curve25519_mul_dev(self, d_scalars, d_points, d_out, n, stream=None):
        _check(self._lib.fec_curve25519_mul_dev(self._h, d_scalars, d_points, d_out, n, stream), "fec_curve25519_mul_dev")

    def ed25519_sign_dev(self, d_private_keys, d_msgs, d_msg_off, msg_len, d_sig, d_status, n, stream=None):
        _check(self._lib.fec_ed25519_sign_dev(self._h, d_private_keys, d_msgs, d_msg_off, msg_len, d_sig, d_status, n, stream),
               "fec_ed25519_sign_dev")

    def ed25519_derive_public_key_dev(self, d_private_keys, d_public_keys, d_status, n, stream=None):
        _check(self._lib.fec_ed25519_derive_public_key_dev(self._h, d_private_keys, d_public_keys, d_status, n, stream),
               "fec_ed25519_derive_public_key_dev")

    def eddsa_sign_ed25519_dev(self, d_sk, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_status, n, stream=None):
        _check(self._lib.fec_eddsa_sign_ed25519_dev(self._h, d_sk, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_status, n,
                                                    stream), "fec_eddsa_sign_ed25519_dev")

    def ed25519_verify_dev(self, d_public_keys, d_msgs, d_msg_off, msg_len, d_sigs, d_status, n, stream=None):
        _check(self._lib.fec_ed25519_verify_dev(self._h, d_public_keys, d_msgs, d_msg_off, msg_len, d_sigs, d_status, n, stream),
               "fec_ed25519_verify_dev")

    def eddsa_verify_ed25519_msg_dev(self, d_pk_xy, d_pk_inf, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_status, n,
                                     stream=None):
        _check(self._lib.fec_eddsa_verify_ed25519_msg_dev(self._h, d_pk_xy, d_pk_inf, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf,
                                                          d_s, d_status, n, stream), "fec_eddsa_verify_ed25519_msg_dev")

    def sha512_dev(self, d_msgs, d_msg_off, msg_len, d_digests, d_status, n, stream=None):
        _check(self._lib.fec_sha512_dev(self._h, d_msgs, d_msg_off, msg_len, d_digests, d_status, n, stream), "fec_sha512_dev")

    def sha256_dev(self, d_msgs, d_msg_off, msg_len, d_digests, d_status, n, stream=None):
        _check(self._lib.fec_sha256_dev(self._h, d_msgs, d_msg_off, msg_len, d_digests, d_status, n, stream), "fec_sha256_dev")

    def ecdsa_verify_msg_dev(self, curve, d_msgs, d_msg_off, msg_len, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n, stream=None):
        _check(self._lib.fec_ecdsa_verify_msg_dev(self._h, curve, d_msgs, d_msg_off, msg_len, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n,
                                                  stream), "fec_ecdsa_verify_msg_dev")

    def bip340_sign_dev(self, d_private_keys, d_msgs, d_msg_off, msg_len, d_signatures, d_status, n, stream=None):
        _check(self._lib.fec_bip340_sign_dev(self._h, d_private_keys, d_msgs, d_msg_off, msg_len, d_signatures, d_status, n, stream),
               "fec_bip340_sign_dev")

    def ecdsa_sign_msg_dev(self, curve, d_sk, d_msgs, d_msg_off, msg_len, d_sig, d_status, n, stream=None):
        _check(self._lib.fec_ecdsa_sign_msg_dev(self._h, curve, d_sk, d_msgs, d_msg_off, msg_len, d_sig, d_status, n, stream),
               "fec_ecdsa_sign_msg_dev")

    def scalar_from_bytes_reduced_dev(self, curve, d_bytes, d_out, n, stream=None):
        _check(self._lib.fec_scalar_from_bytes_reduced_dev(self._h, curve, d_bytes, d_out, n, stream), "fec_scalar_from_bytes_reduced_dev")

    def schnorr_challenge_dev(self, curve, d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, d_msgs, d_msg_off, msg_len, d_e, d_status, n, stream=None):
        _check(self._lib.fec_schnorr_challenge_dev(self._h, curve, d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, d_msgs, d_msg_off, msg_len, d_e,
                                                   d_status, n, stream), "fec_schnorr_challenge_dev")

    def schnorr_sign_msg_dev(self, curve, d_sk, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_sig_bytes, d_status, n, stream=None):
        _check(self._lib.fec_schnorr_sign_msg_dev(self._h, curve, d_sk, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_sig_bytes,
                                                  d_status, n, stream), "fec_schnorr_sign_msg_dev")

    def rfc6979_k_dev(self, curve, d_sk, d_msgs, d_msg_off, msg_len, d_k, d_status, n, stream=None):
        _check(self._lib.fec_rfc6979_k_dev(self._h, curve, d_sk, d_msgs, d_msg_off, msg_len, d_k, d_status, n, stream), "fec_rfc6979_k_dev")

    def ecdsa_sign_dev(self, curve, d_sk, d_digests, d_k, d_sig, d_status, n, stream=None):
        _check(self._lib.fec_ecdsa_sign_dev(self._h, curve, d_sk, d_digests, d_k, d_sig, d_status, n, stream), "fec_ecdsa_sign_dev")

    def eddsa_verify_ed25519_dev(self, d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, d_s, d_k, d_status, n, stream=None):
        _check(self._lib.fec_eddsa_verify_ed25519_dev(self._h, d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, d_s, d_k, d_status, n,
                                                      stream), "fec_eddsa_verify_ed25519_dev")

    def ecdsa_verify_p256_dev(self, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n, stream=None):
        _check(self._lib.fec_ecdsa_verify_p256_dev(self._h, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n,
                                                   stream), "fec_ecdsa_verify_p256_dev")

    def generator(self, curve):
        out = np.empty(L.POINT_LIMBS[curve], dtype=np.uint64)
        _check(self._lib.fec_generator(self._h, curve, _ptr(out)), "fec_generator")
        return out

    def generator_dev(self, curve):
        """Device address of the ctx's generator (pass it to batch_mul_fixed_dev)."""
        return self._lib.fec_generator_dev(self._h, curve)

    def set_chunk(self, elements):
        """Elements per pipeline chunk of the host-pointer entry points (default 2^18)."""
        _check(self._lib.fec_ctx_set_chunk(self._h, int(elements)))

    def set_canon_msm_window(self, bits):
        """Window width of canonical mode's multi-scalar multiplication (CanonCurve.msm): 0 = chosen from n, 2..16 = forced."""
        _check(self._lib.fec_ctx_set_canon_msm_window(self._h, int(bits)))

    # ---- measurement ----
    def set_timing(self, enabled=True):
        _check(self._lib.fec_ctx_set_timing(self._h, 1 if enabled else 0))

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        name = ctypes.c_char_p()
        _check(self._lib.fec_ctx_last_kernel_ms(self._h, ctypes.byref(ms), ctypes.byref(name)), "last_kernel_ms")
        return float(ms.value), (name.value or b"").decode()

    def measure_peak_mad32(self):
        v = ctypes.c_double()
        _check(self._lib.fec_measure_peak_mad32(self._h, ctypes.byref(v)), "fec_measure_peak_mad32")
        return float(v.value)

    def device_info(self):
        buf = ctypes.create_string_buffer(256)
        cus, khz = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.fec_ctx_device_info(self._h, buf, 256, ctypes.byref(cus), ctypes.byref(khz)))
        return {"name": buf.value.decode(), "compute_units": cus.value, "clock_khz": khz.value}


class _Curve:
    """Common `Curve` trait surface.  Subclasses fix ID, NAME and the reference's constants."""
    ID = None
    NAME = None
    POINT_LIMBS = 12
    _IDENTITY = None

    def __init__(self, ctx=None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)

    # Curve::identity / generator (as the reference builds them, raw limbs)
    @classmethod
    def identity(cls):
        return np.array(cls._IDENTITY, dtype=np.uint64)

    def generator(self):
        return self.ctx.generator(self.ID)

    # Curve::multiply
    def multiply(self, point, scalar):
        return self.ctx.batch_mul(self.ID, _u64(scalar).reshape(1, 4), _u64(point).reshape(1, -1))[0]

    # batched forms
    def batch_multiply(self, points, scalars):
        return self.ctx.batch_mul(self.ID, scalars, points)

    def batch_multiply_fixed(self, base, scalars):
        return self.ctx.batch_mul_fixed(self.ID, scalars, base)

    def batch_double_multiply(self, u1, u2, q):
        """R[i] = multiply(G, u1[i]) + multiply(q[i], u2[i])  (ecdsa.rs:254-256)."""
        return self.ctx.batch_double_mul(self.ID, u1, u2, q)

    def multi_scalar_multiply(self, points, scalars):
        """Curve::multi_scalar_multiply (core lib.rs:934-951): identity for empty or mismatched input."""
        pts, ks = _u64(points, self.POINT_LIMBS), _u64(scalars, 4)
        if pts.shape[0] != ks.shape[0] or pts.shape[0] == 0:
            return self.identity()
        return self.ctx.multi_scalar_mul(self.ID, ks, pts)

    # Curve::to_affine, batched
    def batch_to_affine(self, points):
        return self.ctx.batch_to_affine(self.ID, points)

    # PointProjective
    def add(self, p, q):
        return self.ctx.point_op(self.ID, L.P_ADD, p, q)

    def double(self, p):
        return self.ctx.point_op(self.ID, L.P_DOUBLE, p)

    def negate(self, p):
        return self.ctx.point_op(self.ID, L.P_NEGATE, p)

    # FieldElement
    def fe_add(self, a, b):
        return self.ctx.field_op(self.ID, L.F_ADD, a, b)

    def fe_sub(self, a, b):
        return self.ctx.field_op(self.ID, L.F_SUB, a, b)

    def fe_mul(self, a, b):
        return self.ctx.field_op(self.ID, L.F_MUL, a, b)

    def fe_square(self, a):
        return self.ctx.field_op(self.ID, L.F_SQR, a)

    def fe_neg(self, a):
        return self.ctx.field_op(self.ID, L.F_NEG, a)


class Secp256k1(_Curve):
    ID, NAME, POINT_LIMBS = SECP256K1, "secp256k1", 12
    _IDENTITY = [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]  # secp256k1.rs:1322-1324

    def double_trait(self, p):
        """trait PointProjective::double (secp256k1.rs:1375-1418), not the ladder's inherent one."""
        return self.ctx.point_op(self.ID, L.P_DOUBLE_TRAIT, p)


class P256Curve(_Curve):
    ID, NAME, POINT_LIMBS = P256, "p256", 12
    _IDENTITY = [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]  # p256.rs:1827-1829


class Ed25519Curve(_Curve):
    ID, NAME, POINT_LIMBS = ED25519, "ed25519", 16
    _IDENTITY = [0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]  # ed25519.rs:1776-1783


CURVES = {SECP256K1: Secp256k1, P256: P256Curve, ED25519: Ed25519Curve}
