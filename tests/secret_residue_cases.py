"""
The tables behind tests/test_gpu_secret_residue.py, importable without a GPU (tests/test_work_area_census.py compares
them with the source of forge_ec_amd/csrc):

  HOST_ROWS   one row per extern "C" host-pointer entry point that stages a secret (secret_input / secret_output), some
              entry points more than once (a scheme, a curve, a flag each take another path through the launcher);
  DEV_ROWS    one row per canonical *_dev form whose launcher handles secrets: those that open a SignArea, and the two
              that keep everything in registers and LDS (`work_area` False).

A row knows how to draw its inputs from a seed (`make(seed, n)`), how to run the call (`call(ctx, args)` for the host
forms, `call(ctx, args, n, stream)` for the *_dev forms, which uploads the inputs to torch tensors and returns them with the
output tensors: outs_of reads those once the caller has synchronised) and what the project's model of that call says the
outputs are (`want(args, oracle)`; the tests use it at n = 1).  A host call returns (outs, sts): outs are the arrays that
carry results -- every element's row must be non-zero -- and sts the status and infinity flags, all of which must be 0.
Inputs are drawn so that they are: keys below 2^255 (inside both group orders) and odd, secp256k1 wherever parity mode's
P-256 refuses half of all points, and, where the reference refuses about half of all keys, the elements its model accepts
(`accepted`).
"""
import hashlib

import numpy as np

SECP, P256, ED = 0, 1, 2
INFO = b"secret residue: info"
DST = b"QUUX-V01-CS02-with-residue"
CANON_NAMES = {SECP: "secp256k1", P256: "p256", ED: "ed25519"}
HARDENED = 1 << 31


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(0x5EC0 + seed)


def limbs(rng, n, cols=4):
    """(n, cols) uint64: per 4-limb value below 2^255 and odd"""
    a = rng.integers(0, 1 << 64, size=(n, cols), dtype=np.uint64)
    a[:, 3::4] >>= np.uint64(1)
    a[:, 0::4] |= np.uint64(1)
    return a


def be_keys(rng, n):
    """(n, 32) uint8 big-endian: below 2^255 and odd"""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 0] &= 0x7F
    a[:, 31] |= 1
    return a


def raw_bytes(rng, n, width=32):
    return rng.integers(0, 256, size=(n, width), dtype=np.uint8)


def messages(rng, n):
    """n messages of 1..90 bytes: either side of SHA-256's one-block limit, none of them the reference's "test message" """
    return [rng.integers(0, 256, size=int(L), dtype=np.uint8).tobytes() for L in rng.integers(1, 91, size=n)]


def _val(row):
    return sum(int(x) << (64 * i) for i, x in enumerate(row))


def _rows(bs):
    return np.frombuffer(b"".join(bytes(b) for b in bs), dtype=np.uint8).reshape(len(bs), -1).copy()


def _words(vals, cols=4):
    return np.array([[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(cols)] for v in vals], dtype=np.uint64)


def _flat(rows_of_limbs):
    return np.array([[int(v) for part in r for v in part] for r in rows_of_limbs], dtype=np.uint64)


def accepted(make, status):
    """make, restricted to the elements whose status the MODEL says is 0: parity mode reproduces the reference's answers,
    and the reference refuses about half of all keys in some calls (Ed25519 signing: status 2; secp256k1 ECDSA from the
    message: Err(InvalidSignature)).  Drawn once per (seed, n)."""
    memo = {}

    def filtered(seed, n):
        if (seed, n) not in memo:
            a = make(seed, 6 * n + 24)
            keep = np.flatnonzero(np.asarray(status(a)) == 0)[:n]
            assert len(keep) == n, "the model accepts too few of the drawn inputs"
            memo[seed, n] = {k: ([v[i] for i in keep] if isinstance(v, list) else v[keep]) for k, v in a.items()}
        return memo[seed, n]
    return filtered


def _st_ed_sign(a):
    import eddsa_sign_ref as R
    return [st for _, st in R.sign_batch(a["keys"], a["msgs"], R.CBackend())]


def _st_eddsa(a):
    import eddsa_sign_ref as R
    return [g[4] for g in R.eddsa_sign_batch(a["sk"], a["msgs"], R.CBackend())]


def _st_ecdsa_msg(curve):
    def status(a):
        import rfc6979_ref as R
        from oracle import c_oracle
        c_oracle.lib()
        return R.sign_msg(c_oracle, curve, a["sk"], a["msgs"])[2]
    return status


class Row:
    def __init__(self, id, fn, make, call, want, launcher=None, work_area=True):
        self.id, self.fn, self.make, self.call, self.want = id, fn, make, call, want
        self.launcher, self.work_area = launcher, work_area

    def __repr__(self):
        return self.id


# ---- parity mode, host forms ------------------------------------------------------------------------------------------
def _mk_ecdh(seed, n):
    r = _rng(seed)
    return dict(sk=limbs(r, n), pk=limbs(r, n, 8), inf=np.zeros(n, dtype=np.uint8))


def _ecdh(ctx, a):
    out, st = ctx.batch_ecdh(SECP, a["sk"], a["pk"], a["inf"])
    return [out], [st]


def _w_ecdh(a, oracle):
    return [oracle.batch_ecdh(SECP, a["sk"], a["pk"], a["inf"])[0]]


def _mk_derive(seed, n):
    return dict(sec=raw_bytes(_rng(seed), n))


def _derive(ctx, a):
    return [ctx.derive_key(SECP, a["sec"], INFO, 33)], []


def _w_derive(a, oracle):
    import ecdh_kdf_ref as K
    return [_rows([K.derive_key(SECP, bytes(s), INFO, 33) for s in a["sec"]])]


def _ecdh_derive(ctx, a):
    keys, st = ctx.ecdh_derive_key(SECP, a["sk"], a["pk"], a["inf"], INFO, 33)
    return [keys], [st]


def _w_ecdh_derive(a, oracle):
    import ecdh_kdf_ref as K
    return [K.ecdh_derive_key(oracle, SECP, a["sk"], a["pk"], a["inf"], INFO, 33)[0]]


def _exchange(ctx, a):
    pub, pinf, keys, st = ctx.ecdh_exchange(SECP, a["sk"], a["pk"], a["inf"], INFO, 33)
    return [pub, keys], [pinf, st]


def _w_exchange(a, oracle):
    import ecdh_kdf_ref as K
    xy, _, keys, _ = K.exchange(oracle, SECP, a["sk"], a["pk"], a["inf"], INFO, 33)
    return [xy, keys]


def _mk_ecdsa(seed, n):
    r = _rng(seed)
    return dict(sk=limbs(r, n), dg=raw_bytes(r, n), k=limbs(r, n))


def _ecdsa(curve):
    def call(ctx, a):
        r, s, st = ctx.ecdsa_sign(curve, a["sk"], a["dg"], a["k"])
        return [r, s], [st]

    def want(a, oracle):
        import ecdsa_sign_ref as E
        r, s, _ = E.sign(oracle, curve, a["sk"], a["dg"], a["k"])
        return [r, s]
    return call, want


def _mk_x25519(seed, n):
    r = _rng(seed)
    return dict(k=raw_bytes(r, n), u=raw_bytes(r, n))


def _x25519(ctx, a):
    return [ctx.x25519(a["k"], a["u"])], []


def _w_x25519(a, oracle):
    import x25519_ref as X
    return [_rows([X.x25519(bytes(k), bytes(u)) for k, u in zip(a["k"], a["u"])])]


def _mk_c25519(seed, n):
    r = _rng(seed)
    return dict(k=limbs(r, n), p=limbs(r, n, 8))


def _c25519(ctx, a):
    return [ctx.curve25519_mul(a["k"], a["p"])], []


def _w_c25519(a, oracle):
    import x25519_ref as X
    return [_flat([X.multiply(p[:4], p[4:], k) for k, p in zip(a["k"], a["p"])])]


def _mk_map(seed, n):
    return dict(u=limbs(_rng(seed), n))


def _map(ctx, a):
    xy, cand, _ = ctx.map_to_curve(SECP, a["u"])
    return [xy, cand], []


def _w_map(a, oracle):
    import h2c_ref as H
    got = [H.map_to_curve(SECP, u) for u in a["u"]]
    return [_flat([g[0] for g in got]), _flat([g[1] for g in got])]


def _mk_msgs(seed, n):
    return dict(msgs=messages(_rng(seed), n))


def _digest(name):
    def call(ctx, a):
        return [getattr(ctx, name)(a["msgs"])], []

    def want(a, oracle):
        return [_rows([getattr(hashlib, name)(m).digest() for m in a["msgs"]])]
    return call, want


def _mk_keys_msgs(seed, n):
    r = _rng(seed)
    return dict(keys=raw_bytes(r, n), msgs=messages(r, n))


def _ed_sign(ctx, a):
    sig, st = ctx.ed25519_sign(a["keys"], a["msgs"])
    return [sig], [st]


def _w_ed_sign(a, oracle):
    import eddsa_sign_ref as R
    return [_rows([s for s, _ in R.sign_batch(a["keys"], a["msgs"], R.CBackend())])]


def _ed_derive(ctx, a):
    pk, st = ctx.ed25519_derive_public_key(a["keys"])
    return [pk], [st]


def _w_ed_derive(a, oracle):
    import eddsa_sign_ref as R
    return [_rows([p for p, _ in R.derive_batch(a["keys"], R.CBackend())])]


def _mk_sk_msgs(seed, n):
    r = _rng(seed)
    return dict(sk=limbs(r, n), msgs=messages(r, n))


def _eddsa(ctx, a):
    r_xy, r_inf, s, st = ctx.eddsa_sign_ed25519(a["sk"], a["msgs"])
    return [r_xy, s], [r_inf, st]


def _w_eddsa(a, oracle):
    import eddsa_sign_ref as R
    got = R.eddsa_sign_batch(a["sk"], a["msgs"], R.CBackend())
    return [_flat([(g[0], g[1]) for g in got]), _flat([(g[3],) for g in got])]


def _bip340(ctx, a):
    sig, st = ctx.bip340_sign(a["keys"], a["msgs"])
    return [sig], [st]


def _w_bip340(a, oracle):
    import bip340_sign_ref as R
    return [_rows([s for s, _ in R.sign_batch(a["keys"], a["msgs"], R.CBackend())])]


def _ecdsa_msg(curve):
    def call(ctx, a):
        r, s, st = ctx.ecdsa_sign_msg(curve, a["sk"], a["msgs"])
        return [r, s], [st]

    def want(a, oracle):
        import rfc6979_ref as R
        r, s, _, _ = R.sign_msg(oracle, curve, a["sk"], a["msgs"])
        return [r, s]
    return call, want


def _rfc6979(ctx, a):
    k, st = ctx.rfc6979_k(SECP, a["sk"], a["msgs"])
    return [k], [st]


def _w_rfc6979(a, oracle):
    import rfc6979_ref as R
    return [R.nonces(SECP, a["sk"], a["msgs"])[0]]


def _debug_rfc6979(ctx, a):
    k, st = ctx.debug_rfc6979_k(SECP, _words([1 << 255])[0], a["sk"], a["msgs"])
    return [k], [st]


def _w_debug_rfc6979(a, oracle):
    import rfc6979_ref as R
    return [R.nonces(SECP, a["sk"], a["msgs"], order=1 << 255)[0]]


def _schnorr(curve):
    def call(ctx, a):
        r, rinf, s, sb, st = ctx.schnorr_sign_msg(curve, a["sk"], a["msgs"])
        return [r, s, sb], [rinf, st]

    def want(a, oracle):
        import schnorr_sign_ref as S
        w = S.sign_many(curve, a["sk"], a["msgs"])
        return [w["r_xy"], w["s"], w["sig_bytes"]]
    return call, want


def _xmd(ctx, a):
    return [ctx.expand_message_xmd(a["msgs"], DST, 48)], []


def _w_xmd(a, oracle):
    import h2c_ref as H
    return [_rows([H.expand_message_xmd(m, DST, 48) for m in a["msgs"]])]


def _h2f(ctx, a):
    return [ctx.hash_to_field(SECP, a["msgs"], DST, 2).reshape(len(a["msgs"]), 8)], []


def _w_h2f(a, oracle):
    import h2c_ref as H
    return [_flat([H.hash_to_field(SECP, m, DST, 2)[0] for m in a["msgs"]])]


def _h2c(curve):
    def call(ctx, a):
        out, cand, _ = ctx.hash_to_curve(curve, a["msgs"], DST)
        return [out, cand.reshape(len(a["msgs"]), 16)], []

    def want(a, oracle):
        import h2c_ref as H
        got = [H.hash_to_curve(curve, m, DST) for m in a["msgs"]]
        return [_flat([g[0] for g in got]), _flat([[v for c in g[1] for v in c] for g in got])]
    return call, want


def _curve_h2c(ctx, a):
    xy, inf = ctx.curve_hash_to_curve(SECP, a["msgs"], DST)
    return [xy], [inf]


def _w_curve_h2c(a, oracle):
    import h2c_ref as H
    return [_flat([H.curve_hash_to_curve(SECP, m, DST)[:2] for m in a["msgs"]])]


PARITY_HOST_ROWS = [
    Row("batch_ecdh", "fec_batch_ecdh", _mk_ecdh, _ecdh, _w_ecdh),
    Row("derive_key", "fec_derive_key", _mk_derive, _derive, _w_derive),
    Row("ecdh_derive_key", "fec_ecdh_derive_key", _mk_ecdh, _ecdh_derive, _w_ecdh_derive),
    Row("ecdh_exchange", "fec_ecdh_exchange", _mk_ecdh, _exchange, _w_exchange),
    Row("ecdsa_sign-secp256k1", "fec_ecdsa_sign", _mk_ecdsa, *_ecdsa(SECP)),
    Row("ecdsa_sign-p256", "fec_ecdsa_sign", _mk_ecdsa, *_ecdsa(P256)),
    Row("x25519", "fec_x25519", _mk_x25519, _x25519, _w_x25519),
    Row("curve25519_mul", "fec_curve25519_mul", _mk_c25519, _c25519, _w_c25519),
    Row("map_to_curve", "fec_map_to_curve", _mk_map, _map, _w_map),
    Row("sha512", "fec_sha512", _mk_msgs, *_digest("sha512")),
    Row("sha256", "fec_sha256", _mk_msgs, *_digest("sha256")),
    Row("ed25519_sign", "fec_ed25519_sign", accepted(_mk_keys_msgs, _st_ed_sign), _ed_sign, _w_ed_sign),
    Row("ed25519_derive_public_key", "fec_ed25519_derive_public_key", _mk_keys_msgs, _ed_derive, _w_ed_derive),
    Row("eddsa_sign_ed25519", "fec_eddsa_sign_ed25519", accepted(_mk_sk_msgs, _st_eddsa), _eddsa, _w_eddsa),
    Row("bip340_sign", "fec_bip340_sign", _mk_keys_msgs, _bip340, _w_bip340),
    Row("ecdsa_sign_msg-secp256k1", "fec_ecdsa_sign_msg", accepted(_mk_sk_msgs, _st_ecdsa_msg(SECP)), *_ecdsa_msg(SECP)),
    Row("ecdsa_sign_msg-p256", "fec_ecdsa_sign_msg", accepted(_mk_sk_msgs, _st_ecdsa_msg(P256)), *_ecdsa_msg(P256)),
    Row("rfc6979_k", "fec_rfc6979_k", _mk_sk_msgs, _rfc6979, _w_rfc6979),
    Row("debug_rfc6979_k", "fec_debug_rfc6979_k", _mk_sk_msgs, _debug_rfc6979, _w_debug_rfc6979),
    Row("schnorr_sign_msg-secp256k1", "fec_schnorr_sign_msg", _mk_sk_msgs, *_schnorr(SECP)),
    Row("schnorr_sign_msg-p256", "fec_schnorr_sign_msg", _mk_sk_msgs, *_schnorr(P256)),
    Row("expand_message_xmd", "fec_expand_message_xmd", _mk_msgs, _xmd, _w_xmd),
    Row("hash_to_field", "fec_hash_to_field", _mk_msgs, _h2f, _w_h2f),
    Row("hash_to_curve-secp256k1", "fec_hash_to_curve", _mk_msgs, *_h2c(SECP)),
    Row("hash_to_curve-p256", "fec_hash_to_curve", _mk_msgs, *_h2c(P256)),   # the one form with a work area (kernels_h2c.hip)
    Row("curve_hash_to_curve", "fec_curve_hash_to_curve", _mk_msgs, _curve_h2c, _w_curve_h2c),
]


# ---- canonical mode: one description per call, used by its host row and its *_dev row ---------------------------------------
# make(seed, n) -> dict of numpy arrays / message lists; `ins`: the order the C call takes them in; `outs`: (name, width in
# bytes, is a status) in the order the C call takes them; `host(ctx, a)` runs the python wrapper; `dev(ctx, t, n, stream)`
# the *_dev wrapper on tensors t[name]; `want(a)` the model's outputs in the order of the non-status outs.
def _canon(ctx, curve):
    from forge_ec_amd.canon import CANON_CURVES
    return CANON_CURVES[CANON_NAMES[curve]](ctx)


def _model(curve):
    from oracle import canon_model as M
    return {SECP: M.SECP256K1, P256: M.P256, ED: M.ED25519}[curve]


def _mk_canon(seed, n):
    r = _rng(seed)
    return dict(keys=be_keys(r, n), digests=raw_bytes(r, n), aux=raw_bytes(r, n), tweaks=be_keys(r, n), msgs=messages(r, n),
                us=raw_bytes(r, n), scalars=limbs(r, n), ccs=raw_bytes(r, n),
                idx=(r.integers(0, HARDENED, size=n, dtype=np.uint32) | (r.integers(0, 2, size=n, dtype=np.uint32) << np.uint32(31))))


def _ints(a):
    return [int.from_bytes(bytes(k), "big") for k in a]


class Canon:
    def __init__(self, id, fn, launcher, host, dev, outs, want, work_area=True, make=_mk_canon):
        self.id, self.fn, self.launcher, self.host, self.dev, self.outs, self.want = id, fn, launcher, host, dev, outs, want
        self.work_area, self.make = work_area, make


def _split(res, outs):
    """a wrapper's return value -> (outs, sts) by the description's flags"""
    res = res if isinstance(res, tuple) else (res,)
    assert len(res) == len(outs)
    return [r for r, (_, _, is_st) in zip(res, outs) if not is_st], [r for r, (_, _, is_st) in zip(res, outs) if is_st]


def _mul_base_secret(curve):
    def want(a):
        import oracle.canon_model as M
        C = _model(curve)
        return [np.array([M.xy_limbs(C.mul(_val(k), C.G)) for k in a["scalars"]], dtype=np.uint64)]
    return Canon("mul_base_secret-" + CANON_NAMES[curve], "fec_canon_mul_base_secret", "launch_canon_mul_base_secret",
                 lambda ctx, a: _canon(ctx, curve).mul_base_secret(a["scalars"]),
                 lambda ctx, t, n, s: _canon(ctx, curve).mul_base_secret_dev(t["scalars"], t["xy"], t["st"], n, s),
                 [("xy", 64, False), ("st", 1, True)], want)


def _public_key(curve, scheme, out_len):
    import_scheme = {SECP: 0, P256: 1, ED: 2, 3: 3}[scheme]

    def want(a):
        import canon_sign_ref as S
        return [_rows([S.public_key(import_scheme, bytes(k), out_len)[0] for k in a["keys"]])]
    name = "bip340" if scheme == 3 else CANON_NAMES[curve]
    return Canon("public_key-%s-%d" % (name, out_len), "fec_canon_public_key", "launch_canon_public_key",
                 lambda ctx, a: _canon(ctx, curve).public_key(a["keys"], out_len, scheme),
                 lambda ctx, t, n, s: _canon(ctx, curve).public_key_dev(t["keys"], t["out"], out_len, t["st"], n, s, scheme),
                 [("out", out_len, False), ("st", 1, True)], want)


def _sign_digest(curve):
    def want(a):
        import canon_sign_ref as S
        return [_rows([S.ecdsa_sign_digest(_model(curve), d, bytes(h), S.LOW_S)[0] for d, h in zip(_ints(a["keys"]), a["digests"])])]
    return Canon("ecdsa_sign_digest-" + CANON_NAMES[curve], "fec_canon_ecdsa_sign_digest", "launch_canon_ecdsa_sign",
                 lambda ctx, a: _canon(ctx, curve).ecdsa_sign_digest(a["digests"], a["keys"], 1),
                 lambda ctx, t, n, s: _canon(ctx, curve).ecdsa_sign_digest_dev(t["digests"], t["keys"], 1, t["sigs"], t["st"], n, s),
                 [("sigs", 64, False), ("st", 1, True)], want)


def _sign_msg(curve):
    def want(a):
        import canon_sign_ref as S
        return [_rows([S.ecdsa_sign_msg(_model(curve), d, m)[0] for d, m in zip(_ints(a["keys"]), a["msgs"])])]
    return Canon("ecdsa_sign_msg-" + CANON_NAMES[curve], "fec_canon_ecdsa_sign_msg", "launch_canon_ecdsa_sign",
                 lambda ctx, a: _canon(ctx, curve).ecdsa_sign_msg(a["msgs"], a["keys"]),
                 lambda ctx, t, n, s: _canon(ctx, curve).ecdsa_sign_msg_dev(t["msgs"], t["off"], t["total"], t["keys"], 0, t["sigs"], t["st"], n, s),
                 [("sigs", 64, False), ("st", 1, True)], want)


def _sign_recoverable(curve):
    def want(a):
        import canon_recover_ref as RV
        import canon_sign_ref as S
        got = [RV.sign_recoverable_digest(_model(curve), d, bytes(h), S.LOW_S) for d, h in zip(_ints(a["keys"]), a["digests"])]
        return [_rows([g[0] for g in got])]   # (the recovery ids, 0..3, are checked as they come: see the test)
    return Canon("ecdsa_sign_recoverable_digest-" + CANON_NAMES[curve], "fec_canon_ecdsa_sign_recoverable_digest",
                 "launch_canon_ecdsa_sign",
                 lambda ctx, a: _canon(ctx, curve).ecdsa_sign_recoverable_digest(a["digests"], a["keys"], 1)[::2],
                 lambda ctx, t, n, s: _canon(ctx, curve).ecdsa_sign_recoverable_digest_dev(t["digests"], t["keys"], 1, t["sigs"], t["rec"],
                                                                                           t["st"], n, s),
                 [("sigs", 64, False), ("st", 1, True)], want)


def _rfc6979_k(curve):
    def want(a):
        import canon_sign_ref as S
        C = _model(curve)
        return [_rows([S.rfc6979_k(C.N, d, bytes(h)).to_bytes(32, "big") for d, h in zip(_ints(a["keys"]), a["digests"])])]
    return Canon("rfc6979_k-" + CANON_NAMES[curve], "fec_canon_rfc6979_k", "launch_canon_ecdsa_sign",
                 lambda ctx, a: _canon(ctx, curve).rfc6979_k(a["digests"], a["keys"]),
                 lambda ctx, t, n, s: _canon(ctx, curve).rfc6979_k_dev(t["digests"], t["keys"], t["k"], t["st"], n, s),
                 [("k", 32, False), ("st", 1, True)], want)


def _w_bip340_msg(a):
    import canon_sign_ref as S
    return [_rows([S.bip340_sign(d, m, bytes(x))[0] for d, m, x in zip(_ints(a["keys"]), a["msgs"], a["aux"])])]


def _w_ed25519_msg(a):
    import canon_sign_ref as S
    got = [S.ed25519_sign(bytes(k), m) for k, m in zip(a["keys"], a["msgs"])]
    return [_rows([g[0] for g in got]), _rows([g[1] for g in got])]


def _w_cx25519(a):
    import canon_x25519_ref as X
    return [_rows([X.x25519(bytes(k), bytes(u)) for k, u in zip(a["keys"], a["us"])])]


def _w_cx25519_base(a):
    import canon_x25519_ref as X
    return [_rows([X.x25519_base(bytes(k)) for k in a["keys"]])]


def _seckey_tweak(curve):
    def want(a):
        import canon_bip32_ref as B
        return [_rows([B.seckey_tweak_add(_model(curve), bytes(k), bytes(t))[0] for k, t in zip(a["keys"], a["tweaks"])])]
    return Canon("seckey_tweak_add-" + CANON_NAMES[curve], "fec_canon_seckey_tweak_add", "launch_canon_seckey_tweak_add",
                 lambda ctx, a: _canon(ctx, curve).seckey_tweak_add(a["keys"], a["tweaks"]),
                 lambda ctx, t, n, s: _canon(ctx, curve).seckey_tweak_add_dev(t["keys"], t["tweaks"], t["out"], t["st"], n, s),
                 [("out", 32, False), ("st", 1, True)], want, work_area=False)


def _bip32():
    from forge_ec_amd.canon import CanonBip32
    return CanonBip32


def _derive_priv(kind):
    """kind: "each" a parent per element, "shared" one parent, "nocomb" FEC_CANON_BIP32_NO_COMB (hardened indices only)"""
    flags = 1 if kind == "nocomb" else 0

    def make(seed, n):
        a = _mk_canon(seed, n)
        if kind == "nocomb":
            a["idx"] = a["idx"] | np.uint32(HARDENED)
        if kind == "shared":
            a["pkeys"], a["pccs"] = a["keys"][:1].copy(), a["ccs"][:1].copy()
        else:
            a["pkeys"], a["pccs"] = a["keys"], a["ccs"]
        return a

    def want(a):
        import canon_bip32_ref as B
        m = a["pkeys"].shape[0]
        got = [B.ckd_priv(bytes(a["pkeys"][i % m]), bytes(a["pccs"][i % m]), int(ix), flags) for i, ix in enumerate(a["idx"])]
        return [_rows([g[0] for g in got]), _rows([g[1] for g in got])]
    return Canon("bip32_derive_priv-" + kind, "fec_canon_bip32_derive_priv", "launch_canon_bip32_derive_priv",
                 lambda ctx, a: _bip32()(ctx).derive_priv(a["pkeys"], a["pccs"], a["idx"], flags),
                 lambda ctx, t, n, s: _bip32()(ctx).derive_priv_dev(t["pkeys"], t["pccs"], 1 if kind == "shared" else n, t["idx"], flags,
                                                                    t["okeys"], t["occs"], t["st"], n, s),
                 [("okeys", 32, False), ("occs", 32, False), ("st", 1, True)], want, make=make)


def _x(ctx):
    from forge_ec_amd.canon import CanonX25519
    return CanonX25519(ctx)


CANON_CALLS = [
    _mul_base_secret(SECP), _mul_base_secret(P256), _mul_base_secret(ED),
    _public_key(SECP, SECP, 33), _public_key(P256, P256, 65), _public_key(ED, ED, 32), _public_key(SECP, 3, 32),
    _sign_digest(SECP), _sign_digest(P256),
    _sign_msg(SECP), _sign_msg(P256),
    _sign_recoverable(SECP), _sign_recoverable(P256),
    _rfc6979_k(SECP), _rfc6979_k(P256),
    Canon("bip340_sign_msg", "fec_canon_bip340_sign_msg", "launch_canon_bip340_sign",
          lambda ctx, a: _canon(ctx, SECP).bip340_sign_msg(a["msgs"], a["keys"], a["aux"]),
          lambda ctx, t, n, s: _canon(ctx, SECP).bip340_sign_msg_dev(t["msgs"], t["off"], t["total"], t["keys"], t["aux"], t["sigs"], t["st"], n, s),
          [("sigs", 64, False), ("st", 1, True)], _w_bip340_msg),
    Canon("ed25519_sign_msg", "fec_canon_ed25519_sign_msg", "launch_canon_ed25519_sign",
          lambda ctx, a: _canon(ctx, ED).ed25519_sign_msg(a["msgs"], a["keys"]),
          lambda ctx, t, n, s: _canon(ctx, ED).ed25519_sign_msg_dev(t["msgs"], t["off"], t["total"], t["keys"], t["sigs"], t["pks"], t["st"], n, s),
          [("sigs", 64, False), ("pks", 32, False), ("st", 1, True)], _w_ed25519_msg),
    Canon("x25519", "fec_canon_x25519", "launch_canon_x25519",
          lambda ctx, a: _x(ctx).x25519(a["keys"], a["us"]),
          lambda ctx, t, n, s: _x(ctx).x25519_dev(t["keys"], t["us"], t["out"], t["st"], n, s),
          [("out", 32, False), ("st", 1, True)], _w_cx25519, work_area=False),
    Canon("x25519_base", "fec_canon_x25519_base", "launch_canon_x25519_base",
          lambda ctx, a: _x(ctx).x25519_base(a["keys"]),
          lambda ctx, t, n, s: _x(ctx).x25519_base_dev(t["keys"], t["out"], n, s),
          [("out", 32, False)], _w_cx25519_base),
    _seckey_tweak(SECP), _seckey_tweak(P256),
    _derive_priv("each"), _derive_priv("shared"), _derive_priv("nocomb"),
]


def _host_row(c):
    return Row("canon-" + c.id, c.fn, c.make, lambda ctx, a: _split(c.host(ctx, a), c.outs), lambda a, oracle: c.want(a),
               launcher=c.launcher, work_area=c.work_area)


def dev_tensors(c, a, n):
    """torch tensors of one *_dev call: the inputs uploaded, the outputs pre-filled with 0xEE (name -> raw pointer), and
    the tensors themselves, which the caller keeps alive"""
    import torch
    keep, t = {}, {}
    for k, v in a.items():
        if k == "msgs":
            off = np.zeros(len(v) + 1, dtype=np.uint64)
            np.cumsum([len(m) for m in v], out=off[1:])
            keep["msgs"] = torch.from_numpy(np.frombuffer(b"".join(v), dtype=np.uint8).copy()).cuda()
            keep["off"] = torch.from_numpy(off.view(np.uint8).copy()).cuda()
            t["total"] = int(off[-1])
        else:
            keep[k] = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()).cuda()
    for name, width, _ in list(c.outs) + ([("rec", 1, True)] if "recoverable" in c.id else []):
        keep[name] = torch.full((n, width), 0xEE, dtype=torch.uint8, device="cuda")
    t.update({k: v.data_ptr() for k, v in keep.items()})
    return t, keep


def _dev_row(c):
    def call(ctx, a, n, stream):
        t, keep = dev_tensors(c, a, n)
        c.dev(ctx, t, n, stream)
        return keep   # read after the caller has synchronised: outs_of
    return Row("canon-" + c.id + "_dev", c.fn + "_dev", c.make, call, lambda a, oracle: c.want(a), launcher=c.launcher, work_area=c.work_area)


def outs_of(row_id, keep):
    """(outs, sts) of a finished *_dev call, as numpy"""
    c = next(c for c in CANON_CALLS if "canon-" + c.id + "_dev" == row_id)
    outs = [keep[name].cpu().numpy() for name, _, is_st in c.outs if not is_st]
    sts = [keep[name].cpu().numpy().reshape(-1) for name, _, is_st in c.outs if is_st]
    return outs, sts


CANON_HOST_ROWS = [_host_row(c) for c in CANON_CALLS]
HOST_ROWS = PARITY_HOST_ROWS + CANON_HOST_ROWS
DEV_ROWS = [_dev_row(c) for c in CANON_CALLS]

# what the census compares with the source
HOST_FUNCTIONS = sorted({r.fn for r in HOST_ROWS})
DEV_LAUNCHERS = sorted({r.launcher for r in DEV_ROWS})
DEV_WITHOUT_WORK_AREA = sorted({r.launcher for r in DEV_ROWS if not r.work_area})
