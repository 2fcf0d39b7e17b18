"""
Every element-wise host-pointer entry point goes through one host engine (forge_ec_amd/csrc/host_ctx.hpp: `sharded`
over the devices of a multi-device ctx, `chunked` on each).  Here each of them runs at n = 1000 with chunks of 2^18
(one chunk), 1001, 1000, 999, 333 and 64 elements, and on a [0, 0] multi-device ctx with chunks of 333; every output
-- values and per-element statuses -- must equal the call's *_dev form run as one launch (the host form's one-chunk
result where there is no *_dev form).  Optional arrays run absent and present; the message calls run ragged messages.
The argument checks give every host form a null ctx, a null required array, a bad curve and an unsupported curve, on
a single-device and a [0, 0] ctx.
"""
import ctypes

import numpy as np
import pytest

import vectors as V

pytestmark = pytest.mark.gpu

N = 1000
CHUNKS = (1 << 18, 1001, 1000, 999, 333, 64)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -5
SECP, P256, ED = 0, 1, 2
vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


class In:
    def __init__(self, a):
        self.a = None if a is None else np.ascontiguousarray(a)


class Out:
    def __init__(self, cols, dtype=np.uint8):
        self.shape, self.dtype = ((N, cols) if cols else (N,)), dtype


class Size:   # a size_t argument other than n (msg_len)
    def __init__(self, v):
        self.v = v


def _rng(seed):
    return np.random.default_rng(seed)


def _bytes(rows, cols, seed):
    return _rng(seed).integers(0, 256, size=(rows, cols), dtype=np.uint8)


def _flags(seed):
    return (_rng(seed).integers(0, 8, size=N) == 0).astype(np.uint8)


_AFFINE = {}


def _affine(ctx, curve, seed):
    """Affine points of the curve (with a few at infinity)."""
    if (curve, seed) not in _AFFINE:
        xy, inf = ctx.batch_to_affine(curve, V.points(N, curve, seed))
        _AFFINE[(curve, seed)] = (xy, inf)
    return _AFFINE[(curve, seed)]


def _messages(seed):
    lens = _rng(seed).integers(0, 200, size=N)
    lens[:3] = (0, 111, 112)   # an empty message and both sides of a SHA-512 padding boundary
    off = np.zeros(N + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    msgs = _rng(seed + 1).integers(0, 256, size=max(int(off[-1]), 1), dtype=np.uint8)
    return msgs, off, int(off[-1])


def _forms(ctx):
    """(id, host symbol, host args, *_dev symbol or None, *_dev args or None = the host args)."""
    f = []
    for c in (SECP, P256, ED):
        pl = 16 if c == ED else 12
        k, k2 = V.scalars(N, c, 11), V.scalars(N, c, 12)
        p, q = V.points(N, c, 13), V.points(N, c, 14)
        xy, inf = _affine(ctx, c, 15)
        rxy, _ = _affine(ctx, c, 16)
        f.append(("batch_mul-%d" % c, "fec_batch_mul", [ci(c), In(k), In(p), Out(pl, np.uint64)], "fec_batch_mul_dev", None))
        for tag, base in (("gen", ctx.generator(c)), ("other", V.points(1, c, 17)[0])):
            f.append(("batch_mul_fixed-%s-%d" % (tag, c), "fec_batch_mul_fixed", [ci(c), In(k), In(base), Out(pl, np.uint64)],
                      "fec_batch_mul_fixed_dev", None))
        f.append(("batch_double_mul-%d" % c, "fec_batch_double_mul", [ci(c), In(k), In(k2), In(p), Out(pl, np.uint64)],
                  "fec_batch_double_mul_dev", None))
        f.append(("batch_to_affine-%d" % c, "fec_batch_to_affine", [ci(c), In(p), Out(8, np.uint64), Out(0)],
                  "fec_batch_to_affine_dev", None))
        for tag, fl in (("noinf", None), ("inf", inf)):
            f.append(("validate_point-%s-%d" % (tag, c), "fec_batch_validate_point", [ci(c), In(xy), In(fl), Out(0)],
                      "fec_batch_validate_point_dev", None))
            f.append(("compress-%s-%d" % (tag, c), "fec_batch_compress", [ci(c), In(xy), In(fl), Out(33)], "fec_batch_compress_dev", None))
            f.append(("encode-%s-%d" % (tag, c), "fec_batch_encode_uncompressed", [ci(c), In(xy), In(fl), Out(65)], None, None))
            f.append(("schnorr_verify-%s-%d" % (tag, c), "fec_schnorr_verify",
                      [ci(c), In(xy), In(fl), In(rxy), In(None if fl is None else _flags(18)), In(k), In(k2), Out(0)],
                      "fec_schnorr_verify_dev", None))
        comp = ctx.batch_compress(c, xy, inf)
        comp[::7, 5] ^= 0x5A   # some encodings that do not decode: per-element ok = 0
        unc = ctx.batch_encode_uncompressed(c, xy, inf)
        unc[::9, 9] ^= 0x33
        f.append(("decompress-%d" % c, "fec_batch_decompress", [ci(c), In(comp), Out(8, np.uint64), Out(0), Out(0)], None, None))
        f.append(("decode_uncompressed-%d" % c, "fec_batch_decode_uncompressed", [ci(c), In(unc), Out(8, np.uint64), Out(0), Out(0)],
                  None, None))
        a, b = V.field_elements(N, c, 19), V.field_elements(N, c, 20)
        f.append(("field_mul-%d" % c, "fec_field_op", [ci(c), ci(2), In(a), In(b), Out(4, np.uint64)], None, None))
        f.append(("field_sqr-%d" % c, "fec_field_op", [ci(c), ci(3), In(a), In(None), Out(4, np.uint64)], None, None))
        f.append(("point_add-%d" % c, "fec_point_op", [ci(c), ci(0), In(p), In(q), Out(pl, np.uint64)], None, None))
        f.append(("point_double-%d" % c, "fec_point_op", [ci(c), ci(1), In(p), In(None), Out(pl, np.uint64)], None, None))
        # canonical-math mode
        f.append(("canon_mul_base-%d" % c, "fec_canon_mul_base", [ci(c), In(k), Out(8, np.uint64), Out(0)], "fec_canon_mul_base_dev", None))
        f.append(("canon_mul-%d" % c, "fec_canon_mul", [ci(c), In(k), In(xy), Out(8, np.uint64), Out(0)], "fec_canon_mul_dev", None))
        f.append(("canon_double_mul-%d" % c, "fec_canon_double_mul", [ci(c), In(k), In(k2), In(xy), Out(8, np.uint64), Out(0)],
                  "fec_canon_double_mul_dev", None))
        f.append(("canon_scalar_muladd-%d" % c, "fec_canon_scalar_op", [ci(c), ci(0), In(k), In(k2), In(V.scalars(N, c, 21)),
                                                                         Out(4, np.uint64)], None, None))
        f.append(("canon_scalar_unary-%d" % c, "fec_canon_scalar_op", [ci(c), ci(1), In(k), In(None), In(None), Out(4, np.uint64)],
                  None, None))
        f.append(("canon_field_mul-%d" % c, "fec_canon_field_op", [ci(c), ci(2), In(a), In(b), Out(4, np.uint64)], None, None))
        f.append(("canon_field_inv-%d" % c, "fec_canon_field_op", [ci(c), ci(5), In(a), In(None), Out(4, np.uint64)], None, None))
    for c in (SECP, P256):
        k, k2, k3 = V.scalars(N, c, 31), V.scalars(N, c, 32), V.scalars(N, c, 33)
        xy, inf = _affine(ctx, c, 34)
        dg = _bytes(N, 32, 35)
        name = "fec_ecdsa_verify_secp256k1" if c == SECP else "fec_ecdsa_verify_p256"
        for tag, fl in (("noinf", None), ("inf", inf)):
            f.append(("ecdsa_verify-%s-%d" % (tag, c), name, [In(dg), In(k), In(k2), In(xy), In(fl), Out(0)], name + "_dev", None))
            f.append(("ecdh-%s-%d" % (tag, c), "fec_batch_ecdh", [ci(c), In(k), In(xy), In(fl), Out(32), Out(0)], "fec_batch_ecdh_dev", None))
        f.append(("ecdsa_sign-%d" % c, "fec_ecdsa_sign", [ci(c), In(k), In(dg), In(k3), Out(8, np.uint64), Out(0)], "fec_ecdsa_sign_dev", None))
        f.append(("canon_ecdsa_verify-%d" % c, "fec_canon_ecdsa_verify", [ci(c), In(k3), In(k), In(k2), In(xy), Out(0)],
                  "fec_canon_ecdsa_verify_dev", None))
    rxy, rinf = _affine(ctx, ED, 41)
    pxy, pinf = _affine(ctx, ED, 42)
    s, k = V.scalars(N, ED, 43), V.scalars(N, ED, 44)
    for tag, ri, pi in (("noinf", None, None), ("inf", rinf, pinf)):
        f.append(("eddsa_verify-%s" % tag, "fec_eddsa_verify_ed25519", [In(rxy), In(ri), In(pxy), In(pi), In(s), In(k), Out(0)],
                  "fec_eddsa_verify_ed25519_dev", None))
    f.append(("canon_bip340_verify", "fec_canon_bip340_verify", [In(V.field_elements(N, SECP, 45)), In(V.scalars(N, SECP, 46)),
                                                                 In(V.scalars(N, SECP, 47)), In(V.scalars(N, SECP, 48)), Out(0)],
              "fec_canon_bip340_verify_dev", None))
    f.append(("canon_eddsa_verify", "fec_canon_eddsa_verify", [In(_bytes(N, 32, 49)), In(_bytes(N, 32, 50)), In(s), In(k), Out(0)],
              "fec_canon_eddsa_verify_dev", None))
    su, uu = _bytes(N, 32, 51), _bytes(N, 32, 52)
    f.append(("x25519", "fec_x25519", [In(su), In(uu), Out(32)], "fec_x25519_dev", None))
    f.append(("curve25519_mul", "fec_curve25519_mul", [In(V.scalars(N, ED, 53)), In(_bytes(N, 64, 54)), Out(8, np.uint64)],
              "fec_curve25519_mul_dev", None))
    a, b = _bytes(N, 32, 55), _bytes(N, 32, 56)
    f.append(("curve25519_field_mul", "fec_curve25519_field_op", [ci(2), In(a), In(b), Out(4, np.uint64)], None, None))
    f.append(("curve25519_field_neg", "fec_curve25519_field_op", [ci(4), In(a), In(None), Out(4, np.uint64)], None, None))
    msgs, off, total = _messages(57)
    keys = _bytes(N, 32, 58)
    f.append(("sha512", "fec_sha512", [In(msgs), In(off), Size(total), Out(64)], "fec_sha512_dev",
              [In(msgs), In(off), Size(total), Out(64), Out(0)]))
    f.append(("ed25519_sign", "fec_ed25519_sign", [In(keys), In(msgs), In(off), Size(total), Out(64), Out(0)], "fec_ed25519_sign_dev", None))
    f.append(("ed25519_derive_public_key", "fec_ed25519_derive_public_key", [In(keys), Out(32), Out(0)],
              "fec_ed25519_derive_public_key_dev", None))
    f.append(("eddsa_sign_ed25519", "fec_eddsa_sign_ed25519", [In(V.scalars(N, ED, 59)), In(msgs), In(off), Size(total),
                                                               Out(8, np.uint64), Out(0), Out(4, np.uint64), Out(0)],
              "fec_eddsa_sign_ed25519_dev", None))
    return f


def _host(lib, h, name, args):
    outs, cargs = [], [h]
    for a in args:
        if isinstance(a, In):
            cargs.append(vp(None if a.a is None else a.a.ctypes.data))
        elif isinstance(a, Out):
            o = np.full(a.shape, 0xA5 if a.dtype == np.uint8 else 0xA5A5A5A5A5A5A5A5, dtype=a.dtype)   # (nothing left unwritten)
            outs.append(o)
            cargs.append(vp(o.ctypes.data))
        elif isinstance(a, Size):
            cargs.append(sz(a.v))
        else:
            cargs.append(a)
    rc = getattr(lib, name)(*cargs, sz(N))
    return rc, outs


def _dev(lib, h, name, args):
    import torch
    dev = torch.device("cuda:0")
    keep, outs, cargs = [], [], [h]
    for a in args:
        if isinstance(a, In):
            if a.a is None:
                cargs.append(vp(None))
                continue
            t = torch.from_numpy(a.a.view(np.uint8).reshape(-1).copy()).to(dev)
            keep.append(t)
            cargs.append(vp(t.data_ptr()))
        elif isinstance(a, Out):
            t = torch.zeros(int(np.prod(a.shape)) * np.dtype(a.dtype).itemsize, dtype=torch.uint8, device=dev)
            outs.append((t, a))
            cargs.append(vp(t.data_ptr()))
        elif isinstance(a, Size):
            cargs.append(sz(a.v))
        else:
            cargs.append(a)
    torch.cuda.synchronize()
    rc = getattr(lib, name)(*cargs, sz(N), vp(None))
    assert rc == OK, (name, rc)
    assert lib.fec_ctx_check(h) == OK
    return [t.cpu().numpy().view(a.dtype).reshape(a.shape) for t, a in outs]


@pytest.fixture(scope="module")
def forms(gpu_ctx):
    return {f[0]: f for f in _forms(gpu_ctx)}


@pytest.fixture(scope="module")
def multi_ctx():
    import forge_ec_amd as F
    ctx = F.Context(devices=[0, 0])
    yield ctx
    ctx.close()


def _ids():
    ids = []
    for c in (SECP, P256, ED):
        ids += ["batch_mul-%d" % c, "batch_mul_fixed-gen-%d" % c, "batch_mul_fixed-other-%d" % c, "batch_double_mul-%d" % c,
                "batch_to_affine-%d" % c, "decompress-%d" % c, "decode_uncompressed-%d" % c, "field_mul-%d" % c,
                "field_sqr-%d" % c, "point_add-%d" % c, "point_double-%d" % c, "canon_mul_base-%d" % c, "canon_mul-%d" % c,
                "canon_double_mul-%d" % c, "canon_scalar_muladd-%d" % c, "canon_scalar_unary-%d" % c,
                "canon_field_mul-%d" % c, "canon_field_inv-%d" % c]
        for tag in ("noinf", "inf"):
            ids += ["validate_point-%s-%d" % (tag, c), "compress-%s-%d" % (tag, c), "encode-%s-%d" % (tag, c),
                    "schnorr_verify-%s-%d" % (tag, c)]
    for c in (SECP, P256):
        ids += ["ecdsa_sign-%d" % c, "canon_ecdsa_verify-%d" % c]
        for tag in ("noinf", "inf"):
            ids += ["ecdsa_verify-%s-%d" % (tag, c), "ecdh-%s-%d" % (tag, c)]
    ids += ["eddsa_verify-noinf", "eddsa_verify-inf", "canon_bip340_verify", "canon_eddsa_verify", "x25519", "curve25519_mul",
            "curve25519_field_mul", "curve25519_field_neg", "sha512", "ed25519_sign", "ed25519_derive_public_key",
            "eddsa_sign_ed25519"]
    return ids


@pytest.mark.parametrize("form", _ids())
def test_host_call_equals_dev_form_at_every_chunk_size(gpu_ctx, multi_ctx, forms, form):
    from forge_ec_amd._lib import lib
    L = lib()
    _, name, args, dev_name, dev_args = forms[form]
    try:
        if dev_name:
            want = _dev(L, gpu_ctx._h, dev_name, dev_args or args)
            if dev_args:   # (fec_sha512_dev's extra per-element status: not an output of the host form)
                want = want[:1]
        else:
            gpu_ctx.set_chunk(1 << 18)
            rc, want = _host(L, gpu_ctx._h, name, args)
            assert rc == OK, (name, rc)
        for ctx, chunk in [(gpu_ctx, c) for c in CHUNKS] + [(multi_ctx, 333)]:
            ctx.set_chunk(chunk)
            rc, got = _host(L, ctx._h, name, args)
            assert rc == OK, (form, chunk, rc)
            for i, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g, w), "%s: output %d differs at chunk %d (%s)" % (form, i, chunk, ctx.device_count())
    finally:
        gpu_ctx.set_chunk(1 << 18)
        multi_ctx.set_chunk(1 << 18)


def _error_cases(forms):
    """(form, what, curve override or None, expected status)."""
    cases = []
    for form in _ids():
        cases += [(form, "null ctx", None, E_ARG), (form, "null input", None, E_ARG)]
    stems = set()
    for form in _ids():   # the first form of each entry point that takes a curve
        stem = form.rsplit("-", 1)[0]
        if form[-2:] in ("-0", "-1", "-2") and isinstance(forms[form][2][0], ci) and stem not in stems:
            stems.add(stem)
            cases.append((form, "bad curve", 9, E_UNSUPPORTED if stem.startswith(("ecdh", "ecdsa_sign")) else E_ARG))
    for form in ("ecdh-noinf-0", "ecdsa_sign-0", "canon_ecdsa_verify-0"):
        cases.append((form, "unsupported curve", ED, E_UNSUPPORTED))
    cases.append(("point_double-1", "unsupported op", None, E_UNSUPPORTED))
    return cases


def test_argument_errors_of_every_host_form(gpu_ctx, multi_ctx, forms):
    from forge_ec_amd._lib import lib
    L = lib()
    for ctx in (gpu_ctx, multi_ctx):
        for form, what, curve, want in _error_cases(forms):
            _, name, args, _, _ = forms[form]
            args = list(args)
            if curve is not None:
                args[0] = ci(curve)
            if what == "null input":
                i = next(j for j, a in enumerate(args) if isinstance(a, In))
                args[i] = In(None)
            if what == "unsupported op":   # DOUBLE_TRAIT is secp256k1's alone
                args[1] = ci(3)
            h = vp(None) if what == "null ctx" else ctx._h
            rc, _ = _host(L, h, name, args)
            assert rc == want, (form, what, ctx.device_count(), rc)
    # Ed25519 has no ECDH / ECDSA instance: that answer comes before the ctx is looked at
    for form in ("ecdh-noinf-0", "ecdsa_sign-0"):
        _, name, args, _, _ = forms[form]
        rc, _ = _host(L, vp(None), name, [ci(ED)] + list(args[1:]))
        assert rc == E_UNSUPPORTED, form
