"""
GPU tests of fec_derive_key, fec_ecdh_derive_key, fec_ecdh_exchange and their _dev forms (kernels_ecdh.hip, hkdf.hpp)
against the restatement of tests/ecdh_kdf_ref.py: the fixture byte for byte through the three host calls; derive_key on
both curves with n on both sides of a wavefront and (info_len, out_len) pairs whose rows start at every dword alignment,
host and _dev, NULL info at length 0, guard bytes behind the rows; ecdh_derive_key at n = 200 in chunks of 64 against
derive_key(batch_ecdh(...)) on planted batches; ecdh_exchange against batch_mul_fixed + batch_to_affine and
ecdh_derive_key; the lengths and the curve the ABI refuses; out_len = 0 with NULL keys.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import ecdh_kdf_ref as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "ecdh_kdf_vectors.json")))
GUARD = 64
SHAPES = ((0, 32), (23, 33), (55, 65), (119, 1))       # (info_len, out_len)
_WANT = {}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def _inputs(curve, n, info_len):
    """n seeded 32-byte secrets and one info string, with the reference keys for every out_len of SHAPES computed once."""
    key = (curve, n, info_len)
    if key not in _WANT:
        rng = np.random.default_rng(1700 + 100 * curve + n + info_len)
        sec = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        info = rng.integers(0, 256, size=info_len, dtype=np.uint8).tobytes()
        _WANT[key] = (sec, info, {})
    return _WANT[key]


def _want_keys(curve, n, info_len, out_len):
    sec, info, memo = _inputs(curve, n, info_len)
    if out_len not in memo:
        memo[out_len] = np.array([list(K.derive_key(curve, bytes(s), info, out_len)) for s in sec], dtype=np.uint8).reshape(n, out_len)
    return sec, info, memo[out_len]


def test_fixture_derive_key(gpu_ctx):
    sp, ip = bytes.fromhex(FIXTURE["secret_pool"]), bytes.fromhex(FIXTURE["info_pool"])
    a3 = FIXTURE["a3"]
    assert bytes(gpu_ctx.derive_key(0, [bytes.fromhex(a3["ikm"])], b"", a3["out_len"])[0]).hex() == a3["okm"] == K.A3_OKM.hex()
    for curve, s, i, o, okm in FIXTURE["derive_key"]:
        got = gpu_ctx.derive_key(curve, np.frombuffer(sp[:s], dtype=np.uint8).reshape(1, s), ip[:i] if i else None, o)
        assert got.shape == (1, o) and bytes(got[0]).hex() == okm, (curve, s, i, o)


def test_fixture_ecdh_derive_key_and_exchange(gpu_ctx):
    for c in FIXTURE["exchange"]:
        info = bytes.fromhex(c["info"])
        keys, st = gpu_ctx.ecdh_derive_key(c["curve"], [c["sk"]], [c["pk"]], [c["pk_inf"]], info, c["out_len"])
        assert int(st[0]) == c["status"] and bytes(keys[0]).hex() == c["key"], c["note"]
        pub, pinf, keys, st = gpu_ctx.ecdh_exchange(c["curve"], [c["sk"]], [c["pk"]], [c["pk_inf"]], info, c["out_len"])
        assert int(st[0]) == c["status"] and bytes(keys[0]).hex() == c["key"], c["note"]
        assert pub[0].tolist() == c["public_xy"] and int(pinf[0]) == c["public_inf"], c["note"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("curve", [0, 1])
def test_derive_key_host_form(gpu_ctx, curve, n):
    for info_len, out_len in SHAPES:
        sec, info, want = _want_keys(curve, n, info_len, out_len)
        assert np.array_equal(gpu_ctx.derive_key(curve, sec, info if info_len else None, out_len), want), (info_len, out_len)
        # the raw call into a buffer with guard bytes behind the rows
        buf = np.full(n * out_len + GUARD, 0xA5, dtype=np.uint8)
        ib = ctypes.c_char_p(info) if info_len else None
        rc = gpu_ctx._lib.fec_derive_key(gpu_ctx._h, curve, ctypes.c_void_p(sec.ctypes.data), 32, ib, info_len, out_len,
                                         ctypes.c_void_p(buf.ctypes.data), n)
        assert rc == 0 and np.array_equal(buf[:n * out_len].reshape(n, out_len), want) and (buf[n * out_len:] == 0xA5).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("curve", [0, 1])
def test_derive_key_dev_form(gpu_ctx, curve, n):
    import torch
    for info_len, out_len in SHAPES:
        sec, info, want = _want_keys(curve, n, info_len, out_len)
        d_sec = _dev(torch, sec)
        d_keys = torch.full((n * out_len + GUARD,), 0xA5, dtype=torch.uint8, device=d_sec.device)
        gpu_ctx.derive_key_dev(curve, d_sec.data_ptr(), 32, info if info_len else None, out_len, d_keys.data_ptr(), n)
        torch.cuda.synchronize()
        gpu_ctx.check()
        got = d_keys.cpu().numpy()
        assert np.array_equal(got[:n * out_len].reshape(n, out_len), want), (info_len, out_len)
        assert (got[n * out_len:] == 0xA5).all(), (info_len, out_len)


@pytest.mark.parametrize("curve", [0, 1])
def test_ecdh_derive_key_chunked_on_a_planted_batch(gpu_ctx, curve):
    """n = 200 in chunks of 64: the fused call equals derive_key(batch_ecdh(...)) where the status is 0, has zero rows
    elsewhere and batch_ecdh's statuses.  The shares are conditions on the input (tests/test_ecdh_kdf_model.py asserts
    them on the reference alone)."""
    sk, pk, inf = K.planted_batch(curve)
    info, out_len = b"planted batch, 23 bytes", 33
    sec, st = gpu_ctx.batch_ecdh(curve, sk, pk, inf)
    K.assert_planted_shares(curve, st)
    want = gpu_ctx.derive_key(curve, sec, info, out_len)
    want[st != 0] = 0
    gpu_ctx.set_chunk(64)
    try:
        keys, st2 = gpu_ctx.ecdh_derive_key(curve, sk, pk, inf, info, out_len)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    assert st2.tolist() == st.tolist() and np.array_equal(keys, want)
    ref = np.array([list(K.derive_key(curve, bytes(s), info, out_len)) for s in sec], dtype=np.uint8)   # and the restatement
    ref[st != 0] = 0
    assert np.array_equal(keys, ref)


def _exchange_batch(curve, n):
    sk, pk, inf = K.planted_batch(curve, n=n, seed=0xE8C + n)
    if n > 2:
        sk[2] = 0                                          # the public key is the identity and the product too: status 2
    return sk, pk, inf


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("curve", [0, 1])
def test_ecdh_exchange_host_and_dev(gpu_ctx, curve, n):
    import torch
    sk, pk, inf = _exchange_batch(curve, n)
    info, out_len = b"exchange", 33
    want_xy, want_inf = gpu_ctx.batch_to_affine(curve, gpu_ctx.batch_mul_fixed(curve, sk, gpu_ctx.generator(curve)))
    want_keys, want_st = gpu_ctx.ecdh_derive_key(curve, sk, pk, inf, info, out_len)
    bad = want_st != 0
    want_xy[bad] = 0
    want_inf[bad] = 0
    assert not want_keys[bad].any()
    if n > 2:
        assert bad[2] and (~bad).any()
    pub, pinf, keys, st = gpu_ctx.ecdh_exchange(curve, sk, pk, inf, info, out_len)
    assert st.tolist() == want_st.tolist() and np.array_equal(pub, want_xy) and pinf.tolist() == want_inf.tolist()
    assert np.array_equal(keys, want_keys)
    d_sk, d_pk, d_inf = _dev(torch, sk), _dev(torch, pk), _dev(torch, inf)
    fill = lambda m: torch.full((m,), 7, dtype=torch.uint8, device=d_sk.device)
    d_pub, d_pinf, d_keys, d_st = fill(n * 64), fill(n), fill(n * out_len + GUARD), fill(n)
    gpu_ctx.ecdh_exchange_dev(curve, d_sk.data_ptr(), d_pk.data_ptr(), d_inf.data_ptr(), info, out_len, d_pub.data_ptr(), d_pinf.data_ptr(),
                              d_keys.data_ptr(), d_st.data_ptr(), n)
    torch.cuda.synchronize()
    gpu_ctx.check()
    assert d_st.cpu().numpy().tolist() == want_st.tolist()
    assert np.array_equal(d_pub.cpu().numpy().view(np.uint64).reshape(n, 8), want_xy) and d_pinf.cpu().numpy().tolist() == want_inf.tolist()
    got = d_keys.cpu().numpy()
    assert np.array_equal(got[:n * out_len].reshape(n, out_len), want_keys) and (got[n * out_len:] == 7).all()
    # the _dev form of ecdh_derive_key on the same inputs
    d_keys2, d_st2 = fill(n * out_len + GUARD), fill(n)
    gpu_ctx.ecdh_derive_key_dev(curve, d_sk.data_ptr(), d_pk.data_ptr(), d_inf.data_ptr(), info, out_len, d_keys2.data_ptr(), d_st2.data_ptr(), n)
    torch.cuda.synchronize()
    gpu_ctx.check()
    got = d_keys2.cpu().numpy()
    assert d_st2.cpu().numpy().tolist() == want_st.tolist()
    assert np.array_equal(got[:n * out_len].reshape(n, out_len), want_keys) and (got[n * out_len:] == 7).all()


def test_what_the_abi_refuses(gpu_ctx):
    import forge_ec_amd as F
    sec = np.zeros((2, 32), dtype=np.uint8)
    sk, pk, inf = K.planted_batch(0, n=2)
    calls = [lambda: gpu_ctx.derive_key(2, sec, b"", 32),                                  # Ed25519: no KeyExchange
             lambda: gpu_ctx.derive_key(0, sec, b"", 8129),
             lambda: gpu_ctx.derive_key(1, sec, b"", 8129),
             lambda: gpu_ctx.derive_key(0, sec, bytes(1025), 32),
             lambda: gpu_ctx.derive_key(0, np.zeros((2, 65), dtype=np.uint8), b"", 32),
             lambda: gpu_ctx.ecdh_derive_key(2, sk, pk, inf, b"", 32),
             lambda: gpu_ctx.ecdh_derive_key(0, sk, pk, inf, b"", 8129),
             lambda: gpu_ctx.ecdh_derive_key(1, sk, pk, inf, bytes(1025), 32),
             lambda: gpu_ctx.ecdh_exchange(2, sk, pk, inf, b"", 32),
             lambda: gpu_ctx.ecdh_exchange(0, sk, pk, inf, bytes(1025), 32),
             lambda: gpu_ctx.ecdh_exchange(1, sk, pk, inf, b"", 8129)]
    for i, call in enumerate(calls):
        with pytest.raises(F.FecError) as e:
            call()
        assert e.value.status == -5, i
    assert gpu_ctx.derive_key(0, sec, bytes(1024), 1).shape == (2, 1)                     # the bounds themselves are legal
    assert gpu_ctx.derive_key(0, np.zeros((2, 64), dtype=np.uint8), b"", 1).shape == (2, 1)


@pytest.mark.parametrize("curve", [0, 1])
def test_out_len_zero_with_null_keys_returns_the_statuses(gpu_ctx, curve):
    sk, pk, inf = K.planted_batch(curve, n=70)
    _, want = gpu_ctx.batch_ecdh(curve, sk, pk, inf)
    keys, st = gpu_ctx.ecdh_derive_key(curve, sk, pk, inf, b"abc", 0)
    assert keys.shape == (70, 0) and st.tolist() == want.tolist()
    pub, pinf, keys, st = gpu_ctx.ecdh_exchange(curve, sk, pk, inf, None, 0)
    assert keys.shape == (70, 0) and st.tolist() == want.tolist() and pub[st == 0].any(axis=1).all() and not pub[st != 0].any()
    assert gpu_ctx.derive_key(curve, np.zeros((3, 32), dtype=np.uint8), b"abc", 0).shape == (3, 0)
