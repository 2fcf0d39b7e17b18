"""
GPU tests of fec_schnorr_challenge / _dev and fec_scalar_from_bytes_reduced / _dev (kernels_schnorr.hip) against the
restatement of tests/schnorr_sign_ref.py on the three curves: the challenge fixture; n = 257 with random points, infinity
flags and message lengths, with and without the flag arrays; a planted bad range; every from_bytes_reduced string of the
fixture -- every reachable leg -- and n = 256 with crafted and random strings interleaved, so that the lanes of one
wavefront take different legs.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import schnorr_sign_ref as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = S.load_fixture()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def _points(gpu_ctx, curve, n, seed):
    """n affine points k_i * G from the GPU's own fixed-base multiplication (tested elsewhere), and seeded flags."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    xy, inf = gpu_ctx.batch_to_affine(curve, gpu_ctx.batch_mul_fixed(curve, k, gpu_ctx.generator(curve)))
    assert not inf.any()
    return xy, (rng.random(n) < 0.2).astype(np.uint8)


def _want(curve, r_xy, r_inf, pk_xy, pk_inf, msgs):
    """The restatement over the C oracle's encodings, batched."""
    from oracle import c_oracle
    be = S.CBackend()
    n = len(msgs)
    enc_r = np.asarray(c_oracle.batch_compress(curve, r_xy, r_inf), dtype=np.uint8).reshape(n, 33)
    enc_p = np.asarray(c_oracle.batch_compress(curve, pk_xy, pk_inf), dtype=np.uint8).reshape(n, 33)
    return np.array([S.from_bytes_reduced(curve, hashlib.sha256(bytes(enc_r[i]) + bytes(enc_p[i]) + msgs[i]).digest(), be.reduce_wide)[0]
                     for i in range(n)], dtype=np.uint64).reshape(n, 4)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_challenge_fixture(gpu_ctx, curve):
    rows = [c for c in FIXTURE["challenge"] if c["curve"] == curve]
    e = gpu_ctx.schnorr_challenge(curve, [c["r_xy"] for c in rows], [c["r_inf"] for c in rows], [c["pk_xy"] for c in rows],
                                  [c["pk_inf"] for c in rows], [bytes.fromhex(c["msg"]) for c in rows])
    assert e.tolist() == [c["e"] for c in rows]


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_random_points_flags_and_lengths(gpu_ctx, curve):
    import torch
    n = 257
    r_xy, r_inf = _points(gpu_ctx, curve, n, 10 + curve)
    pk_xy, pk_inf = _points(gpu_ctx, curve, n, 20 + curve)
    rng = np.random.default_rng(30 + curve)
    edge = (0, 53, 54, 61, 62, 63, 117, 118, 126)
    msgs = [rng.integers(0, 256, size=edge[i % 9] if i % 3 == 0 else int(rng.integers(0, 201)), dtype=np.uint8).tobytes() for i in range(n)]
    want = _want(curve, r_xy, r_inf, pk_xy, pk_inf, msgs)
    assert np.array_equal(gpu_ctx.schnorr_challenge(curve, r_xy, r_inf, pk_xy, pk_inf, msgs), want)
    zero = np.zeros(n, dtype=np.uint8)
    want_finite = _want(curve, r_xy, zero, pk_xy, zero, msgs)
    assert np.array_equal(gpu_ctx.schnorr_challenge(curve, r_xy, None, pk_xy, None, msgs), want_finite)     # NULL flag arrays
    # the _dev form, message buffer one byte off alignment, one flag array NULL
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    total = int(off[-1])
    d_r, d_pk, d_pinf, d_off = _dev(torch, r_xy), _dev(torch, pk_xy), _dev(torch, pk_inf), _dev(torch, off)
    big = torch.zeros(total + 16, dtype=torch.uint8, device=d_r.device)
    big[1:1 + total] = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).to(d_r.device)
    d_e = torch.full((n * 32,), 7, dtype=torch.uint8, device=d_r.device)
    d_st = torch.full((n,), 9, dtype=torch.uint8, device=d_r.device)
    gpu_ctx.schnorr_challenge_dev(curve, d_r.data_ptr(), None, d_pk.data_ptr(), d_pinf.data_ptr(), big.data_ptr() + 1, d_off.data_ptr(), total,
                                  d_e.data_ptr(), d_st.data_ptr(), n)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    assert np.array_equal(d_e.cpu().numpy().view(np.uint64).reshape(n, 4), _want(curve, r_xy, zero, pk_xy, pk_inf, msgs))


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_chunked_and_multi_device(gpu_ctx, curve):
    """Chunks of 64 over n = 131: elements 63 and 64 are empty, so one chunk's rebased offsets end and the next one's
    start on an empty range; the other lengths cycle through the padding edges of SHA-256."""
    import forge_ec_amd as F
    n = 131
    r_xy, r_inf = _points(gpu_ctx, curve, n, 80 + curve)
    pk_xy, pk_inf = _points(gpu_ctx, curve, n, 90 + curve)
    rng = np.random.default_rng(95 + curve)
    msgs = [rng.integers(0, 256, size=0 if i in (63, 64) else (0, 1, 55, 56, 64, 119)[i % 6], dtype=np.uint8).tobytes() for i in range(n)]
    want = _want(curve, r_xy, r_inf, pk_xy, pk_inf, msgs)
    gpu_ctx.set_chunk(64)
    try:
        assert np.array_equal(gpu_ctx.schnorr_challenge(curve, r_xy, r_inf, pk_xy, pk_inf, msgs), want)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    with F.Context(devices=[0, 0]) as multi:
        multi.set_chunk(64)
        assert np.array_equal(multi.schnorr_challenge(curve, r_xy, r_inf, pk_xy, pk_inf, msgs), want)


def test_dev_form_bad_range_planted(gpu_ctx):
    import torch
    n, bad, curve = 70, 37, 1
    r_xy, r_inf = _points(gpu_ctx, curve, n, 41)
    pk_xy, pk_inf = _points(gpu_ctx, curve, n, 42)
    rng = np.random.default_rng(43)
    msgs = [rng.integers(0, 256, size=int(rng.integers(1, 100)), dtype=np.uint8).tobytes() for _ in range(n)]
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    total = int(off[-1])
    want = _want(curve, r_xy, r_inf, pk_xy, pk_inf, msgs)
    planted = off.copy()
    planted[bad + 1] = total + 1
    d = [_dev(torch, a) for a in (r_xy, r_inf, pk_xy, pk_inf, planted)]
    body = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).to(d[0].device)
    d_e = torch.full((n * 32,), 7, dtype=torch.uint8, device=d[0].device)
    d_st = torch.full((n,), 9, dtype=torch.uint8, device=d[0].device)
    gpu_ctx.schnorr_challenge_dev(curve, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), body.data_ptr(), d[4].data_ptr(),
                                  total, d_e.data_ptr(), d_st.data_ptr(), n)
    torch.cuda.synchronize()
    e, st = d_e.cpu().numpy().view(np.uint64).reshape(n, 4), d_st.cpu().numpy()
    for i in range(n):
        if i in (bad, bad + 1):
            assert st[i] == 4 and not e[i].any(), i
        else:
            assert st[i] == 0 and np.array_equal(e[i], want[i]), i


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_from_bytes_reduced_fixture_every_leg(gpu_ctx, curve):
    rows = [c for c in FIXTURE["reduced"] if c["curve"] == curve]
    assert {c["leg"] for c in rows} == set(S.REACHABLE[curve])
    out = gpu_ctx.scalar_from_bytes_reduced(curve, np.array([list(bytes.fromhex(c["bytes"])) for c in rows], dtype=np.uint8))
    assert out.tolist() == [c["out"] for c in rows]


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_from_bytes_reduced_mixed_legs_in_one_wavefront(gpu_ctx, curve):
    """n = 256: crafted strings (the fixture's, cycled) at the even positions, random ones at the odd positions; host
    and _dev."""
    import torch
    rows = [bytes.fromhex(c["bytes"]) for c in FIXTURE["reduced"] if c["curve"] == curve]
    rng = np.random.default_rng(50 + curve)
    data = [rows[(i // 2) % len(rows)] if i % 2 == 0 else rng.integers(0, 256, size=32, dtype=np.uint8).tobytes() for i in range(256)]
    be = S.CBackend()
    want = [S.from_bytes_reduced(curve, b, be.reduce_wide) for b in data]
    assert {leg for _, leg in want[:64]} == set(S.REACHABLE[curve])                       # the first wavefront takes every leg
    arr = np.array([list(b) for b in data], dtype=np.uint8)
    assert gpu_ctx.scalar_from_bytes_reduced(curve, arr).tolist() == [v for v, _ in want]
    d_in = _dev(torch, arr)
    d_out = torch.full((256 * 32,), 7, dtype=torch.uint8, device=d_in.device)
    gpu_ctx.scalar_from_bytes_reduced_dev(curve, d_in.data_ptr(), d_out.data_ptr(), 256)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().view(np.uint64).reshape(256, 4).tolist() == [v for v, _ in want]
