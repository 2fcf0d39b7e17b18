"""
GPU tests of batched Ecdsa::<C, D>::sign (fec_ecdsa_sign / fec_ecdsa_sign_dev) for secp256k1 and P-256: bit-exact r,
s and status against the restatement fixture (tests/golden/ecdsa_sign_vectors.json) and against the C-oracle
composition (tests/ecdsa_sign_ref.py); chunked host calls against the device-pointer form on a caller's stream; a
multi-device ctx, and the prefix table on and off, against a single default ctx; a sign -> verify round trip against the
C oracle's verify; argument errors.
"""
import json
import os

import numpy as np
import pytest

import ecdsa_sign_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ecdsa_sign_vectors.json")
CURVES = [0, 1]
M64 = (1 << 64) - 1


def _limbs(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def _inputs(curve, n, seed):
    """sk and k mostly in [1, n), one in 64 an arbitrary 256-bit value or zero; random digests (some >= n)."""
    rng = np.random.default_rng(seed)
    nv = R._val(R.N[curve])
    sk = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    k = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    for a, z in ((sk, 9), (k, 11)):
        a[:, 3] >>= np.uint64(1)                                  # below 2^255 < n: in range
        a[5::64, 3] |= np.uint64(1 << 63)                          # arbitrary top bits: some >= n
        a[z::97] = 0
    sk[3] = _limbs(nv - 1)
    k[4] = _limbs(nv - 1)
    d = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    d[7::53] = 0xFF
    return np.ascontiguousarray(sk), np.ascontiguousarray(d), np.ascontiguousarray(k)


def _same(got, want, what):
    (gr, gs, gst), (wr, ws, wst) = got, want
    bad = np.nonzero((gst != wst) | (gr != wr).any(axis=1) | (gs != ws).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first %d: got st %d r %s s %s, want st %d r %s s %s" % (
        what, bad.size, bad[0], gst[bad[0]], gr[bad[0]], gs[bad[0]], wst[bad[0]], wr[bad[0]], ws[bad[0]])


@pytest.mark.parametrize("curve", CURVES)
def test_fixture(gpu_ctx, curve):
    cases = [c for c in json.load(open(FIXTURE))["cases"] if c["curve"] == curve]
    sk = np.array([c["sk"] for c in cases], dtype=np.uint64)
    d = np.array([list(bytes.fromhex(c["digest"])) for c in cases], dtype=np.uint8)
    k = np.array([c["k"] for c in cases], dtype=np.uint64)
    want = (np.array([c["r"] for c in cases], dtype=np.uint64), np.array([c["s"] for c in cases], dtype=np.uint64),
            np.array([c["status"] for c in cases], dtype=np.uint8))
    _same(gpu_ctx.ecdsa_sign(curve, sk, d, k), want, "fixture")


@pytest.mark.parametrize("curve", CURVES)
def test_random_against_oracle_composition(gpu_ctx, oracle, curve):
    sk, d, k = _inputs(curve, 4096, 7100 + curve)
    want = R.sign(oracle, curve, sk, d, k, nthreads=16)
    assert set(int(v) for v in np.unique(want[2])) >= {0, 1, 3}
    _same(gpu_ctx.ecdsa_sign(curve, sk, d, k), want, "4096 random")


@pytest.mark.parametrize("curve", CURVES)
def test_chunked_host_call_equals_dev_on_caller_stream(gpu_ctx, oracle, curve):
    """N = 2^16 + 37 in chunks of 2^14 through the host form, edge elements at both ends; the same batch through
    fec_ecdsa_sign_dev on a caller's stream; a sample and both ends against the oracle composition."""
    import torch
    n = (1 << 16) + 37
    sk, d, k = _inputs(curve, n, 7200 + curve)
    nv = R._val(R.N[curve])
    for j in (0, n - 1):
        sk[j], k[j] = _limbs(nv - 1), _limbs(1)
    sk[1], sk[n - 2] = _limbs(0), _limbs((1 << 256) - 1)
    k[2], k[n - 3] = _limbs(0), _limbs(nv - 1)
    d[n - 4] = 0xFF
    gpu_ctx.set_chunk(1 << 14)
    try:
        got = gpu_ctx.ecdsa_sign(curve, sk, d, k)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev) for a in (sk, d, k)]
    sig = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.ecdsa_sign_dev(curve, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), sig.data_ptr(), st.data_ptr(), n,
                           stream.cuda_stream)
    stream.synchronize()
    sg = sig.cpu().numpy().view(np.uint64).reshape(n, 8)
    _same(got, (sg[:, :4], sg[:, 4:], st.cpu().numpy()), "host (chunked) vs dev")
    idx = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), np.random.default_rng(5).integers(0, n, 496)]))
    want = R.sign(oracle, curve, sk[idx], d[idx], k[idx], nthreads=16)
    _same((got[0][idx], got[1][idx], got[2][idx]), want, "sample vs oracle")


@pytest.mark.parametrize("curve", CURVES)
def test_multi_ctx_equals_single(gpu_ctx, curve):
    import forge_ec_amd as F
    sk, d, k = _inputs(curve, 3001, 7300 + curve)
    with F.Context(devices=[0, 0]) as multi:
        _same(multi.ecdsa_sign(curve, sk, d, k), gpu_ctx.ecdsa_sign(curve, sk, d, k), "[0, 0] multi ctx")


@pytest.mark.parametrize("curve", CURVES)
def test_prefix_table_on_and_off(curve):
    import forge_ec_amd as F
    sk, d, k = _inputs(curve, 1 << 16, 7400 + curve)
    with F.Context(0) as off, F.Context(0) as on:
        off.set_fixed_prefix_bits(0)
        on.set_fixed_prefix_bits(12)
        on.build_fixed_prefix(curve)
        _same(on.ecdsa_sign(curve, sk, d, k), off.ecdsa_sign(curve, sk, d, k), "prefix table on vs off")


@pytest.mark.parametrize("curve", CURVES)
def test_sign_then_verify_round_trip(gpu_ctx, oracle, curve):
    """pk = to_affine(multiply(G, sk)) on the GPU, then the GPU verifier on (digest, r, s, pk): its statuses equal the
    C oracle's verify, element for element, whatever they are (the reference's own round-trip test is ignored)."""
    sk, d, k = _inputs(curve, 2048, 7500 + curve)
    r, s, _ = gpu_ctx.ecdsa_sign(curve, sk, d, k)
    xy, inf = gpu_ctx.batch_to_affine(curve, gpu_ctx.batch_mul_fixed(curve, sk, gpu_ctx.generator(curve)))
    if curve == 0:
        got = gpu_ctx.ecdsa_verify_secp256k1(d, r, s, xy, inf)
        want = oracle.batch_secp256k1_ecdsa_verify(d, r, s, xy, inf, nthreads=16)
    else:
        got = gpu_ctx.ecdsa_verify_p256(d, r, s, xy, inf)
        want = oracle.batch_p256_ecdsa_verify(d, r, s, xy, inf, nthreads=16)
    assert np.array_equal(got, want)


def test_argument_errors(gpu_ctx):
    import torch
    from forge_ec_amd import _lib as L
    lib = L.lib()
    h = gpu_ctx._h
    n = 64
    sk, d, k = _inputs(0, n, 7600)
    sig = np.zeros((n, 8), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    p = [a.ctypes.data for a in (sk, d, k, sig, st)]
    assert lib.fec_ecdsa_sign(h, 2, *p, n) == -5                        # Ed25519: no Ecdsa instance
    assert lib.fec_ecdsa_sign(h, 0, None, p[1], p[2], p[3], p[4], n) == -1
    assert lib.fec_ecdsa_sign(h, 1, p[0], p[1], p[2], None, p[4], n) == -1
    assert lib.fec_ecdsa_sign(None, 0, *p, n) == -1
    assert lib.fec_ecdsa_sign(h, 0, None, None, None, None, None, 0) == 0
    dev = torch.device("cuda:0")
    t = [torch.zeros(n * 64 + 64, dtype=torch.uint8, device=dev) for _ in range(5)]
    q = [x.data_ptr() for x in t]
    assert lib.fec_ecdsa_sign_dev(h, 2, *q, n, None) == -5
    assert lib.fec_ecdsa_sign_dev(h, 0, q[0], None, q[2], q[3], q[4], n, None) == -1
    assert lib.fec_ecdsa_sign_dev(h, 0, None, None, None, None, None, 0, None) == 0
    for j in range(4):                                                   # sk, digests, k, sig must be 16-byte aligned
        r = list(q)
        r[j] += 8
        assert lib.fec_ecdsa_sign_dev(h, 1, *r, n, None) == -1, j
    torch.cuda.synchronize()
    assert gpu_ctx.ecdsa_sign(0, sk, d, k)[2].shape == (n,)              # the ctx is still usable
