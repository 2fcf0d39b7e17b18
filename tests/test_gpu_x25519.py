"""
GPU tests of the reference's Curve25519 (fec_x25519, fec_curve25519_mul, fec_curve25519_field_op and the _dev forms),
bit-exact against the restatements: the fixture of tests/x25519_ref.py (tests/golden/x25519_vectors.json) through all
three entry points; random batches of 1, 63, 64, 65 and 2^16 + 37 and one whole 2^20 batch against the threaded C++
restatement (tests/cpp/x25519_ref.cpp); crafted elements (the special scalar, the identity, a Mul rare leg) at
wavefront, workgroup and chunk edges; host against _dev on a caller's stream; a small chunk against the default; a
[0, 0] multi-device ctx against a single ctx; argument errors.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "x25519_vectors.json")))
THREADS = 16


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("x25519") / "x25519_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so,
                           os.path.join(HERE, "cpp", "x25519_ref.cpp")])
    lib = ctypes.CDLL(so)
    lib.xr_x25519_batch.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int]
    lib.xr_multiply_batch.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int]
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def ref_x25519(ref, s, u):
    s, u = np.ascontiguousarray(s), np.ascontiguousarray(u)
    out = np.zeros_like(s)
    ref.xr_x25519_batch(_p(s), _p(u), _p(out), s.shape[0], THREADS)
    return out


def ref_mul(ref, k, pts):
    k, pts = np.ascontiguousarray(k), np.ascontiguousarray(pts)
    out = np.zeros_like(pts)
    ref.xr_multiply_batch(_p(k), _p(pts), _p(out), k.shape[0], THREADS)
    return out


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)


def _mul_inputs(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    pts = rng.integers(0, 1 << 63, size=(n, 8), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 8), dtype=np.uint64)
    return k, pts


def _crafted_x25519(s, u, positions):
    """the special scalar [2, 0, ...], u = 0 (final z2 = 0) and u >= p at the given indices"""
    for j, i in enumerate(positions):
        if j % 3 == 0:
            s[i] = 0
            s[i, 0] = 2
        elif j % 3 == 1:
            u[i] = 0
        else:
            u[i] = 0xFF
    return s, u


def test_fixture_field_ops(gpu_ctx):
    for op in range(5):
        cases = [c for c in FIX["field"] if c["op"] == op]
        a = np.array([c["a"] for c in cases], dtype=np.uint64)
        b = np.array([c["b"] for c in cases], dtype=np.uint64)
        got = gpu_ctx.curve25519_field_op(op, a, b)
        assert got.tolist() == [c["expect"] for c in cases], op
    legs = {leg for c in FIX["field"] for leg in c["legs"]}
    assert legs == {"c1", "c3", "f2"}


def test_fixture_x25519(gpu_ctx):
    s = np.array([list(bytes.fromhex(c["scalar"])) for c in FIX["x25519"]], dtype=np.uint8)
    u = np.array([list(bytes.fromhex(c["u"])) for c in FIX["x25519"]], dtype=np.uint8)
    got = gpu_ctx.x25519(s, u)
    assert [bytes(r).hex() for r in got] == [c["expect"] for c in FIX["x25519"]]


def test_fixture_multiply(gpu_ctx):
    k = np.array([c["scalar"] for c in FIX["multiply"]], dtype=np.uint64)
    p = np.array([c["point"] for c in FIX["multiply"]], dtype=np.uint64)
    got = gpu_ctx.curve25519_mul(k, p)
    assert got.tolist() == [c["expect"] for c in FIX["multiply"]]


@pytest.mark.parametrize("n", [1, 63, 64, 65, (1 << 16) + 37])
def test_random_batches(gpu_ctx, ref, n):
    s, u = _bytes(n, 100 + n), _bytes(n, 200 + n)
    s, u = _crafted_x25519(s, u, sorted({i for i in (0, 63, 64, 255, 256, n - 1) if i < n}))
    assert np.array_equal(gpu_ctx.x25519(s, u), ref_x25519(ref, s, u))
    k, p = _mul_inputs(n, 300 + n)
    for i, v in ((63, [2, 0, 0, 0]), (64, [0, 0, 0, 2 << 56]), (n - 1, [1, 0, 0, 0])):
        if i < n and n > 1:
            k[i] = v
    if n > 255:
        p[255, 4:] = 0
    assert np.array_equal(gpu_ctx.curve25519_mul(k, p), ref_mul(ref, k, p))


def test_whole_2p20_batch(gpu_ctx, ref):
    n = 1 << 20
    s, u = _bytes(n, 11), _bytes(n, 12)
    s, u = _crafted_x25519(s, u, [0, 255, 256, (1 << 18) - 1, 1 << 18, n - 1])
    assert np.array_equal(gpu_ctx.x25519(s, u), ref_x25519(ref, s, u))


def test_rare_leg_operands_at_edges(gpu_ctx):
    """the Mul rare-leg operands of the fixture at wavefront, workgroup and chunk edges of a field-op batch, random
    operands elsewhere: every lane equal to the restatement's expectation"""
    legs = [c for c in FIX["field"] if c["legs"]]
    n = 3 * 1024 + 5
    rng = np.random.default_rng(21)
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    b = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    pos = [0, 63, 64, 255, 256, 1023, 1024, n - 1]
    for j, i in enumerate(pos):
        c = legs[j % len(legs)]
        a[i], b[i] = c["a"], c["b"]
    gpu_ctx.set_chunk(1024)
    try:
        got = gpu_ctx.curve25519_field_op(2, a, b)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    for j, i in enumerate(pos):
        assert got[i].tolist() == legs[j % len(legs)]["expect"], i
    assert np.array_equal(got, gpu_ctx.curve25519_field_op(2, a, b))


def test_host_equals_dev_on_caller_stream_and_small_chunk(gpu_ctx):
    import torch
    n = (1 << 14) + 7
    s, u = _crafted_x25519(_bytes(n, 31), _bytes(n, 32), [0, 4095, 4096, n - 1])
    k, p = _mul_inputs(n, 33)
    k[4096] = [2, 0, 0, 0]
    want_x, want_m = gpu_ctx.x25519(s, u), gpu_ctx.curve25519_mul(k, p)
    gpu_ctx.set_chunk(4096)
    try:
        assert np.array_equal(gpu_ctx.x25519(s, u), want_x)
        assert np.array_equal(gpu_ctx.curve25519_mul(k, p), want_m)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    dev = torch.device("cuda:0")
    ts, tu, tk, tp = (torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev) for a in (s, u, k, p))
    ox = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    om = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.x25519_dev(ts.data_ptr(), tu.data_ptr(), ox.data_ptr(), n, stream.cuda_stream)
    gpu_ctx.curve25519_mul_dev(tk.data_ptr(), tp.data_ptr(), om.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(ox.cpu().numpy().reshape(n, 32), want_x)
    assert np.array_equal(om.cpu().numpy().view(np.uint64).reshape(n, 8), want_m)


def test_multi_ctx_equals_single(gpu_ctx):
    import forge_ec_amd as F
    n = 3001
    s, u = _bytes(n, 41), _bytes(n, 42)
    k, p = _mul_inputs(n, 43)
    a, b = _mul_inputs(n, 44)[1][:, :4], _mul_inputs(n, 45)[1][:, 4:]
    with F.Context(devices=[0, 0]) as multi:
        assert np.array_equal(multi.x25519(s, u), gpu_ctx.x25519(s, u))
        assert np.array_equal(multi.curve25519_mul(k, p), gpu_ctx.curve25519_mul(k, p))
        for op in range(5):
            assert np.array_equal(multi.curve25519_field_op(op, a, b), gpu_ctx.curve25519_field_op(op, a, b)), op


def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib = L.lib()
    h = gpu_ctx._h
    n = 64
    s, u = _bytes(n, 51), _bytes(n, 52)
    out = np.zeros_like(s)
    k, p = _mul_inputs(n, 53)
    om = np.zeros_like(p)
    assert lib.fec_x25519(h, None, _p(u), _p(out), n) == -1
    assert lib.fec_x25519(h, _p(s), _p(u), None, n) == -1
    assert lib.fec_x25519(None, _p(s), _p(u), _p(out), n) == -1
    assert lib.fec_x25519(h, None, None, None, 0) == 0
    assert lib.fec_curve25519_mul(h, _p(k), None, _p(om), n) == -1
    assert lib.fec_curve25519_mul(h, None, None, None, 0) == 0
    assert lib.fec_curve25519_field_op(h, 2, _p(k), None, _p(om), n) == -1   # Mul needs b
    assert lib.fec_curve25519_field_op(h, 7, _p(k), _p(k), _p(om), n) == -1
    assert lib.fec_curve25519_field_op(h, 0, None, None, None, 0) == 0
    dev = torch.device("cuda:0")
    t = [torch.zeros(n * 64 + 64, dtype=torch.uint8, device=dev) for _ in range(3)]
    q = [x.data_ptr() for x in t]
    assert lib.fec_x25519_dev(h, q[0], None, q[2], n, None) == -1
    assert lib.fec_x25519_dev(h, None, None, None, 0, None) == 0
    assert lib.fec_curve25519_mul_dev(h, None, q[1], q[2], n, None) == -1
    for j in range(3):                                                   # 16-byte alignment
        r = list(q)
        r[j] += 8
        assert lib.fec_x25519_dev(h, *r, n, None) == -1, j
        assert lib.fec_curve25519_mul_dev(h, *r, n, None) == -1, j
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_x25519_dev(multi._h, *q, n, None) == -5
        assert lib.fec_curve25519_mul_dev(multi._h, *q, n, None) == -5
    torch.cuda.synchronize()
    assert gpu_ctx.x25519(s, u).shape == (n, 32)                          # the ctx is still usable
