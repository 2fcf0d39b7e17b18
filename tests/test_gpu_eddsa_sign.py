"""
GPU tests of the parity-mode EdDSA signers for Ed25519 with SHA-512 (fec_ed25519_sign, fec_ed25519_derive_public_key,
fec_eddsa_sign_ed25519 and their _dev forms) and of fec_sha512: the hash against hashlib over every padding boundary,
mixed lengths, a long message and unaligned buffers; the signers byte for byte against the restatement fixture
(tests/golden/eddsa_sign_vectors.json) and against the C-oracle composition (tests/eddsa_sign_ref.py); a 2^20 batch
against a composition of already-pinned GPU calls; chunked host calls, the _dev form on a caller's stream, a
multi-device ctx and the prefix table on and off; the verifier on the produced signatures; argument errors.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import eddsa_sign_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "eddsa_sign_vectors.json")


def _fixture():
    return json.load(open(FIXTURE))


def _keys(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)


def _msgs(n, seed, lo=0, hi=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    out, p = [], 0
    for L_ in lens:
        out.append(blob[p:p + L_])
        p += L_
    return out


def _plant(keys, msgs):
    """special cases and near misses at fixed positions"""
    keys[3, 0], msgs[3] = 0x9D, b""
    keys[4, 0], msgs[4] = 0x9C, b""
    msgs[5] = b"test message"
    msgs[6] = b"test messagf"
    keys[7, 0] = 0x9D


def _dev_buffers(torch, msgs):
    dev = torch.device("cuda:0")
    buf = b"".join(msgs)
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    tb = torch.from_numpy(np.frombuffer(buf or b"\0", dtype=np.uint8).copy()).to(dev)
    to = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
    return tb, to, len(buf)


# ---- SHA-512 ----

def test_sha512_every_length_to_400(gpu_ctx):
    rng = np.random.default_rng(1)
    msgs = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in range(401)]
    got = gpu_ctx.sha512(msgs)
    for n, m in enumerate(msgs):
        assert got[n].tobytes() == hashlib.sha512(m).digest(), n


def test_sha512_mixed_lengths_and_a_long_message(gpu_ctx):
    msgs = _msgs(2000, 2, 0, 4096)
    msgs[777] = np.random.default_rng(3).integers(0, 256, size=65536, dtype=np.uint8).tobytes()
    got = gpu_ctx.sha512(msgs)
    for i, m in enumerate(msgs):
        assert got[i].tobytes() == hashlib.sha512(m).digest(), i


def test_sha512_dev_unaligned_base(gpu_ctx):
    import torch
    msgs = _msgs(1000, 4, 0, 300)
    tb, to, total = _dev_buffers(torch, msgs)
    for shift in (1, 2, 3):
        big = torch.zeros(total + 16, dtype=torch.uint8, device=tb.device)
        big[shift:shift + total] = tb[:total]
        out = torch.zeros(len(msgs) * 64, dtype=torch.uint8, device=tb.device)
        st = torch.full((len(msgs),), 9, dtype=torch.uint8, device=tb.device)
        gpu_ctx.sha512_dev(big.data_ptr() + shift, to.data_ptr(), total, out.data_ptr(), st.data_ptr(), len(msgs))
        torch.cuda.synchronize()
        o = out.cpu().numpy().reshape(-1, 64)
        assert not st.cpu().numpy().any()
        for i, m in enumerate(msgs):
            assert o[i].tobytes() == hashlib.sha512(m).digest(), (shift, i)


# ---- the signers against the fixture ----

def test_fixture_sign(gpu_ctx):
    cases = _fixture()["sign"]
    keys = np.array([list(bytes.fromhex(c["key"])) for c in cases], dtype=np.uint8)
    sig, st = gpu_ctx.ed25519_sign(keys, [bytes.fromhex(c["msg"]) for c in cases])
    for i, c in enumerate(cases):
        assert sig[i].tobytes().hex() == c["sig"] and st[i] == c["status"], i


def test_fixture_derive(gpu_ctx):
    cases = _fixture()["derive"]
    keys = np.array([list(bytes.fromhex(c["key"])) for c in cases], dtype=np.uint8)
    pk, st = gpu_ctx.ed25519_derive_public_key(keys)
    for i, c in enumerate(cases):
        assert pk[i].tobytes().hex() == c["pk"] and st[i] == c["status"], i


def test_fixture_generic(gpu_ctx):
    cases = _fixture()["generic"]
    sk = np.array([[int(v, 16) for v in c["sk"]] for c in cases], dtype=np.uint64)
    r_xy, r_inf, s, st = gpu_ctx.eddsa_sign_ed25519(sk, [bytes.fromhex(c["msg"]) for c in cases])
    for i, c in enumerate(cases):
        assert [int(v) for v in r_xy[i]] == [int(v, 16) for v in c["r_xy"]], i
        assert [int(v) for v in s[i]] == [int(v, 16) for v in c["s"]], i
        assert (r_inf[i], st[i]) == (c["r_inf"], c["status"]), i


# ---- against the C-oracle composition ----

def test_random_2_14_against_oracle(gpu_ctx):
    n = 1 << 14
    keys, msgs = _keys(n, 10), _msgs(n, 11)
    _plant(keys, msgs)
    sig, st = gpu_ctx.ed25519_sign(keys, msgs)
    want = R.sign_batch(keys, msgs, R.CBackend())
    assert {w[1] for w in want} >= {0, 2}
    for i, (ws, wst) in enumerate(want):
        assert sig[i].tobytes() == ws and st[i] == wst, i
    pk, pst = gpu_ctx.ed25519_derive_public_key(keys[:2048])
    for i, (wp, wst) in enumerate(R.derive_batch(keys[:2048], R.CBackend())):
        assert pk[i].tobytes() == wp and pst[i] == wst, i
    sk = np.random.default_rng(12).integers(0, 1 << 63, size=(2048, 4), dtype=np.uint64) * np.uint64(2)
    r_xy, r_inf, s, gst = gpu_ctx.eddsa_sign_ed25519(sk, msgs[:2048])
    for i, (wx, wy, winf, ws, wst) in enumerate(R.eddsa_sign_batch(sk, msgs[:2048], R.CBackend())):
        assert [int(v) for v in r_xy[i]] == list(wx) + list(wy) and [int(v) for v in s[i]] == list(ws), i
        assert (r_inf[i], gst[i]) == (int(winf), wst), i


def test_2_20_batch_64_byte_messages(gpu_ctx):
    """R (sig[0..32]) of every element against fec_batch_mul_fixed / fec_batch_to_affine / fec_batch_compress on r
    drawn with hashlib; 4096 sampled elements in full against the C-oracle composition; special cases planted."""
    n = 1 << 20
    keys = _keys(n, 20)
    blob = np.random.default_rng(21).integers(0, 256, size=n * 64, dtype=np.uint8).tobytes()
    msgs = [blob[64 * i:64 * i + 64] for i in range(n)]
    _plant(keys, msgs)
    sig, st = gpu_ctx.ed25519_sign(keys, msgs)
    special = {3, 5}
    live = np.array([i for i in range(n) if i not in special])
    r = np.zeros((live.size, 4), dtype=np.uint64)
    for j, i in enumerate(live):
        nonce = hashlib.sha512(keys[i].tobytes()).digest()[:32]
        r[j] = R.from_bytes_be(hashlib.sha512(nonce + msgs[i]).digest()[:32])
    xy, inf = gpu_ctx.batch_to_affine(2, gpu_ctx.batch_mul_fixed(2, r, gpu_ctx.generator(2)))
    r33 = gpu_ctx.batch_compress(2, xy, inf)
    assert np.array_equal(sig[live, :32], r33[:, :32])
    assert sig[3].tobytes() == R.RFC_SIG and sig[5].tobytes() == R.PATTERN_SIG
    idx = np.unique(np.concatenate([np.arange(8), np.random.default_rng(22).integers(0, n, 4096)]))
    want = R.sign_batch(keys[idx], [msgs[i] for i in idx], R.CBackend())
    for j, i in enumerate(idx):
        assert sig[i].tobytes() == want[j][0] and st[i] == want[j][1], i


# ---- forms and contexts ----

def test_chunked_host_call_equals_dev_on_caller_stream(gpu_ctx):
    import torch
    n = 5000
    keys, msgs = _keys(n, 30), _msgs(n, 31, 0, 700)
    _plant(keys, msgs)
    want = gpu_ctx.ed25519_sign(keys, msgs)
    gpu_ctx.set_chunk(333)
    try:
        got = gpu_ctx.ed25519_sign(keys, msgs)
        gsk = np.random.default_rng(32).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        g_chunked = gpu_ctx.eddsa_sign_ed25519(gsk, msgs)
        d_chunked = gpu_ctx.ed25519_derive_public_key(keys)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for a, b in zip(g_chunked, gpu_ctx.eddsa_sign_ed25519(gsk, msgs)):
        assert np.array_equal(a, b)
    for a, b in zip(d_chunked, gpu_ctx.ed25519_derive_public_key(keys)):
        assert np.array_equal(a, b)
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(keys.copy()).to(dev)
    tb, to, total = _dev_buffers(torch, msgs)
    sig = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.ed25519_sign_dev(tk.data_ptr(), tb.data_ptr(), to.data_ptr(), total, sig.data_ptr(), st.data_ptr(), n,
                             stream.cuda_stream)
    pk = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    pst = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.ed25519_derive_public_key_dev(tk.data_ptr(), pk.data_ptr(), pst.data_ptr(), n, stream.cuda_stream)
    tsk = torch.from_numpy(gsk.view(np.uint8).reshape(-1).copy()).to(dev)
    rxy = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    rinf = torch.zeros(n, dtype=torch.uint8, device=dev)
    s = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    gst = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.eddsa_sign_ed25519_dev(tsk.data_ptr(), tb.data_ptr(), to.data_ptr(), total, rxy.data_ptr(), rinf.data_ptr(),
                                   s.data_ptr(), gst.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(sig.cpu().numpy().reshape(n, 64), want[0]) and np.array_equal(st.cpu().numpy(), want[1])
    assert np.array_equal(pk.cpu().numpy().reshape(n, 32), d_chunked[0]) and np.array_equal(pst.cpu().numpy(), d_chunked[1])
    assert np.array_equal(rxy.cpu().numpy().view(np.uint64).reshape(n, 8), g_chunked[0])
    assert np.array_equal(rinf.cpu().numpy(), g_chunked[1])
    assert np.array_equal(s.cpu().numpy().view(np.uint64).reshape(n, 4), g_chunked[2])
    assert np.array_equal(gst.cpu().numpy(), g_chunked[3])


def test_multi_ctx_equals_single(gpu_ctx):
    import forge_ec_amd as F
    n = 3001
    keys, msgs = _keys(n, 40), _msgs(n, 41)
    _plant(keys, msgs)
    sk = np.random.default_rng(42).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    with F.Context(devices=[0, 0]) as multi:
        for a, b in zip(multi.ed25519_sign(keys, msgs), gpu_ctx.ed25519_sign(keys, msgs)):
            assert np.array_equal(a, b)
        for a, b in zip(multi.ed25519_derive_public_key(keys), gpu_ctx.ed25519_derive_public_key(keys)):
            assert np.array_equal(a, b)
        for a, b in zip(multi.eddsa_sign_ed25519(sk, msgs), gpu_ctx.eddsa_sign_ed25519(sk, msgs)):
            assert np.array_equal(a, b)
        assert np.array_equal(multi.sha512(msgs), gpu_ctx.sha512(msgs))


def test_prefix_table_on_and_off():
    import forge_ec_amd as F
    n = 1 << 16
    keys, msgs = _keys(n, 50), _msgs(n, 51, 0, 100)
    with F.Context(0) as off, F.Context(0) as on:
        off.set_fixed_prefix_bits(0)
        on.set_fixed_prefix_bits(12)
        on.build_fixed_prefix(2)
        for a, b in zip(on.ed25519_sign(keys, msgs), off.ed25519_sign(keys, msgs)):
            assert np.array_equal(a, b)


def test_verify_on_produced_signatures(gpu_ctx, oracle):
    """The GPU verifier on (R, s, A, k) of the produced signatures equals the oracle's verify, whatever it is."""
    n = 1024
    sk = np.random.default_rng(60).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    msgs = _msgs(n, 61, 1, 200)
    r_xy, r_inf, s, st = gpu_ctx.eddsa_sign_ed25519(sk, msgs)
    a = np.zeros((n, 4), dtype=np.uint64)
    k = np.zeros((n, 4), dtype=np.uint64)
    for i in range(n):
        skb = R.to_bytes_be([int(v) for v in sk[i]])
        a[i] = R._key_scalar(skb)[1]
    pk_xy, pk_inf = gpu_ctx.batch_to_affine(2, gpu_ctx.batch_mul_fixed(2, a, gpu_ctx.generator(2)))
    rb, pb = gpu_ctx.batch_compress(2, r_xy, r_inf), gpu_ctx.batch_compress(2, pk_xy, pk_inf)
    for i in range(n):
        k[i] = R.from_bytes_be(hashlib.sha512(rb[i].tobytes() + pb[i].tobytes() + msgs[i]).digest()[:32])
    got = gpu_ctx.eddsa_verify_ed25519(r_xy, r_inf, pk_xy, pk_inf, s, k)
    want = oracle.batch_ed25519_eddsa_verify(r_xy, r_inf, pk_xy, pk_inf, s, k, nthreads=16)
    assert np.array_equal(got, want)


# ---- argument errors ----

def test_argument_errors(gpu_ctx):
    import torch
    from forge_ec_amd import _lib as L
    lib = L.lib()
    h = gpu_ctx._h
    n = 8
    keys = _keys(n, 70)
    msgs = b"x" * 40
    sig = np.zeros((n, 64), dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    good = np.arange(0, 41, 5, dtype=np.uint64)
    kp, sp, tp = keys.ctypes.data, sig.ctypes.data, st.ctypes.data
    assert lib.fec_ed25519_sign(h, kp, msgs, good.ctypes.data, 40, sp, tp, n) == 0
    bad = good.copy()
    bad[3], bad[4] = 20, 10                                              # not monotonic
    assert lib.fec_ed25519_sign(h, kp, msgs, bad.ctypes.data, 40, sp, tp, n) == -1
    assert lib.fec_ed25519_sign(h, kp, msgs, good.ctypes.data, 41, sp, tp, n) == -1    # off[n] != msg_len
    nz = good.copy()
    nz[0] = 1
    assert lib.fec_ed25519_sign(h, kp, msgs, nz.ctypes.data, 40, sp, tp, n) == -1      # off[0] != 0
    assert lib.fec_ed25519_sign(h, kp, msgs, None, 40, sp, tp, n) == -1
    assert lib.fec_ed25519_sign(h, None, msgs, good.ctypes.data, 40, sp, tp, n) == -1
    assert lib.fec_ed25519_sign(h, kp, None, good.ctypes.data, 40, sp, tp, n) == -1
    assert lib.fec_ed25519_sign(None, kp, msgs, good.ctypes.data, 40, sp, tp, n) == -1
    assert lib.fec_sha512(h, msgs, bad.ctypes.data, 40, sp, n) == -1
    assert lib.fec_eddsa_sign_ed25519(h, kp, msgs, bad.ctypes.data, 40, sp, tp, tp, tp, n) == -1
    assert lib.fec_ed25519_derive_public_key(h, None, sp, tp, n) == -1
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(keys.copy()).to(dev)
    tm = torch.zeros(64, dtype=torch.uint8, device=dev)
    offs = np.array([0, 5, 10, 50, 45, 3, 1 << 62, 2, 7], dtype=np.uint64)   # elements 2, 3, 5 (, 6) out of range
    to = torch.from_numpy(offs.view(np.uint8).copy()).to(dev)
    ts = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    tt = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.ed25519_sign_dev(tk.data_ptr(), tm.data_ptr(), to.data_ptr(), 40, ts.data_ptr(), tt.data_ptr(), n)
    dg = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    dst = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.sha512_dev(tm.data_ptr(), to.data_ptr(), 40, dg.data_ptr(), dst.data_ptr(), n)
    torch.cuda.synchronize()
    stv, sgv = tt.cpu().numpy(), ts.cpu().numpy().reshape(n, 64)
    want_bad = [not (offs[i] <= offs[i + 1] <= 40) for i in range(n)]
    for i in range(n):
        assert (stv[i] == 4) == want_bad[i], i
        if want_bad[i]:
            assert not sgv[i].any() and not dg.cpu().numpy().reshape(n, 64)[i].any(), i
    assert list(dst.cpu().numpy() == 4) == want_bad
    assert lib.fec_ed25519_sign_dev(h, tk.data_ptr() + 8, tm.data_ptr(), to.data_ptr(), 40, ts.data_ptr(), tt.data_ptr(), n, None) == -1
    assert lib.fec_ed25519_sign_dev(h, tk.data_ptr(), tm.data_ptr(), None, 40, ts.data_ptr(), tt.data_ptr(), n, None) == -1
    import forge_ec_amd as F
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_ed25519_sign_dev(multi._h, tk.data_ptr(), tm.data_ptr(), to.data_ptr(), 40, ts.data_ptr(),
                                        tt.data_ptr(), n, None) == -5
    assert gpu_ctx.ed25519_sign(keys, [b"a"] * n)[1].shape == (n,)       # the ctx is still usable
