"""
GPU tests of fec_sha256 / fec_sha256_dev against hashlib: mixed lengths 0..200 at unaligned offsets (n = 257, more than
one workgroup), batches of one fixed message length on each side of the padding edges (0, 55, 56, 64), one 2^14 batch of
64-byte messages, and the argument errors fec_sha512 rejects.
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _msgs(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    out, p = [], 0
    for L_ in lens:
        out.append(blob[p:p + L_])
        p += int(L_)
    return out


def _dev_buffers(torch, msgs):
    dev = torch.device("cuda:0")
    buf = b"".join(msgs)
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    tb = torch.from_numpy(np.frombuffer(buf or b"\0", dtype=np.uint8).copy()).to(dev)
    to = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
    return tb, to, len(buf)


def _check(got, msgs):
    for i, m in enumerate(msgs):
        assert got[i].tobytes() == hashlib.sha256(m).digest(), (i, len(m))


def test_mixed_lengths_host_and_dev_unaligned(gpu_ctx):
    import torch
    msgs = _msgs(257, 1, 0, 200)
    msgs[0], msgs[256] = b"", b"abc"
    _check(gpu_ctx.sha256(msgs), msgs)
    tb, to, total = _dev_buffers(torch, msgs)
    for shift in (1, 2, 3):
        big = torch.zeros(total + 16, dtype=torch.uint8, device=tb.device)
        big[shift:shift + total] = tb[:total]
        out = torch.zeros(len(msgs) * 32, dtype=torch.uint8, device=tb.device)
        st = torch.full((len(msgs),), 9, dtype=torch.uint8, device=tb.device)
        gpu_ctx.sha256_dev(big.data_ptr() + shift, to.data_ptr(), total, out.data_ptr(), st.data_ptr(), len(msgs))
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
        _check(out.cpu().numpy().reshape(-1, 32), msgs)


@pytest.mark.parametrize("length", [0, 55, 56, 64])
def test_one_fixed_message_length(gpu_ctx, length):
    msgs = _msgs(300, 10 + length, length, length)
    _check(gpu_ctx.sha256(msgs), msgs)


def test_batch_of_2_to_the_14(gpu_ctx):
    n = 1 << 14
    blob = np.random.default_rng(3).integers(0, 256, size=n * 64, dtype=np.uint8).tobytes()
    msgs = [blob[64 * i:64 * i + 64] for i in range(n)]
    _check(gpu_ctx.sha256(msgs), msgs)


def test_chunked_and_multi_device(gpu_ctx):
    import forge_ec_amd as F
    msgs = _msgs(1000, 4, 0, 130)
    gpu_ctx.set_chunk(77)
    try:
        _check(gpu_ctx.sha256(msgs), msgs)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    with F.Context(devices=[0, 0]) as multi:
        _check(multi.sha256(msgs), msgs)


def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib, h = L.lib(), gpu_ctx._h
    n = 8
    msgs = np.zeros(64, dtype=np.uint8).ctypes.data
    good = np.arange(0, 45, 5, dtype=np.uint64)                       # 9 offsets, off[8] = 40
    out = np.zeros((n, 32), dtype=np.uint8)
    op = out.ctypes.data
    assert lib.fec_sha256(h, msgs, good.ctypes.data, 40, op, n) == 0
    bad = good.copy()
    bad[3], bad[4] = 20, 10                                           # not monotonic
    assert lib.fec_sha256(h, msgs, bad.ctypes.data, 40, op, n) == -1
    assert lib.fec_sha256(h, msgs, good.ctypes.data, 41, op, n) == -1  # off[n] != msg_len
    nz = good.copy()
    nz[0] = 1
    assert lib.fec_sha256(h, msgs, nz.ctypes.data, 40, op, n) == -1    # off[0] != 0
    assert lib.fec_sha256(h, msgs, None, 40, op, n) == -1
    assert lib.fec_sha256(h, None, good.ctypes.data, 40, op, n) == -1
    assert lib.fec_sha256(h, msgs, good.ctypes.data, 40, None, n) == -1
    assert lib.fec_sha256(None, msgs, good.ctypes.data, 40, op, n) == -1
    dev = torch.device("cuda:0")
    tm = torch.zeros(64, dtype=torch.uint8, device=dev)
    offs = np.array([0, 5, 10, 50, 45, 3, 1 << 62, 2, 7], dtype=np.uint64)   # elements 2..6 out of range
    to = torch.from_numpy(offs.view(np.uint8).copy()).to(dev)
    dg = torch.full((n * 32,), 7, dtype=torch.uint8, device=dev)
    dst = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.sha256_dev(tm.data_ptr(), to.data_ptr(), 40, dg.data_ptr(), dst.data_ptr(), n)
    torch.cuda.synchronize()
    want_bad = [not (offs[i] <= offs[i + 1] <= 40) for i in range(n)]
    assert list(dst.cpu().numpy() == 4) == want_bad
    d = dg.cpu().numpy().reshape(n, 32)
    for i in range(n):
        if want_bad[i]:
            assert not d[i].any(), i
        else:
            assert d[i].tobytes() == hashlib.sha256(bytes(int(offs[i + 1] - offs[i]))).digest(), i
    assert lib.fec_sha256_dev(h, tm.data_ptr(), to.data_ptr(), 40, dg.data_ptr() + 8, dst.data_ptr(), n, None) == -1
    assert lib.fec_sha256_dev(h, tm.data_ptr(), to.data_ptr() + 4, 40, dg.data_ptr(), dst.data_ptr(), n, None) == -1
    assert lib.fec_sha256_dev(h, tm.data_ptr(), None, 40, dg.data_ptr(), dst.data_ptr(), n, None) == -1
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_sha256_dev(multi._h, tm.data_ptr(), to.data_ptr(), 40, dg.data_ptr(), dst.data_ptr(), n, None) == -5
