"""
GPU tests of fec_bip340_sign / _dev (BipSchnorr::sign, schnorr.rs:302-420): the restatement fixture
(tests/golden/bip340_sign_vectors.json) byte for byte and status for status; random keys and messages of mixed lengths
and one 2^14 batch against tests/bip340_sign_ref.py over the C oracle; the prefix table and the chunk size do not show
in the result; the _dev form on a caller's stream with an unaligned message base, a {0, 0} multi-device ctx, a batch in
which every lane is decided before the first multiplication; argument errors.
"""
import functools
import json
import os

import numpy as np
import pytest

import bip340_sign_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "bip340_sign_vectors.json")


def _inputs(n, seed, lo=0, hi=200):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    lens = rng.integers(lo, hi + 1, size=n)
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    msgs, p = [], 0
    for L_ in lens:
        msgs.append(blob[p:p + L_])
        p += int(L_)
    # the decided legs and their near misses at fixed positions
    msgs[3] = b"test message"
    msgs[4] = b"test messagf"
    msgs[5] = b""
    keys[6] = 0xFF                                                   # d >= N
    keys[7] = np.frombuffer(R.N_VALUE.to_bytes(32, "little"), dtype=np.uint8)
    keys[8] = np.frombuffer((R.N_VALUE - 1).to_bytes(32, "little"), dtype=np.uint8)
    keys[9] = 0                                                      # d = 0
    return keys, msgs


@functools.lru_cache(maxsize=None)
def _reference(n, seed):
    keys, msgs = _inputs(n, seed)
    want = R.sign_batch(keys, msgs, R.CBackend(16))
    sig = np.array([list(s) for s, _ in want], dtype=np.uint8)
    st = np.array([t for _, t in want], dtype=np.uint8)
    return keys, msgs, sig, st


def _assert_equal(got, sig, st):
    bad = np.nonzero((got[0] != sig).any(axis=1) | (got[1] != st))[0]
    assert len(bad) == 0, "first mismatch at %d: status %d want %d" % (bad[0], got[1][bad[0]], st[bad[0]])


def test_fixture(gpu_ctx):
    cases = json.load(open(FIXTURE))["sign"]
    keys = np.array([list(bytes.fromhex(c["key"])) for c in cases], dtype=np.uint8)
    sig, st = gpu_ctx.bip340_sign(keys, [bytes.fromhex(c["msg"]) for c in cases])
    for i, c in enumerate(cases):
        assert sig[i].tobytes().hex() == c["sig"] and st[i] == c["status"], i


@pytest.mark.parametrize("n", [257, 1 << 14])
def test_random_batch_against_the_c_oracle_composition(gpu_ctx, n):
    keys, msgs, sig, st = _reference(n, n)
    assert set(int(v) for v in st) == {0, 1, 2}
    _assert_equal(gpu_ctx.bip340_sign(keys, msgs), sig, st)


def test_prefix_table_and_chunk_size_do_not_show(gpu_ctx):
    import forge_ec_amd as F
    keys, msgs, sig, st = _reference(257, 257)
    with F.Context(0) as off:
        off.set_fixed_prefix_bits(0)
        _assert_equal(off.bip340_sign(keys, msgs), sig, st)
    with F.Context(0) as on:
        on.set_fixed_prefix_bits(12)
        on.build_fixed_prefix(0)
        assert on.fixed_prefix_bits(0) == 12
        _assert_equal(on.bip340_sign(keys, msgs), sig, st)
    gpu_ctx.set_chunk(100)
    try:
        got = gpu_ctx.bip340_sign(keys, msgs)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    _assert_equal(got, sig, st)


def test_dev_form_unaligned_messages_and_multi_device(gpu_ctx):
    import torch
    import forge_ec_amd as F
    n = 257
    keys, msgs, sig, st = _reference(n, n)
    dev = torch.device("cuda:0")
    buf = b"".join(msgs)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    tk = torch.from_numpy(keys.copy()).to(dev)
    to = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
    stream = torch.cuda.Stream()
    for shift in (0, 1, 3):
        big = torch.zeros(len(buf) + 16, dtype=torch.uint8, device=dev)
        big[shift:shift + len(buf)] = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to(dev)
        ts = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
        tt = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        stream.wait_stream(torch.cuda.current_stream())
        gpu_ctx.bip340_sign_dev(tk.data_ptr(), big.data_ptr() + shift, to.data_ptr(), len(buf), ts.data_ptr(), tt.data_ptr(), n,
                                stream.cuda_stream)
        stream.synchronize()
        _assert_equal((ts.cpu().numpy().reshape(n, 64), tt.cpu().numpy()), sig, st)
    gpu_ctx.check()
    with F.Context(devices=[0, 0]) as multi:
        _assert_equal(multi.bip340_sign(keys, msgs), sig, st)


def test_every_lane_decided_early(gpu_ctx):
    n = 130
    keys = np.full((n, 32), 0xFF, dtype=np.uint8)                    # d >= N everywhere ...
    msgs = [b"x" * (i % 7) for i in range(n)]
    for i in range(0, n, 2):
        msgs[i] = b"test message"                                    # ... and the message case first where it applies
    sig, st = gpu_ctx.bip340_sign(keys, msgs)
    assert all(sig[i].tobytes() == R.PATTERN_SIG for i in range(n))
    assert list(st) == [1 if i % 2 == 0 else 2 for i in range(n)]


def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib, h = L.lib(), gpu_ctx._h
    n = 8
    keys, _ = _inputs(10 + n, 70)
    keys = np.ascontiguousarray(keys[10:10 + n])                     # past the decided legs of _inputs
    assert keys.shape == (n, 32)
    msgs = np.zeros(64, dtype=np.uint8).ctypes.data
    good = np.arange(0, 45, 5, dtype=np.uint64)
    sig = np.zeros((n, 64), dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    kp, sp, tp = keys.ctypes.data, sig.ctypes.data, st.ctypes.data
    assert lib.fec_bip340_sign(h, kp, msgs, good.ctypes.data, 40, sp, tp, n) == 0
    bad = good.copy()
    bad[3], bad[4] = 20, 10
    assert lib.fec_bip340_sign(h, kp, msgs, bad.ctypes.data, 40, sp, tp, n) == -1
    assert lib.fec_bip340_sign(h, kp, msgs, good.ctypes.data, 41, sp, tp, n) == -1
    assert lib.fec_bip340_sign(h, kp, msgs, None, 40, sp, tp, n) == -1
    assert lib.fec_bip340_sign(h, None, msgs, good.ctypes.data, 40, sp, tp, n) == -1
    assert lib.fec_bip340_sign(h, kp, None, good.ctypes.data, 40, sp, tp, n) == -1
    assert lib.fec_bip340_sign(h, kp, msgs, good.ctypes.data, 40, None, tp, n) == -1
    assert lib.fec_bip340_sign(h, kp, msgs, good.ctypes.data, 40, sp, None, n) == -1
    assert lib.fec_bip340_sign(None, kp, msgs, good.ctypes.data, 40, sp, tp, n) == -1
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(keys.copy()).to(dev)
    tm = torch.zeros(64, dtype=torch.uint8, device=dev)
    offs = np.array([0, 5, 10, 50, 45, 3, 1 << 62, 2, 7], dtype=np.uint64)   # elements 2..6 out of range
    to = torch.from_numpy(offs.view(np.uint8).copy()).to(dev)
    ts = torch.full((n * 64,), 7, dtype=torch.uint8, device=dev)
    tt = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.bip340_sign_dev(tk.data_ptr(), tm.data_ptr(), to.data_ptr(), 40, ts.data_ptr(), tt.data_ptr(), n)
    torch.cuda.synchronize()
    want_bad = [not (offs[i] <= offs[i + 1] <= 40) for i in range(n)]
    stv, sgv = tt.cpu().numpy(), ts.cpu().numpy().reshape(n, 64)
    live = [i for i in range(n) if not want_bad[i]]
    want = R.sign_batch([keys[i] for i in live], [bytes(int(offs[i + 1] - offs[i])) for i in live], R.CBackend(4))
    for i in range(n):
        if want_bad[i]:
            assert stv[i] == 4 and not sgv[i].any(), i
    for i, (s_, t_) in zip(live, want):
        assert sgv[i].tobytes() == s_ and stv[i] == t_, i
    assert lib.fec_bip340_sign_dev(h, tk.data_ptr() + 8, tm.data_ptr(), to.data_ptr(), 40, ts.data_ptr(), tt.data_ptr(), n, None) == -1
    assert lib.fec_bip340_sign_dev(h, tk.data_ptr(), tm.data_ptr(), None, 40, ts.data_ptr(), tt.data_ptr(), n, None) == -1
    assert lib.fec_bip340_sign_dev(h, tk.data_ptr(), tm.data_ptr(), to.data_ptr() + 4, 40, ts.data_ptr(), tt.data_ptr(), n, None) == -1
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_bip340_sign_dev(multi._h, tk.data_ptr(), tm.data_ptr(), to.data_ptr(), 40, ts.data_ptr(), tt.data_ptr(), n, None) == -5
