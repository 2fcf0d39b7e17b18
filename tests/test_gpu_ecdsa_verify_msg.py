"""
GPU tests of fec_ecdsa_verify_msg / _dev (Ecdsa::<C, Sha256>::verify from the message, ecdsa.rs:213-281) on secp256k1
and P-256, at n = 257 and 2^14, against the oracle's digest-form verifier fed hashlib.sha256(msg).

Where the rows come from.  The rejecting rows are signatures made by tests/ecdsa_sign_ref.py on sha256(msg) -- the
reference's own signer -- and corrupted copies of them (wrong message, r, s, key; r, s in {0, n}).  The reference's
sign -> verify does NOT round-trip under its own scalar arithmetic (on secp256k1 s^-1 collapses to 0 for about half of
all s and normalize always returns n - s; measured on the CPU: 0 of 64 of its signatures verify on either curve), so these
alone give no accepting row: test_reference_signatures_do_not_round_trip pins that.  The accepting rows therefore use
the construction of tests/golden/gen_ecdsa_p256.py and tests/test_gpu_parity.py (the sources tests/test_gpu_golden.py
and the digest-form parity test draw theirs from): with the public key at infinity R = multiply(G, h * s^-1) does not
depend on r, so r is set to the x the reference derives.  Each batch must hold at least 25 % of status 1 and 25 % of
status 0 ON THE ORACLE'S VERDICTS.
"""
import functools
import hashlib

import numpy as np
import pytest

import ecdsa_sign_ref as S

pytestmark = pytest.mark.gpu

ONE = np.array([1, 0, 0, 0], dtype=np.uint64)
SIZES = (257, 1 << 14)


def _digests(msgs):
    return np.array([list(hashlib.sha256(m).digest()) for m in msgs], dtype=np.uint8).reshape(-1, 32)


def _limbs(v):
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def _verify(oracle, curve, dg, r, s, pk, inf):
    f = oracle.batch_secp256k1_ecdsa_verify if curve == 0 else oracle.batch_p256_ecdsa_verify
    return f(dg, r, s, pk, inf, nthreads=16)


@functools.lru_cache(maxsize=None)
def _batch_cached(curve, n):
    from oracle import c_oracle as oracle
    rng = np.random.default_rng(1000 * curve + n)
    lens = rng.integers(0, 201, size=n)
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    msgs, p = [], 0
    for L_ in lens:
        msgs.append(blob[p:p + L_])
        p += int(L_)
    msgs[1] = b"test message"          # no special case in ecdsa.rs:213-281: hashed like any other
    msgs[2] = b""
    sk = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
    k = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
    dg = _digests(msgs)
    g = oracle.generator(curve)
    n_acc = (7 * n) // 10 if curve == 0 else (4 * n) // 10
    r, s = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    r[n_acc:], s[n_acc:], _ = S.sign(oracle, curve, sk[n_acc:], dg[n_acc:], k[n_acc:], nthreads=16)   # the reference's own signatures
    pk, inf = oracle.batch_to_affine(curve, oracle.batch_mul_fixed(curve, sk, g, nthreads=16), nthreads=16)
    pk, inf = np.ascontiguousarray(pk), np.ascontiguousarray(inf).astype(np.uint8)
    # accepting rows: the key at infinity, r = x of multiply(G, h * s^-1) as the reference derives it
    op = oracle.secp256k1_scalar_op if curve == 0 else oracle.p256_scalar_op
    u1 = np.zeros((n_acc, 4), dtype=np.uint64)
    s[:n_acc] = rng.integers(1, 1 << 62, size=(n_acc, 4), dtype=np.uint64)
    for i in range(n_acc):
        h = np.array(_limbs(int.from_bytes(dg[i].tobytes(), "big")), dtype=np.uint64)
        s_inv, ok = op("inv", s[i])
        u1[i] = op("mul", h, s_inv)[0] if ok else 0
    xy, xinf = oracle.batch_to_affine(curve, oracle.batch_mul_fixed(curve, u1, g, nthreads=16), nthreads=16)
    for i in range(n_acc):
        inf[i] = 1
        r[i] = oracle.field_op(0, "mul", xy[i, :4], ONE) if curve == 0 else xy[i, :4]
    # corrupted copies, spread over both kinds of row
    order = S.N[curve]
    for i in range(5, n, 11):
        kind = (i // 11) % 7
        if kind == 0:
            msgs[i] = msgs[i] + b"!"                                       # wrong message
        elif kind == 1:
            r[i, 0] ^= np.uint64(1)
        elif kind == 2:
            s[i, 1] ^= np.uint64(4)
        elif kind == 3:
            inf[i] = 0                                                     # wrong key
            pk[i, 0] ^= np.uint64(2)
        elif kind == 4:
            r[i] = 0 if i % 2 else order
        elif kind == 5:
            s[i] = 0 if i % 2 else order
    dg = _digests(msgs)
    want = _verify(oracle, curve, dg, r, s, pk, inf)
    return msgs, dg, r, s, pk, inf, want


def _batch(curve, n):
    msgs, dg, r, s, pk, inf, want = _batch_cached(curve, n)
    return list(msgs), dg.copy(), r.copy(), s.copy(), pk.copy(), inf.copy(), want.copy()


@pytest.mark.parametrize("curve", [0, 1])
def test_reference_signatures_do_not_round_trip(oracle, curve):
    """The CPU-side finding that decides where the accepting rows come from (module docstring)."""
    n = 32
    rng = np.random.default_rng(curve)
    sk = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
    k = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
    dg = _digests([bytes([i]) * i for i in range(n)])
    r, s, _ = S.sign(oracle, curve, sk, dg, k, nthreads=16)
    pk, inf = oracle.batch_to_affine(curve, oracle.batch_mul_fixed(curve, sk, oracle.generator(curve), nthreads=16), nthreads=16)
    assert not (_verify(oracle, curve, dg, r, s, pk, inf) == 1).any()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_matches_oracle_on_the_digest(gpu_ctx, oracle, curve, n):
    msgs, dg, r, s, pk, inf, want = _batch(curve, n)
    assert int((want == 1).sum()) * 4 >= n and int((want == 0).sum()) * 4 >= n, np.bincount(want, minlength=3)
    got = gpu_ctx.ecdsa_verify_msg(curve, msgs, r, s, pk, inf)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first mismatch at %d: got %d want %d" % (bad[0], got[bad[0]], want[bad[0]])
    finite = gpu_ctx.ecdsa_verify_msg(curve, msgs, r, s, pk, None)           # NULL pk_inf: every key a finite point
    assert np.array_equal(finite, _verify(oracle, curve, dg, r, s, pk, None))


def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


@pytest.mark.parametrize("curve", [0, 1])
def test_dev_form_equals_sha256_then_digest_form(gpu_ctx, curve):
    import torch
    n = 257
    msgs, dg, r, s, pk, inf, want = _batch(curve, n)
    buf = b"".join(msgs)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    dev = torch.device("cuda:0")
    big = torch.zeros(len(buf) + 16, dtype=torch.uint8, device=dev)
    big[3:3 + len(buf)] = _to_dev(torch, np.frombuffer(buf, dtype=np.uint8))   # an unaligned message base
    to, tr, ts, tpk, tinf = (_to_dev(torch, a) for a in (off, r, s, pk, inf))
    st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.ecdsa_verify_msg_dev(curve, big.data_ptr() + 3, to.data_ptr(), len(buf), tr.data_ptr(), ts.data_ptr(), tpk.data_ptr(),
                                 tinf.data_ptr(), st.data_ptr(), n, stream.cuda_stream)
    d2 = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    st2 = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    gpu_ctx.sha256_dev(big.data_ptr() + 3, to.data_ptr(), len(buf), d2.data_ptr(), None, n, stream.cuda_stream)
    f = gpu_ctx.ecdsa_verify_secp256k1_dev if curve == 0 else gpu_ctx.ecdsa_verify_p256_dev
    f(d2.data_ptr(), tr.data_ptr(), ts.data_ptr(), tpk.data_ptr(), tinf.data_ptr(), st2.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d2.cpu().numpy().reshape(n, 32), dg)
    assert np.array_equal(st.cpu().numpy(), st2.cpu().numpy()) and np.array_equal(st.cpu().numpy(), want)


@pytest.mark.parametrize("curve", [0, 1])
def test_chunked_and_multi_device_host_forms(gpu_ctx, curve):
    import forge_ec_amd as F
    n = 257
    msgs, dg, r, s, pk, inf, want = _batch(curve, n)
    gpu_ctx.set_chunk(100)
    try:
        got = gpu_ctx.ecdsa_verify_msg(curve, msgs, r, s, pk, inf)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    assert np.array_equal(got, want)
    with F.Context(devices=[0, 0]) as multi:
        assert np.array_equal(multi.ecdsa_verify_msg(curve, msgs, r, s, pk, inf), want)


def test_argument_errors_and_bad_ranges(gpu_ctx):
    import torch
    from forge_ec_amd import _lib as L
    import forge_ec_amd as F
    lib, h = L.lib(), gpu_ctx._h
    n = 4
    msgs, dg, r, s, pk, inf, want = _batch(0, 257)
    r, s, pk = r[:n].copy(), s[:n].copy(), pk[:n].copy()
    st = np.zeros(n, dtype=np.uint8)
    good = np.array([0, 10, 20, 30, 40], dtype=np.uint64)
    mb = np.zeros(40, dtype=np.uint8)
    p = lambda a: a.ctypes.data
    call = lambda *a: lib.fec_ecdsa_verify_msg(*a)
    assert call(h, 0, p(mb), p(good), 40, p(r), p(s), p(pk), None, p(st), n) == 0
    bad = good.copy()
    bad[2], bad[3] = 30, 20
    assert call(h, 0, p(mb), p(bad), 40, p(r), p(s), p(pk), None, p(st), n) == -1        # not monotonic
    assert call(h, 0, p(mb), p(good), 41, p(r), p(s), p(pk), None, p(st), n) == -1       # off[n] != msg_len
    assert call(h, 0, p(mb), None, 40, p(r), p(s), p(pk), None, p(st), n) == -1
    assert call(h, 0, None, p(good), 40, p(r), p(s), p(pk), None, p(st), n) == -1
    assert call(h, 0, p(mb), p(good), 40, None, p(s), p(pk), None, p(st), n) == -1
    assert call(None, 0, p(mb), p(good), 40, p(r), p(s), p(pk), None, p(st), n) == -1
    assert call(h, 2, p(mb), p(good), 40, p(r), p(s), p(pk), None, p(st), n) == -5       # Ed25519 has no Ecdsa instance
    dev = torch.device("cuda:0")
    tm = torch.zeros(64, dtype=torch.uint8, device=dev)
    offs = np.array([0, 10, 5, 30, 41], dtype=np.uint64)                                 # elements 1 and 3 out of range
    to, tr, ts, tpk = (_to_dev(torch, a) for a in (offs, r, s, pk))
    tst = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    gpu_ctx.ecdsa_verify_msg_dev(0, tm.data_ptr(), to.data_ptr(), 40, tr.data_ptr(), ts.data_ptr(), tpk.data_ptr(), None,
                                 tst.data_ptr(), n)
    torch.cuda.synchronize()
    assert [int(v) == 4 for v in tst.cpu().numpy()] == [False, True, False, True]
    assert lib.fec_ecdsa_verify_msg_dev(h, 0, tm.data_ptr(), to.data_ptr(), 40, tr.data_ptr() + 8, ts.data_ptr(), tpk.data_ptr(), None,
                                        tst.data_ptr(), n, None) == -1
    assert lib.fec_ecdsa_verify_msg_dev(h, 0, tm.data_ptr(), None, 40, tr.data_ptr(), ts.data_ptr(), tpk.data_ptr(), None,
                                        tst.data_ptr(), n, None) == -1
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_ecdsa_verify_msg_dev(multi._h, 0, tm.data_ptr(), to.data_ptr(), 40, tr.data_ptr(), ts.data_ptr(),
                                            tpk.data_ptr(), None, tst.data_ptr(), n, None) == -5
