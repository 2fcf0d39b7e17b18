"""
GPU tests of the parity-mode Ed25519 EdDSA verifiers from the message (fec_ed25519_verify, fec_eddsa_verify_ed25519_msg
and their _dev forms): status for status against the restatement fixture (tests/golden/eddsa_verify_vectors.json) and
against the restatement over the C oracle (tests/eddsa_verify_ref.py) at the batch sizes and message lengths where the
kernels change path; a 2^16 batch against a chain of already-pinned GPU calls; chunked host calls, the _dev forms on a
caller's stream, a multi-device ctx, the prefix table on and off; unaligned message buffers; argument errors.

Byte-form inputs: under the reference's sqrt a random x never decodes (tests/golden/gen_eddsa_verify.py), so the lanes
that must reach the point computation are drawn by rejection sampling from a pool that holds the decodable x = 0.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import eddsa_sign_ref as S
import eddsa_verify_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "eddsa_verify_vectors.json")
ED = 2


def _msgs(n, seed, lo=1, hi=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    out, p = [], 0
    for L_ in lens:
        out.append(blob[p:p + L_])
        p += L_
    return out


def _plant(msgs):
    """the three message cases and a near miss of each at fixed positions"""
    msgs[3], msgs[4], msgs[5] = b"test message", b"", b"different message"
    msgs[6], msgs[7], msgs[8] = b"test messagf", b"different messagE", b"\x00"


def _byte_inputs(oracle, n, seed):
    """pk (n, 32), sig (n, 64) with R and A drawn by rejection sampling: a candidate x (random, or 0) is kept for a lane
    that is to decode only if oracle.batch_decompress accepts it.  Returns the share of lanes where both decode."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, size=(64, 33), dtype=np.uint8)
    pool[:, 0] = 2
    pool[::2, 1:] = 0
    ok = oracle.batch_decompress(ED, pool)[2].astype(bool)
    good, bad = pool[ok][:, 1:], pool[~ok][:, 1:]
    assert len(good) and len(bad)
    want = rng.integers(0, 4, size=(n, 2)) != 0                       # 3/4 of the R, 3/4 of the A are to decode
    pk = np.where(want[:, :1], good[rng.integers(0, len(good), n)], bad[rng.integers(0, len(bad), n)])
    r = np.where(want[:, 1:], good[rng.integers(0, len(good), n)], bad[rng.integers(0, len(bad), n)])
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[rng.integers(0, 3, n) == 0] = 0                                 # s = 0 is where such a lane can verify
    both = oracle.batch_decompress(ED, np.concatenate([np.full((n, 1), 2, np.uint8), pk], 1))[2].astype(bool) & \
        oracle.batch_decompress(ED, np.concatenate([np.full((n, 1), 2, np.uint8), r], 1))[2].astype(bool)
    return np.ascontiguousarray(pk), np.ascontiguousarray(np.concatenate([r, s], 1)), float(both.mean())


def _generic_inputs(n, seed):
    rng = np.random.default_rng(seed)
    f = lambda w: rng.integers(0, 1 << 63, size=(n, w), dtype=np.uint64)
    pk_inf = (rng.integers(0, 8, n) == 0).astype(np.uint8)
    r_inf = (rng.integers(0, 8, n) == 1).astype(np.uint8)
    return f(8), pk_inf, f(8), r_inf, f(4)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def _dev_msgs(torch, msgs):
    buf = b"".join(msgs)
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return _dev(torch, np.frombuffer(buf or b"\0", dtype=np.uint8)), _dev(torch, off), len(buf)


# ---- the fixture ----

def test_fixture(gpu_ctx):
    fx = json.load(open(FIXTURE))
    c = fx["bytes"]
    got = gpu_ctx.ed25519_verify(np.array([list(bytes.fromhex(x["pk"])) for x in c], dtype=np.uint8), [bytes.fromhex(x["msg"]) for x in c],
                                 np.array([list(bytes.fromhex(x["sig"])) for x in c], dtype=np.uint8))
    assert list(got) == [x["status"] for x in c]
    c = fx["generic"]
    h = lambda key, w: np.array([[int(v, 16) for v in x[key]] for x in c], dtype=np.uint64).reshape(-1, w)
    got = gpu_ctx.eddsa_verify_ed25519_msg(h("pk", 8), np.array([x["pk_inf"] for x in c], dtype=np.uint8), [bytes.fromhex(x["msg"]) for x in c],
                                           h("r", 8), np.array([x["r_inf"] for x in c], dtype=np.uint8), h("s", 4))
    assert list(got) == [x["status"] for x in c]


# ---- sizes and lengths against the restatement over the C oracle ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_and_lengths(gpu_ctx, oracle, n):
    be = R.CBackend()
    rng = np.random.default_rng(100 + n)
    pk, sig, _ = _byte_inputs(oracle, n, 200 + n)
    lens = [1, 47, 48, 63, 64, 65, 175, 176, 192, 300]               # 64 + len crosses 111/112 and 239/240
    msgs = [rng.integers(0, 256, size=lens[i % len(lens)], dtype=np.uint8).tobytes() for i in range(n)]
    assert list(gpu_ctx.ed25519_verify(pk, msgs, sig)) == R.verify_batch(pk, msgs, sig, be)
    pkx, pinf, rx, rinf, s = _generic_inputs(n, 300 + n)
    lens = [45, 46, 173, 174]                                         # 66 + len likewise
    msgs = [rng.integers(0, 256, size=lens[i % len(lens)], dtype=np.uint8).tobytes() for i in range(n)]
    assert list(gpu_ctx.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s)) == R.eddsa_verify_batch(pkx, pinf, msgs, rx, rinf, s, be)


def test_2_14_byte_form(gpu_ctx, oracle):
    n = 1 << 14
    pk, sig, both = _byte_inputs(oracle, n, 10)
    assert both >= 0.5                                                 # at least half of the lanes reach the point computation
    msgs = _msgs(n, 11)
    _plant(msgs)
    want = R.verify_batch(pk, msgs, sig, R.CBackend(16))
    got = gpu_ctx.ed25519_verify(pk, msgs, sig)
    assert list(got) == want
    assert {0, 1} <= set(want[9:])


def _signed_batch(gpu_ctx, n, seed, msgs):
    """(pk_xy, pk_inf, r_xy, r_inf, s): signatures of fec_eddsa_sign_ed25519 on random keys, the public keys from
    fec_batch_mul_fixed and fec_batch_to_affine."""
    sk = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    r_xy, r_inf, s, _ = gpu_ctx.eddsa_sign_ed25519(sk, msgs)
    a = np.array([S._key_scalar(S.to_bytes_be([int(v) for v in k]))[1] for k in sk], dtype=np.uint64)
    pk_xy, pk_inf = gpu_ctx.batch_to_affine(ED, gpu_ctx.batch_mul_fixed(ED, a, gpu_ctx.generator(ED)))
    return pk_xy, pk_inf, r_xy, r_inf, s


def test_2_14_generic_form(gpu_ctx):
    n, m = 1 << 14, 256
    msgs = _msgs(n, 21)
    _plant(msgs)
    pk_xy, pk_inf, r_xy, r_inf, s = _signed_batch(gpu_ctx, n, 20, msgs)
    # 256 constructed verifying signatures: the public key at infinity, R = to_affine(multiply(G, s))
    cs = np.random.default_rng(22).integers(1, 1 << 60, size=(m, 4), dtype=np.uint64)
    cr, cinf = gpu_ctx.batch_to_affine(ED, gpu_ctx.batch_mul_fixed(ED, cs, gpu_ctx.generator(ED)))
    assert not cinf.any()
    at = np.arange(100, 100 + 4 * m, 4)
    r_xy[at], r_inf[at], s[at], pk_inf[at] = cr, 0, cs, 1
    want = R.eddsa_verify_batch(pk_xy, pk_inf, msgs, r_xy, r_inf, s, R.CBackend(16))
    got = gpu_ctx.eddsa_verify_ed25519_msg(pk_xy, pk_inf, msgs, r_xy, r_inf, s)
    assert list(got) == want
    assert all(want[i] == 1 for i in at) and {0, 1} <= set(want[9:])


def test_2_16_composition(gpu_ctx, oracle):
    """Every element of the new calls equals a chain of already-pinned GPU calls: fec_batch_decompress, hashlib on the
    host, fec_eddsa_verify_ed25519 (and fec_batch_compress for the generic form's prefix)."""
    n = 1 << 16
    pk, sig, _ = _byte_inputs(oracle, n, 30)
    msgs = _msgs(n, 31, 1, 100)
    _plant(msgs)
    got = gpu_ctx.ed25519_verify(pk, msgs, sig)
    two = np.full((n, 1), 2, np.uint8)
    a_xy, _, a_ok = gpu_ctx.batch_decompress(ED, np.concatenate([two, pk], 1))
    r_xy, _, r_ok = gpu_ctx.batch_decompress(ED, np.concatenate([two, sig[:, :32]], 1))
    s = np.array([R.from_bytes_be(sig[i, 32:]) for i in range(n)], dtype=np.uint64)
    k = np.array([R.from_bytes_be(hashlib.sha512(sig[i, :32].tobytes() + pk[i].tobytes() + msgs[i]).digest()[:32]) for i in range(n)], dtype=np.uint64)
    want = gpu_ctx.eddsa_verify_ed25519(r_xy, None, a_xy, None, s, k)
    want[(a_ok == 0) | (r_ok == 0)] = 0
    for i, m in enumerate(msgs):
        c = R.message_case(m)
        if c is not None:
            want[i] = c
    assert np.array_equal(got, want)
    pkx, pinf, rx, rinf, gs = _generic_inputs(n, 32)
    got = gpu_ctx.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, gs)
    rb, pb = gpu_ctx.batch_compress(ED, rx, np.zeros(n, np.uint8)), gpu_ctx.batch_compress(ED, pkx, pinf)
    k = np.array([R.from_bytes_be(hashlib.sha512(rb[i].tobytes() + pb[i].tobytes() + msgs[i]).digest()[:32]) for i in range(n)], dtype=np.uint64)
    want = gpu_ctx.eddsa_verify_ed25519(rx, rinf, pkx, pinf, gs, k)
    for i, m in enumerate(msgs):
        c = R.message_case(m)
        if c is not None:
            want[i] = c
    assert np.array_equal(got, want)


# ---- forms and contexts ----

def test_chunked_host_call_equals_dev_on_caller_stream(gpu_ctx, oracle):
    import torch
    n = 5000
    msgs = _msgs(n, 41, 0, 700)
    _plant(msgs)
    pk, sig, _ = _byte_inputs(oracle, n, 40)
    pkx, pinf, rx, rinf, s = _generic_inputs(n, 42)
    want_b = gpu_ctx.ed25519_verify(pk, msgs, sig)
    want_g = gpu_ctx.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s)
    gpu_ctx.set_chunk(333)
    try:
        got_b = gpu_ctx.ed25519_verify(pk, msgs, sig)
        got_g = gpu_ctx.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_g, want_g)
    assert {0, 1} <= set(want_b) and 0 in set(want_g)
    tb, to, total = _dev_msgs(torch, msgs)
    tpk, tsig, tpkx, tpinf, trx, trinf, ts = (_dev(torch, a) for a in (pk, sig, pkx, pinf, rx, rinf, s))
    st_b = torch.full((n,), 9, dtype=torch.uint8, device=tb.device)
    st_g = torch.full((n,), 9, dtype=torch.uint8, device=tb.device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.ed25519_verify_dev(tpk.data_ptr(), tb.data_ptr(), to.data_ptr(), total, tsig.data_ptr(), st_b.data_ptr(), n, stream.cuda_stream)
    gpu_ctx.eddsa_verify_ed25519_msg_dev(tpkx.data_ptr(), tpinf.data_ptr(), tb.data_ptr(), to.data_ptr(), total, trx.data_ptr(),
                                         trinf.data_ptr(), ts.data_ptr(), st_g.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(st_b.cpu().numpy(), want_b) and np.array_equal(st_g.cpu().numpy(), want_g)


def test_multi_ctx_equals_single(gpu_ctx, oracle):
    import forge_ec_amd as F
    n = 3001
    msgs = _msgs(n, 51, 0, 300)
    _plant(msgs)
    pk, sig, _ = _byte_inputs(oracle, n, 50)
    pkx, pinf, rx, rinf, s = _generic_inputs(n, 52)
    with F.Context(devices=[0, 0]) as multi:
        assert np.array_equal(multi.ed25519_verify(pk, msgs, sig), gpu_ctx.ed25519_verify(pk, msgs, sig))
        assert np.array_equal(multi.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s),
                              gpu_ctx.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s))


def test_prefix_table_on_and_off(oracle):
    import forge_ec_amd as F
    n = 1 << 16
    msgs = _msgs(n, 61, 1, 100)
    pk, sig, _ = _byte_inputs(oracle, n, 60)
    pkx, pinf, rx, rinf, s = _generic_inputs(n, 62)
    with F.Context(0) as off, F.Context(0) as on:
        off.set_fixed_prefix_bits(0)
        on.set_fixed_prefix_bits(12)
        on.build_fixed_prefix(ED)
        a = on.ed25519_verify(pk, msgs, sig)
        assert np.array_equal(a, off.ed25519_verify(pk, msgs, sig)) and {0, 1} <= set(a)
        assert np.array_equal(on.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s), off.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s))


def test_dev_unaligned_message_base(gpu_ctx, oracle):
    import torch
    n = 1000
    msgs = _msgs(n, 71, 0, 300)
    _plant(msgs)
    pk, sig, _ = _byte_inputs(oracle, n, 70)
    pkx, pinf, rx, rinf, s = _generic_inputs(n, 72)
    want_b = gpu_ctx.ed25519_verify(pk, msgs, sig)
    want_g = gpu_ctx.eddsa_verify_ed25519_msg(pkx, pinf, msgs, rx, rinf, s)
    tb, to, total = _dev_msgs(torch, msgs)
    tpk, tsig, tpkx, tpinf, trx, trinf, ts = (_dev(torch, a) for a in (pk, sig, pkx, pinf, rx, rinf, s))
    for shift in (1, 2, 3):
        big = torch.zeros(total + 16, dtype=torch.uint8, device=tb.device)
        big[shift:shift + total] = tb[:total]
        st_b = torch.full((n,), 9, dtype=torch.uint8, device=tb.device)
        st_g = torch.full((n,), 9, dtype=torch.uint8, device=tb.device)
        gpu_ctx.ed25519_verify_dev(tpk.data_ptr(), big.data_ptr() + shift, to.data_ptr(), total, tsig.data_ptr(), st_b.data_ptr(), n)
        gpu_ctx.eddsa_verify_ed25519_msg_dev(tpkx.data_ptr(), tpinf.data_ptr(), big.data_ptr() + shift, to.data_ptr(), total,
                                             trx.data_ptr(), trinf.data_ptr(), ts.data_ptr(), st_g.data_ptr(), n)
        torch.cuda.synchronize()
        assert np.array_equal(st_b.cpu().numpy(), want_b) and np.array_equal(st_g.cpu().numpy(), want_g), shift


# ---- argument errors ----

def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib = L.lib()
    h = gpu_ctx._h
    n = 8
    rng = np.random.default_rng(80)
    pk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sig = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    xy = rng.integers(0, 1 << 63, size=(n, 8), dtype=np.uint64)
    sc = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    msgs = b"x" * 40
    good = np.arange(0, 41, 5, dtype=np.uint64)
    pp, sp, tp, xp, cp = pk.ctypes.data, sig.ctypes.data, st.ctypes.data, xy.ctypes.data, sc.ctypes.data
    byte = lambda ctx=h, p=pp, m=msgs, o=good, ln=40, s=sp, t=tp: lib.fec_ed25519_verify(ctx, p, m, o.ctypes.data if o is not None else None, ln, s, t, n)
    gen = lambda ctx=h, p=xp, m=msgs, o=good, ln=40, r=xp, s=cp, t=tp: lib.fec_eddsa_verify_ed25519_msg(
        ctx, p, None, m, o.ctypes.data if o is not None else None, ln, r, None, s, t, n)
    bad, nz = good.copy(), good.copy()
    bad[3], bad[4] = 20, 10                                              # not monotonic
    nz[0] = 1                                                            # off[0] != 0
    for call in (byte, gen):
        assert call() == 0
        assert call(o=bad) == -1 and call(o=nz) == -1 and call(ln=41) == -1 and call(o=None) == -1
        assert call(p=None) == -1 and call(m=None) == -1 and call(ctx=None) == -1 and call(t=None) == -1
    assert byte(s=None) == -1 and gen(r=None) == -1 and gen(s=None) == -1
    dev = torch.device("cuda:0")
    tpk, tsig, txy, tsc = (_dev(torch, a) for a in (pk, sig, xy, sc))
    tm = torch.zeros(64, dtype=torch.uint8, device=dev)
    offs = np.array([0, 5, 10, 50, 45, 3, 1 << 62, 2, 7], dtype=np.uint64)   # elements 2, 3, 5 (, 6) out of range
    to = _dev(torch, offs)
    tb = torch.zeros(n, dtype=torch.uint8, device=dev)
    tg = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.ed25519_verify_dev(tpk.data_ptr(), tm.data_ptr(), to.data_ptr(), 40, tsig.data_ptr(), tb.data_ptr(), n)
    gpu_ctx.eddsa_verify_ed25519_msg_dev(txy.data_ptr(), None, tm.data_ptr(), to.data_ptr(), 40, txy.data_ptr(), None, tsc.data_ptr(), tg.data_ptr(), n)
    torch.cuda.synchronize()
    want_bad = [not (offs[i] <= offs[i + 1] <= 40) for i in range(n)]
    assert list(tb.cpu().numpy() == 4) == want_bad and list(tg.cpu().numpy() == 4) == want_bad
    d = (tpk.data_ptr(), tm.data_ptr(), to.data_ptr(), 40, tsig.data_ptr(), tb.data_ptr(), n, None)
    assert lib.fec_ed25519_verify_dev(h, tpk.data_ptr() + 8, *d[1:]) == -1                     # misaligned keys
    assert lib.fec_ed25519_verify_dev(h, d[0], d[1], d[2], 40, tsig.data_ptr() + 8, *d[5:]) == -1
    assert lib.fec_ed25519_verify_dev(h, d[0], d[1], to.data_ptr() + 4, *d[3:]) == -1          # misaligned offsets
    assert lib.fec_ed25519_verify_dev(h, d[0], d[1], None, *d[3:]) == -1
    g = (txy.data_ptr(), None, tm.data_ptr(), to.data_ptr(), 40, txy.data_ptr(), None, tsc.data_ptr(), tg.data_ptr(), n, None)
    assert lib.fec_eddsa_verify_ed25519_msg_dev(h, g[0] + 8, *g[1:]) == -1
    assert lib.fec_eddsa_verify_ed25519_msg_dev(h, *g[:7], tsc.data_ptr() + 8, *g[8:]) == -1
    assert lib.fec_eddsa_verify_ed25519_msg_dev(h, *g[:7], None, *g[8:]) == -1
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_ed25519_verify_dev(multi._h, *d) == -5
        assert lib.fec_eddsa_verify_ed25519_msg_dev(multi._h, *g) == -5
    assert gpu_ctx.ed25519_verify(pk, [b"a"] * n, sig).shape == (n,)      # the ctx is still usable
