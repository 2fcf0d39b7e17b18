"""
GPU tests of fec_schnorr_sign_msg / fec_schnorr_sign_msg_dev (kernels_schnorr.hip: k_rfc6979, one fixed-base launch over
the 2n scalars k and sk, k_schnorr_sign_finish) against the restatement of tests/schnorr_sign_ref.py: the fixture byte for
byte with its statuses; on each curve (their fixed-base kernels differ) n on both sides of a wavefront -- an odd n puts the k half and the sk half of the 2n-scalar launch
across a wavefront edge, n = 1 is two scalars -- host and _dev with the message buffer at byte offsets 0..3; n = 200 in
chunks of 64 with "test message" planted; the fused call against its own parts; a planted bad range; Ed25519 unsupported.
"""
import json
import os

import numpy as np
import pytest

import schnorr_sign_ref as S
from test_schnorr_sign_model import planted_batch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = S.load_fixture()
_WANT = {}


def _batch(n, seed):
    """n arbitrary 256-bit keys (Schnorr::sign has no key check) and messages of 0..200 bytes, the edge lengths of the
    66-byte prefix among them; every 16th message is b"test message"."""
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    edge = (0, 53, 54, 61, 62, 63, 117, 118, 126)
    lens = [edge[i % 9] if i % 3 == 0 else int(rng.integers(0, 201)) for i in range(n)]
    msgs = [rng.integers(0, 256, size=L_, dtype=np.uint8).tobytes() for L_ in lens]
    return sk, [b"test message" if i % 16 == 5 else m for i, m in enumerate(msgs)]


def _want(curve, n):
    """The reference of the seeded batch of n elements on `curve`, computed once for the host and the _dev test."""
    if (curve, n) not in _WANT:
        sk, msgs = _batch(n, 300 + 1000 * curve + n)
        _WANT[curve, n] = (sk, msgs, S.sign_many(curve, sk, msgs))
    return _WANT[curve, n]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def _offsets(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return off


def _assert_equal(got, want, where=""):
    r, rinf, s, sb, st = got
    assert st.tolist() == want["status"].tolist(), where
    assert np.array_equal(r, want["r_xy"]) and rinf.tolist() == want["r_inf"].tolist(), where
    assert np.array_equal(s, want["s"]), where
    assert np.array_equal(sb, want["sig_bytes"]), where


@pytest.mark.parametrize("curve", [0, 1])
def test_fixture(gpu_ctx, curve):
    cases = [c for c in FIXTURE["sign"] if c["curve"] == curve]
    r, rinf, s, sb, st = gpu_ctx.schnorr_sign_msg(curve, [c["sk"] for c in cases], [bytes.fromhex(c["msg"]) for c in cases])
    assert st.tolist() == [c["status"] for c in cases]
    assert r.tolist() == [c["r_xy"] for c in cases] and rinf.tolist() == [c["r_inf"] for c in cases]
    assert s.tolist() == [c["s"] for c in cases]
    assert [bytes(x).hex() for x in sb] == [c["sig_bytes"] for c in cases]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("curve", [0, 1])
def test_host_form(gpu_ctx, curve, n):
    sk, msgs, want = _want(curve, n)
    _assert_equal(gpu_ctx.schnorr_sign_msg(curve, sk, msgs), want)
    r, rinf, s, sb, st = gpu_ctx.schnorr_sign_msg(curve, sk, msgs, with_bytes=False)       # sig_bytes = NULL
    assert sb is None and np.array_equal(s, want["s"]) and np.array_equal(r, want["r_xy"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("curve", [0, 1])
def test_dev_form_message_buffer_at_offsets_0_to_3(gpu_ctx, curve, n):
    import torch
    sk, msgs, want = _want(curve, n)
    off = _offsets(msgs)
    total = int(off[-1])
    d_sk, d_off = _dev(torch, sk), _dev(torch, off)
    body = torch.from_numpy(np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()).to(d_sk.device)
    for shift in (0, 1, 2, 3):
        big = torch.zeros(total + 16, dtype=torch.uint8, device=d_sk.device)
        big[shift:shift + total] = body[:total]
        fill = lambda m: torch.full((m,), 7, dtype=torch.uint8, device=d_sk.device)
        d_r, d_rinf, d_s, d_sb, d_st = fill(n * 64), fill(n), fill(n * 32), fill(n * 64), fill(n)
        gpu_ctx.schnorr_sign_msg_dev(curve, d_sk.data_ptr(), big.data_ptr() + shift, d_off.data_ptr(), total, d_r.data_ptr(),
                                     d_rinf.data_ptr(), d_s.data_ptr(), d_sb.data_ptr(), d_st.data_ptr(), n)
        torch.cuda.synchronize()
        got = (d_r.cpu().numpy().view(np.uint64).reshape(n, 8), d_rinf.cpu().numpy(), d_s.cpu().numpy().view(np.uint64).reshape(n, 4),
               d_sb.cpu().numpy().reshape(n, 64), d_st.cpu().numpy())
        _assert_equal(got, want, shift)


@pytest.mark.parametrize("curve", [0, 1])
def test_chunked_with_planted_test_messages(gpu_ctx, curve):
    """n = 200 in chunks of 64: chunk edges and rebased offsets; no position may be skipped."""
    sk, msgs = planted_batch(200, 12 + curve)
    want = S.sign_many(curve, sk, msgs)
    gpu_ctx.set_chunk(64)
    try:
        got = gpu_ctx.schnorr_sign_msg(curve, sk, msgs)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    st = got[4]
    assert st.shape == (200,) and set(st.tolist()) <= {0, 1}
    assert (st == 0).sum() >= 180 and (st == 1).sum() >= 4
    _assert_equal(got, want)


@pytest.mark.parametrize("curve", [0, 1])
def test_fused_call_equals_its_parts(gpu_ctx, curve):
    """k = rfc6979_k, R and P = to_affine(batch_mul_fixed(.)), e = schnorr_challenge: then the signer's R is that R and its
    s the oracle's k + e * sk."""
    n = 65
    rng = np.random.default_rng(77 + curve)
    sk = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sk[3] = 0                                                                             # P is the identity, s = k
    msgs = [rng.integers(0, 256, size=int(rng.integers(0, 150)), dtype=np.uint8).tobytes() for _ in range(n)]
    k, kst = gpu_ctx.rfc6979_k(curve, sk, msgs)
    assert not kst.any()
    g = gpu_ctx.generator(curve)
    r_xy, r_inf = gpu_ctx.batch_to_affine(curve, gpu_ctx.batch_mul_fixed(curve, k, g))
    p_xy, p_inf = gpu_ctx.batch_to_affine(curve, gpu_ctx.batch_mul_fixed(curve, sk, g))
    assert p_inf[3] == 1 and p_inf.sum() == 1
    e = gpu_ctx.schnorr_challenge(curve, r_xy, r_inf, p_xy, p_inf, msgs)
    be = S.CBackend()
    r, rinf, s, sb, st = gpu_ctx.schnorr_sign_msg(curve, sk, msgs)
    assert not st.any() and np.array_equal(r, r_xy) and np.array_equal(rinf, r_inf)
    for i in range(n):
        assert s[i].tolist() == be.sc_add(curve, k[i].tolist(), be.sc_mul(curve, e[i].tolist(), sk[i].tolist())), i
    assert np.array_equal(s[3], k[3])


def test_dev_form_bad_range_planted(gpu_ctx):
    import torch
    n, bad, curve = 70, 37, 0
    sk, msgs = _batch(n, 5)
    off = _offsets(msgs)
    total = int(off[-1])
    want = S.sign_many(curve, sk, msgs)
    planted = off.copy()
    planted[bad + 1] = total + 1                     # element `bad` ends past the buffer, its successor starts there
    d_sk, d_off = _dev(torch, sk), _dev(torch, planted)
    body = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).to(d_sk.device)
    fill = lambda m: torch.full((m,), 7, dtype=torch.uint8, device=d_sk.device)
    d_r, d_rinf, d_s, d_sb, d_st = fill(n * 64), fill(n), fill(n * 32), fill(n * 64), fill(n)
    gpu_ctx.schnorr_sign_msg_dev(curve, d_sk.data_ptr(), body.data_ptr(), d_off.data_ptr(), total, d_r.data_ptr(), d_rinf.data_ptr(),
                                 d_s.data_ptr(), d_sb.data_ptr(), d_st.data_ptr(), n)
    torch.cuda.synchronize()
    r, rinf, s = d_r.cpu().numpy().view(np.uint64).reshape(n, 8), d_rinf.cpu().numpy(), d_s.cpu().numpy().view(np.uint64).reshape(n, 4)
    sb, st = d_sb.cpu().numpy().reshape(n, 64), d_st.cpu().numpy()
    for i in range(n):
        if i in (bad, bad + 1):                      # off[bad] <= total + 1 fails the range test; so does total + 1 <= off[bad + 2]
            assert st[i] == 4 and not r[i].any() and rinf[i] == 0 and not s[i].any() and not sb[i].any(), i
        else:
            assert st[i] == want["status"][i] and np.array_equal(r[i], want["r_xy"][i]) and np.array_equal(s[i], want["s"][i]), i
            assert np.array_equal(sb[i], want["sig_bytes"][i]) and rinf[i] == want["r_inf"][i], i


def test_ed25519_is_unsupported(gpu_ctx):
    import forge_ec_amd as F
    sk, msgs = _batch(2, 3)
    with pytest.raises(F.FecError) as e:
        gpu_ctx.schnorr_sign_msg(2, sk, msgs)
    assert e.value.status == -5
