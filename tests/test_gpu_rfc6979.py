"""
GPU tests of fec_rfc6979_k / fec_rfc6979_k_dev / fec_debug_rfc6979_k (kernels_rfc6979.hip) against the hashlib / hmac
restatement of tests/rfc6979_ref.py: the fixture (which holds the reference's own recorded nonces), both curves; n on both
sides of a wavefront and of a workgroup with mixed message lengths, the _dev form at the unaligned message starts of
tests/test_gpu_sha256.py; a planted bad range; and the retry loop under a lowered comparison constant, the only place
where lanes of one wavefront leave it after different numbers of rounds.
"""
import json
import os

import numpy as np
import pytest

import rfc6979_ref as R
from test_rfc6979_host import assert_retry_mix, retry_pairs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "rfc6979_vectors.json")))


def _batch(n, seed):
    """n arbitrary 256-bit keys (generate_k has no key check) and messages of 0..200 bytes, the edge lengths among them."""
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    edge = (0, 55, 56, 63, 64, 65, 119, 120)
    lens = [edge[i % 8] if i % 3 == 0 else int(rng.integers(0, 201)) for i in range(n)]
    return sk, [rng.integers(0, 256, size=L_, dtype=np.uint8).tobytes() for L_ in lens]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def _offsets(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return off


def test_recorded_reference_nonces(gpu_ctx):
    rec = FIXTURE["recorded"]
    k, st = gpu_ctx.rfc6979_k(0, [c["sk"] for c in rec], [bytes.fromhex(c["msg"]) for c in rec])
    assert k.tolist() == [c["k"] for c in rec] and not st.any()


@pytest.mark.parametrize("curve", [0, 1])
def test_fixture(gpu_ctx, curve):
    cases = [c for c in FIXTURE["cases"] if c["curve"] == curve]
    k, st = gpu_ctx.rfc6979_k(curve, [c["sk"] for c in cases], [bytes.fromhex(c["msg"]) for c in cases])
    assert not st.any()
    assert k.tolist() == [c["k"] for c in cases]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_mixed_lengths_host_and_dev_unaligned(gpu_ctx, n):
    import torch
    curve = n & 1
    sk, msgs = _batch(n, 100 + n)
    want, _ = R.nonces(curve, sk, msgs)
    k, st = gpu_ctx.rfc6979_k(curve, sk, msgs)
    assert not st.any() and np.array_equal(k, want)
    off = _offsets(msgs)
    total = int(off[-1])
    d_sk, d_off = _dev(torch, sk), _dev(torch, off)
    body = torch.from_numpy(np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()).to(d_sk.device)
    for shift in (1, 2, 3):
        big = torch.zeros(total + 16, dtype=torch.uint8, device=d_sk.device)
        big[shift:shift + total] = body[:total]
        d_k = torch.full((n * 32,), 7, dtype=torch.uint8, device=d_sk.device)
        d_st = torch.full((n,), 9, dtype=torch.uint8, device=d_sk.device)
        gpu_ctx.rfc6979_k_dev(curve, d_sk.data_ptr(), big.data_ptr() + shift, d_off.data_ptr(), total, d_k.data_ptr(), d_st.data_ptr(), n)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any()
        assert np.array_equal(d_k.cpu().numpy().view(np.uint64).reshape(n, 4), want), shift


@pytest.mark.parametrize("curve", [0, 1])
def test_chunked_and_multi_device(gpu_ctx, curve):
    """Chunks of 64 over n = 131: elements 63 and 64 are empty, so one chunk's rebased offsets end and the next one's
    start on an empty range; the other lengths cycle through the padding edges of SHA-256."""
    import forge_ec_amd as F
    n = 131
    rng = np.random.default_rng(300 + curve)
    sk = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    msgs = [rng.integers(0, 256, size=0 if i in (63, 64) else (0, 1, 55, 56, 64, 119)[i % 6], dtype=np.uint8).tobytes() for i in range(n)]
    want, _ = R.nonces(curve, sk, msgs)
    gpu_ctx.set_chunk(64)
    try:
        k, st = gpu_ctx.rfc6979_k(curve, sk, msgs)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    assert not st.any() and np.array_equal(k, want)
    with F.Context(devices=[0, 0]) as multi:
        multi.set_chunk(64)
        k, st = multi.rfc6979_k(curve, sk, msgs)
    assert not st.any() and np.array_equal(k, want)


def test_dev_form_bad_range_planted(gpu_ctx):
    import torch
    n, bad = 70, 37
    sk, msgs = _batch(n, 5)
    off = _offsets(msgs)
    total = int(off[-1])
    want, _ = R.nonces(0, sk, msgs)
    planted = off.copy()
    planted[bad + 1] = planted[bad] - 1 if planted[bad] else total + 1     # element `bad` and its successor lose their range
    ok = [planted[i] <= planted[i + 1] <= total for i in range(n)]
    assert not ok[bad] and sum(ok) >= n - 2
    d_sk, d_off = _dev(torch, sk), _dev(torch, planted)
    body = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).to(d_sk.device)
    d_k = torch.full((n * 32,), 7, dtype=torch.uint8, device=d_sk.device)
    d_st = torch.full((n,), 9, dtype=torch.uint8, device=d_sk.device)
    gpu_ctx.rfc6979_k_dev(0, d_sk.data_ptr(), body.data_ptr(), d_off.data_ptr(), total, d_k.data_ptr(), d_st.data_ptr(), n)
    torch.cuda.synchronize()
    st, k = d_st.cpu().numpy(), d_k.cpu().numpy().view(np.uint64).reshape(n, 4)
    for i in range(n):
        if not ok[i]:
            assert st[i] == 4 and not k[i].any(), i
        elif planted[i] == off[i] and planted[i + 1] == off[i + 1]:
            assert st[i] == 0 and np.array_equal(k[i], want[i]), i
        else:                                   # the successor of a shrunken element reads another, valid range
            m = b"".join(msgs)[int(planted[i]):int(planted[i + 1])]
            assert st[i] == 0 and k[i].tolist() == R.E._limbs(R.generate_k(sk[i].tolist(), m, R.ORDER[0])[0]), i


@pytest.mark.parametrize("curve", [0, 1])
def test_retry_loop_under_a_lowered_constant(gpu_ctx, curve):
    """n = 256 = four wavefronts; under 2^255 every second candidate fails, so the lanes of each wavefront leave the
    loop after 0..11 retries."""
    order = 1 << 255
    pairs = retry_pairs()
    want = [R.generate_k(sk, msg, order) for sk, msg in pairs]
    assert_retry_mix([r for _, r in want])
    k, st = gpu_ctx.debug_rfc6979_k(curve, R.E._limbs(order), [sk for sk, _ in pairs], [m for _, m in pairs])
    assert not st.any()
    assert k.tolist() == [R.E._limbs(v) for v, _ in want]


def test_debug_constant_below_2_to_the_254_is_refused(gpu_ctx):
    import forge_ec_amd as F
    sk, msgs = _batch(4, 9)
    for order in ((1 << 254) - 1, 1, 0):
        with pytest.raises(F.FecError) as e:
            gpu_ctx.debug_rfc6979_k(0, R.E._limbs(order), sk, msgs)
        assert e.value.status == -1
    k, st = gpu_ctx.debug_rfc6979_k(0, R.E._limbs(1 << 254), sk, msgs)
    assert not st.any() and np.array_equal(k, R.nonces(0, sk, msgs, order=1 << 254)[0])


def test_ed25519_is_unsupported(gpu_ctx):
    import forge_ec_amd as F
    sk, msgs = _batch(2, 3)
    with pytest.raises(F.FecError) as e:
        gpu_ctx.rfc6979_k(2, sk, msgs)
    assert e.value.status == -5
