"""
GPU tests of fec_ecdsa_sign_msg / fec_ecdsa_sign_msg_dev -- Ecdsa::<C, Sha256>::sign from the message: the fixture byte
for byte with its status; 200 elements in chunks of 64 (chunk edges, rebased message offsets) against
rfc6979_ref.sign_msg over the threaded C oracle; the fused call against its own parts on the same context; a planted bad
range in the _dev form; Ed25519.
(Status 2 by digest -- h not below the order constant -- needs a SHA-256 whose top word is all ones; no such message is
known and none is searched for.  That leg is k_ecdsa_sign_finish's, unchanged here: tests/test_gpu_ecdsa_sign.py covers
it with crafted digests.)
"""
import json
import os

import numpy as np
import pytest

import rfc6979_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "rfc6979_vectors.json")))
ONE = [1, 0, 0, 0]


def _batch(curve, n, seed):
    """Keys: every fifth zero (status 1 on both curves), every seventh at or above the order constant (status 1 on
    secp256k1 only), the rest random below it; messages of 0..150 bytes."""
    rng = np.random.default_rng(seed)
    nv = R.ORDER[curve]
    sk = []
    for i in range(n):
        v = int.from_bytes(rng.bytes(32), "little")
        sk.append(R.E._limbs(0 if i % 5 == 0 else (nv + v % ((1 << 256) - nv) if i % 7 == 3 else 1 + v % (nv - 1))))
    lens = rng.integers(0, 151, size=n)
    return np.array(sk, dtype=np.uint64), [rng.integers(0, 256, size=int(L_), dtype=np.uint8).tobytes() for L_ in lens]


@pytest.fixture(scope="module")
def reference(oracle):
    """(sk, msgs, r, s, status) per curve from sign_msg over the C oracle, computed once."""
    out = {}
    for curve in (0, 1):
        sk, msgs = _batch(curve, 200, 40 + curve)
        r, s, st, _ = R.sign_msg(oracle, curve, sk, msgs)
        out[curve] = (sk, msgs, r, s, st)
    return out


@pytest.mark.parametrize("curve", [0, 1])
def test_fixture(gpu_ctx, curve):
    cases = [c for c in FIXTURE["cases"] if c["curve"] == curve]
    r, s, st = gpu_ctx.ecdsa_sign_msg(curve, [c["sk"] for c in cases], [bytes.fromhex(c["msg"]) for c in cases])
    assert st.tolist() == [c["status"] for c in cases]
    assert r.tolist() == [c["r"] for c in cases] and s.tolist() == [c["s"] for c in cases]


@pytest.mark.parametrize("curve", [0, 1])
def test_chunked_against_the_oracle(gpu_ctx, reference, curve):
    sk, msgs, wr, ws, wst = reference[curve]
    n = len(msgs)
    assert (wst == 0).sum() * 4 >= n and (wst == 1).sum() * 10 >= n, np.bincount(wst)
    gpu_ctx.set_chunk(64)
    try:
        r, s, st = gpu_ctx.ecdsa_sign_msg(curve, sk, msgs)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    assert st.tolist() == wst.tolist()
    assert np.array_equal(r, wr) and np.array_equal(s, ws)


@pytest.mark.parametrize("curve", [0, 1])
def test_fused_call_equals_its_parts(gpu_ctx, reference, curve):
    sk, msgs, _, _, wst = reference[curve]
    r, s, st = gpu_ctx.ecdsa_sign_msg(curve, sk, msgs)
    k, kst = gpu_ctx.rfc6979_k(curve, sk, msgs)
    assert not kst.any()
    r2, s2, st2 = gpu_ctx.ecdsa_sign(curve, sk, gpu_ctx.sha256(msgs), k)
    checked = wst != 1                        # where the key passes the check; a rejected key is (1, 1), status 1 in both
    assert checked.sum() * 2 >= len(msgs)
    assert np.array_equal(st, st2) and np.array_equal(r, r2) and np.array_equal(s, s2)
    assert st[~checked].tolist() == [1] * int((~checked).sum())


@pytest.mark.parametrize("curve", [0, 1])
def test_dev_form_bad_range_planted(gpu_ctx, reference, curve):
    import torch
    n, bad = 70, 41
    sk, msgs, wr, ws, wst = (x[:n] for x in reference[curve])
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    total = int(off[-1])
    planted = off.copy()
    planted[bad + 1] = total + 1                 # element `bad` ends, and its successor starts, past the buffer
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_sk, d_off, body = up(sk), up(planted), up(np.frombuffer(b"".join(msgs), dtype=np.uint8))
    d_sig = torch.full((n * 64,), 7, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    gpu_ctx.ecdsa_sign_msg_dev(curve, d_sk.data_ptr(), body.data_ptr(), d_off.data_ptr(), total, d_sig.data_ptr(), d_st.data_ptr(), n)
    torch.cuda.synchronize()
    gpu_ctx.check()
    st, sig = d_st.cpu().numpy(), d_sig.cpu().numpy().view(np.uint64).reshape(n, 8)
    for i in range(n):
        if i in (bad, bad + 1):
            assert st[i] == 4 and not sig[i].any(), i
        else:
            assert st[i] == wst[i] and sig[i, :4].tolist() == wr[i].tolist() and sig[i, 4:].tolist() == ws[i].tolist(), i


def test_ed25519_is_unsupported(gpu_ctx):
    import forge_ec_amd as F
    with pytest.raises(F.FecError) as e:
        gpu_ctx.ecdsa_sign_msg(2, [ONE], [b"abc"])
    assert e.value.status == -5
