"""
GPU tests of canonical-mode X25519 (include/fecgpu_canon.h: fec_canon_x25519, fec_canon_x25519_base and their *_dev forms)
against the fixture tests/golden/canon_x25519_vectors.json, which the model tests/canon_x25519_ref.py wrote and
tests/test_canon_x25519_model.py pins by the vectors of RFC 7748 and by the openssl program.  X25519 is a function: every
comparison is byte-exact, status included.  Also: each low-order and non-canonical u alone among ordinary elements, the
RFC's 1000-step chain as 1000 calls, Diffie-Hellman symmetry, the ladder at u = 9 against the comb-and-map public key,
chunks, shard workers, refused arguments.
"""
import json
import os
import random

import numpy as np
import pytest

import canon_x25519_ref as X

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_x25519_vectors.json")))
CASES = FIXTURE["cases"]
COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]
ARG, UNSUPPORTED = -1, -5
AMONG = 64 * 3 + 5
LANES = (0, 31, 32, 63, AMONG - 1)


def _dev(ctx):
    from forge_ec_amd.canon import CanonX25519
    return CanonX25519(ctx)


def _rows(hexes):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), dtype=np.uint8).reshape(len(hexes), 32).copy()


def _batch(pick):
    return (_rows([c["k"] for c in pick]), _rows([c["u"] for c in pick]), _rows([c["out"] for c in pick]),
            np.array([c["status"] for c in pick], dtype=np.uint8))


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _x25519_dev(ctx, k, u):
    import torch
    n = k.shape[0]
    tk, tu = _to_dev(k), _to_dev(u)
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    _dev(ctx).x25519_dev(tk.data_ptr(), tu.data_ptr(), out.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _base_dev(ctx, k):
    import torch
    n = k.shape[0]
    tk = _to_dev(k)
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    _dev(ctx).x25519_base_dev(tk.data_ptr(), out.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _rand_rows(rng, n):
    return np.frombuffer(bytes(rng.randrange(256) for _ in range(32 * n)), dtype=np.uint8).reshape(n, 32).copy()


def test_every_fixture_case_host_and_dev_forms(gpu_ctx):
    k, u, want, wst = _batch(CASES)
    assert (wst == X.ZERO_SHARED).sum() == 16
    for out, st in (_dev(gpu_ctx).x25519(k, u), _x25519_dev(gpu_ctx, k, u)):
        bad = [i for i in range(len(CASES)) if st[i] != wst[i] or bytes(out[i]) != bytes(want[i])]
        assert not bad, [(i, CASES[i]["name"]) for i in bad]
    # the public keys of the fixture's scalars: the cases whose u is 9
    nine = [c for c in CASES if c["u"] == X.BASE_U.hex()]
    assert len(nine) >= 11
    kk, _, pk, _ = _batch(nine)
    assert np.array_equal(_dev(gpu_ctx).x25519_base(kk), pk) and np.array_equal(_base_dev(gpu_ctx, kk), pk)
    gpu_ctx.check()


@pytest.mark.parametrize("n", COUNTS)
def test_element_counts(gpu_ctx, n):
    """n cases, cycling from inside the low-order class so that n = 1 is not an ordinary case; host and *_dev forms; the
    public keys of the same scalars by both algorithms"""
    start = 3
    pick = [CASES[(start + i) % len(CASES)] for i in range(n)]
    assert pick[0]["status"] == X.ZERO_SHARED
    k, u, want, wst = _batch(pick)
    for out, st in (_dev(gpu_ctx).x25519(k, u), _x25519_dev(gpu_ctx, k, u)):
        assert np.array_equal(st, wst) and np.array_equal(out, want)
    nine = np.tile(np.frombuffer(X.BASE_U, dtype=np.uint8), (n, 1))
    pk = _dev(gpu_ctx).x25519_base(k)
    by_ladder, st = _dev(gpu_ctx).x25519(k, nine)
    assert np.array_equal(pk, by_ladder) and not st.any() and np.array_equal(_base_dev(gpu_ctx, k), pk)
    assert bytes(pk[0]) == X.x25519_base(bytes(k[0]))
    gpu_ctx.check()


def test_rare_inputs_alone_among_ordinary_ones(gpu_ctx):
    """each low-order and each non-canonical u alone at lanes 0, 31, 32, 63 and at the last of 197 ordinary elements, whose
    results must be right as well"""
    ordinary = [c for c in CASES if c["class"] == "random"][:AMONG]
    rare = [c for c in CASES if c["class"] in ("low-order", "non-canonical")]
    assert len(ordinary) == AMONG and len(rare) == 14 + 19
    k0, u0, want0, st0 = _batch(ordinary)
    dev = _dev(gpu_ctx)
    for j, c in enumerate(rare):
        ck, cu, cw, cs = _batch([c])
        for lane in LANES:
            k, u, want, wst = k0.copy(), u0.copy(), want0.copy(), st0.copy()
            k[lane], u[lane], want[lane], wst[lane] = ck[0], cu[0], cw[0], cs[0]
            out, st = dev.x25519(k, u) if (j + lane) % 2 else _x25519_dev(gpu_ctx, k, u)
            assert np.array_equal(st, wst) and np.array_equal(out, want), (c["name"], lane)
    gpu_ctx.check()


def test_published_vectors_and_the_chain(gpu_ctx):
    """RFC 7748 section 5.2 and 6.1, and the chain from k = u = 9 as 1000 calls of n = 1 on the *_dev form (three buffers
    taking turns: nothing is copied between the calls)"""
    import torch
    dev = _dev(gpu_ctx)
    for name, v in X.PUBLISHED.items():
        out, st = dev.x25519(bytes.fromhex(v["k"]), bytes.fromhex(v["u"]))
        assert bytes(out[0]).hex() == v["out"] and st[0] == 0, name
    d = X.DH
    pk = dev.x25519_base(bytes.fromhex(d["a"]) + bytes.fromhex(d["b"]))
    assert [bytes(p).hex() for p in pk] == [d["A"], d["B"]]
    out, st = dev.x25519(bytes.fromhex(d["a"]) + bytes.fromhex(d["b"]), bytes.fromhex(d["B"]) + bytes.fromhex(d["A"]))
    assert [bytes(o).hex() for o in out] == [d["shared"]] * 2 and not st.any()
    bufs = [_to_dev(np.frombuffer(X.BASE_U, dtype=np.uint8)), _to_dev(np.frombuffer(X.BASE_U, dtype=np.uint8)),
            torch.zeros(32, dtype=torch.uint8, device="cuda")]
    st = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
    k, u, r = 0, 1, 2
    first = None
    for i in range(1000):
        dev.x25519_dev(bufs[k].data_ptr(), bufs[u].data_ptr(), bufs[r].data_ptr(), st.data_ptr(), 1)
        k, u, r = r, k, u
        if i == 0:
            torch.cuda.synchronize()
            first = bytes(bufs[k].cpu().numpy()).hex()
    torch.cuda.synchronize()
    assert first == X.ITERATED_1
    assert bytes(bufs[k].cpu().numpy()).hex() == X.ITERATED_1000 and int(st[0]) == 0
    gpu_ctx.check()


def test_symmetry_and_the_two_public_key_algorithms(gpu_ctx):
    """x25519(a, base(b)) == x25519(b, base(a)) for 513 random pairs; base(k) == x25519(k, 9)"""
    rng = random.Random(0x25519)
    n = 513
    a, b = _rand_rows(rng, n), _rand_rows(rng, n)
    dev = _dev(gpu_ctx)
    pa, pb = dev.x25519_base(a), dev.x25519_base(b)
    s1, st1 = dev.x25519(a, pb)
    s2, st2 = dev.x25519(b, pa)
    assert np.array_equal(s1, s2) and not st1.any() and not st2.any() and s1.any(axis=1).all()
    nine = np.tile(np.frombuffer(X.BASE_U, dtype=np.uint8), (n, 1))
    assert np.array_equal(dev.x25519(a, nine)[0], pa) and np.array_equal(_x25519_dev(gpu_ctx, b, nine)[0], pb)
    for i in (0, 256, 512):
        assert bytes(pa[i]) == X.x25519_base(bytes(a[i])) and bytes(s1[i]) == X.x25519(bytes(a[i]), bytes(pb[i]))
    gpu_ctx.check()


def test_chunks_and_a_multi_device_ctx(gpu_ctx):
    """n = 200 in chunks of 64; two shard workers on one GPU"""
    import forge_ec_amd as F
    n = 200
    pick = [CASES[i % len(CASES)] for i in range(n)]
    k, u, want, wst = _batch(pick)
    gpu_ctx.set_chunk(64)
    try:
        out, st = _dev(gpu_ctx).x25519(k, u)
        pk = _dev(gpu_ctx).x25519_base(k)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    assert np.array_equal(out, want) and np.array_equal(st, wst)
    assert np.array_equal(pk, _dev(gpu_ctx).x25519_base(k)) and bytes(pk[150]) == X.x25519_base(bytes(k[150]))
    with F.Context(devices=[0, 0]) as multi:
        out, st = _dev(multi).x25519(k, u)
        assert np.array_equal(out, want) and np.array_equal(st, wst)
        assert np.array_equal(_dev(multi).x25519_base(k), pk)


def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    assert L.CANON_ZERO_SHARED == X.ZERO_SHARED == 7
    lib, h = L.lib(), gpu_ctx._h
    p = lambda a: a.ctypes.data   # noqa: E731
    n = 4
    k, u, want, wst = _batch(CASES[:n])
    out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert lib.fec_canon_x25519(h, p(k), p(u), p(out), p(st), n) == 0 and np.array_equal(out, want) and np.array_equal(st, wst)
    assert lib.fec_canon_x25519(h, None, None, None, None, 0) == 0
    assert lib.fec_canon_x25519_base(h, None, None, 0) == 0
    for args in ((None, p(k), p(u), p(out), p(st), n), (h, None, p(u), p(out), p(st), n), (h, p(k), None, p(out), p(st), n),
                 (h, p(k), p(u), None, p(st), n), (h, p(k), p(u), p(out), None, n)):
        assert lib.fec_canon_x25519(*args) == ARG, args
    for args in ((None, p(k), p(out), n), (h, None, p(out), n), (h, p(k), None, n)):
        assert lib.fec_canon_x25519_base(*args) == ARG, args
    # the *_dev forms: n = 0, nulls, misalignment, a multi-device ctx
    tk, tu = _to_dev(np.concatenate([k.reshape(-1), np.zeros(16, np.uint8)])), _to_dev(np.concatenate([u.reshape(-1), np.zeros(16, np.uint8)]))
    to = torch.zeros(n * 32 + 16, dtype=torch.uint8, device="cuda")
    ts = torch.zeros(n, dtype=torch.uint8, device="cuda")
    K, U, O, S = tk.data_ptr(), tu.data_ptr(), to.data_ptr(), ts.data_ptr()
    assert lib.fec_canon_x25519_dev(h, K, U, O, S, n, None) == 0
    assert lib.fec_canon_x25519_base_dev(h, K, O, n, None) == 0
    torch.cuda.synchronize()
    assert lib.fec_canon_x25519_dev(h, K, U, O, S, 0, None) == 0 and lib.fec_canon_x25519_dev(h, None, None, None, None, 0, None) == 0
    assert lib.fec_canon_x25519_base_dev(h, K, O, 0, None) == 0 and lib.fec_canon_x25519_base_dev(h, None, None, 0, None) == 0
    for args in ((None, K, U, O, S, n, None), (h, None, U, O, S, n, None), (h, K, None, O, S, n, None), (h, K, U, None, S, n, None),
                 (h, K, U, O, None, n, None), (h, K + 8, U, O, S, n, None), (h, K, U + 4, O, S, n, None), (h, K, U, O + 8, S, n, None)):
        assert lib.fec_canon_x25519_dev(*args) == ARG, args
    for args in ((None, K, O, n, None), (h, None, O, n, None), (h, K, None, n, None), (h, K + 8, O, n, None), (h, K, O + 1, n, None)):
        assert lib.fec_canon_x25519_base_dev(*args) == ARG, args
    torch.cuda.synchronize()
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_canon_x25519_dev(multi._h, K, U, O, S, n, None) == UNSUPPORTED
        assert lib.fec_canon_x25519_base_dev(multi._h, K, O, n, None) == UNSUPPORTED
