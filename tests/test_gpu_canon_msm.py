"""
GPU tests of canonical mode's multi-scalar multiplication (fec_canon_msm, fec_canon_msm_dev, fec_ctx_set_canon_msm_window):
every case through the host form and the *_dev form, on secp256k1, P-256 and Ed25519, every expected value from
oracle/canon_model.py through tests/canon_msm_ref.py (points are known multiples of the generator -- plus a multiple of a
point of order 8 on Ed25519 -- so a sum of any size costs one model multiplication).

The result is a canonical affine point, so it is the same 64 bytes for every window width and slice size: sizes and windows,
slices that accumulate into the same buckets (n = 2^14 at chunk 64 / 4096 / default), the scalars that steer the recoding,
the buckets that steer the arithmetic (one bucket per window split over many lanes, one point throughout, sums that cancel
inside a bucket and across buckets, the highest bucket), bad points, three calls on three streams, and the argument table.

"A sum whose only non-empty bucket is the highest of the top window": with W = ceil(257 / c) windows the topmost window only
ever holds the recoding's carry, so two readings are tested -- every scalar 2^255, whose one non-zero digit is 2^(c-1), the
highest bucket index there is, in the highest window that holds scalar bits (c = 4, 8: nothing else is non-empty); and
every scalar 2^256 - 1, which reaches the carry window's bucket 1.
"""
import numpy as np
import pytest

import canon_msm_ref as R
from abi_arg_table import Buffers, arr, call_args, spoils
from oracle import canon_model as CM

pytestmark = pytest.mark.gpu

FX = R.load_fixture()
NAMES = ["secp256k1", "p256", "ed25519"]
E_ARG, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module", params=NAMES)
def cv(request, gpu_ctx):
    """(curve name, device wrapper, ctx); the window and the chunk are back at their defaults afterwards"""
    from forge_ec_amd.canon import CANON_CURVES
    yield request.param, CANON_CURVES[request.param](gpu_ctx), gpu_ctx
    gpu_ctx.set_canon_msm_window(0)
    gpu_ctx.set_chunk(1 << 18)


def _host(dev, k, p):
    xy, st = dev.msm(k, p)
    return [int(v) for v in xy], st


def _dev(dev, k, p, stream=None):
    import torch
    n = k.shape[0]
    dk = torch.from_numpy(np.ascontiguousarray(k).view(np.int64).reshape(-1)).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(p).view(np.int64).reshape(-1)).cuda()
    out = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
    dev.msm_dev(dk.data_ptr() if n else None, dp.data_ptr() if n else None, n, out.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    return [int(v) for v in out.cpu().numpy().view(np.uint64)], int(st.cpu()[0])


def _both(dev, k, p):
    h, d = _host(dev, k, p), _dev(dev, k, p)
    assert h == d
    return h


def _case(name, ks, refs):
    """(scalars, points, expected result) of scalars ks on point references refs"""
    k, p = R.pack(ks, FX.points(name, refs))
    return k, p, tuple(R.result(name, FX.expected(name, ks, refs)))


def _pool_case(name, n, seed):
    """a drawn case of n elements: the arrays by indexing the pool, the expected sum by the logarithms"""
    ks, refs = R.draw(name, n, seed)
    pool = FX.pool(name)
    pool_xy = np.array([CM.xy_limbs(pt) for _, _, pt in pool], dtype=np.uint64)
    k = np.array([CM.limbs(v) for v in ks], dtype=np.uint64).reshape(-1, 4)
    want = R.msm_by_logs(name, ks, [pool[r][0] for r in refs], [pool[r][1] for r in refs], FX.T(name))
    return k, pool_xy[np.array(refs, dtype=np.int64)].reshape(-1, 8), tuple(R.result(name, want))


# ---- sizes and windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 513])
def test_sizes_and_windows(cv, n):
    name, dev, ctx = cv
    k, p, want = _pool_case(name, n, 1)
    if n == 0:
        assert want == (([0] * 8, R.INFINITY) if not R.is_ed(name) else (CM.limbs(0) + CM.limbs(1), R.FINITE))
    for c in R.WINDOWS + (0,):
        ctx.set_canon_msm_window(c)
        assert tuple(_both(dev, k, p)) == want, (n, c)
    ctx.check()


def test_slices_accumulate_into_the_same_buckets(cv):
    name, dev, ctx = cv
    k, p, want = _pool_case(name, 1 << 14, 2)
    for c in (0, 16):
        ctx.set_canon_msm_window(c)
        assert tuple(_dev(dev, k, p)) == want, c
        for chunk in (64, 4096, 1 << 18):
            ctx.set_chunk(chunk)
            assert tuple(_host(dev, k, p)) == want, (c, chunk)
    ctx.check()


# ---- scalars that steer the recoding --------------------------------------------------------------------------------------
def test_steering_scalars_alone(cv):
    name, dev, ctx = cv
    for c in (4, 13):
        ctx.set_canon_msm_window(c)
        for s in R.steering_scalars(name):
            k, p, want = _case(name, [s], [11])
            assert tuple(_both(dev, k, p)) == want, (c, hex(s))
    ctx.check()


@pytest.mark.parametrize("lane", [0, 31, 32, 63])
def test_steering_scalars_among_64(cv, lane):
    name, dev, ctx = cv
    ks, refs = R.draw(name, 64, 3)
    for c in (5, 16):
        ctx.set_canon_msm_window(c)
        for s in R.steering_scalars(name):
            row = list(ks)
            row[lane] = s
            k, p, want = _case(name, row, refs)
            assert tuple(_both(dev, k, p)) == want, (c, lane, hex(s))
    ctx.check()


# ---- buckets that steer the arithmetic: windows 4 and 8, n <= 513 ---------------------------------------------------------
def _steer(cv, k, p, want):
    name, dev, ctx = cv
    for c in (4, 8):
        ctx.set_canon_msm_window(c)
        assert tuple(_both(dev, k, p)) == tuple(want), c
    ctx.check()


def test_513_equal_scalars_distinct_points(cv):
    name = cv[0]
    pts, logs, js = R.chain(name, 513, 0x5EED, FX.T(name))
    assert len(set(pts)) == 513
    s = R.draw(name, 1, 4)[0][0]
    k, p = R.pack([s] * 513, pts)
    _steer(cv, k, p, R.result(name, R.msm_by_logs(name, [s] * 513, logs, js, FX.T(name))))


def test_513_scalars_one_point(cv):
    name = cv[0]
    ks = R.draw(name, 513, 5)[0]
    k, p, want = _case(name, ks, [9] * 513)
    _steer(cv, k, p, want)


def test_pairs_that_cancel_inside_each_bucket(cv):
    name = cv[0]
    ks = R.draw(name, 200, 6)[0]
    k, p, want = _case(name, [v for v in ks for _ in (0, 1)], [r for i in range(200) for r in (i % 64, -(i % 64) - 1)])
    assert want == tuple(R.result(name, R.identity(name)))
    _steer(cv, k, p, want)


def test_pairs_that_cancel_across_buckets(cv):
    name = cv[0]
    N = R.MODELS[name].N
    ks = [v % N for v in R.draw(name, 200, 7)[0]]
    if R.is_ed(name):   # (N - k) P = -k P only without a torsion part: multiples of 8 in the pool
        refs = [8 * (i % 8) for i in range(200) for _ in (0, 1)]
    else:
        refs = [i % 64 for i in range(200) for _ in (0, 1)]
    k, p, want = _case(name, [v for q in ks for v in (q, N - q)], refs)
    assert want == tuple(R.result(name, R.identity(name)))
    _steer(cv, k, p, want)


@pytest.mark.parametrize("scalar", [0, R.TOP, 2**255], ids=["zeros", "all-ones", "highest-bucket"])
def test_one_scalar_throughout(cv, scalar):
    name = cv[0]
    refs = R.draw(name, 300, 8)[1]
    k, p, want = _case(name, [scalar] * 300, refs)
    _steer(cv, k, p, want)


@pytest.fixture(scope="module")
def ed(gpu_ctx):
    from forge_ec_amd.canon import CanonEd25519
    yield "ed25519", CanonEd25519(gpu_ctx), gpu_ctx
    gpu_ctx.set_canon_msm_window(0)


def test_ed25519_torsion_points_as_inputs(ed):
    cv = ed
    name, dev, ctx = cv
    E = CM.ED25519
    tk = [1, 7, 8, E.N, E.N + 1, R.TOP]
    ks, refs = [q for q in tk for _ in range(8)], ["t%d" % j for _ in tk for j in range(8)]
    k, p, want = _case(name, ks, refs)
    reduced = R.result(name, FX.expected(name, [q % E.N for q in ks], refs))
    assert tuple(reduced) != want   # a run with k mod l would give another answer
    _steer(cv, k, p, want)
    for q in tk:   # each scalar on each torsion point alone
        for j in range(8):
            k, p, want = _case(name, [q], ["t%d" % j])
            ctx.set_canon_msm_window(4)
            assert tuple(_both(dev, k, p)) == want, (hex(q), j)
    ks, refs = R.draw(name, 40, 9)
    refs = [("id" if i % 5 == 2 else r) for i, r in enumerate(refs)]
    k, p, want = _case(name, ks, refs)
    _steer(cv, k, p, want)


# ---- bad points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 98, 196])
def test_bad_points(cv, at):
    name, dev, ctx = cv
    C = R.MODELS[name]
    ks, refs = R.draw(name, 197, 10)
    k, p, want = _case(name, ks, refs)
    x, y = FX.points(name, refs)[at]
    for c in (0, 8):
        ctx.set_canon_msm_window(c)
        for bad in ((C.P, y), (x, C.P), (x, (y + 1) % C.P)):
            q = p.copy()
            q[at] = CM.limbs(bad[0]) + CM.limbs(bad[1])
            assert _both(dev, k, q) == ([0] * 8, R.BAD_POINT), (c, at)
            assert tuple(_both(dev, k, p)) == want   # a following call on good input is right
    ctx.check()


# ---- ordering: an MSM, an ECDSA verification and a second MSM on three streams of one ctx ------------------------------------
def test_three_calls_on_three_streams(cv):
    import torch
    from forge_ec_amd.canon import CanonSecp256k1
    name, dev, ctx = cv
    ctx.set_canon_msm_window(0)
    S = CM.SECP256K1
    n_sig = 256
    d, kk, z = 0x1234567, 0x7654321, 0xABCDEF
    Rp = S.mul(kk, S.G)
    r = Rp[0] % S.N
    s = pow(kk, -1, S.N) * (z + r * d) % S.N
    sig = {w: torch.from_numpy(np.tile(np.array(CM.limbs(v), dtype=np.uint64), (n_sig, 1)).view(np.int64)).cuda() for w, v in (("z", z), ("r", r), ("s", s))}
    sig["r"][5, 0] ^= 1   # one signature is wrong
    pk = torch.from_numpy(np.tile(np.array(CM.xy_limbs(S.mul(d, S.G)), dtype=np.uint64), (n_sig, 1)).view(np.int64)).cuda()
    res = torch.full((n_sig,), 9, dtype=torch.uint8, device="cuda")
    k1, p1, want1 = _pool_case(name, 3000, 11)
    k2, p2, want2 = _pool_case(name, 777, 12)
    assert want1 != want2
    t = [torch.from_numpy(a.view(np.int64).reshape(-1)).cuda() for a in (k1, p1, k2, p2)]
    outs = [torch.full((8,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
    sts = [torch.full((1,), 9, dtype=torch.uint8, device="cuda") for _ in range(2)]
    _dev(dev, k1[:8], p1[:8])   # the work area and the comb tables exist before the three calls: growing them would synchronise
    CanonSecp256k1(ctx).ecdsa_verify_dev(sig["z"].data_ptr(), sig["r"].data_ptr(), sig["s"].data_ptr(), pk.data_ptr(), res.data_ptr(), n_sig, None)
    _dev(dev, k1, p1)
    torch.cuda.synchronize()
    res.fill_(9)
    streams = [torch.cuda.Stream() for _ in range(3)]
    dev.msm_dev(t[0].data_ptr(), t[1].data_ptr(), 3000, outs[0].data_ptr(), sts[0].data_ptr(), streams[0].cuda_stream)
    CanonSecp256k1(ctx).ecdsa_verify_dev(sig["z"].data_ptr(), sig["r"].data_ptr(), sig["s"].data_ptr(), pk.data_ptr(), res.data_ptr(), n_sig,
                                         streams[1].cuda_stream)
    dev.msm_dev(t[2].data_ptr(), t[3].data_ptr(), 777, outs[1].data_ptr(), sts[1].data_ptr(), streams[2].cuda_stream)
    torch.cuda.synchronize()
    got = [([int(v) for v in o.cpu().numpy().view(np.uint64)], int(q.cpu()[0])) for o, q in zip(outs, sts)]
    assert tuple(got[0]) == want1 and tuple(got[1]) == want2
    assert res.cpu().tolist() == [0 if i == 5 else 1 for i in range(n_sig)]
    ctx.check()


# ---- arguments ----------------------------------------------------------------------------------------------------------------
MSM = ["ctx", "curve3", arr("scalars", 32), arr("points_xy", 64), "n", arr("out_xy", 64), arr("status", 1)]
SPECS = {"fec_canon_msm": (MSM, False), "fec_canon_msm_dev": (MSM + ["stream"], True)}


def test_argument_codes_and_nothing_launched(gpu_ctx):
    """The case set of tests/test_gpu_abi_arg_codes.py by the same machinery; the expected statuses follow from the header: a
    multi-device ctx is FEC_E_UNSUPPORTED in both forms, every other case FEC_E_ARG -- n = 0 with every array null included,
    because the result is written whatever n is.  No case is a legal call, so nothing may be launched: every buffer of the
    table is zero-filled, and a launched call would leave status 2 (the zero point is on no curve) or 1 behind."""
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib, buf = L.lib(), Buffers()
    seen = set()
    with F.Context(devices=[0, 0]) as multi:
        for fn, (spec, dev) in SPECS.items():
            cases = spoils(spec, dev) + ([] if dev else [("ctx=multi", {"ctx": "multi"})])
            for case, spoil in cases:
                spoil = dict(spoil)
                want = E_ARG
                if spoil.get("ctx") == "multi":
                    spoil["ctx"], want = multi._h, E_UNSUPPORTED
                assert int(getattr(lib, fn)(*call_args(spec, dev, buf, gpu_ctx._h, spoil))) == want, (fn, case)
                seen.add(case.split("=")[0].split("+")[0])
        for bits in (-1, 1, 17):
            assert int(lib.fec_ctx_set_canon_msm_window(gpu_ctx._h, bits)) == E_ARG
            assert int(lib.fec_ctx_set_canon_msm_window(multi._h, bits)) == E_ARG
        assert int(lib.fec_ctx_set_canon_msm_window(None, 4)) == E_ARG
        for bits in (2, 16, 0):
            assert int(lib.fec_ctx_set_canon_msm_window(gpu_ctx._h, bits)) == 0
    assert {"ctx", "n", "scalars", "points_xy", "out_xy", "status", "curve"} <= seen
    buf.torch.cuda.synchronize()
    for keep in buf.keep:
        if isinstance(keep, buf.torch.Tensor):
            assert int(keep.count_nonzero()) == 0
        else:
            assert not np.asarray(keep).any()
    gpu_ctx.check()
