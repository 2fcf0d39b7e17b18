"""
The composed callers of fecgpu.hip above the sizes where they change how they use memory, bit-exact against the C
oracle on every element (or on every output of a batch verifier: verdict, both affine sides, their infinity flags,
the Ed25519 debug-build flag, ECDSA's folded sums).

  n >= 2^16        the Ed25519 table kernel sorts the whole batch by popcount in a work area of the launch stream's
                   scratch (ed_fixed_work_bytes); a fixed base of the caller's own gets a prefix table in that scratch
                   behind the caller's own bytes (acquire_with_prefix)
  n > 2^15         launch_double_mul stops forking the Ed25519 fixed-base product to the second stream
  n > ctx chunk    the host-pointer pipeline and multi_scalar_mul run chunks on two lanes, each with its own scratch

A stream's scratch is one buffer.  Each launcher lays out all of its regions (its own, the sort area, a per-call prefix
table) in one WorkArea and holds that scratch until its last enqueue: a second acquisition on the same stream in the
meantime fails with an error instead of overlaying the holder's data.  Below these sizes an overlay could not show.  The batches are ragged
(N = 2^16 + 37) and carry the edge inputs of the small tests at both ends -- zero and all-ones scalars, single-bit
and low-popcount runs, zero weights, identity points, infinity flags -- so that the popcount sort moves elements
across the whole batch.
"""
import numpy as np
import pytest

import vectors as V

pytestmark = pytest.mark.gpu

N = (1 << 16) + 37
CHUNK = (1 << 16) + 5                  # set_chunk: two pipeline lanes of >= 2^16 elements each and a ragged third chunk
N_CHUNKED = 2 * CHUNK + 37
THREADS = 16
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
NAMES = {0: "secp256k1", 1: "P-256", 2: "Ed25519"}


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        rows = got.reshape(got.shape[0], -1) if got.ndim else got.reshape(1, 1)
        wrows = want.reshape(want.shape[0], -1) if want.ndim else want.reshape(1, 1)
        bad = np.nonzero((rows != wrows).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, first at %d" % (what, len(bad), rows.shape[0], bad[0]))


def _edge_scalars(k):
    """Edge scalars at both ends of k (n >= 2^15) and the popcount runs of the batch-wide sort test in the middle."""
    n = k.shape[0]
    for lo in (0, n - 330):
        k[lo] = 0                                      # multiply's zero-scalar early-out (popcount 0: sorts last)
        k[lo + 329] = 0
        k[lo + 1:lo + 65] = ALL_ONES                   # popcount 256, consumed as is
        for i in range(256):                           # single-bit scalars: one addend each
            k[lo + 65 + i] = 0
            k[lo + 65 + i, i // 64] = np.uint64(1) << np.uint64(i % 64)
        k[lo + 321:lo + 329, 1:] = 0                   # low popcounts
    k[3000:9000, 1:] = 0                               # a long low-popcount run
    k[20000:30000] = k[20000]                          # one popcount bin with 10^4 elements
    return k


def _edge_flags(n):
    inf = np.zeros(n, dtype=np.uint8)
    inf[[0, 1, 7, n - 8, n - 2, n - 1]] = 1
    inf[1000::4099] = 1
    return inf


def _sample_idx(n, k, seed):
    rng = np.random.default_rng(seed)
    head = np.arange(min(4096, n))
    tail = np.arange(max(0, n - 4096), n)
    mid = rng.integers(0, n, size=k)
    return np.unique(np.concatenate([head, tail, mid]))


def _pairs(n, curve, seed):
    """n (x, y) rows of raw field limbs (the Schnorr / ECDSA entry points take any coordinates)."""
    return np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, seed), V.field_elements(n, curve, seed + 1)], axis=1))


def _p256_true_points(n, seed):
    """n affine points of the real P-256: the reference's is_on_curve accepts about half of them."""
    import random
    p = V.PRIME[1]
    b = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
    rng = random.Random(seed)
    rows = []
    while len(rows) < n:
        x = rng.randrange(p)
        rhs = (x * x * x - 3 * x + b) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs:
            rows.append(V.limbs_of(x) + V.limbs_of(y))
    return np.array(rows, dtype=np.uint64)


def _points_with_identities(n, curve, seed, oracle):
    p = V.points(n, curve, seed)
    ident = oracle.identity(curve)
    for i in (0, 1, 5, n - 6, n - 2, n - 1):
        p[i] = ident
    return p


# ---- schnorr::batch_verify -------------------------------------------------------------------------------------------

def _schnorr_batch_inputs(n, curve, seed):
    pk, r = _pairs(n, curve, seed), _pairs(n, curve, seed + 2)
    s, a, e = V.scalars(n, curve, seed + 4), V.scalars(n, curve, seed + 5), V.scalars(n, curve, seed + 6)
    _edge_scalars(s)
    _edge_scalars(e)
    a[[2, 3, n - 4, n - 3]] = 0                        # zero weights at both ends
    a[3000:9000] = np.array([1, 0, 0, 0], dtype=np.uint64)   # s_i * a_i = s_i: the low-popcount run reaches the sort
    a[n - 200:n - 100] = np.array([1, 0, 0, 0], dtype=np.uint64)
    return pk, r, s, a, e


def _check_schnorr_batch(ctx, oracle, curve, n, seed):
    pk, r, s, a, e = _schnorr_batch_inputs(n, curve, seed)
    what = "%s schnorr batch_verify n=%d seed=%d" % (NAMES[curve], n, seed)
    if curve == 2:
        want, w_sides, w_inf, w_dbg = oracle.ed25519_schnorr_batch_verify(pk, None, r, None, s, a, e, nthreads=THREADS)
        got, sides, sinf, dbg = ctx.schnorr_batch_verify_ed25519(pk, r, s, a, e)
        _same(sides, w_sides, what + ": affine sides")
        _same(sinf, w_inf, what + ": sides' infinity flags")
        assert (got, dbg) == (want, bool(w_dbg)), what
        assert dbg                                     # full-size s_i * a_i wrap a u128 sum
    else:
        want, w_sides, w_inf = oracle.schnorr_batch_verify(curve, pk, None, r, None, s, a, e, nthreads=THREADS)
        if curve == 0:
            got, sides, sinf = ctx.schnorr_batch_verify_secp256k1(pk, r, s, a, e)
            _same(sides, w_sides, what + ": affine sides (secp256k1 entry point)")
            assert got == (want == 1), what
    g2, sides2, sinf2 = ctx.schnorr_batch_verify(curve, pk, r, s, a, e)   # the generic entry point
    _same(sides2, w_sides, what + ": affine sides (generic entry point)")
    _same(sinf2, w_inf, what + ": sides' infinity flags (generic entry point)")
    assert g2 == (want == 1), what
    assert w_sides.any()
    return pk, r, s, a, e


@pytest.mark.parametrize("n, seed", [(N, 5100), (N, 5120), (1 << 16, 5140), ((1 << 16) - 1, 5160)])
def test_schnorr_batch_ed25519_above_sort_threshold(gpu_ctx, oracle, n, seed):
    """The Ed25519 branch of schnorr_batch_verify holds s_i * a_i in the stream's scratch while the table kernel sorts
    them by popcount (n >= 2^16): the sort area must lie behind them, not on them.  (With the sort area on them the
    histogram and the scatter read scalars the other kernels are overwriting, the cursors stop partitioning [0, n),
    and unwritten permutation slots send the table kernel to indices outside the batch: the call failed with
    FEC_E_DEVICE.)  N twice (the second call finds the scratch already grown), 2^16 exactly, and 2^16 - 1 (no sort
    area)."""
    pk, r, s, a, e = _check_schnorr_batch(gpu_ctx, oracle, 2, n, seed)
    # all weights zero: true through (infinity, infinity); an identity input rejects before any product
    got, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, np.zeros_like(a), e)
    assert got == 1 and list(sinf) == [1, 1] and not sides.any() and not dbg
    assert gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, a, e, pk_inf=_edge_flags(n))[0] == 0


@pytest.mark.parametrize("curve", [0, 1])
def test_schnorr_batch_weierstrass_large(gpu_ctx, oracle, curve):
    """secp256k1 / P-256 schnorr_batch_verify at N: the implicit generator prefix, the A terms on the second stream."""
    pk, r, s, a, e = _check_schnorr_batch(gpu_ctx, oracle, curve, N, 5200 + 20 * curve)
    got, sides, sinf = gpu_ctx.schnorr_batch_verify(curve, pk, r, s, np.zeros_like(a), e)
    assert got is True and list(sinf) == [1, 1] and not sides.any()
    assert gpu_ctx.schnorr_batch_verify(curve, pk, r, s, a, e, r_inf=_edge_flags(N))[0] is False


# ---- per-signature verifiers, double_mul, validate_point, ECDH -----------------------------------------------------

@pytest.mark.parametrize("curve", [0, 1, 2])
def test_schnorr_verify_large(gpu_ctx, oracle, curve):
    """Schnorr::verify per signature at N (Ed25519: the sort area behind the three work arrays)."""
    pk, r = _pairs(N, curve, 5300), _pairs(N, curve, 5302)
    s, e = _edge_scalars(V.scalars(N, curve, 5304)), _edge_scalars(V.scalars(N, curve, 5305))
    e[N - 50] = np.array([1, 0, 0, 0], dtype=np.uint64)
    pinf, rinf = _edge_flags(N), _edge_flags(N)[::-1].copy()
    want = oracle.batch_schnorr_verify(curve, pk, pinf, r, rinf, s, e, nthreads=THREADS)
    _same(gpu_ctx.schnorr_verify(curve, pk, r, s, e, pk_inf=pinf, r_inf=rinf), want, "%s schnorr_verify" % NAMES[curve])


@pytest.mark.parametrize("curve, n", [(2, N), (2, 1 << 15), (2, (1 << 15) + 1), (1, N)])
def test_batch_double_mul_large(gpu_ctx, oracle, curve, n):
    """u1*G + u2*Q: Ed25519 with the fixed-base product beside the variable one (n <= 2^15), after it on one stream
    (2^15 + 1), and sorted in the sort area behind the two product arrays (N); P-256 at N."""
    u1, u2 = _edge_scalars(V.scalars(n, curve, 5400)), V.scalars(n, curve, 5401)
    u2[:400] = u1[n - 400:]
    u2[n - 400:] = u1[:400]
    q = _points_with_identities(n, curve, 5402, oracle)
    want = oracle.batch_double_mul(curve, u1, u2, q, nthreads=THREADS)
    _same(gpu_ctx.batch_double_mul(curve, u1, u2, q), want, "%s batch_double_mul n=%d" % (NAMES[curve], n))


def test_batch_validate_point_ed25519_large(gpu_ctx, oracle):
    """Ed25519 validate_point at N: the n * 417-byte work area with two scheduler launches inside."""
    xy = _pairs(N, 2, 5500)
    g, _ = oracle.to_affine(2, oracle.generator(2))
    for lo in (0, N - 64):
        xy[lo:lo + 20, :4] = 0                         # (0, 1): on the curve, order 1
        xy[lo:lo + 20, 4:] = np.array([1, 0, 0, 0], dtype=np.uint64)
        xy[lo + 20:lo + 40, :4] = 0
        xy[lo + 40] = g
    inf = _edge_flags(N)
    want = oracle.batch_validate_point(2, xy, inf, nthreads=THREADS)
    assert set(int(v) for v in np.unique(want)) == {0, 1}
    _same(gpu_ctx.batch_validate_point(2, xy, inf), want, "Ed25519 batch_validate_point")


@pytest.mark.parametrize("curve", [0, 1])
def test_batch_ecdh_large(gpu_ctx, oracle, curve):
    sk = _edge_scalars(V.scalars(N, curve, 5600))
    pk = _pairs(N, curve, 5601)
    if curve == 1:                                     # accepted keys at both ends and in the middle
        pk[:3000] = _p256_true_points(3000, 5603)
        pk[N - 3000:] = _p256_true_points(3000, 5604)
        pk[30000:32000] = _p256_true_points(2000, 5605)
    inf = _edge_flags(N)
    want, wst = oracle.batch_ecdh(curve, sk, pk, inf, nthreads=THREADS)
    got, gst = gpu_ctx.batch_ecdh(curve, sk, pk, inf)
    _same(gst, wst, "%s batch_ecdh status" % NAMES[curve])
    _same(got, want, "%s batch_ecdh secrets" % NAMES[curve])


# ---- Ecdsa::batch_verify ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", [0, 1])
def test_ecdsa_batch_verify_large(gpu_ctx, oracle, curve):
    """Ecdsa::batch_verify at N: a random batch (the final comparison fails: both folded sums compared), a batch that
    verifies under the reference's arithmetic, and batches whose first failing signature lies late in index order."""
    n = N
    order = 0xFFFFFFFFFFFFFFFEFFFFFFFFFFFFFFFFBAAEDCE6AF48A03BBFD25E8CD0364141 if curve == 0 else V.ORDER[1]
    op = oracle.secp256k1_scalar_op if curve == 0 else oracle.p256_scalar_op
    rng = np.random.default_rng(5700 + curve)
    dg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    dg[:, 0] &= 0x7F
    r, s, a = V.scalars(n, curve, 5701), V.scalars(n, curve, 5702), V.scalars(n, curve, 5703)
    a[[0, n - 1]] = 0
    pk = _pairs(n, curve, 5704)
    inf = _edge_flags(n)
    what = "%s ecdsa_batch_verify" % NAMES[curve]

    def both(dg, r, s, pk, inf, a, label):
        want, wd = oracle.ecdsa_batch_verify(curve, dg, r, s, pk, inf, a, nthreads=THREADS)
        got, gd = gpu_ctx.ecdsa_batch_verify(curve, dg, r, s, pk, inf, a)
        _same(gd, wd, "%s (%s): r_sum, scalar sum" % (what, label))
        assert got == want, (what, label)
        return want, wd

    st, detail = both(dg, r, s, pk, inf, a, "random")
    assert st == 0 and detail.any()
    # all keys at infinity: r_sum does not depend on r; last weight 1, last r = x(r_sum) - (ordered sum of the rest)
    inf1 = np.ones(n, dtype=np.uint8)
    a2 = a.copy()
    a2[n - 1] = [1, 0, 0, 0]
    _, d = oracle.ecdsa_batch_verify(curve, dg, r, s, pk, inf1, a2, nthreads=THREADS)
    xy, is_inf = oracle.to_affine(curve, d[:12])
    assert not is_inf
    xs = V.int_of(oracle.field_op(0, "mul", xy[:4], np.array([1, 0, 0, 0], dtype=np.uint64))) if curve == 0 else V.int_of(xy[:4])
    base = np.zeros(4, dtype=np.uint64)
    for i in range(n - 2):
        base = op("add", base, op("mul", a2[i], r[i])[0])[0]
    r2 = r.copy()
    made = False
    for attempt in range(32):
        r2[n - 2] = V.scalars(1, curve, 5710 + attempt)[0]
        partial = op("add", base, op("mul", a2[n - 2], r2[n - 2])[0])[0]
        if 0 < xs < order and xs > V.int_of(partial):
            r2[n - 1] = V.limbs_of(xs - V.int_of(partial))
            made = True
            break
    assert made
    assert both(dg, r2, s, pk, inf1, a2, "verifies")[0] == 1
    # the first failing signature in index order decides, late in the batch
    r3 = r.copy()
    r3[n - 5] = 0
    assert both(dg, r3, s, pk, inf, a, "r = 0 at n - 5")[0] == 0
    dg4 = dg.copy()
    dg4[n - 2] = 0xFF
    assert both(dg4, r, s, pk, inf, a, "digest panic at n - 2")[0] == 2
    assert both(dg4, r3, s, pk, inf, a, "r = 0 at n - 5 before the panic at n - 2")[0] == 0


# ---- multi_scalar_mul and the host chunk pipeline (a ctx of the test's own: set_chunk) ------------------------------

@pytest.mark.parametrize("curve", [0, 1, 2])
def test_multi_scalar_mul_two_lanes(oracle, curve):
    """multi_scalar_mul over three chunks (products written at offsets), then the ordered fold."""
    import forge_ec_amd as F
    n = N_CHUNKED
    k = _edge_scalars(V.scalars(n, curve, 5800 + curve))
    p = _points_with_identities(n, curve, 5810 + curve, oracle)
    prods = oracle.batch_mul(curve, k, p, nthreads=THREADS)
    acc = oracle.identity(curve)
    for i in range(n):
        acc = oracle.point_add(curve, acc, prods[i])
    ctx = F.Context(0)
    try:
        ctx.set_chunk(CHUNK)
        _same(ctx.multi_scalar_mul(curve, k, p), acc, "%s multi_scalar_mul n=%d chunk=%d" % (NAMES[curve], n, CHUNK))
    finally:
        ctx.close()


@pytest.mark.parametrize("curve, base_kind", [(2, "generator"), (2, "own"), (0, "own")])
def test_host_batch_mul_fixed_two_lanes(oracle, curve, base_kind):
    """Host batch_mul_fixed through the two-lane chunk pipeline, both lanes >= 2^16: each lane stream's own sort area
    (Ed25519) and per-call prefix table (a base of the caller's own: projective, z != 1)."""
    import forge_ec_amd as F
    n = N_CHUNKED
    k = _edge_scalars(V.scalars(n, curve, 5900 + curve))
    if base_kind == "generator":
        base = oracle.generator(curve)
    else:
        base = oracle.batch_mul_fixed(curve, V.scalars(1, curve, 5910 + curve), oracle.generator(curve))[0]
        assert V.int_of(base[8:12]) not in (0, 1)     # Z
    want = oracle.batch_mul_fixed(curve, k, base, nthreads=THREADS)
    ctx = F.Context(0)
    try:
        ctx.set_chunk(CHUNK)
        _same(ctx.batch_mul_fixed(curve, k, base), want, "%s batch_mul_fixed(%s) n=%d chunk=%d" % (NAMES[curve], base_kind, n, CHUNK))
    finally:
        ctx.close()


# ---- *_dev forms on a stream of the caller's own ---------------------------------------------------------------------

def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def test_dev_forms_on_a_caller_stream_ed25519(gpu_ctx, oracle):
    """batch_mul_fixed_dev with a base of the caller's own and schnorr_verify_dev at N on a torch stream: that stream's
    scratch holds the sort area (and the per-call prefix table behind it)."""
    import torch
    k = _edge_scalars(V.scalars(N, 2, 6000))
    base = oracle.batch_mul_fixed(2, V.scalars(1, 2, 6001), oracle.generator(2))[0]
    want = oracle.batch_mul_fixed(2, k, base, nthreads=THREADS)
    dk, db = _to_dev(k), _to_dev(base)
    out = torch.zeros(N * 128, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.batch_mul_fixed_dev(2, dk.data_ptr(), db.data_ptr(), out.data_ptr(), N, stream.cuda_stream)
    stream.synchronize()
    gpu_ctx.check()
    _same(out.cpu().numpy().view(np.uint64).reshape(N, 16), want, "Ed25519 batch_mul_fixed_dev(own base), caller stream")

    pk, r = _pairs(N, 2, 6002), _pairs(N, 2, 6004)
    s, e = _edge_scalars(V.scalars(N, 2, 6006)), V.scalars(N, 2, 6007)
    pinf, rinf = _edge_flags(N), np.zeros(N, dtype=np.uint8)
    want = oracle.batch_schnorr_verify(2, pk, pinf, r, rinf, s, e, nthreads=THREADS)
    t = [_to_dev(x) for x in (pk, pinf, r, rinf, s, e)]
    st = torch.zeros(N, dtype=torch.uint8, device="cuda:0")
    stream2 = torch.cuda.Stream()
    stream2.wait_stream(torch.cuda.current_stream())
    gpu_ctx.schnorr_verify_dev(2, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                               t[5].data_ptr(), st.data_ptr(), N, stream2.cuda_stream)
    stream2.synchronize()
    gpu_ctx.check()
    _same(st.cpu().numpy(), want, "Ed25519 schnorr_verify_dev, caller stream")


# ---- the largest single launch ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", [1, 2])
def test_batch_mul_dev_one_launch_2p22(gpu_ctx, oracle, curve):
    """One unchunked batch_mul_dev launch of 2^22 elements on the lock-free scheduler kernels (P-256, Ed25519): the
    most elements per workgroup one call puts on the schedulers' watchdogs.  It must return FEC_OK and agree with the
    oracle on the first and last 4096 rows and a random sample."""
    import torch
    n = 1 << 22
    limbs = V.POINT_LIMBS[curve]
    k, p = _edge_scalars(V.scalars(n, curve, 6100 + curve)), V.points(n, curve, 6110 + curve)
    dk = torch.from_numpy(k.view(np.int64)).cuda()
    dp = torch.from_numpy(p.view(np.int64)).cuda()
    out = torch.empty((n, limbs), dtype=torch.int64, device="cuda")
    gpu_ctx.batch_mul_dev(curve, dk.data_ptr(), dp.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gpu_ctx.check()
    got = out.cpu().numpy().view(np.uint64)
    idx = _sample_idx(n, 4000, 6130 + curve)
    _same(got[idx], oracle.batch_mul(curve, k[idx], p[idx], nthreads=THREADS), "%s batch_mul_dev n=2^22" % NAMES[curve])
