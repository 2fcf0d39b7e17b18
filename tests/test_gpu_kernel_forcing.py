"""
The multiply-family kernels on inputs that force their rare legs (tests/golden/kernel_forcing_vectors.json, census in
tests/rare_legs.json): every case is a (scalar, point) pair on which a named leg fires in an operation whose result the
kernel keeps.  Results are compared bit-exactly with the fixture (py_model) and with the threaded C oracle.
"""
import numpy as np
import pytest

import sched_geometry
import vectors as V
from forcing_cases import FORCING, cases as _cases, mixed as _mixed

THREADS = 16
NAMES = {0: "secp256k1", 1: "P-256", 2: "Ed25519"}
CHUNK = 1 << 12


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(~(got == want).all(axis=-1))[0] if got.ndim > 1 else [0]
        raise AssertionError("%s: %d rows differ, first at %s" % (what, len(bad), list(bad[:8])))


def _range_edges(n):
    """Element indices at the edges of the P-256 / Ed25519 schedulers' workgroup ranges (p256_launch_mul,
    ed_launch_mul; sched_geometry.sched_grid mirrors their rule: workgroup w owns [w * per_wg, ...)) and of
    the 64-element claims inside a range, including the last (partial) claim; plus wavefront edges 0 / 31 / 32 / 63."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid, per_wg = sched_geometry.sched_grid(cus, n)
    at = {0, 31, 32, 63, n - 1}
    for w in (0, 1, grid // 2, grid - 2, grid - 1):
        lo, hi = w * per_wg, min(n, (w + 1) * per_wg)
        last_claim = lo + (hi - lo - 1) // 64 * 64
        at |= {lo, lo + 63, lo + 64, last_claim, hi - 1}
    return sorted(a for a in at if 0 <= a < n)


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_batch_mul_crafted_wavefronts_and_lanes(gpu_ctx, oracle, curve):
    k, p, e, _ = _cases(curve)
    # whole wavefronts of crafted lanes (every lane of four wavefronts takes a rare leg)
    reps = -(-256 // k.shape[0])
    kt, pt = np.tile(k, (reps, 1))[:256], np.tile(p, (reps, 1))[:256]
    got = gpu_ctx.batch_mul(curve, kt, pt)
    _same(got, np.tile(e, (reps, 1))[:256], "%s batch_mul crafted wavefronts vs fixture" % NAMES[curve])
    # crafted elements among random ones at wavefront edges, scheduler range and claim edges, and the last element;
    # ranges of 151 elements take three claims, the last one partial
    n = 256 * 150 + 37
    at = _range_edges(n)
    ks, ps, (pos, want) = _mixed(curve, n, at, 700 + 10 * curve)
    got = gpu_ctx.batch_mul(curve, ks, ps)
    _same(got[pos], want, "%s batch_mul crafted elements at range edges vs fixture" % NAMES[curve])
    _same(got, oracle.batch_mul(curve, ks, ps, nthreads=THREADS), "%s batch_mul crafted elements vs oracle" % NAMES[curve])


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_batch_mul_crafted_on_chunk_boundaries(oracle, curve):
    """The host pipeline with small chunks: crafted elements first and last in chunks."""
    import forge_ec_amd as F
    n = 3 * CHUNK + 5
    at = [0, 1, CHUNK // 2, CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 2, 2 * CHUNK - 1, 2 * CHUNK,
          2 * CHUNK + 1, 2 * CHUNK + CHUNK // 2, 3 * CHUNK - 2, 3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1, 3 * CHUNK + 2,
          n - 2, n - 1]
    ks, ps, (pos, want) = _mixed(curve, n, at, 760 + 10 * curve)
    ctx = F.Context(0)
    try:
        ctx.set_chunk(CHUNK)
        got = ctx.batch_mul(curve, ks, ps)
    finally:
        ctx.close()
    _same(got[pos], want, "%s batch_mul chunk=%d vs fixture" % (NAMES[curve], CHUNK))
    _same(got, oracle.batch_mul(curve, ks, ps, nthreads=THREADS), "%s batch_mul chunk=%d vs oracle" % (NAMES[curve], CHUNK))


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_batch_mul_fixed_crafted_bases(gpu_ctx, oracle, curve):
    """Every crafted base through the fixed-base kernels: below 2^16, and at 2^16 + 37, where the launch builds a prefix
    table from the base (k_secp_mul<3>/<2>, k_p256_prefix_level, k_ed_prefix_level) and Ed25519 takes its table and
    sorted kernels.  At the large size the same call on a ctx without prefix tables must agree row for row."""
    import forge_ec_amd as F
    off = F.Context(0)
    try:
        off.set_fixed_prefix_bits(0)
        for b in (b for b in FORCING["bases"] if b["curve"] == curve):
            base = np.array(b["point"], dtype=np.uint64)
            kb, eb = np.array(b["scalars"], dtype=np.uint64), np.array(b["expect"], dtype=np.uint64)
            for n in (300, (1 << 16) + 37):
                ks = V.scalars(n, curve, 800 + curve)
                at = np.array([0, 63, 64, n // 2, n - 1])
                idx = np.arange(at.size) % kb.shape[0]
                ks[at] = kb[idx]
                got = gpu_ctx.batch_mul_fixed(curve, ks, base)
                what = "%s batch_mul_fixed(%s base) n=%d" % (NAMES[curve], b["family"], n)
                _same(got[at], eb[idx], what + " vs fixture")
                if n < 1 << 16:
                    _same(got, oracle.batch_mul_fixed(curve, ks, base, nthreads=THREADS), what + " vs oracle")
                    continue
                s = np.arange(0, n, 97)   # the oracle on a sample; the table-free run on every row
                _same(got[s], oracle.batch_mul(curve, ks[s], np.tile(base, (s.size, 1)), nthreads=THREADS), what + " vs oracle")
                _same(got, off.batch_mul_fixed(curve, ks, base), what + " prefix tables on vs off")
    finally:
        off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_double_mul_msm_affine_compress_crafted(gpu_ctx, oracle, curve):
    """batch_double_mul with crafted Q, multi_scalar_mul over crafted points, and every output through batch_to_affine
    and batch_compress."""
    k, p, _, _ = _cases(curve)
    n = k.shape[0]
    u1 = V.scalars(n, curve, 900 + curve)
    got = gpu_ctx.batch_double_mul(curve, u1, k, p)
    _same(got, oracle.batch_double_mul(curve, u1, k, p, nthreads=THREADS), "%s batch_double_mul crafted Q" % NAMES[curve])
    prods = oracle.batch_mul(curve, k, p, nthreads=THREADS)
    acc = oracle.identity(curve)
    for i in range(n):
        acc = oracle.point_add(curve, acc, prods[i])
    _same(gpu_ctx.multi_scalar_mul(curve, k, p), acc, "%s multi_scalar_mul crafted" % NAMES[curve])
    outs = np.concatenate([got, prods])
    xy, inf = gpu_ctx.batch_to_affine(curve, outs)
    wxy, winf = oracle.batch_to_affine(curve, outs, nthreads=THREADS)
    _same(xy, wxy, "%s batch_to_affine of crafted outputs" % NAMES[curve])
    assert np.array_equal(inf.astype(bool), np.asarray(winf).astype(bool))
    _same(gpu_ctx.batch_compress(curve, xy, inf), oracle.batch_compress(curve, wxy, winf),
          "%s batch_compress of crafted outputs" % NAMES[curve])


@pytest.mark.gpu
def test_secp256k1_ecdh_crafted_keys(gpu_ctx, oracle):
    """batch_ecdh (secp256k1 takes keys without validation) on the crafted points whose z is 1 (the *_affine families
    and those whose leg does not depend on z): the key (x, y) is the crafted point itself."""
    k, p, _, fam = _cases(0, affine=True)
    assert any(f.endswith("_affine") for f in fam)
    xy = np.ascontiguousarray(p[:, 0:8])
    got, st = gpu_ctx.batch_ecdh(0, k, xy)
    want, wst = oracle.batch_ecdh(0, k, xy, nthreads=THREADS)
    assert np.array_equal(st, wst) and np.array_equal(got, want), "secp256k1 batch_ecdh crafted keys"
