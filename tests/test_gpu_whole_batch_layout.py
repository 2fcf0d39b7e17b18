"""
GPU tests of the three calls that stage a whole batch at once -- fec_multi_scalar_mul, fec_ecdsa_batch_verify and
schnorr_batch_verify -- at the smallest shapes where their device layout can go wrong: the inputs side by side in one
staging slot, the products and the result record (sums, sides, flags, counter, wrapped byte) in another.  Against the CPU
oracle, as tests/test_gpu_parity.py; tests/test_gpu_size_regimes.py has the same calls above the size thresholds.
"""
import numpy as np
import pytest

import vectors as V
from test_gpu_size_regimes import NAMES, _pairs, _same

pytestmark = pytest.mark.gpu

ONE = np.array([1, 0, 0, 0], dtype=np.uint64)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_multi_scalar_mul_small_chunks(oracle, curve):
    """n = 0 (the fold of nothing), 1, and 130 in chunks of 64: three chunks, a short last one, each product at its offset."""
    import forge_ec_amd as F
    k, p = V.scalars(130, curve, 7100 + curve), V.points(130, curve, 7110 + curve)
    k[5] = 0
    p[7] = oracle.identity(curve)
    prods = oracle.batch_mul(curve, k, p)
    with F.Context(0) as ctx:
        ctx.set_chunk(64)
        for n in (0, 1, 130):
            acc = oracle.identity(curve)
            for i in range(n):
                acc = oracle.point_add(curve, acc, prods[i])
            _same(ctx.multi_scalar_mul(curve, k[:n], p[:n]), acc, "%s multi_scalar_mul n=%d chunk=64" % (NAMES[curve], n))
        ctx.check()


@pytest.mark.parametrize("curve", [0, 1])
def test_ecdsa_batch_verify_small(gpu_ctx, oracle, curve):
    """n = 1 and 3: the folded sums of the result record; a signature that fails at index 1 (r = 0: the early return, and a
    digest the reference panics on) decides before anything is folded."""
    rng = np.random.default_rng(7200 + curve)
    for n in (1, 3):
        dg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        dg[:, 0] &= 0x7F
        r, s, a = V.scalars(n, curve, 7201 + n), V.scalars(n, curve, 7202 + n), V.scalars(n, curve, 7203 + n)
        pk = _pairs(n, curve, 7204 + n)
        cases = [("random", dg, r, None), ("first key at infinity", dg, r, np.array([1] + [0] * (n - 1), dtype=np.uint8))]
        if n == 3:
            r0, dg2 = r.copy(), dg.copy()
            r0[1] = 0
            dg2[1] = 0xFF
            cases += [("r = 0 at 1", dg, r0, None), ("digest panic at 1", dg2, r, None), ("r = 0 at 1, digest panic at 2", np.roll(dg2, 1, axis=0), r0, None)]
        for label, d_, r_, inf in cases:
            want, wd = oracle.ecdsa_batch_verify(curve, d_, r_, s, pk, inf, a)
            got, gd = gpu_ctx.ecdsa_batch_verify(curve, d_, r_, s, pk, inf, a)
            _same(gd, wd, "%s ecdsa_batch_verify n=%d (%s): r_sum, scalar sum" % (NAMES[curve], n, label))
            assert got == want, (NAMES[curve], n, label)
            assert wd.any() == label.startswith(("random", "first"))   # an early return leaves no sums
    gpu_ctx.check()


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_schnorr_batch_verify_small(gpu_ctx, oracle, curve):
    """n = 1 and 3: both sums, the affine sides and their flags; Ed25519 also with and without the wrapped byte (weights of 1
    wrap nothing; s_0 and a_0 with three low limbs of all ones do: the column i + j = 2 of s_0 * a_0 adds three products of
    (2^64 - 1)^2, more than a u128 holds)."""
    ones = np.array([0xFFFFFFFFFFFFFFFF] * 3 + [0x0FFFFFFFFFFFFFFF], dtype=np.uint64)
    for n in (1, 3):
        pk, r = _pairs(n, curve, 7300 + n), _pairs(n, curve, 7302 + n)
        s, a, e = V.scalars(n, curve, 7304 + n), V.scalars(n, curve, 7305 + n), V.scalars(n, curve, 7306 + n)
        s1, a1 = s.copy(), a.copy()
        s1[0] = a1[0] = ones
        for label, s_, a_, wraps in (("random weights", s, a, None), ("weights of 1", s, np.tile(ONE, (n, 1)), False), ("all-ones limbs", s1, a1, True)):
            what = "%s schnorr batch_verify n=%d (%s)" % (NAMES[curve], n, label)
            if curve == 2:
                want, w_sides, w_inf, w_dbg = oracle.ed25519_schnorr_batch_verify(pk, None, r, None, s_, a_, e)
                got, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s_, a_, e)
                assert (got, dbg) == (want, bool(w_dbg)), what
                assert wraps is None or dbg == wraps, what
            else:
                want, w_sides, w_inf = oracle.schnorr_batch_verify(curve, pk, None, r, None, s_, a_, e)
                got, sides, sinf = gpu_ctx.schnorr_batch_verify(curve, pk, r, s_, a_, e)
                assert got == (want == 1), what
            _same(sides, w_sides, what + ": affine sides")
            _same(sinf, w_inf, what + ": sides' infinity flags")
            assert w_sides.any()
        # an identity input at index n - 1 rejects before anything is staged: no sides
        flags = np.array([0] * (n - 1) + [1], dtype=np.uint8)
        got, sides, sinf = gpu_ctx.schnorr_batch_verify(curve, pk, r, s, a, e, r_inf=flags)
        assert got is False and not sides.any() and not sinf.any()
    gpu_ctx.check()
