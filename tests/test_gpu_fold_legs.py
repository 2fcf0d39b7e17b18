"""
GPU tests of every early-out of the cooperative additions (secp::, p256::, ed::padd_coop) that the ordered folds run:
k_fold_sum (multi_scalar_mul, Ecdsa::batch_verify) and k_schnorr_fold_compare (schnorr::batch_verify), both through
fold_coop.  Random products take one early-out only -- "p is the identity" at term 0 -- so the others need chosen terms.

  * Every case of tests/fold_cases.py (its premise is checked on the oracle by tests/test_fold_cases_model.py) through
    fec_debug_fold_terms, which launches multi_scalar_mul's k_fold_sum on the caller's terms: bit-exact against the
    oracle's left-to-right point_add fold, no tolerance.  A failure names the case, its special terms' kinds, indices and
    legs.
  * The same legs through the real callers wherever public inputs can construct them: multi_scalar_mul with a duplicated
    leading (k, P) pair (the doubling at index 1), zero scalars (identity terms) at index 0, in the middle and last, and
    only zero scalars; on P-256 and Ed25519, where multiply(P, 1) == P bit for bit, the cancelling pair P, -P with
    scalars 1 at the start and mid-chain, and the running sum S given again as (1, S) (the doubling mid-chain; on
    Ed25519 an ordinary addition of equal operands).  schnorr::batch_verify on the three curves and Ecdsa::batch_verify on
    secp256k1 and P-256 with two identical leading signatures of identical weight (both folds double at index 1) and a
    zero weight in the middle (an identity term).  Expectations are the oracle's restatements of the same callers.

Only the hook reaches: the secp256k1 cancel leg (u1 == u2, s1 != s2) and a doubling on secp256k1 after index 1 -- there
multiply(P, 1) != P, and negating y of an input does not negate the product, so no public input makes a product equal or
opposite to a running sum the caller does not control; likewise every leg on a non-canonical or all-zero identity term
(the products' identities are the canonical one), P-256's near miss ueq_general, and Ed25519's idq-with-opposite step.
"""
import numpy as np
import pytest

import fold_cases as FC
import vectors as V
from test_fold_cases_model import flags, leg

pytestmark = pytest.mark.gpu

CURVES = (FC.SECP, FC.P256, FC.ED)
ONE = np.array([1, 0, 0, 0], dtype=np.uint64)


@pytest.mark.parametrize("curve", CURVES)
def test_hook_folds_every_case_of_the_table_bit_exactly(gpu_ctx, oracle, curve):
    table = FC.cases(oracle, curve)
    bad = []
    for c in table:
        assert len(c.terms) <= 65
        got = gpu_ctx.debug_fold_terms(curve, c.terms)
        if not np.array_equal(got, c.expect):
            bad.append(c.describe())
    assert not bad, "%d of %d cases differ from the oracle's fold:\n%s" % (len(bad), len(table), "\n".join(bad))
    gpu_ctx.check()


@pytest.mark.parametrize("curve", CURVES)
def test_hook_edges(gpu_ctx, oracle, curve):
    """n == 0 gives the identity; one term is that term (idp); the hook is multi_scalar_mul's fold: the same sum from the
    oracle's products as from the call itself; a multi-device ctx runs it on its first device."""
    import forge_ec_amd as F
    pl = oracle.POINT_LIMBS[curve]
    assert np.array_equal(gpu_ctx.debug_fold_terms(curve, np.zeros((0, pl), dtype=np.uint64)), oracle.identity(curve))
    k, p = V.scalars(7, curve, 6301), V.points(7, curve, 6302)
    prods = oracle.batch_mul(curve, k, p)
    assert np.array_equal(gpu_ctx.debug_fold_terms(curve, prods[:1]), prods[0])
    want = FC.fold(oracle, curve, prods)
    assert np.array_equal(gpu_ctx.debug_fold_terms(curve, prods), want)
    assert np.array_equal(gpu_ctx.multi_scalar_mul(curve, k, p), want)
    c = next(c for c in FC.cases(oracle, curve) if c.name == "cancel_then_ident")
    with F.Context(devices=[0, 0]) as multi:
        assert np.array_equal(multi.debug_fold_terms(curve, c.terms), c.expect)


def _legs_of(oracle, curve, terms):
    f, acc, out = FC.Field(oracle, curve), oracle.identity(curve), []
    for t in terms:
        out.append(leg(curve, flags(f, curve, acc, t)))
        acc = oracle.point_add(curve, acc, t)
    return out, acc


def _msm(gpu_ctx, oracle, curve, k, p, want_legs, what):
    """multi_scalar_mul against the oracle's products folded by the oracle's Add; the fold takes the legs the inputs are for"""
    k, p = np.ascontiguousarray(k), np.ascontiguousarray(p)
    prods = oracle.batch_mul(curve, k, p)
    legs, want = _legs_of(oracle, curve, prods)
    for i, l in want_legs.items():
        assert legs[i] == l, "%s %s: step %d takes %s, not %s" % (FC.NAMES[curve], what, i, legs[i], l)
    got = gpu_ctx.multi_scalar_mul(curve, k, p)
    assert np.array_equal(got, want), "%s multi_scalar_mul %s (legs %s)" % (FC.NAMES[curve], what, legs)
    return prods, want


@pytest.mark.parametrize("curve", CURVES)
def test_multi_scalar_mul_duplicates_and_zero_scalars(gpu_ctx, oracle, curve):
    same = "none" if curve == FC.ED else "double"   # Ed25519's Add has no doubling branch
    k, p = V.scalars(16, curve, 6311), V.points(16, curve, 6312)
    k[1], p[1] = k[0], p[0]
    _msm(gpu_ctx, oracle, curve, k[:2], p[:2], {0: "idp", 1: same}, "[T, T]")
    _msm(gpu_ctx, oracle, curve, k[:5], p[:5], {1: same, 2: "none"}, "[T, T, ...]")
    k[1] = V.scalars(1, curve, 6313)[0]
    for idx in ([0], [8], [15], [0, 1, 8, 9, 15]):
        kz = k.copy()
        kz[idx] = 0
        want = {i: ("idq" if i and not (i == 1 and 0 in idx) else "idp") for i in idx}
        _msm(gpu_ctx, oracle, curve, kz, p, want, "zero scalars at %s" % idx)
    _, s = _msm(gpu_ctx, oracle, curve, np.zeros((3, 4), dtype=np.uint64), p[:3], {0: "idp", 1: "idp", 2: "idp"}, "only zero scalars")
    assert np.array_equal(s, oracle.identity(curve))
    gpu_ctx.check()


@pytest.mark.parametrize("curve", (FC.P256, FC.ED))
def test_multi_scalar_mul_unit_scalars_cancel_and_double(gpu_ctx, oracle, curve):
    """multiply(P, 1) == P bit for bit on P-256 and Ed25519: a point given with scalar 1 IS the term"""
    f = FC.Field(oracle, curve)
    cancel = "opposite" if curve == FC.ED else "cancel"
    same = "none" if curve == FC.ED else "double"

    def negated(pt):
        c = FC.coords(curve, pt)
        return FC.point(f.neg(c[0]), c[1], c[2], f.neg(c[3])) if curve == FC.ED else FC.point(c[0], f.neg(c[1]), c[2])

    k = V.scalars(6, curve, 6321)
    p = oracle.batch_mul_fixed(curve, V.scalars(6, curve, 6322), oracle.generator(curve))   # points of the curve, Z != 1
    assert np.array_equal(oracle.multiply(curve, p[0], ONE), p[0])
    # the pair P, -P with scalars 1 at the start, ordinary terms after it; then the pair alone (the cancel last)
    kk, pp = k.copy(), p.copy()
    kk[0], kk[1], pp[1] = ONE, ONE, negated(p[0])
    _msm(gpu_ctx, oracle, curve, kk, pp, {1: cancel, 2: "idp", 3: "none"}, "P, -P, ...")
    _, s = _msm(gpu_ctx, oracle, curve, kk[:2], pp[:2], {1: cancel}, "P, -P")
    assert np.array_equal(s, oracle.identity(curve))
    # mid-chain: the running sum S of the first three products, then (1, -S), and (1, S)
    running = FC.fold(oracle, curve, oracle.batch_mul(curve, k[:3], p[:3]))
    for term, want, what in ((negated(running), cancel, "(1, -S)"), (running, same, "(1, S)")):
        kk, pp = k.copy(), p.copy()
        kk[3], pp[3] = ONE, term
        _msm(gpu_ctx, oracle, curve, kk, pp, {3: want, 4: "idp" if want == cancel else "none"}, what + " mid-chain")
        _msm(gpu_ctx, oracle, curve, kk[:4], pp[:4], {3: want}, what + " last")
    gpu_ctx.check()


def _pairs(n, curve, seed):
    return np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, seed), V.field_elements(n, curve, seed + 1)], axis=1))


N_SIG = 9


def _duplicate_and_zero(arrays, a):
    """signature 1 = signature 0 with the same weight; weight 4 is zero"""
    for x in arrays:
        x[1] = x[0]
    a[1] = a[0]
    a[4] = 0


@pytest.mark.parametrize("curve", CURVES)
def test_schnorr_batch_verify_duplicate_signatures_and_zero_weight(gpu_ctx, oracle, curve):
    """Both folds (A_i = multiply(G, s_i a_i), B_i = multiply(R_i + e_i P_i, a_i)) add a term to an equal running sum at
    index 1 and meet an identity term at index 4."""
    pk, r = _pairs(N_SIG, curve, 6331), _pairs(N_SIG, curve, 6333)
    s, a, e = V.scalars(N_SIG, curve, 6335), V.scalars(N_SIG, curve, 6336), V.scalars(N_SIG, curve, 6337)
    _duplicate_and_zero((pk, r, s, e), a)
    what = "%s schnorr batch_verify" % FC.NAMES[curve]
    if curve == FC.ED:
        want, w_sides, w_inf, w_dbg = oracle.ed25519_schnorr_batch_verify(pk, None, r, None, s, a, e)
        got, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, a, e)
        assert (got, dbg) == (want, bool(w_dbg)), what
        assert np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf), what
    else:
        want, w_sides, w_inf = oracle.schnorr_batch_verify(curve, pk, None, r, None, s, a, e)
        if curve == FC.SECP:
            got, sides, sinf = gpu_ctx.schnorr_batch_verify_secp256k1(pk, r, s, a, e)
            assert got == (want == 1) and np.array_equal(sides, w_sides), what
    got, sides, sinf = gpu_ctx.schnorr_batch_verify(curve, pk, r, s, a, e)
    assert np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf), what + " (generic entry point)"
    assert got == (want == 1) and w_sides.any(), what
    # the A fold restated: its terms are multiples of the generator, so the legs can be named here
    mul = oracle.ed25519_scalar_mul_release if curve == FC.ED else (oracle.secp256k1_scalar_op if curve == FC.SECP else oracle.p256_scalar_op)
    sa = np.array([(mul(s[i], a[i])[0] if curve == FC.ED else mul("mul", s[i], a[i])[0]) for i in range(N_SIG)], dtype=np.uint64)
    legs, _ = _legs_of(oracle, curve, oracle.batch_mul_fixed(curve, sa, oracle.generator(curve)))
    assert legs[1] == ("none" if curve == FC.ED else "double") and legs[4] == "idq", legs
    gpu_ctx.check()


@pytest.mark.parametrize("curve", (FC.SECP, FC.P256))
def test_ecdsa_batch_verify_duplicate_signatures_and_zero_weight(gpu_ctx, oracle, curve):
    """The fold of a_i (u1_i G + u2_i Q_i).  (On secp256k1 the reference's scalar arithmetic makes many of these terms the
    identity -- random batches meet idp and idq there all the time; the seed is one of those, 17 of 40 tried, whose term 0
    is finite.)  The premise is read off the oracle's sums of the batch's prefixes: the sum of two terms is double(the
    sum of one), and term 4 changes nothing."""
    seed = 6430
    rng = np.random.default_rng(seed)
    dg = rng.integers(0, 256, size=(N_SIG, 32), dtype=np.uint8)
    dg[:, 0] &= 0x7F
    r, s, a = V.scalars(N_SIG, curve, seed + 1), V.scalars(N_SIG, curve, seed + 2), V.scalars(N_SIG, curve, seed + 3)
    pk = _pairs(N_SIG, curve, seed + 4)
    _duplicate_and_zero((dg, r, s, pk), a)
    what = "%s ecdsa_batch_verify" % FC.NAMES[curve]
    sums = {}
    for n in (1, 2, 4, 5, N_SIG):   # the prefixes too go through the kernel: the early-out in the last iteration
        want, wd = oracle.ecdsa_batch_verify(curve, dg[:n], r[:n], s[:n], pk[:n], None, a[:n])
        got, gd = gpu_ctx.ecdsa_batch_verify(curve, dg[:n], r[:n], s[:n], pk[:n], None, a[:n])
        assert np.array_equal(gd, wd), "%s n=%d: r_sum, scalar sum" % (what, n)
        assert got == want, (what, n)
        sums[n] = wd[:12]
    assert not oracle.is_identity(curve, sums[1]) and np.array_equal(sums[2], oracle.point_double(curve, sums[1]))   # the doubling at index 1
    assert not oracle.is_identity(curve, sums[4]) and np.array_equal(sums[5], sums[4])                              # idq at index 4
    assert not np.array_equal(sums[N_SIG], sums[5])
    gpu_ctx.check()
