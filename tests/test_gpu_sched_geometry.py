"""
The persistent scheduler kernels (k_p256_mul_sched in its variable-base 864- and 1 024-slot forms and its fixed-base
form, k_ed_mul_pers<864|1024>) at launch geometries the device's own CU count never produces: refills of a slot, both
slot counts at one to five fills, short last ranges, ring F past the wrap of its lap tag, scalars that load one ring
only, and the CU splits of the composed callers on small chips.  fec_ctx_debug_set_cus sizes a ctx's scheduler launches
for fewer CUs than the device has (fewer workgroups than CUs is always safe: they do not depend on each other), so a
workgroup owns thousands of elements in a batch of a few thousand.

Every test makes a ctx of its own (the shared gpu_ctx keeps its geometry), compares every element bit-exactly with the
C oracle, asks ctx.check() for a clean device error word, and asserts through tests/sched_geometry.py -- the Python
mirror of the launch rules, pinned against the real headers by tests/test_sched_launch_rules.py -- that the case lands
in the kernel form and fill count its name claims.  A broken ring does not hang: the kernels' watchdogs zero-fill the
outputs and the call (or check()) raises FEC_E_LAUNCH, which fails the test.
"""
import time

import numpy as np
import pytest

import sched_geometry as G
import vectors as V
from forcing_cases import cases as forcing_cases

pytestmark = pytest.mark.gpu

THREADS = 16
NAMES = {1: "P-256", 2: "Ed25519"}
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
ONE = np.array([1, 0, 0, 0], dtype=np.uint64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, first at %s" % (what, len(bad), got.shape[0], list(bad[:8])))


def _shape(cus, n, fixed=False, cu_divisor=1):
    assert (cus, cu_divisor, n) in G.PINNED, "not among the points the mirror is pinned at: %r" % ((cus, cu_divisor, n),)
    return G.shape(cus, n, fixed=fixed, cu_divisor=cu_divisor)


class _Clock:
    """oracle and GPU seconds of a test, printed with its geometry (pytest -s shows the lines)"""

    def __init__(self):
        self.oracle = self.gpu = 0.0

    def ref(self, fn, *a):
        t = time.perf_counter()
        r = fn(*a, nthreads=THREADS)
        self.oracle += time.perf_counter() - t
        return r

    def run(self, fn, *a):
        t = time.perf_counter()
        r = fn(*a)
        self.gpu += time.perf_counter() - t
        return r

    def report(self, what, *shapes):
        geo = "; ".join("cus %d n %d per_wg %d %d slots %d fills" % (s.cus, s.n, s.per_wg, s.slots, s.fills) for s in shapes)
        print("\nGEOMETRY %s | %s | oracle %.2f s, GPU calls %.2f s" % (what, geo, self.oracle, self.gpu))


def _ctx(cus, prefix_bits=0):
    """a ctx of its own sized for `cus` CUs; fixed-base prefix tables off, or (None) left to the ctx's defaults"""
    import forge_ec_amd as F
    ctx = F.Context(0)
    try:
        ctx.debug_set_cus(cus)
        if prefix_bits is not None:
            ctx.set_fixed_prefix_bits(prefix_bits)
    except Exception:
        ctx.close()
        raise
    return ctx


def _identity(curve):
    return np.array([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0] if curve == 1 else [0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0],
                    dtype=np.uint64)


def _in_claim(curve, k, p=None):
    """the elements claim() answers by itself, which never enter a ring: a zero scalar, the identity point, and in the
    P-256 kernel the scalar 1 (p: None for a fixed base that is not the identity)"""
    m = ~k.any(axis=1)
    if curve == 1:
        m |= (k == ONE).all(axis=1)
        if p is not None:
            m |= ~p[:, 8:12].any(axis=1)
    elif p is not None:
        m |= (p == _identity(2)).all(axis=1)
    return m


def _limbs(values):
    return np.array([V.limbs_of(int(v)) for v in values], dtype=np.uint64)


# ---- a. forms and fills ------------------------------------------------------------------------------------------------

# n on two CUs -> the form and the fills of the variable-base kernel: per_wg 701, 1 001, 1 701, 2 001, 2 591, 3 501
A_SIZES = [(1401, False, 1), (2001, True, 1), (3401, False, 2), (4001, True, 2), (5181, False, 3), (7001, False, 5)]


def _forms_and_fills(oracle, curve, cus, n, what, var_shape, fixed_shape):
    clock = _Clock()
    k, p = V.scalars(n, curve, 7100 + curve), V.points(n, curve, 7110 + curve)
    k[[5, n - 3]] = 0
    k[[6, n - 2]] = ONE
    p[[7, n - 4]] = _identity(curve)
    g, base = oracle.generator(curve), V.points(1, curve, 7120 + curve)[0]
    assert base[8:12].any() and list(base[8:12]) != [1, 0, 0, 0]          # projective, z != 1
    want_var = clock.ref(oracle.batch_mul, curve, k, p)
    want_g = clock.ref(oracle.batch_mul_fixed, curve, k, g)
    want_base = clock.ref(oracle.batch_mul_fixed, curve, k, base)
    ctx = _ctx(cus)
    try:
        _same(clock.run(ctx.batch_mul, curve, k, p), want_var, what + " variable base")
        _same(clock.run(ctx.batch_mul_fixed, curve, k, g), want_g, what + " fixed base G, no prefix table")
        _same(clock.run(ctx.batch_mul_fixed, curve, k, base), want_base, what + " fixed projective base")
        assert ctx.fixed_prefix_bits(curve) == 0
        ctx.set_fixed_prefix_bits(7)                   # 128 entries: a slot starts at step 7 of its ladder, refilled ones too
        _same(clock.run(ctx.batch_mul_fixed, curve, k, g), want_g, what + " fixed base G, 7-bit prefix table")
        assert ctx.fixed_prefix_bits(curve) == 7
        ctx.check()
    finally:
        ctx.close()
    clock.report(what, var_shape, fixed_shape)


@pytest.mark.parametrize("curve", [1, 2])
@pytest.mark.parametrize("n, wide, fills", A_SIZES)
def test_forms_and_fills_on_two_cus(oracle, curve, n, wide, fills):
    """Variable base in the form and fill count of the table above; fixed base (P-256: the scheduler's fixed-base form,
    always 864 slots; Ed25519: its table kernels, which no CU count sizes) from the generator without and with a small
    prefix table and from a projective base.  n is odd: the second range is one element short."""
    s, sf = _shape(2, n), _shape(2, n, fixed=True)
    assert (s.grid, s.wide, s.fills) == (2, wide, fills) and s.slots == (1024 if wide else 864)
    assert s.ranges[1][1] - s.ranges[1][0] == s.per_wg - 1
    assert not sf.wide and sf.fills == -(-s.per_wg // 864)
    _forms_and_fills(oracle, curve, 2, n, "%s n=%d on 2 CUs (%d slots, %d fills)" % (NAMES[curve], n, s.slots, fills), s, sf)


@pytest.mark.parametrize("curve", [1, 2])
def test_last_workgroup_owns_less_than_a_claim(oracle, curve):
    """100 CUs, 14 901 elements: 99 ranges of 150 and a last one of 51 -- less than one 64-element claim."""
    s = _shape(100, 14901)
    lo, hi = s.ranges[-1]
    assert (s.grid, s.per_wg, hi - lo) == (100, 150, 51)
    _forms_and_fills(oracle, curve, 100, 14901, "%s n=14901 on 100 CUs (last range 51)" % NAMES[curve], s, _shape(100, 14901, fixed=True))


# ---- b. a reused slot carries nothing over -----------------------------------------------------------------------------

def _base_kinds(curve, k, p, s, seed):
    """Bases by kind -- P-256: projective, affine (z = 1: bit 15 of the slot's step word, the twelve-product addition),
    affine with x or y >= p (all-ones top word: the addition's general body); Ed25519: projective, z = 1, x = 0 (its
    doubling's rare exit) -- in blocks of 64 and singly by turns of 512, per range: whatever order the rings hand slots
    out in, a slot sees every kind after every other."""
    raw = V.splitmix64(8 * p.shape[0], V.SEED, seed).reshape(-1, 8)
    for lo, hi in s.ranges:
        rel = np.arange(hi - lo)
        kind = np.where((rel // 512) % 2 == 0, (rel // 64) % 3, rel % 3)
        idx = lo + rel
        aff, odd = idx[kind >= 1], idx[kind == 2]
        p[aff, 8:12] = ONE
        if curve == 1:
            p[odd[0::2], 3] = raw[odd[0::2], 3] | np.uint64(0xFFFFFFFF00000002)      # x >= p
            p[odd[1::2], 7] = raw[odd[1::2], 7] | np.uint64(0xFFFFFFFF00000002)      # y >= p
        else:
            p[odd, 0:4] = 0
            p[odd[0::2], 12:16] = 0
            p[odd[1::3], 8:12] = p[odd[1::3], 4:8]                                   # y == z, t != 0: not the identity


def _crafted_at_reused_positions(curve, k, p, s):
    """the curve's forcing cases at range-relative positions >= 1 024 -- slots in their second or later occupancy in
    either form -- among them lo + 1 024 and the last element of every range; and at lo and lo + 864 (the first element
    of a range, and the first refill of the 864-slot form).  Returns (indices, fixture results)."""
    fk, fp, fe, fam = forcing_cases(curve)
    m = len(fk)
    at, rel = [], []
    for lo, hi in s.ranges:
        assert hi - lo > 1500 + 2 * m
        r = sorted(set([0, 864] + list(range(1024, 1024 + m)) + list(range(1500, hi - lo - m, 97)) + list(range(hi - lo - m, hi - lo))))
        at += [lo + x for x in r]
        rel += r
    at, rel = np.array(at), np.array(rel)
    idx = np.arange(at.size) % m
    assert {fam[i] for i in idx[rel >= 1024]} == set(fam) and (np.bincount(idx[rel >= 1024], minlength=m) >= 2).all()
    k[at], p[at] = fk[idx], fp[idx]
    return at, fe[idx]


def _rare_bases_at_reused_positions(curve, k, p, s):
    """P-256: the self-doubling base (0, 2^63, z), on which the ladder's addition finds equal points; Ed25519: points with
    x = 0 -- at range-relative positions >= 1 024, every 53rd."""
    j = 0
    for lo, hi in s.ranges:
        for i in range(lo + 1100, hi - 40, 53):
            if curve == 1:
                p[i] = np.array([0, 0, 0, 0] + V.limbs_of(1 << 63) + V.limbs_of(1 + 977 * j), dtype=np.uint64)
                if j % 3 == 0:
                    k[i] = V.limbs_of(3 + 4 * j)
            else:
                y = V.field_elements(1, 2, 7290 + j)[0]
                pt = np.zeros(16, dtype=np.uint64)
                pt[4:8] = y
                pt[8:12] = y if j % 3 == 0 else ONE
                if j % 2:
                    pt[12:16] = V.limbs_of(7 + j)
                p[i] = pt
                if j % 4 == 0:
                    k[i] = V.limbs_of(1 + 2 * j)
            j += 1
    assert j >= 20


@pytest.mark.parametrize("curve", [1, 2])
@pytest.mark.parametrize("n, wide, fills", [(7001, False, 5), (4001, True, 2)])
def test_reused_slots_carry_nothing_over(oracle, curve, n, wide, fills):
    """Everything a slot keeps between two elements -- the z == 1 flag in bit 15 of lds_step, z2z2 in lds_zq, the scalar
    in lds_k (or, with 1 024 slots, read back from the caller's array through lds_gid), the Ed25519 addend -- must be
    the new element's: bases of three kinds by turns, and every crafted rare-leg input, which so far only ever ran in
    a slot's first occupancy, in a reused slot."""
    clock = _Clock()
    s = _shape(2, n)
    assert (s.grid, s.wide, s.fills) == (2, wide, fills) and (wide or s.per_wg >= 3 * 864)
    k, p = V.scalars(n, curve, 7200 + curve), V.points(n, curve, 7210 + curve)
    _base_kinds(curve, k, p, s, 7220 + curve)
    _rare_bases_at_reused_positions(curve, k, p, s)
    at, expect = _crafted_at_reused_positions(curve, k, p, s)
    want = clock.ref(oracle.batch_mul, curve, k, p)
    what = "%s n=%d on 2 CUs (%d slots, %d fills), mixed base kinds" % (NAMES[curve], n, s.slots, fills)
    ctx = _ctx(2)
    try:
        got = clock.run(ctx.batch_mul, curve, k, p)
        ctx.check()
    finally:
        ctx.close()
    _same(got[at], expect, what + ": crafted elements vs fixture")
    _same(got, want, what + " vs oracle")
    clock.report(what, s)


# ---- c. skewed scalars through refills ---------------------------------------------------------------------------------

C_N = 7001
PATTERNS = ["all_ones", "powers_of_two", "few_bits", "long_then_short", "short_then_long", "one_long_among_twos",
            "runs_answered_in_claim", "a_range_of_nothing_else"]


def _skewed(pattern, curve, s, fixed):
    """(scalars, points) of one batch; elements answered inside claim() are zero scalars, identity points (variable
    base) and, for P-256, scalars equal to 1"""
    n = s.n
    rng = np.random.default_rng(7300 + len(pattern))
    k, p = V.scalars(n, curve, 7310 + curve), V.points(n, curve, 7320 + curve)
    inside = [np.zeros(4, dtype=np.uint64)] + ([ONE] if curve == 1 else []) + ([] if fixed else [None])   # None: identity point

    def answered(lo, count, turn):          # `count` consecutive elements of one kind from lo on
        kind = inside[turn % len(inside)]
        if kind is None:
            p[lo:lo + count] = _identity(curve)
        else:
            k[lo:lo + count] = kind

    if pattern == "all_ones":               # every step an addition: ring A alone
        k[:] = ALL_ONES
    elif pattern == "powers_of_two":        # P-256: one addition, then ring D alone; Ed25519: ring D but for one step
        e = (np.arange(n) * 37) % 256
        k[:] = 0
        k[np.arange(n), e // 64] = np.uint64(1) << (e % 64).astype(np.uint64)
    elif pattern == "few_bits":             # P-256: one to seven steps per element, ring F churns
        k[:] = _limbs(rng.choice([2, 3, 5, 255], size=n))
    elif pattern in ("long_then_short", "short_then_long"):
        for lo, hi in s.ranges:
            mid = (lo + hi) // 2
            a, b = (mid, hi) if pattern == "long_then_short" else (lo, mid)
            k[a:b] = _limbs(rng.choice([2, 3], size=b - a))
    elif pattern == "one_long_among_twos":  # one full ladder left alone in the tail of each range
        lone = [hi - 5 for _, hi in s.ranges]
        keep = k[lone] | np.array([0, 0, 0, 1 << 63], dtype=np.uint64)
        k[:] = _limbs([2])[0]
        k[lone] = keep
    elif pattern == "runs_answered_in_claim":   # runs of 200 at the start, in the middle and at the end of a range
        (lo0, hi0), (lo1, hi1) = s.ranges
        for t, lo in enumerate([lo0, lo0 + 200, lo0 + 400, lo0 + 1500, lo0 + 1700, lo0 + 1900, lo1 + 1400, lo1 + 1600, lo1 + 1800,
                                hi1 - 600, hi1 - 400, hi1 - 200]):
            answered(lo, 200, t)
    elif pattern == "a_range_of_nothing_else":  # every slot of the first workgroup dies in its first claim
        lo, hi = s.ranges[0]
        for t, at in enumerate(range(lo, hi, 200)):
            answered(at, min(200, hi - at), t)
    else:
        raise ValueError(pattern)
    return k, p


# (a scalar of few bits is a short ladder in the P-256 kernel only: Ed25519 takes 256 steps whatever the scalar)
C_CASES = [(curve, fixed, pattern) for curve, fixed in [(1, False), (1, True), (2, False)] for pattern in PATTERNS
           if curve == 1 or pattern != "few_bits"]


@pytest.mark.parametrize("curve, fixed, pattern", C_CASES)
def test_skewed_scalars_through_refills(oracle, curve, fixed, pattern):
    """The pop policy (ring F first, then the fuller of D and A, the tail threshold) with scalars that are not half ones,
    through five fills of 864 slots."""
    clock = _Clock()
    s = _shape(2, C_N, fixed=fixed)
    assert (s.grid, s.wide, s.fills, s.per_wg) == (2, False, 5, 3501)
    k, p = _skewed(pattern, curve, s, fixed)
    inside = _in_claim(curve, k, None if fixed else p)
    per_range = [int(inside[lo:hi].sum()) for lo, hi in s.ranges]
    if pattern == "runs_answered_in_claim":
        assert per_range == [1200, 1200]
    elif pattern == "a_range_of_nothing_else":
        assert per_range[0] == s.per_wg and per_range[1] < 5       # the first workgroup's rings D and A stay empty
    else:
        assert sum(per_range) <= (64 if pattern == "powers_of_two" else 4)
    what = "%s %s n=%d on 2 CUs, %s" % (NAMES[curve], "fixed base" if fixed else "variable base", C_N, pattern)
    g = oracle.generator(curve)
    want = clock.ref(oracle.batch_mul_fixed, curve, k, g) if fixed else clock.ref(oracle.batch_mul, curve, k, p)
    ctx = _ctx(2)
    try:
        got = clock.run(ctx.batch_mul_fixed, curve, k, g) if fixed else clock.run(ctx.batch_mul, curve, k, p)
        ctx.check()
    finally:
        ctx.close()
    _same(got, want, what)
    clock.report(what, s)


# ---- d. ring F past its lap wrap ---------------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.mark.parametrize("curve, fixed, n", [(1, False, 40037), (1, True, 40037), (2, False, 34037)])
def test_ring_f_passes_its_lap_wrap(oracle, curve, fixed, n):
    """A ring entry carries its lap modulo 32, and ring F takes one entry per finished element: in ONE workgroup of the
    864-slot forms (1 024 ring positions) its tag wraps at position 32 768.  One CU, one launch through the *_dev call;
    more than 32 768 elements of the one range go through the rings (the handful claim() answers do not count).  P-256:
    half of the scalars are 2 or 3 (a step or two each), so the wrap comes after a quarter of the ladder work."""
    import torch
    clock = _Clock()
    s = _shape(1, n, fixed=fixed)
    assert (s.grid, s.wide, s.slots, s.per_wg) == (1, False, 864, n)
    limbs = V.POINT_LIMBS[curve]
    k, p = V.scalars(n, curve, 7400 + curve), V.points(n, curve, 7410 + curve)
    if curve == 1:
        rng = np.random.default_rng(7420)
        short = rng.permutation(n)[:n // 2]
        k[short] = _limbs(rng.choice([2, 3], size=short.size))
    k[[11, n - 9]] = 0
    k[[12, n - 8]] = ONE
    if not fixed:
        p[[13, n - 7]] = _identity(curve)
    through_rings = n - int(_in_claim(curve, k, None if fixed else p).sum())
    assert through_rings > 32 * 1024 and through_rings >= n - 6
    what = "%s %s n=%d on 1 CU, one launch" % (NAMES[curve], "fixed base" if fixed else "variable base", n)
    g = oracle.generator(curve)
    want = clock.ref(oracle.batch_mul_fixed, curve, k, g) if fixed else clock.ref(oracle.batch_mul, curve, k, p)
    ctx = _ctx(1)
    try:
        dk, dp = _dev(k), _dev(g if fixed else p)
        out = torch.zeros((n, limbs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        t = time.perf_counter()
        if fixed:
            ctx.batch_mul_fixed_dev(curve, dk.data_ptr(), dp.data_ptr(), out.data_ptr(), n, stream)
        else:
            ctx.batch_mul_dev(curve, dk.data_ptr(), dp.data_ptr(), out.data_ptr(), n, stream)
        torch.cuda.synchronize()
        clock.gpu += time.perf_counter() - t
        ctx.check()
        got = out.cpu().numpy().view(np.uint64)
    finally:
        ctx.close()
    _same(got, want, what)
    clock.report(what, s)


# ---- e. the composed callers on small chips ----------------------------------------------------------------------------

E_CUS = [1, 2, 3, 8, 16, 24, 32]


@pytest.mark.parametrize("curve", [1, 2])
@pytest.mark.parametrize("n", [3000, (1 << 16) + 37])
def test_batch_double_mul_on_small_chips(oracle, curve, n):
    """u1*G + u2*Q: P-256 runs its two scheduler launches side by side, each on its share of the CUs (p256_cu_split: no
    split on one CU, 1 + 2 on three, multiples of eight from sixteen on); Ed25519's scheduler takes every second CU
    beside the table kernel (n <= 2^15).  The device's own count (0), and 10^6, which is clamped to it, come last."""
    clock = _Clock()
    u1, u2, q = V.scalars(n, curve, 7500 + curve), V.scalars(n, curve, 7510 + curve), V.points(n, curve, 7520 + curve)
    u1[[0, n - 1]] = 0
    u2[[1, n - 2]] = 0
    q[[2, n - 3]] = _identity(curve)
    q[::2, 8:12] = ONE                                  # keys that came through from_affine, as in the verifiers
    shapes = []
    for cus in E_CUS:
        if curve == 1:
            cf, cv = G.p256_cu_split(cus, n, G.VAR_MS)
            assert (cf, cv) == {1: (1, 1), 2: (1, 1), 3: (1, 2), 8: (4, 4), 16: (8, 8), 24: (16, 8), 32: (16, 16)}[cus]
            shapes += [_shape(cf, n, fixed=True), _shape(cv, n)]
        else:
            shapes.append(_shape(cus, n, cu_divisor=2 if n <= 1 << 15 else 1))
    assert {sh.fills for sh in shapes} >= ({1, 3} if n == 3000 else {5, 10, 76})
    want = clock.ref(oracle.batch_double_mul, curve, u1, u2, q)
    results = {}
    for cus in E_CUS + [0, 10 ** 6]:
        ctx = _ctx(cus, prefix_bits=None)
        try:
            results[cus] = clock.run(ctx.batch_double_mul, curve, u1, u2, q)
            ctx.check()
        finally:
            ctx.close()
    for cus, got in results.items():
        _same(got, want, "%s batch_double_mul n=%d, debug_set_cus(%d)" % (NAMES[curve], n, cus))
    clock.report("%s batch_double_mul n=%d on %s CUs and the device's own" % (NAMES[curve], n, E_CUS), *shapes)


def test_p256_ecdsa_batch_verify_on_three_cus(oracle):
    """Ecdsa::batch_verify at 4 096 signatures on three CUs: u1*G on one workgroup beside u2*Q on two."""
    clock = _Clock()
    n = 4096
    assert G.p256_cu_split(3, n, G.VAR_AFFINE_MS) == (1, 2) and G.p256_cu_split(3, n, G.VAR_MS) == (1, 2)
    shapes = [_shape(1, n, fixed=True), _shape(2, n)]
    assert [sh.fills for sh in shapes] == [5, 2] and shapes[1].wide
    rng = np.random.default_rng(7600)
    dg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    dg[:, 0] &= 0x7F
    r, s_, a = V.scalars(n, 1, 7601), V.scalars(n, 1, 7602), V.scalars(n, 1, 7603)
    a[[0, n - 1]] = 0
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, 1, 7604), V.field_elements(n, 1, 7605)], axis=1))
    inf = np.zeros(n, dtype=np.uint8)
    inf[[0, 7, n - 2]] = 1
    want, wd = clock.ref(oracle.ecdsa_batch_verify, 1, dg, r, s_, pk, inf, a)
    ctx = _ctx(3, prefix_bits=None)
    try:
        got, gd = clock.run(ctx.ecdsa_batch_verify, 1, dg, r, s_, pk, inf, a)
        ctx.check()
    finally:
        ctx.close()
    _same(gd, wd, "P-256 ecdsa_batch_verify on 3 CUs: r_sum, scalar sum")
    assert got == want and wd.any()
    clock.report("P-256 ecdsa_batch_verify n=4096 on 3 CUs", *shapes)


def test_ed25519_schnorr_batch_verify_on_three_cus(oracle):
    """schnorr::batch_verify for Ed25519 at 4 096 signatures on three CUs."""
    clock = _Clock()
    n = 4096
    shapes = [_shape(3, n)]                             # (the scheduler launches follow each other: no share of the CUs)
    assert [(sh.grid, sh.wide, sh.fills) for sh in shapes] == [(3, False, 2)]
    pairs = lambda seed: np.ascontiguousarray(np.concatenate([V.field_elements(n, 2, seed), V.field_elements(n, 2, seed + 1)], axis=1))
    pk, r = pairs(7700), pairs(7702)
    s_, a, e = V.scalars(n, 2, 7704), V.scalars(n, 2, 7705), V.scalars(n, 2, 7706)
    a[[2, n - 3]] = 0
    a[100:200] = ONE
    want, w_sides, w_inf, w_dbg = clock.ref(oracle.ed25519_schnorr_batch_verify, pk, None, r, None, s_, a, e)
    ctx = _ctx(3, prefix_bits=None)
    try:
        got, sides, sinf, dbg = clock.run(ctx.schnorr_batch_verify_ed25519, pk, r, s_, a, e)
        ctx.check()
    finally:
        ctx.close()
    _same(sides, w_sides, "Ed25519 schnorr batch_verify on 3 CUs: affine sides")
    _same(sinf, w_inf, "Ed25519 schnorr batch_verify on 3 CUs: sides' infinity flags")
    assert (got, dbg) == (want, bool(w_dbg)) and w_sides.any()
    clock.report("Ed25519 schnorr_batch_verify n=4096 on 3 CUs", *shapes)


@pytest.mark.parametrize("curve", [1, 2])
def test_multi_device_ctx_hands_the_cu_count_to_its_shard_workers(oracle, curve):
    """A [0, 0] ctx with two CUs: each shard worker runs its half on two workgroups of 1 750 (the 1 024-slot form, two
    fills), where the single ctx it is compared with runs two workgroups of 3 501 (864 slots, five fills)."""
    import forge_ec_amd as F
    clock = _Clock()
    n = C_N
    shapes = [_shape(2, n // 2), _shape(2, n - n // 2)]
    assert [(sh.grid, sh.wide, sh.fills) for sh in shapes] == [(2, True, 2), (2, True, 2)]
    k, p = V.scalars(n, curve, 7800 + curve), V.points(n, curve, 7810 + curve)
    want = clock.ref(oracle.batch_mul, curve, k, p)
    ctx = F.Context(devices=[0, 0])
    try:
        ctx.debug_set_cus(2)
        got = clock.run(ctx.batch_mul, curve, k, p)
        ctx.check()
    finally:
        ctx.close()
    _same(got, want, "%s batch_mul n=%d, [0, 0] ctx on 2 CUs" % (NAMES[curve], n))
    one = _ctx(2, prefix_bits=None)
    try:
        _same(clock.run(one.batch_mul, curve, k, p), got, "%s batch_mul n=%d, single ctx on 2 CUs" % (NAMES[curve], n))
        one.check()
    finally:
        one.close()
    clock.report("%s batch_mul n=%d, [0, 0] ctx on 2 CUs" % (NAMES[curve], n), *shapes)
