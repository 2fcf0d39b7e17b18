"""
GPU parity tests: the HIP path (through the C ABI, libfecgpu.so) against the CPU oracle on the
same seeded inputs.  Bit-exact -- integer work, no tolerance.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import numpy as np
import pytest

import vectors as V

pytestmark = pytest.mark.gpu

CURVES = [0, 1, 2]
NAMES = {0: "secp256k1", 1: "p256", 2: "ed25519"}
F_ADD, F_SUB, F_MUL, F_SQR, F_NEG = 0, 1, 2, 3, 4
P_ADD, P_DOUBLE, P_NEGATE, P_DOUBLE_TRAIT = 0, 1, 2, 3
OPNAME = {F_ADD: "add", F_SUB: "sub", F_MUL: "mul", F_SQR: "sqr", F_NEG: "neg"}


def _oracle_field(oracle, curve, op, a, b=None):
    out = np.empty_like(a)
    for i in range(a.shape[0]):
        out[i] = oracle.field_op(curve, OPNAME[op], a[i], None if b is None else b[i])
    return out


def _assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        i = int(bad[0])
        raise AssertionError("%s: %d/%d rows differ; first at %d\n got  %s\n want %s" % (
            what, len(bad), got.shape[0], i, [hex(int(v)) for v in got[i]], [hex(int(v)) for v in want[i]]))


def _field_operands(curve, n_random):
    """canonical random, arbitrary 256-bit random, and an edge x edge grid."""
    edges = V.edge_field_values(curve)
    ea = np.array([V.limbs_of(x) for x in edges for _ in edges], dtype=np.uint64)
    eb = np.array([V.limbs_of(y) for _ in edges for y in edges], dtype=np.uint64)
    ca = V.field_elements(n_random, curve, 101)
    cb = V.field_elements(n_random, curve, 102)
    ra = V.splitmix64(4 * n_random, V.SEED, 103).reshape(-1, 4)
    rb = V.splitmix64(4 * n_random, V.SEED, 104).reshape(-1, 4)
    # canonical vs arbitrary mixes exercise the reference's non-canonical code paths (P-256 Sub)
    a = np.concatenate([ea, ca, ra, ca, ra])
    b = np.concatenate([eb, cb, rb, rb, cb])
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("op", [F_ADD, F_SUB, F_MUL, F_SQR, F_NEG])
def test_field_ops_match_oracle(gpu_ctx, oracle, curve, op):
    a, b = _field_operands(curve, 4000)
    binary = op in (F_ADD, F_SUB, F_MUL)
    got = gpu_ctx.field_op(curve, op, a, b if binary else None)
    want = _oracle_field(oracle, curve, op, a, b if binary else None)
    _assert_same(got, want, "%s field %s" % (NAMES[curve], OPNAME[op]))


def test_secp256k1_square_ripple_operands(gpu_ctx, oracle):
    """square() operands whose carries ripple past the first limb: the kernel's fast path must fall
    back to the literal routine for the wavefront.  Mixed with ordinary operands so fast and slow
    lanes share wavefronts."""
    import json
    import os
    ops = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                      "secp256k1_sqr_ripple_operands.json")))["operands"]
    rare = np.array(ops, dtype=np.uint64)
    plain = V.field_elements(1000, 0, 881)
    a = np.ascontiguousarray(np.concatenate([rare, plain, rare[:7], plain[:300], rare[40:41]]))
    got = gpu_ctx.field_op(0, F_SQR, a)
    want = _oracle_field(oracle, 0, F_SQR, a)
    _assert_same(got, want, "secp256k1 square with travelling ripples")


def test_field_reference_kats(gpu_ctx):
    """The reference's own unit-test vectors, through the GPU kernels."""
    import json
    import os
    kats = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")))
    for k in kats["field"]:
        a = np.array([k["a"]], dtype=np.uint64)
        b = np.array([k["b"]], dtype=np.uint64) if k.get("b") is not None else None
        op = {"add": F_ADD, "sub": F_SUB, "mul": F_MUL, "sqr": F_SQR, "neg": F_NEG}[k["op"]]
        got = [int(v) for v in gpu_ctx.field_op(k["curve"], op, a, b)[0]]
        if "expect" in k:
            assert got == k["expect"], k
        else:
            assert got[0] == k["expect_limb0"], k


def _special_points(oracle, curve):
    g = oracle.generator(curve)
    g2 = oracle.point_double(curve, g)
    g3 = oracle.point_add(curve, g, g2)
    ident = oracle.identity(curve)
    neg = oracle.point_negate(curve, g)
    neg3 = oracle.point_negate(curve, g3)
    pts = [g, g2, g3, ident, neg, neg3]
    if curve == 2:
        # X = 0 but not the identity: doubling takes the raw-coordinate negation early-out (1878)
        y = V.limbs_of(5)
        pts.append(np.array([0, 0, 0, 0] + y + V.limbs_of(7) + [0, 0, 0, 0], dtype=np.uint64))
        pts.append(np.array([0, 0, 0, 0] + y + y + V.limbs_of(9), dtype=np.uint64))
    else:
        # Z = 1 and an all-zero point (secp256k1's is_identity special case, 1331-1336)
        pts.append(np.zeros(12, dtype=np.uint64))
        p = V.points(1, curve, 77)[0].copy()
        p[8:12] = [1, 0, 0, 0]
        pts.append(p)
    return pts


@pytest.mark.parametrize("curve", CURVES)
def test_point_ops_match_oracle(gpu_ctx, oracle, curve):
    n = 1500
    p = V.points(n, curve, 201)
    q = V.points(n, curve, 202)
    sp = _special_points(oracle, curve)
    sa = np.array([a for a in sp for _ in sp], dtype=np.uint64)
    sb = np.array([b for _ in sp for b in sp], dtype=np.uint64)
    # scaled-projective copies of the same point: force u1 == u2 && s1 == s2 with different Z where
    # the arithmetic allows it (P-256 is a true field for canonical operands)
    p = np.ascontiguousarray(np.concatenate([sa, p, p[:64]]))
    q = np.ascontiguousarray(np.concatenate([sb, q, p[len(sa):len(sa) + 64]]))
    got = gpu_ctx.point_op(curve, P_ADD, p, q)
    want = np.array([oracle.point_add(curve, p[i], q[i]) for i in range(p.shape[0])], dtype=np.uint64)
    _assert_same(got, want, "%s point add" % NAMES[curve])
    got = gpu_ctx.point_op(curve, P_DOUBLE, p)
    want = np.array([oracle.point_double(curve, p[i]) for i in range(p.shape[0])], dtype=np.uint64)
    _assert_same(got, want, "%s point double" % NAMES[curve])
    got = gpu_ctx.point_op(curve, P_NEGATE, p)
    want = np.array([oracle.point_negate(curve, p[i]) for i in range(p.shape[0])], dtype=np.uint64)
    _assert_same(got, want, "%s point negate" % NAMES[curve])
    if curve == 0:
        got = gpu_ctx.point_op(curve, P_DOUBLE_TRAIT, p)
        want = np.array([oracle.secp256k1_point_double_trait(p[i]) for i in range(p.shape[0])], dtype=np.uint64)
        _assert_same(got, want, "secp256k1 trait double")


@pytest.mark.parametrize("curve", CURVES)
def test_generator_matches_oracle(gpu_ctx, oracle, curve):
    assert np.array_equal(gpu_ctx.generator(curve), oracle.generator(curve))


def _edge_scalars():
    vals = [0, 1, 2, 3, 5, 1 << 255, (1 << 256) - 1, 1 << 248, 0x80, 0xFF, 1 << 64, (1 << 64) - 1,
            0x0102030405060708090A0B0C0D0E0F101112131415161718191A1B1C1D1E1F20, 1 << 128, 7 << 253]
    return np.array([V.limbs_of(v) for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("curve", CURVES)
def test_batch_mul_matches_oracle(gpu_ctx, oracle, curve):
    n = 1200
    k = V.scalars(n, curve, 301)
    p = V.points(n, curve, 302)
    ek = _edge_scalars()
    g = oracle.generator(curve)
    ident = oracle.identity(curve)
    # edge scalars on G and on a random point; identity base; Z = 1 base
    k = np.concatenate([ek, ek, ek[:4], k])
    p = np.concatenate([np.tile(g, (len(ek), 1)), np.tile(p[0], (len(ek), 1)), np.tile(ident, (4, 1)), p])
    k, p = np.ascontiguousarray(k), np.ascontiguousarray(p)
    got = gpu_ctx.batch_mul(curve, k, p)
    want = oracle.batch_mul(curve, k, p, nthreads=8)
    _assert_same(got, want, "%s batch_mul" % NAMES[curve])


@pytest.mark.parametrize("curve", CURVES)
def test_single_bit_and_word_boundary_scalars(gpu_ctx, oracle, curve):
    """Every top-bit position and every scalar-word boundary: the P-256 scheduler answers the ladder's prefix when it
    claims an element (result = point at step 256 - t, t = the scalar's top set bit) and refetches the scalar word
    that holds the current bit once per 32 steps; 2^t, 2^t + 1, 2^t - 1 and runs of ones across the word boundaries,
    on a random point, on G (Z = 1: the doubling's z.is_one() leg right after the copy) and mixed into random
    lanes so that wavefronts hold elements at very different steps."""
    vals = []
    for t in range(256):
        vals += [1 << t, (1 << t) | 1, (1 << t) - 1 if t else 1]
    for w in range(1, 8):
        vals += [0xFFFFFFFF << (32 * w - 16) & ((1 << 256) - 1), (1 << (32 * w)) | (1 << (32 * w - 1)), 3 << (32 * w - 1)]
    ek = np.array([V.limbs_of(v) for v in vals], dtype=np.uint64)
    m = len(ek)
    g = oracle.generator(curve)
    rp = V.points(m, curve, 377)
    k = np.concatenate([ek, ek, V.scalars(m, curve, 378)])
    p = np.concatenate([rp, np.tile(g, (m, 1)), V.points(m, curve, 379)])
    perm = np.random.default_rng(9).permutation(len(k))
    k, p = np.ascontiguousarray(k[perm]), np.ascontiguousarray(p[perm])
    _assert_same(gpu_ctx.batch_mul(curve, k, p), oracle.batch_mul(curve, k, p, nthreads=8), "%s single-bit scalars" % NAMES[curve])
    _assert_same(gpu_ctx.batch_mul_fixed(curve, ek, g), oracle.batch_mul_fixed(curve, ek, g, nthreads=8),
                 "%s single-bit scalars, fixed base" % NAMES[curve])


def test_p256_affine_addend_premise_and_kernel(gpu_ctx, oracle):
    """The P-256 scheduler drops four of Add's sixteen products when the addend has z == 1 and x1, y1 are below p
    (kernels_p256.hip: padd_body<true>).  The premise -- the reference's Mul by the canonical 1 returns the canonical
    form of its operand, and 1 * 1 is 1 -- is checked on the oracle and on the GPU field kernels over random, edge
    and non-canonical operands; then the kernel itself: bases with z == 1 (affine keys, the generator, arbitrary and
    NON-canonical x, y), mixed with projective bases so that wavefronts hold both kinds, fixed and variable base."""
    one = np.array([V.limbs_of(1)], dtype=np.uint64)
    vals = [V.limbs_of(v) for v in V.edge_field_values(1)]
    a = np.ascontiguousarray(np.concatenate([np.array(vals, dtype=np.uint64), V.field_elements(3000, 1, 471),
                                             V.splitmix64(4 * 500, V.SEED, 472).reshape(-1, 4)]))
    b = np.ascontiguousarray(np.tile(one, (a.shape[0], 1)))
    got = gpu_ctx.field_op(1, F_MUL, a, b)
    p = V.PRIME[1]
    for i in range(a.shape[0]):
        v = V.int_of(a[i])
        assert V.int_of(got[i]) == (v if v < p else v - p), hex(v)
        if i < 200:
            assert [int(x) for x in oracle.field_op(1, "mul", a[i], one[0])] == [int(x) for x in got[i]]
    assert [int(x) for x in gpu_ctx.field_op(1, F_SQR, one)[0]] == [1, 0, 0, 0]
    n = 3000
    k = V.scalars(n, 1, 473)
    pts = V.points(n, 1, 474)
    pts[::2, 8:12] = [1, 0, 0, 0]                              # every other base affine: mixed wavefronts
    raw = V.splitmix64(8 * n, V.SEED, 475).reshape(n, 8)
    pts[::6, 0:8] = raw[::6]                                   # some affine bases with arbitrary 256-bit (possibly >= p) x, y
    _assert_same(gpu_ctx.batch_mul(1, k, pts), oracle.batch_mul(1, k, pts, nthreads=8), "p256 mixed affine / projective bases")
    aff = pts.copy()
    aff[:, 8:12] = [1, 0, 0, 0]                                # all affine: every addition batch takes the short form
    _assert_same(gpu_ctx.batch_mul(1, k, aff), oracle.batch_mul(1, k, aff, nthreads=8), "p256 affine bases")
    for base in (oracle.generator(1), np.ascontiguousarray(aff[6])):
        _assert_same(gpu_ctx.batch_mul_fixed(1, k, base), oracle.batch_mul_fixed(1, k, base, nthreads=8), "p256 fixed affine base")


def test_p256_ladder_takes_the_equal_points_branch(gpu_ctx, oracle):
    """P = (0, 2^63, z) satisfies double(P) ~ P under the reference's P-256 arithmetic (its Sub wraps
    mod 2^256: Y3 = 0 - 8*y^4 = 2^256 - 2^255), so `result + *point` finds projectively equal
    operands and returns self.double() (p256.rs:1951-1953).  In the compacted kernel that verdict
    travels from the worker lane back to the owner lane; mix such lanes with ordinary ones."""
    n = 700
    k, p = V.scalars(n, 1, 395), V.points(n, 1, 396)
    rng = np.random.default_rng(3)
    special = rng.choice(n, size=90, replace=False)
    for j, i in enumerate(special):
        p[i] = np.array([0, 0, 0, 0] + V.limbs_of(1 << 63) + V.limbs_of(1 + 977 * j), dtype=np.uint64)
        if j % 3 == 0:
            k[i] = V.limbs_of(3 + 4 * j)
    # the premise: double(P) is projectively P, so Add(double(P), P) == double(double(P))
    d = oracle.point_double(1, p[special[0]])
    assert np.array_equal(oracle.point_add(1, d, p[special[0]]), oracle.point_double(1, d))
    got = gpu_ctx.batch_mul(1, k, p)
    want = oracle.batch_mul(1, k, p, nthreads=8)
    _assert_same(got, want, "p256 ladder with equal-points lanes")
    base = p[special[1]]
    _assert_same(gpu_ctx.batch_mul_fixed(1, k[:300], base), oracle.batch_mul_fixed(1, k[:300], base, nthreads=8),
                 "p256 fixed-base on a self-doubling base")


def test_ed25519_scheduler_takes_the_rare_branches(gpu_ctx, oracle):
    """Ed25519 Add's early-outs inside the scheduler kernel (padd_mem / pdbl_mem re-read both operands in a rare
    branch): points with x = 0 satisfy x == -x, so their doubling takes the "opposite points" exit and yields the
    identity, after which every addition meets an identity addend; y == z with x = 0 but t != 0 is NOT the identity.
    Such lanes are mixed with ordinary ones so that wavefronts hold both kinds."""
    n = 900
    k, p = V.scalars(n, 2, 397), V.points(n, 2, 398)
    rng = np.random.default_rng(4)
    special = rng.choice(n, size=120, replace=False)
    ys = V.field_elements(len(special), 2, 399)
    for j, i in enumerate(special):
        pt = np.zeros(16, dtype=np.uint64)
        pt[4:8] = ys[j]                       # y
        pt[8:12] = ys[j] if j % 3 == 0 else np.array([1, 0, 0, 0], dtype=np.uint64)   # z == y for a third of them
        if j % 2:
            pt[12:16] = V.limbs_of(7 + j)     # t != 0: never the identity
        p[i] = pt
        if j % 4 == 0:
            k[i] = V.limbs_of(1 + 2 * j)      # small scalars: few steps before the high zero bits
    got = gpu_ctx.batch_mul(2, k, p)
    want = oracle.batch_mul(2, k, p, nthreads=8)
    _assert_same(got, want, "ed25519 scheduler with x = 0 lanes")
    dm = gpu_ctx.batch_double_mul(2, k[:300], k[300:600], p[:300])
    _assert_same(dm, oracle.batch_double_mul(2, k[:300], k[300:600], p[:300], nthreads=8), "ed25519 double-mul with x = 0 lanes")
    # the table kernel (padd_table) on bases whose addend table degenerates: identity entries, opposite points
    for i in special[:4]:
        base = np.ascontiguousarray(p[i])
        _assert_same(gpu_ctx.batch_mul_fixed(2, k[:300], base), oracle.batch_mul_fixed(2, k[:300], base, nthreads=8),
                     "ed25519 fixed-base on an x = 0 base")


@pytest.mark.parametrize("curve", CURVES)
def test_batch_mul_fixed_matches_oracle(gpu_ctx, oracle, curve):
    n = 1000
    k = np.ascontiguousarray(np.concatenate([_edge_scalars(), V.scalars(n, curve, 311)]))
    g = oracle.generator(curve)
    got = gpu_ctx.batch_mul_fixed(curve, k, g)
    want = oracle.batch_mul_fixed(curve, k, g, nthreads=8)
    _assert_same(got, want, "%s batch_mul_fixed(G)" % NAMES[curve])
    base = V.points(1, curve, 312)[0]
    got = gpu_ctx.batch_mul_fixed(curve, k[:300], base)
    want = oracle.batch_mul_fixed(curve, k[:300], base, nthreads=8)
    _assert_same(got, want, "%s batch_mul_fixed(random base)" % NAMES[curve])


def _prefix_scalars(curve, bits, seed):
    """Scalars around the fixed-base prefix table's index: the table is indexed by the first `bits` bits the ladder
    consumes -- secp256k1: byte 0 msb first, then byte 1 ... (2655-2659); P-256: from bit 255 down (2126-2134);
    Ed25519: from bit 0 up (2073-2094) -- so both ends of the scalar get all-zero, all-one and one-bit patterns."""
    rows = [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [0x80, 0, 0, 0], [0xFF, 0, 0, 0], [0, 0, 0, 1 << 63], [0, 0, 0, 1]]
    full = (1 << 64) - 1
    for b in sorted({1, bits - 1, bits, bits + 1, 31, 32, 33}):
        if not 0 < b < 64:
            continue
        low, high = (1 << b) - 1, full ^ ((1 << (64 - b)) - 1)
        rows += [[low, 0, 0, 0], [full ^ low, full, full, full >> 4], [1 << b, 0, 0, 0],         # low end
                 [0, 0, 0, high >> 4], [full, full, full, (full ^ high) >> 4], [5, 0, 0, 1 << (63 - b)]]   # high end
    rnd = V.scalars(700, curve, seed)
    zlow = rnd[:100].copy(); zlow[:, 0] &= ~np.uint64((1 << min(bits, 63)) - 1)     # index 0 at the low end
    zhigh = rnd[100:200].copy(); zhigh[:, 3] &= np.uint64((1 << (64 - min(bits, 63))) - 1)   # index 0 at the high end
    return np.ascontiguousarray(np.concatenate([np.array(rows, dtype=np.uint64), zlow, zhigh, rnd]))


@pytest.mark.parametrize("bits", [0, 1, 7, 13, 24])
@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_prefix_table_is_invisible(oracle, curve, bits):
    """fec_ctx_set_fixed_prefix_bits: multiply(G, k) starts from the table entry of k's first `bits` ladder bits; the
    results -- fixed-base call, double multiplication, a second call that reuses the table -- are the oracle's for every
    table size, a base that is not the generator takes the plain kernels."""
    import forge_ec_amd as F
    ctx = F.Context(0)
    try:
        ctx.set_fixed_prefix_bits(bits)
        k = _prefix_scalars(curve, max(bits, 1), 3311 + bits)
        g = oracle.generator(curve)
        want = oracle.batch_mul_fixed(curve, k, g, nthreads=8)
        _assert_same(ctx.batch_mul_fixed(curve, k, g), want, "%s batch_mul_fixed(G), %d-bit prefix table" % (NAMES[curve], bits))
        _assert_same(ctx.batch_mul_fixed(curve, k[::-1].copy(), g), want[::-1], "%s second call on the table" % NAMES[curve])
        base = V.points(1, curve, 3312)[0]
        _assert_same(ctx.batch_mul_fixed(curve, k[:200], base), oracle.batch_mul_fixed(curve, k[:200], base, nthreads=8),
                     "%s batch_mul_fixed(another base) beside the table" % NAMES[curve])
        u2, q = V.scalars(len(k), curve, 3313), V.points(len(k), curve, 3314)
        _assert_same(ctx.batch_double_mul(curve, k, u2, q), oracle.batch_double_mul(curve, k, u2, q, nthreads=8),
                     "%s batch_double_mul, %d-bit prefix table" % (NAMES[curve], bits))
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_of_the_callers_own_gets_a_table_per_launch(gpu_ctx, oracle, curve):
    """From 2^16 elements on a fixed base that is not the generator is multiplied from a prefix table built for that one
    launch (fecgpu.hip: acquire_with_prefix; 2^14 entries here): projective base with z != 1, every element against the oracle,
    and the same call again with the tables switched off."""
    import forge_ec_amd as F
    n = (1 << 16) + 37
    k = V.scalars(n, curve, 3411)
    k[:_prefix_scalars(curve, 14, 1).shape[0]] = _prefix_scalars(curve, 14, 3412)
    base = V.points(1, curve, 3413)[0]
    want = oracle.batch_mul_fixed(curve, k, base, nthreads=8)
    _assert_same(gpu_ctx.batch_mul_fixed(curve, k, base), want, "%s batch_mul_fixed(own base), table per launch" % NAMES[curve])
    ident = oracle.identity(curve)   # multiply's first early-out (identity point) must win over the table
    _assert_same(gpu_ctx.batch_mul_fixed(curve, k, ident), oracle.batch_mul_fixed(curve, k, ident, nthreads=8),
                 "%s batch_mul_fixed(identity), table per launch" % NAMES[curve])
    ctx = F.Context(0)
    try:
        ctx.set_fixed_prefix_bits(0)
        _assert_same(ctx.batch_mul_fixed(curve, k, base), want, "%s batch_mul_fixed(own base), tables off" % NAMES[curve])
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_batch_double_mul_matches_oracle(gpu_ctx, oracle, curve):
    n = 600
    u1 = V.scalars(n, curve, 321)
    u2 = V.scalars(n, curve, 322)
    q = V.points(n, curve, 323)
    g = oracle.generator(curve)
    # Q = G with u1 == u2: both ladders return the same point, the final Add takes the
    # equal-points branch (self.double()); u = 0 and identity Q: early-outs
    q[:8] = g
    u2[:8] = u1[:8]
    u1[8:10] = 0
    q[10:12] = oracle.identity(curve)
    got = gpu_ctx.batch_double_mul(curve, u1, u2, q)
    want = oracle.batch_double_mul(curve, u1, u2, q, nthreads=8)
    _assert_same(got, want, "%s batch_double_mul" % NAMES[curve])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_ragged_sizes_config1(gpu_ctx, oracle, n):
    """BASELINE config 1 shape (1000 secp256k1 variable-base) plus empty/ragged batch sizes."""
    k = V.scalars(max(n, 1), 0, 331)[:n]
    p = V.points(max(n, 1), 0, 332)[:n]
    got = gpu_ctx.batch_mul(0, k, p)
    assert got.shape == (n, 12)
    if n:
        want = oracle.batch_mul(0, k, p, nthreads=8)
        _assert_same(got, want, "secp256k1 n=%d" % n)


@pytest.mark.parametrize("curve", [1, 2])
def test_scheduler_kernels_at_slot_and_wavefront_boundaries(gpu_ctx, oracle, curve):
    """The persistent schedulers (P-256, Ed25519 variable base: 768 threads, 1024 slots per workgroup, ranges
    of at least 64 elements per workgroup) and the Ed25519 table kernel at batch sizes around every boundary of
    that geometry, with zero scalars and identity points sprinkled in (elements answered at claim time)."""
    g = oracle.generator(curve)
    for n in (1, 2, 63, 64, 65, 127, 129, 767, 768, 769, 1023, 1025, 1151, 1153, 4097, 16385 + 7):
        k, p = V.scalars(n, curve, 7000 + n), V.points(n, curve, 7100 + n)
        k[::11] = 0
        p[5::13] = oracle.identity(curve)
        assert np.array_equal(gpu_ctx.batch_mul(curve, k, p), oracle.batch_mul(curve, k, p, nthreads=16)), (curve, n)
        assert np.array_equal(gpu_ctx.batch_mul_fixed(curve, k, g), oracle.batch_mul_fixed(curve, k, g, nthreads=16)), (curve, n)


@pytest.mark.parametrize("curve", [1, 2])
def test_scheduler_kernels_wide_slot_instantiation(gpu_ctx, oracle, curve):
    """A launch whose workgroups own between 864 and 1 024 elements each (here 256 000 elements on 256 CUs) takes the
    1 024-slot instantiation of the scheduler kernel (P-256: the scalar's bits then come from the caller's array, not
    from LDS); 2 000 per workgroup likewise.  Device-pointer call (one launch), every element against the oracle."""
    import torch
    for n in (256 * 1000, 256 * 2000 + 77):
        k, p = V.scalars(n, curve, 3511), V.points(n, curve, 3512)
        k[::997] = 0
        p[3::1009] = oracle.identity(curve)
        dk = torch.from_numpy(k.view(np.int64)).cuda()
        dp = torch.from_numpy(p.view(np.int64)).cuda()
        do = torch.empty_like(dp)
        torch.cuda.synchronize()
        gpu_ctx.batch_mul_dev(curve, dk.data_ptr(), dp.data_ptr(), do.data_ptr(), n)
        gpu_ctx.check()
        torch.cuda.synchronize()
        got = do.cpu().numpy().view(np.uint64)
        _assert_same(got, oracle.batch_mul(curve, k, p, nthreads=16), "%s batch_mul_dev, %d elements" % (NAMES[curve], n))


def test_host_pipeline_chunking_is_invisible(gpu_ctx, oracle):
    """The host-pointer path pipelines chunks over two streams; results must not depend on the
    chunk size (1 chunk, many chunks, ragged last chunk, odd and even chunk counts)."""
    n = 1000
    try:
        for curve in (0, 2):
            k, p = V.scalars(n, curve, 371), V.points(n, curve, 372)
            want = oracle.batch_mul(curve, k, p, nthreads=8)
            g = oracle.generator(curve)
            wantf = oracle.batch_mul_fixed(curve, k, g, nthreads=8)
            for chunk in (1 << 18, 256, 333, 64, 999, 1000, 1001):
                gpu_ctx.set_chunk(chunk)
                _assert_same(gpu_ctx.batch_mul(curve, k, p), want, "chunk %d curve %d" % (chunk, curve))
                _assert_same(gpu_ctx.batch_mul_fixed(curve, k, g), wantf, "fixed chunk %d curve %d" % (chunk, curve))
        u1, u2, q = V.scalars(300, 0, 373), V.scalars(300, 0, 374), V.points(300, 0, 375)
        gpu_ctx.set_chunk(128)
        _assert_same(gpu_ctx.batch_double_mul(0, u1, u2, q), oracle.batch_double_mul(0, u1, u2, q, nthreads=8),
                     "double-mul chunked")
    finally:
        gpu_ctx.set_chunk(1 << 18)


def test_abi_argument_errors(gpu_ctx):
    import ctypes
    import forge_ec_amd as F
    L = F.lib()
    h = gpu_ctx._h
    buf = (ctypes.c_uint64 * 16)()
    assert L.fec_batch_mul(h, 7, buf, buf, buf, 1) == -1          # unknown curve
    assert L.fec_batch_mul(h, 0, None, buf, buf, 1) == -1         # null pointer
    assert L.fec_batch_mul(None, 0, buf, buf, buf, 1) == -1       # null ctx
    assert L.fec_point_op(h, 1, 3, buf, None, buf, 1) == -5       # trait double is secp256k1-only
    assert L.fec_field_op(h, 0, 9, buf, buf, buf, 1) == -1        # unknown op
    assert L.fec_batch_mul(h, 0, None, None, None, 0) == 0        # empty batch is fine
    assert L.fec_batch_mul_dev(h, 0, ctypes.c_void_p(8), ctypes.c_void_p(16), ctypes.c_void_p(16), 1, None) == -1
    assert L.fec_ctx_set_fixed_prefix_bits(h, 29) == -1           # at most 28 bits
    assert L.fec_ctx_set_fixed_prefix_bits(None, 8) == -1
    assert L.fec_ctx_fixed_prefix_bits(h, 5) == -1                # unknown curve
    assert L.fec_ctx_fixed_prefix_bits(None, 0) == -1


def test_ed25519_fixed_base_device_path_reuses_table(gpu_ctx, oracle):
    """fec_batch_mul_fixed_dev on the ctx's own generator (table built once, recognised by address),
    then on another base (table rebuilt), then the generator again."""
    import torch
    n = 900
    k = V.scalars(n, 2, 351)
    dk = torch.from_numpy(k.view(np.int64)).cuda()
    do = torch.empty((n, 16), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    g = oracle.generator(2)
    other = V.points(1, 2, 352)[0]
    d_other = torch.from_numpy(other.view(np.int64)).cuda()
    for base_host, base_dev in ((g, gpu_ctx.generator_dev(2)), (other, d_other.data_ptr()),
                                (g, gpu_ctx.generator_dev(2))):
        gpu_ctx.batch_mul_fixed_dev(2, dk.data_ptr(), base_dev, do.data_ptr(), n, stream)
        torch.cuda.synchronize()
        got = do.cpu().numpy().view(np.uint64)
        _assert_same(got, oracle.batch_mul_fixed(2, k, base_host, nthreads=8), "ed25519 fixed-base dev path")


def test_dev_calls_on_two_streams_share_ctx_scratch_in_call_order(gpu_ctx, oracle):
    """*_dev calls of ONE ctx issued back to back on two different streams with no host synchronisation
    in between: the Ed25519 fixed-base path rebuilds and reads the ctx-owned addend table, the P-256 /
    Ed25519 double-mul writes per-stream scratch.  The library orders a launch after the ctx's previous
    launch when the stream changes, so every result must still be the oracle's.

    Nothing here makes the two calls overlap: two streams created one after the other can share a hardware queue and
    then run one after the other, and the test passes with nothing in flight.  tests/test_gpu_parity_streams.py holds
    the same promise for every parity *_dev entry point behind a gate that has both streams demonstrably running
    (tests/stream_gate.py); this test stays for the batch of 20000, which that module does not reach."""
    import torch
    n = 20000
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    k = V.scalars(n, 2, 371)
    bases = V.points(4, 2, 372)
    dk = torch.from_numpy(k.view(np.int64)).cuda()
    dbases = [torch.from_numpy(b.view(np.int64)).cuda() for b in bases]
    outs = [torch.empty((n, 16), dtype=torch.int64, device="cuda") for _ in bases]
    torch.cuda.synchronize()
    for i in range(4):  # four different bases, alternating streams: the table is rebuilt under the previous user
        st = (s1, s2)[i & 1]
        gpu_ctx.batch_mul_fixed_dev(2, dk.data_ptr(), dbases[i].data_ptr(), outs[i].data_ptr(), n, st.cuda_stream)
    # double-mul on both streams at once (per-stream scratch)
    u1, u2 = V.scalars(n, 1, 373), V.scalars(n, 1, 374)
    q = V.points(n, 1, 375)
    du1, du2, dq = (torch.from_numpy(a.view(np.int64)).cuda() for a in (u1, u2, q))
    dd = [torch.empty((n, 12), dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    gpu_ctx.batch_double_mul_dev(1, du1.data_ptr(), du2.data_ptr(), dq.data_ptr(), dd[0].data_ptr(), n, s1.cuda_stream)
    gpu_ctx.batch_double_mul_dev(1, du2.data_ptr(), du1.data_ptr(), dq.data_ptr(), dd[1].data_ptr(), n, s2.cuda_stream)
    torch.cuda.synchronize()
    for i in range(4):
        _assert_same(outs[i].cpu().numpy().view(np.uint64), oracle.batch_mul_fixed(2, k, bases[i], nthreads=16),
                     "ed25519 fixed-base, call %d of 4 on alternating streams" % i)
    _assert_same(dd[0].cpu().numpy().view(np.uint64), oracle.batch_double_mul(1, u1, u2, q, nthreads=16), "p256 double-mul s1")
    _assert_same(dd[1].cpu().numpy().view(np.uint64), oracle.batch_double_mul(1, u2, u1, q, nthreads=16), "p256 double-mul s2")


@pytest.mark.parametrize("curve", CURVES)
def test_batch_to_affine_matches_oracle(gpu_ctx, oracle, curve):
    """Curve::to_affine with the reference's own field inversion (next row of SURVEY section 8f)."""
    n = 700
    p = V.points(n, curve, 361)
    g = oracle.generator(curve)
    sp = _special_points(oracle, curve)[:6]
    mult = oracle.batch_mul(curve, V.scalars(40, curve, 362), V.points(40, curve, 363), nthreads=8)
    p = np.ascontiguousarray(np.concatenate([np.array(sp, dtype=np.uint64), mult, p]))
    xy, inf = gpu_ctx.batch_to_affine(curve, p)
    wxy, winf = oracle.batch_to_affine(curve, p, nthreads=8)
    assert np.array_equal(inf, winf)
    _assert_same(xy, wxy, "%s to_affine" % NAMES[curve])


def _ecdsa_cases(oracle, n_random, n_valid):
    """digests, r, s, pk_xy, pk_inf covering: random (invalid) signatures, constructed VALID ones,
    zero / out-of-range r and s, and digests >= n (where the reference panics)."""
    rng = np.random.default_rng(99)
    # the reference's own N (secp256k1.rs:27-28) has its two top limbs swapped w.r.t. the true order
    order = 0xFFFFFFFFFFFFFFFEFFFFFFFFFFFFFFFFBAAEDCE6AF48A03BBFD25E8CD0364141
    total = n_random + n_valid + 8
    dg = rng.integers(0, 256, size=(total, 32), dtype=np.uint8)
    dg[:, 0] &= 0x7F                                   # keep the digest below N unless stated otherwise
    r = V.scalars(total, 0, 381)
    s = V.scalars(total, 0, 382)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(total, 0, 383), V.field_elements(total, 0, 384)], axis=1))
    inf = np.zeros(total, dtype=np.uint8)
    g = oracle.generator(0)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    made = 0
    for i in range(n_random, n_random + n_valid):
        # with the public key at infinity R = multiply(G, h * s^-1) does not depend on r, so r can be
        # set to the x the reference will derive: these verify as VALID under the reference's rules
        inf[i] = 1
        h = np.array([int.from_bytes(dg[i].tobytes(), "big") >> (64 * k) & ((1 << 64) - 1) for k in range(4)], dtype=np.uint64)
        s_inv, ok = oracle.secp256k1_scalar_op("inv", s[i])
        u1 = oracle.secp256k1_scalar_op("mul", h, s_inv)[0]
        rp = oracle.multiply(0, g, u1)
        xy, is_inf = oracle.to_affine(0, rp)
        xr = oracle.field_op(0, "mul", xy[:4], one)
        if not is_inf and 0 < V.int_of(xr) < order:
            r[i] = xr
            made += 1
    base = n_random + n_valid
    r[base + 0] = 0                                     # r == 0            -> 0
    s[base + 1] = 0                                     # s == 0            -> 0
    r[base + 2] = V.limbs_of(order)                     # r == n            -> 0
    s[base + 3] = V.limbs_of((1 << 256) - 1)            # s >= n            -> 0
    dg[base + 4] = 0xFF                                 # digest >= n       -> 2 (unwrap panics)
    dg[base + 5] = np.frombuffer(order.to_bytes(32, "big"), dtype=np.uint8)  # digest == n -> 2
    inf[base + 6] = 1                                   # Q at infinity, random r -> 0
    dg[base + 7] = 0                                    # h == 0: u1 == 0, R = u2*Q
    return dg, r, s, pk, inf, made


def test_ecdsa_verify_secp256k1_matches_oracle(gpu_ctx, oracle):
    """Ecdsa::<Secp256k1,_>::verify end to end (next row of SURVEY section 8f): every status the
    reference can produce, including signatures that VERIFY under its arithmetic."""
    # (under the reference's scalar arithmetic s^-1 collapses to 0 for about half of all s, which
    # makes R the identity; the construction only succeeds for the rest)
    dg, r, s, pk, inf, made = _ecdsa_cases(oracle, 300, 80)
    assert made >= 20
    want = oracle.batch_secp256k1_ecdsa_verify(dg, r, s, pk, inf, nthreads=8)
    got = gpu_ctx.ecdsa_verify_secp256k1(dg, r, s, pk, inf)
    assert set(int(v) for v in want) == {0, 1, 2}
    assert int((want == 1).sum()) == made
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first mismatch at %d: got %d want %d" % (bad[0], got[bad[0]], want[bad[0]])
    # without the infinity flags (NULL pk_inf) every key is a finite point
    want2 = oracle.batch_secp256k1_ecdsa_verify(dg, r, s, pk, None, nthreads=8)
    assert np.array_equal(gpu_ctx.ecdsa_verify_secp256k1(dg, r, s, pk, None), want2)


def test_eddsa_verify_ed25519_matches_oracle(gpu_ctx, oracle):
    """Eddsa::<Ed25519, D>::verify / Ed25519::verify from the point computation on (eddsa.rs:174-211, 430-447):
    random inputs, signatures that verify under the reference's arithmetic, infinite R, zero scalars, the
    panic input of the fixture; host and device-pointer entry points."""
    import json
    import os
    import torch
    n_random, n_valid = 500, 60
    n = n_random + n_valid + 6
    s, k = V.scalars(n, 2, 821), V.scalars(n, 2, 822)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, 2, 823), V.field_elements(n, 2, 824)], axis=1))
    r = np.ascontiguousarray(np.concatenate([V.field_elements(n, 2, 825), V.field_elements(n, 2, 826)], axis=1))
    pinf, rinf = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    g = oracle.generator(2)
    sg = oracle.batch_mul_fixed(2, s[n_random:n_random + n_valid], g, nthreads=8)
    axy, ainf = oracle.batch_to_affine(2, sg, nthreads=8)
    for j in range(n_valid):
        i = n_random + j
        r[i] = axy[j]
        if j % 2:
            pinf[i] = 1       # A at infinity: R + k*A = from_affine(R)
        else:
            k[i] = 0          # k = 0: multiply's early-out gives the identity as well
    base = n_random + n_valid
    rinf[base + 0] = 1        # infinite R -> false
    s[base + 1] = 0           # s*G = identity
    k[base + 2] = 0
    pinf[base + 3] = 1
    r[base + 4] = 0           # R = (0, 0), not flagged
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eddsa_ed25519_vectors.json")) as f:
        panic = [c for c in json.load(f)["verify"] if c["status"] == 2][0]
    r[base + 5], pk[base + 5], s[base + 5], k[base + 5] = panic["r"], panic["pk"], panic["s"], panic["k"]
    want = oracle.batch_ed25519_eddsa_verify(r, rinf, pk, pinf, s, k, nthreads=8)
    assert int((want == 1).sum()) >= n_valid and set(int(v) for v in want) == {0, 1, 2}
    got = gpu_ctx.eddsa_verify_ed25519(r, rinf, pk, pinf, s, k)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first mismatch at %d: got %d want %d" % (bad[0], got[bad[0]], want[bad[0]])
    want2 = oracle.batch_ed25519_eddsa_verify(r, None, pk, None, s, k, nthreads=8)
    assert np.array_equal(gpu_ctx.eddsa_verify_ed25519(r, None, pk, None, s, k), want2)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (r, rinf, pk, pinf, s, k)]
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.eddsa_verify_ed25519_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                     t[5].data_ptr(), st.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(st.cpu().numpy(), want)


@pytest.mark.parametrize("curve", [0, 1])
def test_ecdsa_batch_verify_matches_oracle(gpu_ctx, oracle, curve):
    """Ecdsa::<C, D>::batch_verify (ecdsa.rs:287-391) at n = 300: a batch that verifies under the reference's
    arithmetic, random batches (final comparison fails; both folded sums compared), and the loop's early exits
    in index order."""
    n = 300
    order = 0xFFFFFFFFFFFFFFFEFFFFFFFFFFFFFFFFBAAEDCE6AF48A03BBFD25E8CD0364141 if curve == 0 else V.ORDER[1]
    op = oracle.secp256k1_scalar_op if curve == 0 else oracle.p256_scalar_op
    rng = np.random.default_rng(1200 + curve)
    dg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    dg[:, 0] &= 0x7F
    r, s, a = V.scalars(n, curve, 871), V.scalars(n, curve, 872), V.scalars(n, curve, 873)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, 874), V.field_elements(n, curve, 875)], axis=1))

    def both(dg, r, s, pk, inf, a):
        want, wd = oracle.ecdsa_batch_verify(curve, dg, r, s, pk, inf, a)
        got, gd = gpu_ctx.ecdsa_batch_verify(curve, dg, r, s, pk, inf, a)
        assert got == want
        assert np.array_equal(gd, wd)
        return want, wd

    st, detail = both(dg, r, s, pk, None, a)
    assert st == 0 and detail.any()
    # all keys at infinity: r_sum does not depend on r; last weight 1, last r = x(r_sum) - (ordered sum of the rest)
    inf = np.ones(n, dtype=np.uint8)
    made = False
    for attempt in range(8):
        a2, r2 = a.copy(), r.copy()
        a2[n - 1] = [1, 0, 0, 0]
        r2[0] = V.scalars(1, curve, 880 + attempt)[0]
        _, d = oracle.ecdsa_batch_verify(curve, dg, r2, s, pk, inf, a2)
        xy, is_inf = oracle.to_affine(curve, d[:12])
        xs = V.int_of(oracle.field_op(0, "mul", xy[:4], np.array([1, 0, 0, 0], dtype=np.uint64))) if curve == 0 else V.int_of(xy[:4])
        partial = np.zeros(4, dtype=np.uint64)
        for i in range(n - 1):
            partial = op("add", partial, op("mul", a2[i], r2[i])[0])[0]
        if not is_inf and 0 < xs < order and xs > V.int_of(partial):
            r2[n - 1] = V.limbs_of(xs - V.int_of(partial))
            made = True
            break
    assert made
    assert both(dg, r2, s, pk, inf, a2)[0] == 1
    # early exits: the first failing signature in index order decides
    r3 = r.copy(); r3[200] = 0
    assert both(dg, r3, s, pk, None, a)[0] == 0
    dg4 = dg.copy(); dg4[17] = 0xFF
    assert both(dg4, r3, s, pk, None, a)[0] == 2       # panic at 17 before the r = 0 at 200
    s5 = s.copy(); s5[3] = 0
    assert both(dg4, r, s5, pk, None, a)[0] == 0       # s = 0 at 3 before the panic at 17
    assert both(dg[:1], r[:1], s[:1], pk[:1], None, a[:1])[0] == 0
    got, gd = gpu_ctx.ecdsa_batch_verify(curve, dg[:0], r[:0], s[:0], pk[:0], None, a[:0])
    assert got == 0 and not gd.any()                   # empty batch: false


def _p256_true_points(n, seed):
    """n affine points of the real P-256 (x, y as limbs): the reference's is_on_curve accepts about half of them."""
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


@pytest.mark.parametrize("curve", [0, 1])
def test_batch_ecdh_matches_oracle(gpu_ctx, oracle, curve):
    """KeyExchange::derive_shared_secret per element (secp256k1.rs:1884-1904, p256.rs:2281-2312): secrets and
    statuses against the oracle -- accepted and rejected public keys, infinite keys, zero private keys -- through
    the host and the device-pointer entry points."""
    import torch
    n = 1500
    sk = V.scalars(n, curve, 931)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, 932), V.field_elements(n, curve, 933)], axis=1))
    if curve == 1:
        pk[: n - 100] = _p256_true_points(n - 100, 934)      # the last 100 stay off-curve
    inf = np.zeros(n, dtype=np.uint8)
    inf[7::97] = 1
    sk[11::113] = 0
    want, wst = oracle.batch_ecdh(curve, sk, pk, inf, nthreads=8)
    got, gst = gpu_ctx.batch_ecdh(curve, sk, pk, inf)
    assert np.array_equal(gst, wst) and np.array_equal(got, want)
    expect = {0, 2} if curve == 0 else {0, 1, 2}
    assert set(int(v) for v in np.unique(wst)) == expect and int((wst == 0).sum()) > n // 3
    w2, s2 = oracle.batch_ecdh(curve, sk, pk, None, nthreads=8)
    g2, t2 = gpu_ctx.batch_ecdh(curve, sk, pk, None)
    assert np.array_equal(t2, s2) and np.array_equal(g2, w2)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (sk, pk, inf)]
    sec = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.batch_ecdh_dev(curve, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), sec.data_ptr(), st.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(st.cpu().numpy(), wst) and np.array_equal(sec.cpu().numpy().reshape(n, 32), want)
    with pytest.raises(Exception):
        gpu_ctx.batch_ecdh(2, sk, pk, inf)                    # Ed25519 implements no KeyExchange


@pytest.mark.parametrize("curve", CURVES)
def test_batch_validate_point_matches_oracle(gpu_ctx, oracle, curve):
    """Curve::validate_point per affine point: is_on_curve for secp256k1 / P-256 (their overrides), the trait
    default -- on the curve and L * (8 * P) == identity, two multiplications -- for Ed25519."""
    import torch
    n = 1200 if curve != 2 else 700
    xy = np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, 941), V.field_elements(n, curve, 942)], axis=1))
    if curve == 1:
        xy[:800] = _p256_true_points(800, 943)            # about half pass the reference's is_on_curve
    if curve == 2:                                          # x = 0 columns: (0, 1) is on the curve and of order 1
        xy[:40, :4] = 0
        xy[:20, 4:] = np.array([1, 0, 0, 0], dtype=np.uint64)
        g, _ = oracle.to_affine(2, oracle.generator(2))
        xy[40] = g
    inf = np.zeros(n, dtype=np.uint8)
    inf[5::53] = 1
    want = oracle.batch_validate_point(curve, xy, inf, nthreads=16)
    got = gpu_ctx.batch_validate_point(curve, xy, inf)
    assert np.array_equal(got, want)
    assert set(int(v) for v in np.unique(want)) == {0, 1} and int(want.sum()) > (300 if curve == 1 else 20)
    assert np.array_equal(gpu_ctx.batch_validate_point(curve, xy, None), oracle.batch_validate_point(curve, xy, None, nthreads=16))
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (xy, inf)]
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu_ctx.batch_validate_point_dev(curve, t[0].data_ptr(), t[1].data_ptr(), ok.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy(), want)


def _p256_ecdsa_cases(oracle, n_random, n_valid):
    """As _ecdsa_cases for Ecdsa::<P256, D>::verify.  r or s >= n are NOT rejected by the reference (its
    ct_lt is the trait default, a top-byte <= comparison): those lanes run the whole computation."""
    rng = np.random.default_rng(199)
    order = V.ORDER[1]
    total = n_random + n_valid + 10
    dg = rng.integers(0, 256, size=(total, 32), dtype=np.uint8)
    dg[:, 0] &= 0x7F
    r = V.scalars(total, 1, 391)
    s = V.scalars(total, 1, 392)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(total, 1, 393), V.field_elements(total, 1, 394)], axis=1))
    inf = np.zeros(total, dtype=np.uint8)
    g = oracle.generator(1)
    made = 0
    for i in range(n_random, n_random + n_valid):
        inf[i] = 1    # R = multiply(G, h * s^-1) regardless of r: set r to the x the reference derives
        h = np.array(V.limbs_of(int.from_bytes(dg[i].tobytes(), "big")), dtype=np.uint64)
        s_inv, ok = oracle.p256_scalar_op("inv", s[i])
        u1 = oracle.p256_scalar_op("mul", h, s_inv)[0]
        xy, is_inf = oracle.to_affine(1, oracle.multiply(1, g, u1))
        if not is_inf and 0 < V.int_of(xy[:4]) < order:
            r[i] = xy[:4]
            made += 1
    base = n_random + n_valid
    r[base + 0] = 0                                     # r == 0            -> 0
    s[base + 1] = 0                                     # s == 0            -> 0
    r[base + 2] = V.limbs_of(order)                     # r == n: passes the default ct_lt
    s[base + 3] = V.limbs_of((1 << 256) - 1)            # s >= n: passes it too
    dg[base + 4] = 0xFF                                 # digest >= n       -> 2 (unwrap panics)
    dg[base + 5] = np.frombuffer(order.to_bytes(32, "big"), dtype=np.uint8)  # digest == n -> 2
    inf[base + 6] = 1                                   # Q at infinity, random r -> 0
    dg[base + 7] = 0                                    # h == 0: u1 == 0, R = u2*Q
    dg[base + 8] = 0xFF                                 # digest >= n but r == 0: the zero check wins -> 0
    r[base + 8] = 0
    pk[base + 9] = 0                                    # public key (0, 0), not flagged as infinity
    return dg, r, s, pk, inf, made


def test_ecdsa_verify_p256_matches_oracle(gpu_ctx, oracle):
    """Ecdsa::<P256, D>::verify end to end in the reference's P-256 scalar arithmetic: every status the
    reference can produce, including signatures that VERIFY under it; host and device-pointer entry points."""
    dg, r, s, pk, inf, made = _p256_ecdsa_cases(oracle, 600, 60)
    assert made >= 40
    want = oracle.batch_p256_ecdsa_verify(dg, r, s, pk, inf, nthreads=8)
    got = gpu_ctx.ecdsa_verify_p256(dg, r, s, pk, inf)
    assert set(int(v) for v in want) == {0, 1, 2}
    assert int((want == 1).sum()) == made
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first mismatch at %d: got %d want %d" % (bad[0], got[bad[0]], want[bad[0]])
    want2 = oracle.batch_p256_ecdsa_verify(dg, r, s, pk, None, nthreads=8)
    assert np.array_equal(gpu_ctx.ecdsa_verify_p256(dg, r, s, pk, None), want2)
    # device-pointer form, on a caller stream
    import torch
    n = dg.shape[0]
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (dg, r, s, pk, inf)]
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.ecdsa_verify_p256_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                  st.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(st.cpu().numpy(), want)


@pytest.mark.parametrize("curve", CURVES)
def test_multi_scalar_multiply_matches_sequential_fold(gpu_ctx, oracle, curve):
    """Curve::multi_scalar_multiply (core lib.rs:934-951): result = identity; result += product[i]
    strictly in order (the reference's Add is not associative)."""
    n = 300
    k, p = V.scalars(n, curve, 391), V.points(n, curve, 392)
    prods = oracle.batch_mul(curve, k, p, nthreads=8)
    acc = oracle.identity(curve)
    for i in range(n):
        acc = oracle.point_add(curve, acc, prods[i])
    assert np.array_equal(gpu_ctx.multi_scalar_mul(curve, k, p), acc)
    # order matters: the reversed batch gives a different point
    rev = gpu_ctx.multi_scalar_mul(curve, k[::-1].copy(), p[::-1].copy())
    assert not np.array_equal(rev, acc)
    assert np.array_equal(gpu_ctx.multi_scalar_mul(curve, k[:1], p[:1]), prods[0] if not oracle.is_identity(curve, prods[0]) else acc)
    import forge_ec_amd as F
    assert np.array_equal(F.CURVES[curve](gpu_ctx).multi_scalar_multiply(p[:0], k[:0]), oracle.identity(curve))


def test_device_pointer_path_with_torch(gpu_ctx, oracle):
    """The *_dev entry points on torch-owned HBM buffers and torch's current stream."""
    import torch
    n = 700
    k = V.scalars(n, 0, 341)
    p = V.points(n, 0, 342)
    dk = torch.from_numpy(k.view(np.int64)).cuda()
    dp = torch.from_numpy(p.view(np.int64)).cuda()
    do = torch.empty_like(dp)
    stream = torch.cuda.current_stream().cuda_stream
    gpu_ctx.batch_mul_dev(0, dk.data_ptr(), dp.data_ptr(), do.data_ptr(), n, stream)
    torch.cuda.synchronize()
    got = do.cpu().numpy().view(np.uint64)
    want = oracle.batch_mul(0, k, p, nthreads=8)
    _assert_same(got, want, "secp256k1 batch_mul_dev")


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_batch_mul_in_place_output(gpu_ctx, oracle, curve):
    """`out` may be the `points` array itself (an element's point is not read after its result is stored); also
    adjacent input / output ranges inside one allocation."""
    import torch
    n = 1500
    k = V.scalars(n, curve, 351)
    p = V.points(n, curve, 352)
    want = oracle.batch_mul(curve, k, p, nthreads=8)
    dk = torch.from_numpy(k.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    dp = torch.from_numpy(p.view(np.int64)).cuda()
    gpu_ctx.batch_mul_dev(curve, dk.data_ptr(), dp.data_ptr(), dp.data_ptr(), n, stream)
    torch.cuda.synchronize()
    _assert_same(dp.cpu().numpy().view(np.uint64), want, "in-place batch_mul_dev")
    if curve == 1:  # output 5 elements above the points inside one allocation: no element's output slot is its own point's
        limbs = V.POINT_LIMBS[curve]
        buf = torch.zeros((n + 5, limbs), dtype=torch.int64, device="cuda")
        buf[:n] = torch.from_numpy(p.view(np.int64)).cuda()
        gpu_ctx.batch_mul_dev(curve, dk.data_ptr(), buf.data_ptr(), buf[5:].data_ptr(), 5, stream)  # reads rows 0..4, writes 5..9
        torch.cuda.synchronize()
        _assert_same(buf[5:10].cpu().numpy().view(np.uint64), want[:5], "adjacent ranges")


def test_schnorr_batch_verify_secp256k1_matches_oracle(gpu_ctx, oracle):
    """schnorr::batch_verify::<Secp256k1, D> (schnorr.rs:194-290) through the C ABI: the boolean and the
    two affine sums the reference compares, bit-exact with the oracle, over several batch sizes
    (ragged workgroups), with the trivially-true case (all weights zero) and the early rejections."""
    def inputs(n, seed):
        pk = V.field_elements(2 * n, 0, seed).reshape(n, 8)
        r = V.field_elements(2 * n, 0, seed + 1).reshape(n, 8)
        return pk, r, V.scalars(n, 0, seed + 2), V.scalars(n, 0, seed + 3), V.scalars(n, 0, seed + 4)

    for n, seed in ((1, 800), (5, 810), (64, 820), (300, 830)):
        pk, r, s, a, e = inputs(n, seed)
        want, w_sides, w_inf = oracle.secp256k1_schnorr_batch_verify(pk, None, r, None, s, a, e)
        got, sides, sinf = gpu_ctx.schnorr_batch_verify_secp256k1(pk, r, s, a, e)
        assert got == bool(want)
        assert np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf)
        assert sides.any()
    pk, r, s, a, e = inputs(70, 840)
    # scalars with zero weights / zero challenges / zero s mixed in (multiply's early-outs)
    a[3] = 0
    e[5] = 0
    s[7] = 0
    want, w_sides, w_inf = oracle.secp256k1_schnorr_batch_verify(pk, None, r, None, s, a, e)
    got, sides, sinf = gpu_ctx.schnorr_batch_verify_secp256k1(pk, r, s, a, e)
    assert got == bool(want) and np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf)
    # all weights zero -> true via (infinity & infinity)
    a0 = np.zeros_like(a)
    want, w_sides, w_inf = oracle.secp256k1_schnorr_batch_verify(pk, None, r, None, s, a0, e)
    got, sides, sinf = gpu_ctx.schnorr_batch_verify_secp256k1(pk, r, s, a0, e)
    assert want == 1 and got is True and list(sinf) == [1, 1] and not sides.any()
    # identity inputs reject early; the empty batch is false
    inf = np.zeros(70, dtype=np.uint8)
    inf[69] = 1
    assert gpu_ctx.schnorr_batch_verify_secp256k1(pk, r, s, a0, e, pk_inf=inf)[0] is False
    assert gpu_ctx.schnorr_batch_verify_secp256k1(pk, r, s, a0, e, r_inf=inf)[0] is False
    z4, z8 = np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 8), dtype=np.uint64)
    assert gpu_ctx.schnorr_batch_verify_secp256k1(z8, z8, z4, z4, z4)[0] is False


def test_schnorr_batch_verify_p256_matches_oracle(gpu_ctx, oracle):
    """schnorr::batch_verify::<P256, D> (the generic function instantiated for P-256: its point arithmetic, its Scalar
    Mul, the five-lane ordered folds) through fec_schnorr_batch_verify; the secp256k1 instance through the same entry
    point equals the dedicated one."""
    def inputs(n, seed, curve):
        pk = V.field_elements(2 * n, curve, seed).reshape(n, 8)
        r = V.field_elements(2 * n, curve, seed + 1).reshape(n, 8)
        return pk, r, V.scalars(n, curve, seed + 2), V.scalars(n, curve, seed + 3), V.scalars(n, curve, seed + 4)

    for n, seed in ((1, 900), (5, 910), (64, 920), (300, 930)):
        pk, r, s, a, e = inputs(n, seed, 1)
        want, w_sides, w_inf = oracle.schnorr_batch_verify(1, pk, None, r, None, s, a, e)
        got, sides, sinf = gpu_ctx.schnorr_batch_verify(1, pk, r, s, a, e)
        assert got == bool(want) and np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf) and sides.any()
    pk, r, s, a, e = inputs(70, 940, 1)
    a[3] = 0
    e[5] = 0
    s[7] = 0
    want, w_sides, w_inf = oracle.schnorr_batch_verify(1, pk, None, r, None, s, a, e)
    got, sides, sinf = gpu_ctx.schnorr_batch_verify(1, pk, r, s, a, e)
    assert got == bool(want) and np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf)
    a0 = np.zeros_like(a)
    got, sides, sinf = gpu_ctx.schnorr_batch_verify(1, pk, r, s, a0, e)
    assert got is True and list(sinf) == [1, 1] and not sides.any()
    inf = np.zeros(70, dtype=np.uint8)
    inf[0] = 1
    assert gpu_ctx.schnorr_batch_verify(1, pk, r, s, a0, e, pk_inf=inf)[0] is False
    pk, r, s, a, e = inputs(33, 950, 0)
    g1, g2 = gpu_ctx.schnorr_batch_verify(0, pk, r, s, a, e), gpu_ctx.schnorr_batch_verify_secp256k1(pk, r, s, a, e)
    assert g1[0] == g2[0] and np.array_equal(g1[1], g2[1]) and np.array_equal(g1[2], g2[2])


def test_schnorr_batch_verify_ed25519_release_profile_matches_oracle(gpu_ctx, oracle):
    """schnorr::batch_verify::<Ed25519, D> through fec_schnorr_batch_verify_ed25519 (and the generic entry point): the
    scalar Mul of ed25519.rs:1256-1376 as the reference's RELEASE profile runs it (u128 sums wrap), the verdict, the two
    affine points of line 286 and the flag "a debug build panics on these inputs" -- the committed fixture (which holds
    the products the reference's own tests assert), random batches against the C oracle, zero weights, small scalars
    (no sum wraps: the flag stays clear), infinity flags."""
    import json
    import os
    t = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schnorr_vectors.json")))
    for b in t["batch_ed25519"]:
        res, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(b["pk"], b["r"], b["s"], b["a"], b["e"])
        assert res == b["result"] and dbg == bool(b["debug_build_panics"]), b["kind"]
        assert [int(v) for v in sides] == [v for fe in b["sides"] for v in fe] and list(sinf) == b["sides_inf"], b["kind"]
    assert {(b["result"], b["debug_build_panics"]) for b in t["batch_ed25519"]} >= {(0, 0), (0, 1), (1, 0)}

    def inputs(n, seed):
        pk = V.field_elements(2 * n, 2, seed).reshape(n, 8)
        r = V.field_elements(2 * n, 2, seed + 1).reshape(n, 8)
        return pk, r, V.scalars(n, 2, seed + 2), V.scalars(n, 2, seed + 3), V.scalars(n, 2, seed + 4)

    for n, seed in ((1, 1900), (5, 1910), (64, 1920), (257, 1930)):
        pk, r, s, a, e = inputs(n, seed)
        want, w_sides, w_inf, w_dbg = oracle.ed25519_schnorr_batch_verify(pk, None, r, None, s, a, e)
        got, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, a, e)
        assert got == want and dbg == bool(w_dbg) and np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf), n
        if n >= 5:
            assert dbg and sides.any()    # full-size scalars: some s_i * a_i wraps, a debug build would not get here
        g2 = gpu_ctx.schnorr_batch_verify(2, pk, r, s, a, e)   # the generic entry point: the same verdict and points
        assert g2[0] == (got == 1) and np.array_equal(g2[1], sides) and np.array_equal(g2[2], sinf)
    pk, r, s, a, e = inputs(70, 1940)
    a[3] = 0
    e[5] = 0
    s[7] = 0
    s[11] = (1 << 64) - 1
    a[11] = (1 << 64) - 1                      # all-ones operands: every column sum wraps
    want, w_sides, w_inf, w_dbg = oracle.ed25519_schnorr_batch_verify(pk, None, r, None, s, a, e)
    got, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, a, e)
    assert got == want and dbg == bool(w_dbg) and np.array_equal(sides, w_sides) and np.array_equal(sinf, w_inf)
    small_s, small_a = s.copy(), a.copy()
    small_s[:, 1:] = 0
    small_a[:, 1:] = 0                         # one limb each: one product per column, nothing can wrap
    want, w_sides, w_inf, w_dbg = oracle.ed25519_schnorr_batch_verify(pk, None, r, None, small_s, small_a, e)
    got, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(pk, r, small_s, small_a, e)
    assert not dbg and not w_dbg and got == want and np.array_equal(sides, w_sides)
    a0 = np.zeros_like(a)
    got, sides, sinf, dbg = gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, a0, e)
    assert got == 1 and list(sinf) == [1, 1] and not sides.any() and not dbg
    inf = np.zeros(70, dtype=np.uint8)
    inf[0] = 1
    assert gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, a0, e, pk_inf=inf)[0] == 0
    assert gpu_ctx.schnorr_batch_verify_ed25519(pk, r, s, a0, e, r_inf=inf)[0] == 0


@pytest.mark.parametrize("curve", CURVES)
def test_schnorr_verify_matches_oracle(gpu_ctx, oracle, curve):
    """Schnorr::<C, D>::verify per signature (schnorr.rs:90-140) from the point computation on: random inputs (the
    reference answers false: PointAffine::new(x, -y) is None), the fixture's cases -- for P-256 including signatures
    that VERIFY under the reference's arithmetic --, infinite R / infinite key, zero scalars, e = 1; host and
    device-pointer entry points, a ragged size."""
    import json
    import os
    import torch
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schnorr_vectors.json")) as f:
        fx = [c for c in json.load(f)["verify"] if c["curve"] == curve]
    n_random = 700
    n = n_random + len(fx) + 3
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, 961), V.field_elements(n, curve, 962)], axis=1))
    r = np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, 963), V.field_elements(n, curve, 964)], axis=1))
    s, e = V.scalars(n, curve, 965), V.scalars(n, curve, 966)
    pinf, rinf = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for j, c in enumerate(fx):
        i = n_random + j
        pk[i], r[i], s[i], e[i], pinf[i], rinf[i] = c["pk"], c["r"], c["s"], c["e"], c["pk_inf"], c["r_inf"]
    base = n_random + len(fx)
    s[base] = 0
    e[base + 1] = 0
    e[base + 2] = [1, 0, 0, 0]
    want = oracle.batch_schnorr_verify(curve, pk, pinf, r, rinf, s, e, nthreads=8)
    for j, c in enumerate(fx):
        assert int(want[n_random + j]) == c["status"], c["note"]
    if curve == 1:
        assert int((want == 1).sum()) >= 4
    got = gpu_ctx.schnorr_verify(curve, pk, r, s, e, pk_inf=pinf, r_inf=rinf)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first mismatch at %d: got %d want %d" % (bad[0], got[bad[0]], want[bad[0]])
    want2 = oracle.batch_schnorr_verify(curve, pk, None, r, None, s, e, nthreads=8)
    assert np.array_equal(gpu_ctx.schnorr_verify(curve, pk, r, s, e), want2)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (pk, pinf, r, rinf, s, e)]
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gpu_ctx.schnorr_verify_dev(curve, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                               t[5].data_ptr(), st.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    gpu_ctx.check()
    assert np.array_equal(st.cpu().numpy(), want)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_batch_compress_matches_oracle(gpu_ctx, oracle, curve):
    """PointAffine::to_bytes (compressed, 33 bytes) of affine points: identity flags, ragged sizes whose
    byte length is not a multiple of 4, non-canonical Ed25519 limbs, and points produced by the GPU's
    own to_affine of real ladder outputs."""
    for n, seed in ((1, 950), (3, 951), (255, 952), (258, 953), (1027, 954)):
        xy = V.field_elements(2 * n, curve, seed + 10 * curve).reshape(n, 8)
        raw = V.splitmix64(8 * min(n, 64), V.SEED, seed + 100).reshape(-1, 8)   # arbitrary limbs, >= p included
        xy[:raw.shape[0]] = raw if n > 64 else xy[:raw.shape[0]]
        inf = (V.splitmix64(n, V.SEED, seed + 200) % np.uint64(7) == 0).astype(np.uint8)
        want = oracle.batch_compress(curve, xy, inf)
        got = gpu_ctx.batch_compress(curve, xy, inf)
        assert np.array_equal(got, want), (curve, n)
        assert np.array_equal(gpu_ctx.batch_compress(curve, xy), oracle.batch_compress(curve, xy))
    k, p = V.scalars(200, curve, 960), V.points(200, curve, 961)
    pts = gpu_ctx.batch_mul(curve, k, p)
    axy, ainf = gpu_ctx.batch_to_affine(curve, pts)
    assert np.array_equal(gpu_ctx.batch_compress(curve, axy, ainf), oracle.batch_compress(curve, axy, ainf))
    assert gpu_ctx.batch_compress(curve, np.zeros((0, 8), dtype=np.uint64)).shape == (0, 33)
