"""
The carries that the secp256k1 ladder's fast step no longer computes (tools/gen_field_asm.py: FEC_SECP_MUL_ACC_ASM,
FEC_SECP_SQR_ACC_ASM), modelled on 32-bit words and checked against oracle/py_model.py.

Mul: the product scanning adds each 32 x 32-bit product into a 64-bit column accumulator and counts the carry out of
every such addition.  The fast statement drops the count behind the FIRST product of columns 2..13, where the
accumulator starts from the carry-in C < 9 * 2^32: it can pass 2^64 only if both factors are >= 2^32 - 9, and one of
them is always a_0 (columns 2..7) or b_7 (columns 8..13).  The caller flags a lane with a_0 or b_7 >= RARE_WORD.

square(): the +1 of cross term (i, j) enters limb L = i + j + 2 at its low word W[2L]; the fast statement drops the
carry from there into W[2L + 1].  W[2L] is what the limb squares left: it must be all ones to wrap (>= 0xFFFFFFFE for
L = 5, which takes two +1 in one chain), and for L = 4, 6 it is the low word of a square, never 3 mod 4, so never all
ones.  The statement flags a lane with W[6], W[10] or W[14] >= RARE_WORD.

Both models run in two forms, with and without the dropped carries.  Asserted: a dropped carry fires only on flagged
lanes (random operands biased towards words near 2^32, and a crafted grid), unflagged lanes compute what py_model
computes, the dead ripples are dead, and every row of tests/golden/secp256k1_rare_carry_operands.json does what its
label says.
"""
import itertools
import json
import os

import numpy as np

from oracle.py_model import Secp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "secp256k1_rare_carry_operands.json")))

RARE_WORD = 0xFFFFFFF0  # secp_step.hpp
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
WORDS = [0, 1, 0xFFFFFFEF, 0xFFFFFFF0, 0xFFFFFFFE, 0xFFFFFFFF]
CROSS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
PLUS_ONE = [t for t in CROSS if t != (0, 3)]  # (0, 3)'s +1 waits for (1, 2)'s chain


def words_of(limbs):
    """(n, 4) 64-bit limbs -> (n, 8) 32-bit words, each in a uint64"""
    limbs = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    w = np.empty((limbs.shape[0], 8), dtype=np.uint64)
    w[:, 0::2] = limbs & M32
    w[:, 1::2] = limbs >> S32
    return w


def limbs_of_words(w):
    return [int(w[2 * i]) | (int(w[2 * i + 1]) << 32) for i in range(len(w) // 2)]


# ---- Mul: mul_wide_columns ----
def mul_scan(a, b, drop):
    """The column scan on (n, 8) words.  Returns the 16 product words and, per column, whether the carry out of its
    first product fired.  drop: the fast statement, which does not count that carry in columns 2..13."""
    n = a.shape[0]
    t = np.zeros((n, 16), dtype=np.uint64)
    fired = np.zeros((n, 15), dtype=bool)
    c_lo = np.zeros(n, dtype=np.uint64)
    ovf = np.zeros(n, dtype=np.uint64)
    for k in range(15):
        q = None
        for idx, i in enumerate(range(max(0, k - 7), min(k, 7) + 1)):
            p = a[:, i] * b[:, k - i]
            q = p + ((c_lo | (ovf << S32)) if idx == 0 else q)
            cy = (q < p).astype(np.uint64)
            if idx == 0:
                if 2 <= k <= 13:
                    fired[:, k] = cy != 0
                    if not drop:
                        ovf = cy  # the overflow word restarts here
                else:
                    assert not cy.any()  # columns 0, 1 (carry-in < 2^32) and 14 (bounded by the true product)
            elif idx == 1 and drop and k >= 2:
                ovf = cy  # ... or here, from the zero register
            else:
                ovf = ovf + cy
        t[:, k] = q & M32
        if k == 14:
            t[:, 15] = q >> S32
        else:
            c_lo = q >> S32
    return t, fired


def mont_reduce(t):
    """secp256k1.hpp mont_reduce on one row of product words: csub_p((T_hi + M - Q) mod 2^256)"""
    t = [int(x) for x in t]
    m, e = [], 0
    for k in range(8):
        mk = ((t[k] - (e & 0xFFFFFFFF)) * 0xD2253531) & 0xFFFFFFFF
        m.append(mk)
        e = ((mk * 977 + e) >> 32) + mk
    val = lambda ws: sum(w << (32 * i) for i, w in enumerate(ws))
    v = (val(t[8:]) + val(m) - e) % (1 << 256)
    p = (1 << 256) - (1 << 32) - 977
    v = v - p if v >= p else v
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def mul_flag(a, b):
    return np.maximum(a[:, 0], b[:, 7]) >= np.uint64(RARE_WORD)


# ---- square(): limb squares and cross terms of secp_sqr ----
def mul64(x0, x1, y0, y1):
    """four words of (x1:x0) * (y1:y0), as the statement's mul64"""
    pa = x0 * y0
    pb = x0 * y1 + (pa >> S32)
    pb2 = x1 * y0
    pb = pb + pb2
    cy = (pb < pb2).astype(np.uint64)
    pc = x1 * y1 + ((pb >> S32) | (cy << S32))
    return [pa & M32, pb & M32, pc & M32, pc >> S32]


def add32(x, y, c):
    s = x + y + c
    return s & M32, s >> S32


def sqr_cross(a, drop):
    """W[0..15] after the cross terms; fired[term]: the carry from W[2L] into W[2L + 1] (which drop omits);
    left: W as the limb squares left it."""
    n = a.shape[0]
    zero = np.zeros(n, dtype=np.uint64)
    w = [None] * 16
    for i in range(4):
        w[4 * i:4 * i + 4] = mul64(a[:, 2 * i], a[:, 2 * i + 1], a[:, 2 * i], a[:, 2 * i + 1])
    left = list(w)
    fired, e3 = {}, None
    for i, j in CROSS:
        p = mul64(a[:, 2 * i], a[:, 2 * i + 1], a[:, 2 * j], a[:, 2 * j + 1])
        p = [(p[0] << np.uint64(1)) & M32] + [((p[k] << np.uint64(1)) | (p[k - 1] >> np.uint64(31))) & M32 for k in (1, 2, 3)]
        B = 2 * (i + j)
        w[B], c = add32(w[B], p[0], zero)
        w[B + 1], carry = add32(w[B + 1], p[1], c)
        w[B + 2], c = add32(w[B + 2], p[2], zero)
        w[B + 3], carry2 = add32(w[B + 3], p[3], c)
        one = carry | carry2
        if (i, j) == (0, 3):
            e3 = one
            continue
        w[B + 4], c = add32(w[B + 4], e3 if (i, j) == (1, 2) else zero, one)
        fired[(i, j)] = c != 0
        if not drop:
            w[B + 5], _ = add32(w[B + 5], zero, c)
    return w, fired, left


def sqr_flag(left):
    return np.maximum(np.maximum(left[6], left[10]), left[14]) >= np.uint64(RARE_WORD)


def sqr_finish(wrow):
    """the folds (681-707) and reduce of py_model.Secp.sqr on one row of product words"""
    product = limbs_of_words(wrow)
    M64 = (1 << 64) - 1
    result, carry = product[0:4], 0
    for i in range(4, 8):
        m = (product[i] * 0x1000003D1) & M64
        t = (result[0] + m + carry) & M64
        result[0] = t
        carry = (1 if t < m else 0) | ((1 if t < carry else 0) & (1 if m != 0 else 0))
        for j in range(1, 4):
            t2 = (result[j] + carry) & M64
            result[j] = t2
            carry = 1 if t2 < carry else 0
    return Secp.reduce(result)


# ---- inputs ----
def biased_words(n, seed):
    """(n, 8) words: three in eight within 12 of 2^32 (both sides of 2^32 - 9), one in eight below 32, the rest uniform"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64)
    near = np.uint64(1 << 32) - rng.integers(1, 13, size=(n, 8), dtype=np.uint64)
    small = rng.integers(0, 32, size=(n, 8), dtype=np.uint64)
    pick = rng.integers(0, 8, size=(n, 8))
    return np.where(pick < 3, near, np.where(pick == 3, small, u))


def mul_grid():
    """the crafted words in a_0, b_7 and their neighbours a_1, b_6, over operands of all ones, of zeros and random"""
    rows_a, rows_b = [], []
    rng = np.random.default_rng(77)
    for fill in ("ones", "zeros", "random"):
        base = {"ones": np.full(8, 0xFFFFFFFF, dtype=np.uint64), "zeros": np.zeros(8, dtype=np.uint64)}.get(fill)
        for a0, a1, b6, b7 in itertools.product(WORDS, repeat=4):
            a = base.copy() if base is not None else rng.integers(0, 1 << 32, size=8, dtype=np.uint64)
            b = base.copy() if base is not None else rng.integers(0, 1 << 32, size=8, dtype=np.uint64)
            a[0], a[1], b[6], b[7] = a0, a1, b6, b7
            rows_a.append(a)
            rows_b.append(b)
    return np.array(rows_a), np.array(rows_b)


def check_mul(a, b, compare):
    t_exact, fired = mul_scan(a, b, drop=False)
    t_fast, fired2 = mul_scan(a, b, drop=True)
    flag = mul_flag(a, b)
    any_fired = fired.any(axis=1)
    assert not (any_fired & ~flag).any(), "a dropped carry fired on an unflagged lane"
    same = (t_exact == t_fast).all(axis=1)
    assert same[~any_fired].all() and not same[any_fired].any()  # the fast scan is wrong exactly where one fires
    for r in compare:
        al, bl = limbs_of_words(a[r]), limbs_of_words(b[r])
        want = Secp.mul(al, bl)
        assert mont_reduce(t_exact[r]) == want, (al, bl)
        if not flag[r]:
            assert mont_reduce(t_fast[r]) == want, (al, bl)
    return any_fired, flag


def check_sqr(a, compare):
    w_exact, fired, left = sqr_cross(a, drop=False)
    w_fast, _, _ = sqr_cross(a, drop=True)
    flag = sqr_flag(left)
    any_fired = np.zeros(a.shape[0], dtype=bool)
    for t in PLUS_ONE:
        any_fired |= fired[t]
    assert not (any_fired & ~flag).any(), "a dropped ripple fired on an unflagged lane"
    assert not fired[(0, 2)].any() and not fired[(1, 3)].any()  # L = 4, 6: dead
    w_fast = np.stack(w_fast, axis=1)
    for r in compare:
        if not flag[r]:
            al = limbs_of_words(a[r])
            assert sqr_finish(w_fast[r]) == Secp.sqr(al), al
    return fired, flag


# ---- tests ----
N_RANDOM = 100000


def test_mul_dropped_carries_only_on_flagged_lanes_random():
    a, b = biased_words(N_RANDOM, 1), biased_words(N_RANDOM, 2)
    any_fired, flag = check_mul(a, b, compare=range(0, N_RANDOM, 50))
    # the biased draw does reach the carries, on both sides, and leaves most lanes unflagged
    _, fired = mul_scan(a, b, drop=False)
    assert fired[:, 2:8].any() and fired[:, 8:14].any() and any_fired.sum() > 100 and (~flag).sum() > N_RANDOM // 4


def test_mul_dropped_carries_only_on_flagged_lanes_uniform():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 32, size=(20000, 8), dtype=np.uint64)
    b = rng.integers(0, 1 << 32, size=(20000, 8), dtype=np.uint64)
    check_mul(a, b, compare=range(0, 20000, 10))


def test_mul_crafted_grid():
    a, b = mul_grid()
    any_fired, flag = check_mul(a, b, compare=range(a.shape[0]))
    assert any_fired.any() and (~flag).any()


def test_mul_bound_is_tight_enough():
    """both factors >= 2^32 - 9 is necessary: the largest product with one factor at 2^32 - 10 plus the largest
    carry-in stays below 2^64; and RARE_WORD is below 2^32 - 9"""
    assert (2 ** 32 - 10) * (2 ** 32 - 1) + 9 * 2 ** 32 - 1 < 2 ** 64
    assert RARE_WORD <= 2 ** 32 - 10
    # the carry-in bound: eight products and a carry-in below 9 * 2^32 hand on less than 9 * 2^32
    assert (8 * (2 ** 32 - 1) ** 2 + 9 * 2 ** 32 - 1) >> 32 < 9 * 2 ** 32


def test_sqr_dropped_ripples_only_on_flagged_lanes_random():
    a = biased_words(N_RANDOM, 4)
    check_sqr(a, compare=range(0, N_RANDOM, 50))


def test_sqr_crafted_grid():
    """operands around the fixture's square rows: the limb words that decide W[6], W[10], W[14] varied over WORDS"""
    rows = []
    for row in FIXTURE["sqr"]:
        base = words_of([row["a"]])[0]
        for pos in range(8):
            for wv in WORDS:
                x = base.copy()
                x[pos] = wv
                rows.append(x)
    a = np.array(rows)
    check_sqr(a, compare=range(a.shape[0]))


def test_sqr_dead_ripples():
    """L = 4 and L = 6: W[8] and W[12] are x^2 mod 2^32 for the 32-bit low word x of limbs 2 and 3.  x = 2y + r:
    x^2 = 4 (y^2 + y r) + r^2 is 0 or 1 mod 4, all ones is 3 mod 4; so W + 1 never wraps, for any x."""
    assert sorted({(x * x) % 4 for x in range(4)}) == [0, 1] and 0xFFFFFFFF % 4 == 3
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.integers(0, 1 << 32, size=200000, dtype=np.uint64), np.array(WORDS, dtype=np.uint64),
                        np.arange(1 << 16, dtype=np.uint64), M32 - np.arange(1 << 16, dtype=np.uint64)])
    assert not (((x * x) & M32) == M32).any()
    # and through the model, with every cross term's +1 arriving: limbs of all ones but for the low words
    a = np.full((x.shape[0], 8), 0xFFFFFFFF, dtype=np.uint64)
    a[:, 4], a[:, 6] = x, x[::-1]
    _, fired, _ = sqr_cross(a, drop=False)
    assert not fired[(0, 2)].any() and not fired[(1, 3)].any()


def test_fixture_rows_do_what_they_say():
    p = (1 << 256) - (1 << 32) - 977
    val = lambda l: sum(int(x) << (64 * i) for i, x in enumerate(l))
    seen = set()
    for row in FIXTURE["mul"]:
        a, b = words_of([row["a"]]), words_of([row["b"]])
        assert val(row["a"]) < p and val(row["b"]) < p
        _, fired = mul_scan(a, b, drop=False)
        cols = [k for k in range(15) if fired[0, k]]
        assert cols == row["columns"], row
        assert bool(mul_flag(a, b)[0]) == row["flagged"], row
        if row["kind"] == "fires":
            assert cols and row["flagged"]
            seen.add("a0" if min(cols) <= 7 else "b7")
            if max(cols) >= 8:
                seen.add("b7")
        elif row["kind"] == "below":  # 0xFFFFFFEF: not flagged, nothing may fire
            assert not cols and not row["flagged"] and 0xFFFFFFEF in (int(a[0, 0]), int(b[0, 7]))
        else:  # at the threshold: flagged, nothing fires
            assert row["kind"] == "threshold" and not cols and row["flagged"]
            assert RARE_WORD in (int(a[0, 0]), int(b[0, 7]))
        check_mul(a, b, compare=[0])
    assert seen == {"a0", "b7"}
    limbs = set()
    for row in FIXTURE["sqr"]:
        a = words_of([row["a"]])
        assert val(row["a"]) < p
        _, fired, left = sqr_cross(a, drop=False)
        got = sorted(i + j + 2 for (i, j) in PLUS_ONE if fired[(i, j)][0])
        assert got == row["limbs"], row
        assert bool(sqr_flag(left)[0]) == row["flagged"], row
        if row["kind"] == "fires":
            assert got and row["flagged"]
            limbs.update(got)
        elif row["kind"] == "both_plus_ones":  # L = 5 from 0xFFFFFFFE: only the two +1 together wrap it
            assert got == [5] and int(left[10][0]) == 0xFFFFFFFE
            limbs.add("5b")
        elif row["kind"] == "below":
            assert not got and not row["flagged"] and 0xFFFFFFEF in [int(left[k][0]) for k in (6, 10, 14)]
        else:
            assert row["kind"] == "threshold" and not got and row["flagged"]
        check_sqr(a, compare=[0])
    assert limbs == {3, 5, 7, "5b"}
