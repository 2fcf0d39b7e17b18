"""
The case table of the ordered folds' early-outs (tests/test_fold_cases_model.py checks it on the oracle alone,
tests/test_gpu_fold_legs.py runs it through fec_debug_fold_terms, tests/test_coop_wave_model.py through the host wavefront
of tests/cpp/coop_wave.cpp).

A case is a list of terms -- raw projective (Ed25519: extended) limbs -- folded left to right from the identity with the
reference's Add; its expectation is the oracle's fold.  Every step of a case carries the LEG the reference's Add takes there:

  secp256k1, P-256   idp (p is the identity: returns q), idq (q is the identity: returns p), double (u1 == u2, s1 == s2:
                     returns double(p)), cancel (secp256k1: u1 == u2, s1 != s2; P-256: u1 == u2, s1 == neg(s2): returns the
                     identity), none (the general formula).  P-256 only: ueq_general, u1 == u2 with s1 neither s2 nor
                     neg(s2) -- the near miss, on which the reference takes the general formula.
  Ed25519            idp, idq, opposite (x1 == neg(x2) and y1 == y2 on the raw coordinates: returns the identity), none.
                     Add has no doubling branch: a term equal to the running sum is an ordinary addition (kind "same"),
                     and so is a near miss of `opposite` with only one of its two equalities (kinds "near_x", "near_y").

The labels are written down from what each term is BUILT to be (an identity, a copy of the running sum, ...); the model
test recomputes every step's leg from the oracle's field operations and compares.

A step is a KIND of term placed at an index of a chain of ordinary terms (distinct multiples of the generator):
  ident_canon     the reference's identity()
  ident_noncanon  another representative of the identity: (x, y, 0) with random x, y; Ed25519 (0, c, c, 0).  Where both
                  operands are identities the reference returns q, so the order of the selects decides the result
  ident_zero      all limbs zero: the identity on all three curves, with u1 == u2 and s1 == s2 == neg(s2) on the
                  Weierstrass curves, so every early-out's condition holds at once
  same            a copy of the running sum the oracle gives (at index 1: the pair [T, T])
  scaled          Weierstrass: the running sum as (x l^2, y l^3, z l), another representative of the same point
  cancel          secp256k1: the running sum's X and Z with Y + 1; P-256: (x, neg y, z); Ed25519: (neg x, y, z, neg t)
  near            P-256: the running sum's X and Z with Y + 1 (ueq_general); Ed25519 near_x: (neg x, y + 1, z, neg t),
                  near_y: (x + 1, y, z, t)
  x_zero          Ed25519: the point (0, -1) -- x == neg x, so adding it to itself takes `opposite`
  ident_match_y   Ed25519, after x_zero: the identity (0, y, y, 0) with the running sum's y, so that idq and `opposite` hold
                  together and the reference returns p
Lengths 2, 3, 16 and 65, the kind at index 0 (identities only), 1, the middle and the last index: an early-out beside the
prefetch of the next term, and in the last iteration.

SCALED: whether the reference's arithmetic keeps u1 == u2 and s1 == s2 for the scaled representative.
  P-256      it does (40 of 40 scale factors tried): every product is reduced below p, so equal values are equal limbs.
  secp256k1  it does NOT, so the table has no such case: the reference's square() is not Mul(a, a) there (and
             square(a b) != square(a) square(b)), so x2 z1^2 and x1 z2^2 differ for every scale factor tried (0 of 40);
             solving x2, y2 from the two equalities with the reference's invert(), or with a Fermat inverse made of Mul
             alone, does not give them either (0 of 20, 0 of 6).  On secp256k1 only a bit-identical copy of the running sum
             ("same") takes the doubling.
The model test fails if a "scaled" case stops taking the doubling, or if SCALED disagrees with the table.
"""
import numpy as np

import vectors as V

SECP, P256, ED = 0, 1, 2
NAMES = {SECP: "secp256k1", P256: "p256", ED: "ed25519"}
LENGTHS = (2, 3, 16, 65)
POOL = 80            # ordinary terms per curve
SCALED = {SECP: False, P256: True}

WEIERSTRASS_LEGS = ("idp", "idq", "double", "cancel")
LEGS = {SECP: WEIERSTRASS_LEGS, P256: WEIERSTRASS_LEGS + ("ueq_general",), ED: ("idp", "idq", "opposite")}


def _fe(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


class Field:
    """The oracle's field operations of one curve on (4,) uint64 limbs."""

    def __init__(self, oracle, curve):
        self.o, self.c = oracle, curve

    def op(self, name, a, b=None):
        return self.o.field_op(self.c, name, _fe(a), None if b is None else _fe(b))

    def add(self, a, b): return self.op("add", a, b)
    def sub(self, a, b): return self.op("sub", a, b)
    def mul(self, a, b): return self.op("mul", a, b)
    def sqr(self, a): return self.op("sqr", a)
    def neg(self, a): return self.op("neg", a)


ZERO = np.zeros(4, dtype=np.uint64)
ONE = np.array([1, 0, 0, 0], dtype=np.uint64)


def coords(curve, p):
    p = _fe(p)
    return [p[4 * i:4 * i + 4] for i in range(4 if curve == ED else 3)]


def point(*cs):
    return np.concatenate([_fe(c) for c in cs])


class Case:
    def __init__(self, curve, name, terms, legs, kinds, expect, sums):
        self.curve, self.name = curve, name
        self.terms = np.ascontiguousarray(np.array(terms, dtype=np.uint64).reshape(len(terms), -1))
        self.legs = legs        # the leg of every step, "none" for the general formula
        self.kinds = kinds      # what every term was built as, "ord" for an ordinary one
        self.expect = expect    # the oracle's fold
        self.sums = sums        # the running sum after every step

    def special(self):
        """(index, kind, leg) of every term that is not an ordinary one"""
        return [(i, k, self.legs[i]) for i, k in enumerate(self.kinds) if k != "ord"]

    def describe(self):
        return "%s %s [%s]" % (NAMES[self.curve], self.name, ", ".join("%s@%d:%s" % (k, i, l) for i, k, l in self.special()))


class Builder:
    """Appends terms to one chain, following the running sum with the oracle's Add."""

    def __init__(self, oracle, curve, pool, rnd, start=0):
        self.o, self.c, self.f = oracle, curve, Field(oracle, curve)
        self.pool, self.rnd, self.next = pool, rnd, start
        self.acc = oracle.identity(curve)
        self.terms, self.legs, self.kinds, self.sums = [], [], [], []

    def finite(self):
        return not self.o.is_identity(self.c, self.acc)

    def _push(self, term, kind, leg):
        self.terms.append(_fe(term))
        self.kinds.append(kind)
        self.legs.append(leg)
        self.acc = self.o.point_add(self.c, self.acc, term)
        self.sums.append(self.acc.copy())

    def _random(self):
        self.rnd[0] += 1
        return V.field_elements(1, self.c, 900 + self.rnd[0])[0]

    def ordinary(self, count=1):
        for _ in range(count):
            t = self.pool[self.next % len(self.pool)]
            self.next += 1
            self._push(t, "ord", "none" if self.finite() else "idp")

    def add(self, kind):
        c, f = self.c, self.f
        leg_ident = "idq" if self.finite() else "idp"
        if kind == "ident_canon":
            return self._push(self.o.identity(c), kind, leg_ident)
        if kind == "ident_zero":
            return self._push(np.zeros(self.acc.size, dtype=np.uint64), kind, leg_ident)
        if kind == "ident_noncanon":
            if c == ED:
                y = self._random()
                return self._push(point(ZERO, y, y, ZERO), kind, leg_ident)
            return self._push(point(self._random(), self._random(), ZERO), kind, leg_ident)
        if kind == "x_zero":    # Ed25519: (0, -1), which is not the identity
            return self._push(point(ZERO, f.neg(ONE), ONE, ZERO), kind, "none" if self.finite() else "idp")
        assert self.finite(), "%s needs a finite running sum" % kind
        cs = coords(c, self.acc)
        if kind == "ident_match_y":   # Ed25519: the identity (0, y, y, 0) with the running sum's y -- after x_zero, `opposite` holds too
            assert c == ED
            return self._push(point(ZERO, cs[1], cs[1], ZERO), kind, "idq")
        if kind == "same":
            if c == ED:   # an ordinary addition, unless x == neg x
                x_self_opposite = np.array_equal(cs[0], f.neg(cs[0]))
                return self._push(self.acc.copy(), kind, "opposite" if x_self_opposite else "none")
            return self._push(self.acc.copy(), kind, "double")
        if kind == "scaled":
            l = self._random()
            l2 = f.sqr(l)
            return self._push(point(f.mul(cs[0], l2), f.mul(cs[1], f.mul(l2, l)), f.mul(cs[2], l)), kind, "double")
        if kind == "cancel":
            if c == SECP:
                return self._push(point(cs[0], f.add(cs[1], ONE), cs[2]), kind, "cancel")
            if c == P256:
                return self._push(point(cs[0], f.neg(cs[1]), cs[2]), kind, "cancel")
            return self._push(point(f.neg(cs[0]), cs[1], cs[2], f.neg(cs[3])), kind, "opposite")
        if kind == "near":
            assert c == P256
            return self._push(point(cs[0], f.add(cs[1], ONE), cs[2]), kind, "ueq_general")
        if kind == "near_x":
            assert c == ED
            return self._push(point(f.neg(cs[0]), f.add(cs[1], ONE), cs[2], f.neg(cs[3])), kind, "none")
        if kind == "near_y":
            assert c == ED
            return self._push(point(f.add(cs[0], ONE), cs[1], cs[2], cs[3]), kind, "none")
        raise ValueError(kind)

    def case(self, name):
        return Case(self.c, name, self.terms, self.legs, self.kinds, self.acc.copy(), self.sums)


IDENTS = ("ident_canon", "ident_noncanon", "ident_zero")
KINDS = {
    SECP: IDENTS + ("same", "scaled", "cancel"),
    P256: IDENTS + ("same", "scaled", "cancel", "near"),
    ED: IDENTS + ("same", "cancel", "near_x", "near_y"),
}
# the chains with more than one special term: (name, steps), a step an ordinary-term count or a kind
COMPOSITES = [
    ("two_idents_at_start", ["ident_noncanon", "ident_noncanon", 2]),
    ("three_idents_at_start", ["ident_zero", "ident_canon", "ident_noncanon", 1]),
    ("two_idents_mid", [3, "ident_canon", "ident_noncanon", 2]),
    ("two_idents_last", [2, "ident_noncanon", "ident_zero"]),
    ("only_idents", ["ident_canon", "ident_canon", "ident_canon"]),
    ("cancel_then_ordinary", [2, "cancel", 3]),
    ("cancel_then_ident", [2, "cancel", "ident_noncanon", 2]),
    ("cancel_then_ident_last", [3, "cancel", "ident_canon"]),
    ("cancel_at_1_then_same", [1, "cancel", 1, "same", 1]),
    ("same_twice", [1, "same", "same", 1]),
    ("same_then_cancel_last", [1, "same", 2, "cancel"]),
    ("ident_then_same_last", [2, "ident_canon", "same"]),
]
ED_COMPOSITES = [
    ("x_zero_twice", ["x_zero", "same", 2]),             # [T, T] with x == 0: `opposite` on x == neg x
    ("x_zero_twice_last", [0, "x_zero", "same"]),
    ("x_zero_mid", [2, "x_zero", 2]),                    # an ordinary addition of a point with x == 0
    # q an identity while `opposite` holds as well (x1 == neg 0, y1 == y2): the reference returns p, so idq's select comes after
    ("x_zero_then_ident_match_y", ["x_zero", "ident_match_y", 2]),
    ("x_zero_then_ident_match_y_last", [2, "cancel", "x_zero", "ident_match_y"]),
]

_TABLES = {}


def positions(length):
    return sorted({0, 1, length // 2, length - 1})


def cases(oracle, curve):
    """The table of one curve (built once per process)."""
    if curve in _TABLES:
        return _TABLES[curve]
    pool = oracle.batch_mul_fixed(curve, V.scalars(POOL, curve, 881), oracle.generator(curve))
    assert len({p.tobytes() for p in pool}) == POOL
    rnd, out, start = [100 * curve], [], 0
    for length in LENGTHS:
        for kind in KINDS[curve]:
            if kind == "scaled" and not SCALED[curve]:
                continue
            for pos in positions(length):
                if pos == 0 and kind not in IDENTS:
                    continue   # the running sum is still the identity
                b = Builder(oracle, curve, pool, rnd, start)
                start += 7
                b.ordinary(pos)
                b.add(kind)
                b.ordinary(length - pos - 1)
                out.append(b.case("%s_n%d_at%d" % (kind, length, pos)))
    # the running sum back at the identity before the LAST term (idp in the last iteration), at the longer lengths too
    long_tails = [("cancel_then_%s_last_n%d" % (what if isinstance(what, str) else "ordinary", length), [length - 2, "cancel", what])
                  for length in LENGTHS[2:] for what in (1, "ident_noncanon")]
    for name, steps in COMPOSITES + long_tails + (ED_COMPOSITES if curve == ED else []):
        b = Builder(oracle, curve, pool, rnd, start)
        start += 7
        for s in steps:
            b.ordinary(s) if isinstance(s, int) else b.add(s)
        out.append(b.case(name))
    assert len({c.name for c in out}) == len(out)
    _TABLES[curve] = out
    return out


def ordinary_replacement(oracle, curve, index):
    """An ordinary term that no case uses (for `the same chain with the special term replaced'), one per index."""
    k = V.scalars(1, curve, 7000 + index)
    return oracle.batch_mul_fixed(curve, k, oracle.generator(curve))[0]


def fold(oracle, curve, terms):
    acc = oracle.identity(curve)
    for t in terms:
        acc = oracle.point_add(curve, acc, t)
    return acc


def _hex(limbs):
    return " ".join("%016x" % int(v) for v in limbs)


def write_case_file(oracle, path):
    """The table for tests/cpp/coop_wave.cpp: per case `case <curve> <name> <n>`, n lines of a term's limbs in hexadecimal,
    and `sum` with the oracle's fold."""
    with open(path, "w") as f:
        for curve in (SECP, P256, ED):
            for c in cases(oracle, curve):
                f.write("case %d %s %d\n" % (curve, c.name, len(c.terms)))
                for t in c.terms:
                    f.write(_hex(t) + "\n")
                f.write("sum " + _hex(c.expect) + "\n")
