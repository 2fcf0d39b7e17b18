"""
The premise of tests/fold_cases.py, on the oracle alone (no GPU, no device header): every case takes the legs of the
reference's Add it is labelled with, every leg has cases at more than one index, and a leg that was skipped -- the general
formula in its place, or an ordinary term in the special term's place -- would change what the case expects.

Every step's operands are classified here from the oracle's FIELD operations (z == 0; u1, u2, s1, s2 as Add computes them;
Ed25519: the raw-coordinate tests), independently of the labels, which fold_cases.py writes down from how it builds a term.
"""
import numpy as np
import pytest

import fold_cases as FC
from fold_cases import ED, P256, SECP, Field, coords

CURVES = (SECP, P256, ED)


def _eq(a, b):
    return np.array_equal(a, b)


def _zero(a):
    return not np.any(a)


def flags(f, curve, p, q):
    """The conditions of Add's early-outs on (p, q), each by itself"""
    P, Q = coords(curve, p), coords(curve, q)
    if curve == ED:
        return {"idp": _zero(P[0]) and _eq(P[1], P[2]) and _zero(P[3]),
                "idq": _zero(Q[0]) and _eq(Q[1], Q[2]) and _zero(Q[3]),
                "x_opposite": _eq(P[0], f.neg(Q[0])), "y_equal": _eq(P[1], Q[1])}
    z1s, z2s = f.sqr(P[2]), f.sqr(Q[2])
    u1, u2 = f.mul(P[0], z2s), f.mul(Q[0], z1s)
    if curve == SECP:
        s1, s2 = f.mul(P[1], f.mul(z2s, Q[2])), f.mul(Q[1], f.mul(z1s, P[2]))
    else:
        s1, s2 = f.mul(f.mul(P[1], Q[2]), z2s), f.mul(f.mul(Q[1], P[2]), z1s)
    return {"idp": _zero(P[2]), "idq": _zero(Q[2]), "ueq": _eq(u1, u2), "seq": _eq(s1, s2), "sopp": _eq(s1, f.neg(s2))}


def leg(curve, fl):
    """The branch the reference's Add takes"""
    if fl["idp"]:
        return "idp"
    if fl["idq"]:
        return "idq"
    if curve == ED:
        return "opposite" if fl["x_opposite"] and fl["y_equal"] else "none"
    if not fl["ueq"]:
        return "none"
    if fl["seq"]:
        return "double"
    if curve == SECP:
        return "cancel"
    return "cancel" if fl["sopp"] else "ueq_general"


def general(f, curve, p, q):
    """Add's general formula with no early-out, from the oracle's field operations"""
    P, Q = coords(curve, p), coords(curve, q)
    if curve == ED:
        d = np.array([0x75EB4DCA135EDEFF, 0x00E0149A8283B156, 0x198E80F2EEF3D130, 0x2406875CC61A8E3C], dtype=np.uint64)   # the oracle's E_D
        a = f.mul(f.sub(P[1], P[0]), f.sub(Q[1], Q[0]))
        b = f.mul(f.add(P[1], P[0]), f.add(Q[1], Q[0]))
        c = f.mul(f.mul(P[3], Q[3]), d)
        dd = f.mul(P[2], Q[2])
        e, ff, g, h = f.sub(b, a), f.sub(dd, c), f.add(dd, c), f.add(b, a)
        return FC.point(f.mul(e, ff), f.mul(g, h), f.mul(ff, g), f.mul(e, h))
    z1s, z2s = f.sqr(P[2]), f.sqr(Q[2])
    u1, u2 = f.mul(P[0], z2s), f.mul(Q[0], z1s)
    if curve == SECP:
        s1, s2 = f.mul(P[1], f.mul(z2s, Q[2])), f.mul(Q[1], f.mul(z1s, P[2]))
        h, r = f.sub(u2, u1), f.sub(s2, s1)
        h2 = f.sqr(h)
        h3, u1h2 = f.mul(h2, h), f.mul(u1, h2)
        x3 = f.sub(f.sub(f.sub(f.sqr(r), h3), u1h2), u1h2)
        y3 = f.sub(f.mul(r, f.sub(u1h2, x3)), f.mul(s1, h3))
        return FC.point(x3, y3, f.mul(f.mul(h, P[2]), Q[2]))
    s1, s2 = f.mul(f.mul(P[1], Q[2]), z2s), f.mul(f.mul(Q[1], P[2]), z1s)
    h = f.sub(u2, u1)
    i = f.sqr(f.add(h, h))
    j = f.mul(h, i)
    s21 = f.sub(s2, s1)
    r = f.add(s21, s21)
    v = f.mul(u1, i)
    x3 = f.sub(f.sub(f.sub(f.sqr(r), j), v), v)
    y3 = f.sub(f.mul(r, f.sub(v, x3)), f.mul(f.add(s1, s1), j))
    z3 = f.mul(f.sub(f.sub(f.sqr(f.add(P[2], Q[2])), z1s), z2s), h)
    return FC.point(x3, y3, z3)


@pytest.fixture(scope="module")
def walked(oracle):
    """Every step of every case, classified once: {curve: [(case, [(p, q, flags, leg)])]}"""
    out = {}
    for curve in CURVES:
        f, rows = Field(oracle, curve), []
        for c in FC.cases(oracle, curve):
            acc, steps = oracle.identity(curve), []
            for i, t in enumerate(c.terms):
                fl = flags(f, curve, acc, t)
                steps.append((acc, t, fl, leg(curve, fl)))
                acc = oracle.point_add(curve, acc, t)
                assert _eq(acc, c.sums[i]), c.describe()
            assert _eq(acc, c.expect), c.describe()
            rows.append((c, steps))
        out[curve] = rows
    return out


def test_general_formula_is_the_oracles_add_on_ordinary_steps(oracle, walked):
    """general() restates Add's formulas (and Ed25519's constant d): on every step without an early-out it is the oracle's Add"""
    for curve in CURVES:
        f, seen = Field(oracle, curve), 0
        for c, steps in walked[curve]:
            if len(c.terms) > 16:
                continue
            for i, (p, q, fl, l) in enumerate(steps):
                if l == "none":
                    assert _eq(general(f, curve, p, q), c.sums[i]), (c.describe(), i)
                    seen += 1
        assert seen > 100


@pytest.mark.parametrize("curve", CURVES)
def test_every_case_takes_exactly_its_legs(walked, curve):
    for c, steps in walked[curve]:
        got = [s[3] for s in steps]
        assert got == c.legs, "%s: takes %s" % (c.describe(), got)
        assert got[0] == "idp"   # every fold starts from the identity
        assert [l for l in got if l != "none"], c.describe()


@pytest.mark.parametrize("curve", CURVES)
def test_every_leg_has_cases_at_two_indices(walked, curve):
    where = {l: set() for l in FC.LEGS[curve]}
    for c, steps in walked[curve]:
        for i, s in enumerate(steps):
            if s[3] != "none" and (i > 0 or c.kinds[0] != "ord"):   # (term 0 of an ordinary start is every fold's idp)
                where[s[3]].add((c.name, i))
    for l, hits in where.items():
        assert len({n for n, _ in hits}) >= 2 and len({i for _, i in hits}) >= 2, (FC.NAMES[curve], l, sorted(hits))
    # every leg in an early-out's last iteration and beside a prefetch, at every length
    for l in FC.LEGS[curve]:
        lengths_last = {len(steps) for c, steps in walked[curve] if steps[-1][3] == l}
        assert set(FC.LENGTHS) <= lengths_last, (FC.NAMES[curve], l, lengths_last)
        assert any(s[3] == l for c, steps in walked[curve] for s in steps[1:-1]), (FC.NAMES[curve], l)


@pytest.mark.parametrize("curve", CURVES)
def test_conditions_that_hold_together(walked, curve):
    """Where more than one early-out's condition holds, the order of the selects decides: the table has such steps, with
    operands that tell the orders apart."""
    both_ident_differ = ident_q_and_cancel = all_at_once = 0
    for c, steps in walked[curve]:
        for p, q, fl, l in steps:
            if fl["idp"] and fl["idq"] and not _eq(p, q):
                both_ident_differ += 1
            if curve != ED and fl["idq"] and not fl["idp"] and fl["ueq"] and not fl["seq"]:
                ident_q_and_cancel += 1   # secp256k1: the cancel select fires first and idq must override it
            if curve != ED and fl["idp"] and fl["idq"] and fl["ueq"] and fl["seq"] and fl["sopp"]:
                all_at_once += 1
    assert both_ident_differ >= 2
    if curve == ED:   # q an identity and `opposite` at once, p finite: idq must override the identity select
        hits = {i for c, steps in walked[curve] for i, (p, q, fl, l) in enumerate(steps)
                if fl["idq"] and not fl["idp"] and fl["x_opposite"] and fl["y_equal"]}
        assert len(hits) >= 2, hits
    if curve != ED:
        assert all_at_once >= 2
    if curve == SECP:
        assert ident_q_and_cancel >= 2


@pytest.mark.parametrize("curve", CURVES)
def test_a_skipped_leg_changes_the_step(oracle, walked, curve):
    """At every step that takes an early-out, the general formula gives another point than the reference (the near miss
    ueq_general IS the general formula).  One kind of step cannot tell: an identity plus the all-zero term, where the general
    formula's every product is zero and so equals q; those terms are in the table for the other selects -- there
    double(p) and identity() differ from q, so a doubling or a cancel that forgot to exclude the identities shows."""
    f = Field(oracle, curve)
    checked = {l: 0 for l in FC.LEGS[curve]}
    for c, steps in walked[curve]:
        for i, (p, q, fl, l) in enumerate(steps):
            if l == "none":
                continue
            g = general(f, curve, p, q)
            if l == "idp" and _zero(q):
                assert _eq(g, q) and not _eq(oracle.point_double(curve, p), q) and not _eq(oracle.identity(curve), q)
                continue
            if l == "ueq_general":
                assert _eq(g, c.sums[i]), c.describe()
            else:
                assert not _eq(g, c.sums[i]), "%s: step %d (%s) equals the general formula" % (c.describe(), i, l)
            checked[l] += 1
    assert all(v >= 2 for v in checked.values()), checked


@pytest.mark.parametrize("curve", CURVES)
def test_a_case_differs_from_the_chain_without_its_special_term(oracle, walked, curve):
    for c, steps in walked[curve]:
        for i, kind, l in c.special():
            terms = c.terms.copy()
            terms[i] = FC.ordinary_replacement(oracle, curve, i)
            assert not _eq(FC.fold(oracle, curve, terms), c.expect), "%s: term %d" % (c.describe(), i)


@pytest.mark.parametrize("curve", CURVES)
def test_skipping_an_early_out_changes_a_final_sum(oracle, walked, curve):
    """Per leg, some case's FINAL sum -- what a fold returns -- changes when that leg alone is replaced by the general
    formula wherever it is taken (a fold model with the one select missing)."""
    f = Field(oracle, curve)
    for l in FC.LEGS[curve]:
        if l == "ueq_general":
            continue
        told = 0
        for c, steps in walked[curve]:
            if l not in c.legs[1:] and not (l == "idp" and c.kinds[0] != "ord"):
                continue
            if len(c.terms) > 16:
                continue
            acc = oracle.identity(curve)
            for t in c.terms:
                fl = flags(f, curve, acc, t)
                acc = general(f, curve, acc, t) if leg(curve, fl) == l else oracle.point_add(curve, acc, t)
            told += not _eq(acc, c.expect)
        assert told >= 2, (FC.NAMES[curve], l, told)


def test_scaled_representatives_keep_the_equality(oracle, walked):
    """fold_cases.SCALED says where the reference's arithmetic keeps u1 == u2, s1 == s2 for (x l^2, y l^3, z l)"""
    for curve in (SECP, P256):
        # the claim itself, on a running sum of the table and eight scale factors
        f = Field(oracle, curve)
        p = next(c for c, _ in walked[curve] if c.name == "same_n16_at8").sums[5]
        x, y, z = coords(curve, p)
        kept = 0
        for l in FC.V.field_elements(8, curve, 640):
            l2 = f.sqr(l)
            fl = flags(f, curve, p, FC.point(f.mul(x, l2), f.mul(y, f.mul(l2, l)), f.mul(z, l)))
            kept += fl["ueq"] and fl["seq"]
        assert kept == (8 if FC.SCALED[curve] else 0), (curve, kept)
        scaled = [(c, steps) for c, steps in walked[curve] if "scaled" in c.kinds]
        assert bool(scaled) == FC.SCALED[curve]
        for c, steps in scaled:
            i = c.kinds.index("scaled")
            p, q = steps[i][0], steps[i][1]
            assert steps[i][3] == "double"
            assert all(not _eq(a, b) for a, b in zip(coords(curve, p), coords(curve, q))), c.describe()   # all six coordinates differ
