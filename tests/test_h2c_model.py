"""
CPU checks of the HashToCurve restatement (tests/h2c_ref.py) and of its fixture, and -- on the reference's behaviour alone
-- the conditions the GPU tests rely on to tell a real implementation from a constant: the inherent sqrt is None for every
fixture element, so secp256k1's hash is ONE constant and P-256's results must differ per message; both outcomes of the
sign comparison and the u == 0 leg occur among the planted limbs.
"""
import hashlib
import json
import os

import h2c_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "h2c_vectors.json")))


def test_expander_is_rfc9380s():
    for msg, want in R.K1:
        assert R.expand_message_xmd(msg, R.K1_DST, 32).hex() == want
    assert FIXTURE["k1"] == [[m.hex(), h] for m, h in R.K1]
    # written out once more, independently of the restatement's loop: ell = 2
    msg, dst = b"abc", R.K1_DST
    dp = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + b"\x00\x28\x00" + dp).digest()
    b1 = hashlib.sha256(b0 + b"\x01" + dp).digest()
    b2 = hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b1)) + b"\x02" + dp).digest()
    assert R.expand_message_xmd(msg, dst, 40) == (b1 + b2)[:40]


def test_fixture_is_what_the_restatement_gives():
    pool = bytes.fromhex(FIXTURE["pool"])
    for m, d, o, want in FIXTURE["xmd"][::7] + FIXTURE["xmd"][-1:]:
        assert R.expand_message_xmd(pool[:m], R.dst_of(d), o).hex() == want
    for curve, d, count, msgs, u in FIXTURE["field"]:
        got = R.hash_to_field(curve, bytes.fromhex(msgs[0]), R.dst_of(d), count)[0]
        assert [v for f in got for v in f] == u[0]
    for case in FIXTURE["curve"]:
        msg, dst = bytes.fromhex(case["msgs"][1]), R.dst_of(case["dst_len"])
        x, y, inf = R.curve_hash_to_curve(case["curve"], msg, dst)
        assert [list(x) + list(y), int(inf)] == case["trait"][1]
        if case["dst_len"]:
            p, cand, legs = R.hash_to_curve(case["curve"], msg, dst)
            assert [R.flat_proj(p), [list(c[0]) + list(c[1]) for c in cand], legs] == case["hash"][1]


def test_count_one_and_two_share_nothing():
    for curve in (R.SECP, R.P256):
        u1 = R.hash_to_field(curve, b"m", b"dst", 1)[0]
        u2 = R.hash_to_field(curve, b"m", b"dst", 2)[0]
        assert u1[0] != u2[0]


def test_sqrt_is_none_for_every_fixture_element():
    for case in FIXTURE["curve"]:
        for name in ("hash", "encode"):
            for _, _, legs in case.get(name, []):
                assert all(l & R.LEG_SQRT_NONE for l in legs)
                assert not any(l & (R.LEG_OS2IP | R.LEG_INV_ZERO | R.LEG_U_ZERO) for l in legs)
    for curve, note, u, xy, cand, legs in FIXTURE["map"]:
        assert legs & R.LEG_SQRT_NONE, note


def test_secp256k1_hash_is_one_constant_and_p256_results_differ():
    F = R.M.Secp
    d = (list(R.SECP_DEFAULT[0]), list(R.SECP_DEFAULT[1]), [1, 0, 0, 0])
    const = R.flat_proj(F.padd(d, d))
    seen = set()
    for case in FIXTURE["curve"]:
        if not case["dst_len"]:
            continue
        for p, cand, _ in case["hash"]:
            if case["curve"] == R.SECP:
                assert p == const
            else:
                seen.add(tuple(p))
        if case["curve"] == R.SECP:
            for p, _, _ in case["encode"]:
                assert p == list(R.SECP_DEFAULT[0]) + list(R.SECP_DEFAULT[1]) + [1, 0, 0, 0]
            # ... while the candidates the reference throws away differ per message
            assert len({tuple(c[0]) for _, c, _ in case["hash"]}) == len(case["hash"])
    n_p256 = sum(len(c["hash"]) for c in FIXTURE["curve"] if c["curve"] == R.P256 and c["dst_len"])
    assert len(seen) == n_p256 >= 40
    for case in FIXTURE["curve"]:
        if case["curve"] == R.P256:
            assert len({tuple(t[0]) for t in case["trait"]}) == len(case["trait"])
            for xy, inf in case["trait"]:
                assert inf == 0


def test_both_sign_outcomes_and_the_zero_leg_occur():
    for curve in (R.SECP, R.P256):
        legs = [c[5] for c in FIXTURE["map"] if c[0] == curve]
        assert any(l & R.LEG_NEGATE for l in legs) and any(not (l & R.LEG_NEGATE) for l in legs)
        hashed = [l for c in FIXTURE["curve"] if c["curve"] == curve and c["dst_len"] for row in c["hash"] for l in row[2]]
        assert any(l & R.LEG_NEGATE for l in hashed) and any(not (l & R.LEG_NEGATE) for l in hashed)
    zero = [c for c in FIXTURE["map"] if c[1] == "zero"]
    assert len(zero) == 2
    assert [c[5] & R.LEG_U_ZERO for c in zero if c[0] == R.SECP] == [R.LEG_U_ZERO]
    one = [c for c in FIXTURE["map"] if c[0] == R.SECP and c[1] == "one"][0]
    assert zero[0][3:5] == one[3:5]          # secp256k1: a zero u is replaced by one
    # limbs not below p are used as they are
    assert {c[1] for c in FIXTURE["map"]} >= {"p", "p plus one", "all ones"}


def test_forced_legs_of_the_secp256k1_map():
    """valid_point and w == 0 through the finishing step with chosen flags (what tests/cpp/h2c_host.cpp forces too)."""
    eu, legs, w, x, y2 = R.secp_map_parts([1, 0, 0, 0])
    s = [5, 0, 0, 0]
    pt, l = R.secp_map_finish(eu, legs, x, y2, s, True)
    assert pt[0] == x and pt[1] in (s, R.M.Secp.neg(s)) and not l & R.LEG_SQRT_NONE
    pt, l = R.secp_map_finish(eu, legs | R.LEG_INV_ZERO, x, y2, s, True)
    assert pt == (list(R.SECP_DEFAULT[0]), list(R.SECP_DEFAULT[1])) and l & R.LEG_INV_ZERO
