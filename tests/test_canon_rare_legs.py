"""
The rare legs of canonical mode (canon_curves.hpp) on the host, without a GPU: tests/rare_legs.json names each
__builtin_expect site and the reach counter that sits in it, tests/golden/canon_forcing_vectors.json
(gen_canon_forcing.py) holds operands and points on which those counters move.  Here every case goes through the
host emulation with the counters watched and is compared with oracle/canon_model.py;
tests/test_gpu_canon_forcing.py drives the same cases through the kernels.
"""
import ctypes
import os
import random
import re
import sys

import numpy as np

import canon_msg_ref as R
from oracle import canon_model as M
from test_rare_legs import CANON, CANON_FILE, CENSUS, CSRC, Counters, canon_families, canon_sites, emu  # noqa: F401

CURVES = [M.SECP256K1, M.P256, M.ED25519]
OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4}
CANON_LEGS = {k: v for k, v in CENSUS["legs"].items() if k.startswith(CANON_FILE)}
FIELD_LEGS = [k for k in CANON_LEGS if re.search(r"::Fp\w+::", k)]
# the functions of the parity headers that canonical mode calls (FpSecp, FpP256, FpEd)
BORROWED = {"secp256k1.hpp": ("add", "sub", "neg", "csub_p_unlikely"), "p256.hpp": ("add", "neg"), "ed25519.hpp": ("add", "sub", "neg", "reduce")}


def _int(h):
    return int(h, 16)


def _arr(*vals):
    return np.array([l for v in vals for l in M.limbs(v)], dtype=np.uint64)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _pt(h):
    return M.INF if h is None else (_int(h[:64]), _int(h[64:]))


def _run(cnt, fn, *args):
    """-> (return value, counters that moved); arrays go in as pointers"""
    before = cnt.snap()
    ret = getattr(cnt.emu, fn)(*[_p(a) if isinstance(a, np.ndarray) else a for a in args])
    return ret, cnt.lit(before, cnt.snap())


def test_census_counters_sit_in_their_legs():
    """Each canonical site is followed by the FEC_RARE of its census counter, a leg with a nested same-x branch by its inner
    one, and the header holds no other counter: one deleted FEC_RARE, or one new __builtin_expect, fails here or in
    test_rare_legs.py::test_census_names_every_rare_leg."""
    lines = open(os.path.join(CSRC, CANON_FILE)).read().split("\n")
    assert {k for k, _ in canon_sites()} == set(CANON_LEGS)
    want = set()
    for key, at in canon_sites():
        leg = CANON_LEGS[key]
        first = re.search(r"FEC_RARE\((\w+)\)", "\n".join(lines[at:at + 2]))
        assert first and first.group(1) == leg["counter"], key
        want.add(leg["counter"])
        if "inner" in leg:
            body = "\n".join(lines[at:at + 12])
            assert re.search(r"if \(hzero != 0\) \{[^\n]*\n\s*FEC_RARE\(%s\);" % leg["inner"], body), key
            want.add(leg["inner"])
    found = re.findall(r"FEC_RARE\w*\((?:[^,()]*,\s*)?(\w+)\)", "\n".join(l.split("//")[0] for l in lines))
    assert sorted(found) == sorted(want)
    assert len(FIELD_LEGS) == 6 and all(CANON_LEGS[k]["status"] == "forced" for k in FIELD_LEGS)


def test_census_of_the_borrowed_legs():
    """canon_borrowed names exactly the counters inside the parity-header functions that canonical mode calls"""
    inside = set()
    for f, fns in BORROWED.items():
        fn = None
        for line in open(os.path.join(CSRC, f)):
            m = re.match(r"FEC_DEV\b[^(]*?(\w+)\s*\(", line)
            if m:
                fn = m.group(1)
            if fn in fns:
                inside.update(re.findall(r"FEC_RARE\((\w+)\)", line.split("//")[0]))
    assert inside == set(CENSUS["canon_borrowed"])
    fams = canon_families()
    for name, rec in CENSUS["canon_borrowed"].items():
        if rec["status"] == "forced":
            assert rec["families"] and all(name in fams[f] for f in rec["families"]), name
        else:
            assert rec["status"] == "unreached" and rec["reason"] and not any(name in legs for legs in fams.values()), name
    header = open(os.path.join(CSRC, CANON_FILE)).read()
    for f, fns in BORROWED.items():   # ... and canonical mode calls no other function of theirs that has a leg
        ns = {"secp256k1.hpp": "secp", "p256.hpp": "p256", "ed25519.hpp": "ed"}[f]
        assert set(re.findall(r"\b%s::(\w+)\(" % ns, header)) <= set(fns), f


def test_field_families_light_exactly_their_counters(emu):  # noqa: F811
    """every field case: exactly the family's counters move in he_canon_field_op, and the value is the model's"""
    cnt = Counters(emu)
    out = np.zeros(4, dtype=np.uint64)
    seen = {}
    for c in CANON["field"]:
        fam = CANON["families"][c["family"]]
        C, a, b = CURVES[c["curve"]], _int(c["a"]), None if c["b"] is None else _int(c["b"])
        assert (fam["curve"], fam["op"]) == (c["curve"], c["op"]) and a < C.P and (b or 0) < C.P
        _, lit = _run(cnt, "he_canon_field_op", c["curve"], OPS[c["op"]], _arr(a), _arr(b or 0), out)
        assert lit == set(fam["legs"]), (c["family"], lit)
        want = C.field_op(c["op"], a, b or 0)
        assert M.unlimbs(out) == want == _int(c["expect"]), c["family"]
        assert c["t"] is None or _int(c["t"]) == want
        seen[c["family"]] = seen.get(c["family"], 0) + 1
    assert set(seen) == set(CANON["families"]) and min(seen.values()) >= 2
    # every forced leg has a mul family and a sqr family: sqr_wide is not mul_wide on the device
    for key in FIELD_LEGS:
        ops = {CANON["families"][f]["op"] for f in CANON_LEGS[key]["families"] if f in CANON["families"]}
        assert {"mul", "sqr"} <= ops, key


def test_random_operands_light_no_forced_field_leg(emu):  # noqa: F811
    """the forcing is needed: as many random canonical operands per curve as the fixture has cases reach none of them"""
    cnt = Counters(emu)
    forced = {CANON_LEGS[k]["counter"] for k in FIELD_LEGS} | {n for n, r in CENSUS["canon_borrowed"].items() if r["status"] == "forced"}
    out = np.zeros(4, dtype=np.uint64)
    for cid, C in enumerate(CURVES):
        rng = random.Random(0xF1E1D + cid)
        for _ in range(sum(1 for c in CANON["field"] if c["curve"] == cid)):
            a, b = rng.randrange(C.P), rng.randrange(C.P)
            for name, op in OPS.items():
                _, lit = _run(cnt, "he_canon_field_op", cid, op, _arr(a), _arr(b), out)
                assert not lit & forced, (cid, name, hex(a), hex(b), lit)
                assert M.unlimbs(out) == C.field_op(name, a, b)


def test_points_are_on_the_curve_and_light_their_legs(emu):  # noqa: F811
    """every fixture point: on the model's curve, its encodings decode to it, the legs fire inside on_curve and inside the
    point routines, and every recorded answer is the model's"""
    cnt = Counters(emu)
    xy = np.zeros(8, dtype=np.uint64)
    per_leg = {}
    for c in CANON["points"]:
        cid, legs = c["curve"], set(c["legs"])
        C, pt = CURVES[cid], (_int(c["x"]), _int(c["y"]))
        assert C.on_curve(pt)
        pin = _arr(*pt)
        ok, lit = _run(cnt, "he_canon_on_curve", cid, pin)
        assert ok == 1 and legs <= lit, (c["family"], lit)
        twin = _arr(pt[0] ^ 1, pt[1]) if cid == 2 else _arr(pt[0], pt[1] ^ 1)
        assert _run(cnt, "he_canon_on_curve", cid, twin)[0] == 0
        for m in c["mul"]:
            k, want = _int(m["k"]), _pt(m["out"])
            assert want == C.mul(k % C.N if cid < 2 else k, pt)
            st, lit = _run(cnt, "he_ced_mul", _arr(k), pin, xy) if cid == 2 else _run(cnt, "he_canon_mul", cid, _arr(k), pin, xy)
            assert legs <= lit and st == 0 and (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == want, c["family"]
            if cid == 0:   # the kernel's ladder
                st, _ = _run(cnt, "he_glv_mul", _arr(k), pin, xy)
                assert st == 0 and (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == want, c["family"]
        u1, u2 = _int(c["dm"]["u1"]), _int(c["dm"]["u2"])
        assert _pt(c["dm"]["out"]) == C.add(C.mul(u1, C.G), C.mul(u2, pt))
        if cid == 2:
            enc = bytes.fromhex(c["ed"])
            assert R.ed_decode(enc) == pt
            ok, lit = _run(cnt, "he_ed_decode", _arr(int.from_bytes(enc, "little")), xy)
            assert ok == 1 and legs <= lit and (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == pt
            s, h, Rp = _int(c["eddsa"]["s"]), _int(c["eddsa"]["h"]), R.ed_decode(_int(c["eddsa"]["r"]).to_bytes(32, "little"))
            assert s < C.N and h < C.N and C.add(C.mul(s, C.G), C.mul(h, C.neg(pt))) == Rp
        else:
            assert R.sec1_decode(C, bytes.fromhex(c["sec1_33"])) == pt == R.sec1_decode(C, bytes.fromhex(c["sec1_65"]))
            z, r, s = (_int(c["ecdsa"][k]) for k in "zrs")
            w = pow(s, -1, C.N)
            assert 0 < r < C.N and 0 < s < C.N and C.add(C.mul(z * w % C.N, C.G), C.mul(r * w % C.N, pt))[0] % C.N == r
            assert ("x_only" in c) == ("bip340" in c) == (cid == 0 and pt[1] % 2 == 0)
            if "bip340" in c:
                r, s, e = (_int(c["bip340"][k]) for k in "rse")
                Rp = C.add(C.mul(s, C.G), C.mul((C.N - e) % C.N, pt))
                assert R.lift_x(_int(c["x_only"])) == pt and Rp[0] == r and Rp[1] % 2 == 0
        for leg in legs:
            per_leg.setdefault(leg, set()).add(cid)
    for key in FIELD_LEGS:   # at least one point per forced field leg, and a BIP-340 key among secp256k1's
        assert per_leg.get(CANON_LEGS[key]["counter"]), key
    assert any("bip340" in c for c in CANON["points"])


def test_edge_scalars_light_the_addition_legs(emu):  # noqa: F811
    """k * P and k * G with k in {0, 1, n - 1, n, ...}: infinity meets the mixed and the windowed addition, k = n ends on
    P + (-P); the census's point legs are forced by these families"""
    cnt = Counters(emu)
    xy = np.zeros(8, dtype=np.uint64)
    lit_by = {}
    for c in CANON["edge_scalars"]:
        cid, k = c["curve"], _int(c["k"])
        C = CURVES[cid]
        base = C.G if c["point"] is None else _pt(c["point"])
        want = C.mul(k % C.N, base)
        assert want == _pt(c["out"])
        runs = [("he_canon_mul", cid, _arr(k), _arr(*base), xy)] if c["fn"] == "mul" else [("he_canon_mul_base", cid, _arr(k), xy), ("he_canon_mul_base8", cid, _arr(k), xy)]
        for args in runs:
            st, lit = _run(cnt, *args)
            assert set(c["legs"]) <= lit, (c["family"], c["k"])
            assert st == (1 if want is M.INF else 0) and (want is M.INF or (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == want)
        lit_by.setdefault(c["family"], set()).update(c["legs"])
    for key in ("canon_curves.hpp::wei::jadd_affine#0", "canon_curves.hpp::wei::jadd_window#0"):
        leg = CANON_LEGS[key]
        assert leg["status"] == "forced"
        for f in leg["families"]:
            assert {leg["counter"], leg["inner"]} <= lit_by[f], (key, f)


def test_glv_top_window_is_out_of_reach(emu):  # noqa: F811
    """The census may call glv_secp::mul_window's top window unreached only with the bound and the recorded searches: the
    bound is recomputed here from the basis, the header's g1 / g2 and the fixture's structured search are checked against it."""
    sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_canon_forcing as G
    n, lam = M.SECP256K1.N, G.GLV_LAMBDA
    leg, glv = CANON_LEGS["canon_curves.hpp::glv_secp::mul_window#0"], CANON["glv"]
    for a, b in ((G.GLV_A1, G.GLV_B1), (G.GLV_A2, G.GLV_B2)):
        assert (a + b * lam) % n == 0
    assert G.GLV_A1 * G.GLV_B2 - G.GLV_A2 * G.GLV_B1 == n
    # g_i is 2^384 |b| / n rounded: for k < 2^256 the product k g_i / 2^384 is within 2^-129 of b k / n
    assert abs(G.GLV_G1 * n - (G.GLV_B2 << 384)) * 2 <= n and abs(G.GLV_G2 * n - (-G.GLV_B1 << 384)) * 2 <= n
    header = open(os.path.join(CSRC, CANON_FILE)).read()
    for name, g in (("g1", G.GLV_G1), ("g2", G.GLV_G2)):
        words = re.search(r"fe %s\(\) \{ return edw::fe_words\(([^)]*)\)" % name, header).group(1)
        assert sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words.split(","))) == g
    bound1 = (abs(G.GLV_A1) + abs(G.GLV_A2)) // 2 + 2    # (|a1| + |a2|) (1/2 + 2^-129), rounded up
    bound2 = (abs(G.GLV_B1) + abs(G.GLV_B2)) // 2 + 2
    assert (bound1, bound2) == (_int(glv["bound_k1"]), _int(glv["bound_k2"])) and max(bound1, bound2) < 2**128
    assert glv["structured"]["candidates"] >= 1 << 18 and _int(glv["structured"]["largest"]) <= max(bound1, bound2)
    random30 = [r for r in CANON["searches"] if r.get("leg") == leg["counter"]]
    assert random30 and all(r["candidates"] >= 1 << 30 for r in random30)
    hits = glv["structured"]["hits"] + sum(r["hits"] for r in random30)
    assert (hits == 0) == (leg["status"] == "unreached") and (hits > 0) == bool(glv["scalars"])
    k1, k2 = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    rng, cnt = random.Random(0x61F), Counters(emu)
    for k in [rng.randrange(2**256) for _ in range(2000)] + [_int(s) for s in glv["scalars"]]:
        signs, _ = _run(cnt, "he_glv_decompose", _arr(k), k1, k2)
        a, b = M.unlimbs(k1), M.unlimbs(k2)
        assert (-a if signs & 1 else a, -b if signs & 2 else b) == G.glv_model(k)
        assert a <= bound1 and b <= bound2, hex(k)
