"""
The rare legs of canonical mode (canon_curves.hpp) on the host, without a GPU: tests/rare_legs.json names each
__builtin_expect site and the reach counter that sits in it, tests/golden/canon_forcing_vectors.json
(gen_canon_forcing.py) holds operands and points on which those counters move.  Here every case goes through the
host emulation with the counters watched and is compared with oracle/canon_model.py;
tests/test_gpu_canon_forcing.py drives the same cases through the kernels, tests/test_gpu_canon_forcing_points.py the points
through the later kernels that decode or test a caller's point; the census says which kernels those are, and here every
__global__ of csrc/canon*_kernels.hpp must have its place in it.  tests/golden/canon_forcing_keyed_vectors.json
(gen_canon_forcing_keyed.py) holds forcing points with known logarithms.
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


# ---- the kernels that decode or test a caller's point ------------------------------------------------------------------
# the kernels tests/test_gpu_canon_forcing.py drives; every other kernel of a canonical field leg is one of
# tests/test_gpu_canon_forcing_points.py's and must be a key of its DRIVES
DRIVEN_BY_THE_FIRST_FILE = {"k_canon_field_op", "k_canon_mul", "k_canon_decompress", "k_canon_ecdsa_prepare_msg", "k_canon_normalize",
                            "k_canon_bip340_prepare", "k_ced_mul", "k_ced_eddsa_prepare"}
WITHOUT_POINTS = CENSUS["canon_kernels_without_caller_points"]


def canon_kernels():
    """name -> file of every __global__ kernel in csrc/canon*_kernels.hpp (a declaration may run over several lines)"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if re.fullmatch(r"canon\w*_kernels\.hpp", f):
            text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
            for m in re.finditer(r"__global__\b(?:\s*__launch_bounds__\([^)]*\))?\s*void\s+(\w+)\s*\(", text):
                assert m.group(1) not in out, m.group(1)
                out[m.group(1)] = f
            assert len(re.findall(r"__global__", text)) == sum(1 for v in out.values() if v == f), f
    return out


def census_kernels():
    """kernel -> the census keys that name it, over the canonical legs and the borrowed ones"""
    named = {}
    for key, rec in list(CANON_LEGS.items()) + list(CENSUS["canon_borrowed"].items()):
        for k in rec.get("kernels", ()):
            named.setdefault(k, []).append(key)
    return named


def test_every_canon_kernel_is_in_a_leg_or_has_no_caller_point():
    """A new __global__ in a canon*_kernels.hpp fails here until someone decides where it belongs: in the kernels list of the
    legs it can reach with a caller's point, or in canon_kernels_without_caller_points with the reason.  And the census
    names no kernel that the sources do not have."""
    found, named = canon_kernels(), census_kernels()
    assert len(found) >= 71 and len(set(found.values())) >= 8   # (the scan itself: 71 kernels in 8 files when this was written)
    homeless = sorted(set(found) - set(named) - set(WITHOUT_POINTS))
    assert not homeless, "kernels in neither a leg's list nor canon_kernels_without_caller_points: %s" % homeless
    gone = sorted((set(named) | set(WITHOUT_POINTS)) - set(found))
    assert not gone, "the census names kernels that are not in csrc/canon*_kernels.hpp: %s" % gone
    assert not set(named) & set(WITHOUT_POINTS)
    assert all(isinstance(r, str) and len(r) > 8 for r in WITHOUT_POINTS.values())
    # a kernel that calls on_curve or one of the decoders cannot be filed under "no caller's point", and the legs' lists name
    # no other kernel than those -- but the field kernel, the normalisation and the comb kernels of the point legs
    calling = set()
    for f in set(found.values()):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        for body in re.split(r"__global__", text)[1:]:
            name = re.search(r"void\s+(\w+)\s*\(", body).group(1)
            if re.search(r"\bon_curve\(|sec1_record<|sec1_decode<|tweak_key<|taproot_key<|bip340_lift_x\(|canon::bip340_prepare(_msg)?\(|"
                         r"canon::eddsa_prepare(_msg)?\(|ed_decode\(|ecdsa_prepare_msg<|recover_prepare_group<|bip340_element\(|ed25519_element\(", body):
                assert name in named, name
                calling.add(name)
    assert calling == set(named) - {"k_canon_field_op", "k_canon_normalize", "k_canon_mul_base", "k_canon_mul_base8", "k_canon_build_comb",
                                    "k_canon_build_comb8"}, calling ^ set(named)


def test_drives_names_a_test_for_every_later_kernel():
    """every kernel of a canonical field leg that tests/test_gpu_canon_forcing.py does not drive is a key of
    test_gpu_canon_forcing_points.DRIVES, and every function DRIVES names is a test of that module (imported without a GPU)"""
    import test_gpu_canon_forcing_points as G
    later = {k for key in FIELD_LEGS for k in CANON_LEGS[key]["kernels"]} - DRIVEN_BY_THE_FIRST_FILE
    assert len(later) >= 9 and later <= set(G.DRIVES), later - set(G.DRIVES)
    assert set(G.DRIVES) <= set(census_kernels())
    for kernel, tests in G.DRIVES.items():
        assert tests and all(t.startswith("test_") and callable(getattr(G, t, None)) for t in tests), kernel
    for key in FIELD_LEGS:   # each curve's later kernels are on each of its legs
        curve = re.search(r"::Fp(\w+)::", key).group(1)
        same = [k for k in FIELD_LEGS if "::Fp%s::" % curve in k]
        assert all(CANON_LEGS[k]["kernels"] == CANON_LEGS[key]["kernels"] for k in same), key


# the decoding functions the later kernels call, as the host emulation exports them: name -> (curves, call(cnt, cid, point
# record, out) -> (ok, lit), the model's point for it)
def _decoders(c, pt, xy):
    cid = c["curve"]
    if cid == 2:
        enc = _arr(int.from_bytes(bytes.fromhex(c["ed"]), "little"))
        other = _arr(int.from_bytes(M.ED25519.encode(M.ED25519.G), "little"))
        s, h, a, u = _arr(1), _arr(2), np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        neg = (M.ED25519.P - pt[0], pt[1])   # eddsa_prepare negates A
        return {"ed_decode": (("he_ed_decode", enc, xy), pt),
                "eddsa_prepare as A": (("he_eddsa_prepare", enc, other, s, h, xy, a, u), neg),
                "eddsa_prepare as R": (("he_eddsa_prepare", other, enc, s, h, a, xy, u), pt)}
    out = {"sec1_33": (("he_canon_sec1_decode", cid, 2 | (pt[1] & 1), _arr(pt[0]), None, 0, xy), pt),
           "sec1_33 other tag": (("he_canon_sec1_decode", cid, 3 - (pt[1] & 1), _arr(pt[0]), None, 0, xy), CURVES[cid].neg(pt)),
           "sec1_65": (("he_canon_sec1_decode", cid, 4, _arr(pt[0]), _arr(pt[1]), 1, xy), pt)}
    if cid == 0:
        even = pt if pt[1] % 2 == 0 else M.SECP256K1.neg(pt)
        u = np.zeros(4, dtype=np.uint64)
        out["lift_x"] = (("he_bip340_lift_x", _arr(pt[0]), xy), even)
        out["bip340_prepare"] = (("he_bip340_prepare", _arr(pt[0]), _arr(1), _arr(1), _arr(1), xy, u), even)
    return out


def test_every_decoding_function_lights_the_points_legs(emu):  # noqa: F811
    """The points are known to light their legs in he_canon_mul, he_canon_on_curve and he_ed_decode; the later kernels call
    33-byte decompression, bip340_lift_x (which sees x alone) and the batch verifier's decoders.  Every fixture point through
    each of them: the point's legs fire and the function returns the model's point.  A pairing in which a leg does not fire
    belongs in test_gpu_canon_forcing_points.NOT_LIT, which the GPU tests skip; the counters find none."""
    import test_gpu_canon_forcing_points as G
    cnt = Counters(emu)
    xy = np.zeros(8, dtype=np.uint64)
    dark, seen = {}, set()
    for i, c in enumerate(CANON["points"]):
        pt = (_int(c["x"]), _int(c["y"]))
        for name, (call, want) in _decoders(c, pt, xy).items():
            ok, lit = _run(cnt, *call)
            assert ok == 1 and (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == want, (c["family"], name)
            if not set(c["legs"]) <= lit:
                dark[(i, name)] = sorted(lit)
            seen.add(name)
    assert seen == {"sec1_33", "sec1_33 other tag", "sec1_65", "lift_x", "bip340_prepare", "ed_decode", "eddsa_prepare as A", "eddsa_prepare as R"}
    assert dark == G.NOT_LIT, dark


def test_keyed_points_are_multiples_of_g_that_light_their_leg(emu):  # noqa: F811
    """tests/golden/canon_forcing_keyed_vectors.json: every point is k G by the model, lights its legs in on_curve, and each
    decoding function lights exactly what the fixture records for it; lift_x returns the point of the negated logarithm."""
    import json
    import test_gpu_canon_forcing_points as G
    doc, C = G.KEYED, M.SECP256K1
    cnt = Counters(emu)
    xy = np.zeros(8, dtype=np.uint64)
    start, count = _int(doc["start"]), doc["count"]
    assert count in (1 << 19, 1 << 20) and doc["curve"] == 0
    assert [(r["candidates"], r["hits"]) for r in doc["searches"]] and sum(r["hits"] for r in doc["searches"]) >= len(doc["points"])
    assert all(r["candidates"] == count and r["leg"] in cnt.names for r in doc["searches"])
    through = 0
    for p in doc["points"]:
        k, pt = _int(p["k"]), (_int(p["x"]), _int(p["y"]))
        assert start <= k < start + count and C.mul(k, C.G) == pt
        c = {"curve": 0}
        calls = _decoders(c, pt, xy)
        calls["on_curve"] = (("he_canon_on_curve", 0, _arr(*pt)), None)
        for name in ("on_curve", "sec1_33", "sec1_65", "lift_x"):
            call, want = calls[name]
            ok, lit = _run(cnt, *call)
            assert ok == 1 and sorted(lit) == p["lit"][name], (p["k"], name, lit)
            assert want is None or (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == want
        assert p["legs"] == p["lit"]["on_curve"] and p["legs"]
        assert p["through_x"] == bool(set(p["legs"]) & set(p["lit"]["lift_x"]))
        d = _int(p["bip340_d"])
        assert d in (k, C.N - k) and C.mul(d, C.G) == R.lift_x(pt[0])
        through += p["through_x"]
    assert through == doc["through_x"] and (through >= 4 or "SHORTFALL" in doc["note"])
    assert json.dumps(doc, indent=1, sort_keys=True) + "\n" == open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canon_forcing_keyed_vectors.json")).read()


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
