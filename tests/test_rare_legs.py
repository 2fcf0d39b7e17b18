"""
The rare legs of the device arithmetic (the `__builtin_expect` branches of the curve headers and multiply kernels) and
what reaches them, without a GPU:
  * tests/rare_legs.json names every site, keyed file::function#ordinal; a site added or removed in the sources fails
    the census test until the census says how it is reached (or why it is not);
  * the host build of the headers (tools/host_emul.cpp) counts each leg (limbs.hpp FEC_RARE_LEGS);
  * tests/golden/kernel_forcing_vectors.json (gen_kernel_forcing.py) holds (scalar, point) cases on which a named leg
    fires in a kept operation of the multiplication; tests/test_gpu_kernel_forcing.py drives them through the kernels;
  * canonical mode (canon_curves.hpp) is in the same census, keyed canon_curves.hpp::Struct::function#ordinal, with the
    families of tests/golden/canon_forcing_vectors.json (gen_canon_forcing.py); tests/test_canon_rare_legs.py checks them
    on the host, tests/test_gpu_canon_forcing.py through the kernels.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "forge_ec_amd", "csrc")
SO = os.path.join(ROOT, "tools", "libhost_emul.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4}
FILES = ["secp256k1.hpp", "p256.hpp", "ed25519.hpp", "kernels_secp.hip", "kernels_p256.hip", "kernels_ed.hip"]
CENSUS = json.load(open(os.path.join(ROOT, "tests", "rare_legs.json")))
FORCING = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_forcing_vectors.json")))
CANON_FILE = "canon_curves.hpp"
CANON = json.load(open(os.path.join(ROOT, "tests", "golden", "canon_forcing_vectors.json")))


def rare_sites():
    """file::function#ordinal of every __builtin_expect in the multiply family's sources"""
    out = []
    for f in FILES:
        fn, seen = None, {}
        for line in open(os.path.join(CSRC, f)):
            if re.match(r"(FEC_DEV|__global__)\b", line):
                fn = re.search(r"(\w+)\s*\(", re.sub(r"__launch_bounds__\([^)]*\)", "", line)).group(1)
            for _ in re.finditer(r"__builtin_expect\(", line.split("//")[0]):
                k = seen.get(fn, 0)
                seen[fn] = k + 1
                out.append("%s::%s#%d" % (f, fn, k))
    return out + [key for key, _ in canon_sites()]


def canon_sites():
    """(canon_curves.hpp::Struct::function#ordinal, line index) of every __builtin_expect in canonical mode's header: its
    functions are members (FEC_SDEV, indented) of structs that share names such as reduce512"""
    out, struct, fn, seen = [], None, None, {}
    for i, line in enumerate(open(os.path.join(CSRC, CANON_FILE))):
        m = re.match(r"struct (\w+)", line)
        if m:
            struct = m.group(1)
        elif line.startswith("};"):
            struct = None
        m = re.match(r"\s*FEC_S?DEV\b[^(]*?(\w+)\s*\(", line)
        if m:
            fn = "%s::%s" % (struct, m.group(1)) if struct else m.group(1)
        for _ in re.finditer(r"__builtin_expect\(", line.split("//")[0]):
            k = seen.get(fn, 0)
            seen[fn] = k + 1
            out.append(("%s::%s#%d" % (CANON_FILE, fn, k), i))
    return out


def canon_families():
    """family -> counters, for the three kinds of case in canon_forcing_vectors.json"""
    fams = {name: set(f["legs"]) for name, f in CANON["families"].items()}
    for c in CANON["points"] + CANON["edge_scalars"]:
        fams.setdefault(c["family"], set()).update(c["legs"])
    return fams


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not available")
    src = os.path.join(ROOT, "tools", "host_emul.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("limbs.hpp", "secp256k1.hpp", "p256.hpp", "ed25519.hpp", CANON_FILE)]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, src])
    return ctypes.CDLL(SO)


class Counters:
    def __init__(self, emu):
        emu.he_rare_leg_name.restype = ctypes.c_char_p
        self.emu = emu
        self.names = [emu.he_rare_leg_name(i).decode() for i in range(emu.he_rare_leg_count())]
        self.buf = (ctypes.c_ulong * len(self.names))()

    def snap(self):
        self.emu.he_rare_legs(self.buf)
        return np.array(self.buf[:], dtype=np.int64)

    def lit(self, before, after):
        return {self.names[i] for i in np.nonzero(after > before)[0]}


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _multiply(emu, curve, point, scalar, fixed=False):
    p = np.ascontiguousarray(np.array(point, dtype=np.uint64))
    k = np.ascontiguousarray(np.array(scalar, dtype=np.uint64))
    out = np.zeros(p.size, dtype=np.uint64)
    if fixed and curve == 2:
        emu.he_ed_multiply_fixed(_p(p), _p(k), _p(out))
    else:
        emu.he_multiply(curve, _p(p), _p(k), _p(out))
    return out


def test_census_names_every_rare_leg():
    found = rare_sites()
    assert len(found) == len(set(found))
    named = set(CENSUS["legs"]) | set(CENSUS["excluded"])
    assert not set(found) - named, "rare legs missing from tests/rare_legs.json: %s" % sorted(set(found) - named)
    assert not named - set(found), "census names legs that no longer exist: %s" % sorted(named - set(found))
    assert not set(CENSUS["legs"]) & set(CENSUS["excluded"])
    for key, leg in CENSUS["legs"].items():
        assert leg["status"] in ("forced", "routine", "unreached"), key
        assert leg.get("reason") or leg["status"] == "forced", key


def test_padd_coop_sub_legs_have_forcing_cases(oracle):
    """The cooperative additions hold several early-outs inside one __builtin_expect branch: the census names each of them
    (the legs of tests/fold_cases.py), and every one has cases of that table that take it at two indices or more, the
    routes that reach it -- always the hook and the host wavefront -- and, where no public caller can, the reason."""
    import fold_cases as FC
    keys = {"secp256k1.hpp::padd_coop#0": FC.SECP, "p256.hpp::padd_coop#0": FC.P256, "ed25519.hpp::padd_coop#0": FC.ED}
    assert {k for k in CENSUS["legs"] if "::padd_coop#" in k} == set(keys)
    for key, curve in keys.items():
        leg = CENSUS["legs"][key]
        assert "not constructed" not in leg["reason"] and set(leg["kernels"]) == {"k_fold_sum", "k_schnorr_fold_compare"}
        assert set(leg["sub_legs"]) == set(FC.LEGS[curve]), key
        table = {c.name: c for c in FC.cases(oracle, curve)}
        for name, sub in leg["sub_legs"].items():
            assert sub["what"] and sub["cases"], (key, name, "a sub-leg without a forcing case")
            where = set()
            for case in sub["cases"]:
                assert case in table, (key, name, case)
                hits = [i for i, l in enumerate(table[case].legs) if l == name and (i > 0 or table[case].kinds[0] != "ord")]
                assert hits, (key, name, case, "the case does not take the sub-leg")
                where.update(hits)
            assert len(where) >= 2, (key, name, where)
            kinds = [r.split(" ", 1)[0] for r in sub["routes"]]
            assert kinds in (["hook", "public", "host"], ["hook", "host"]), (key, name, kinds)
            assert ("public" in kinds) != bool(sub.get("no_public_caller")), (key, name)


def test_census_counters_and_families(emu):
    names = set(Counters(emu).names)
    fams = {}
    for c in FORCING["cases"]:
        fams.setdefault(c["family"], set()).update(c["legs"])
    assert not set(fams) & set(canon_families())
    fams.update(canon_families())
    for key, leg in CENSUS["legs"].items():
        assert leg["counter"] in names, (key, leg["counter"])
        if leg["status"] == "forced":
            assert leg["families"] and leg["kernels"], key
            for f in leg["families"]:
                assert leg["counter"] in fams.get(f, ()), (key, f, "no case of the family targets the leg")
    # every family lights known counters, at least one of them a leg the census names
    counters = {leg["counter"] for leg in CENSUS["legs"].values()}
    for f, legs in fams.items():
        assert legs <= names and legs & counters, f
    assert {c["curve"] for c in FORCING["cases"]} == {0, 1, 2}
    # no dead counter: each one is a census leg's, or lit by some forcing case
    assert names == counters | set().union(*fams.values()), names - counters - set().union(*fams.values())


def test_census_search_records():
    """A leg whose operand the generator searches for: forced legs have a hit, unreached legs none in the bound."""
    searches = FORCING["searches"] + [r for r in CANON["searches"] if "leg" in r]
    for key, leg in CENSUS["legs"].items():
        if not leg.get("search"):
            continue
        recs = [r for r in searches if r["leg"] == leg["counter"]]
        assert recs and all(r["candidates"] >= 1 << 30 for r in recs), key
        hits = sum(r["hits"] for r in recs)
        assert (hits > 0) == (leg["status"] == "forced"), (key, hits)


# the legs each family of forcing_vectors.json (k_field_op's fixture) is built for
FIELD_FAMILY_LEGS = {
    "p256_noncanonical": {"P256_ADD_GENERAL", "P256_SUB_TOP", "P256_SUB_GE", "P256_PRODUCT_TOP"},
    "secp_mul_borrow": {"SECP_MUL_BW"},
    "secp_mul_ge_p": {"SECP_CSUB_P", "SECP_PRODUCT_TOP"},
    "ed_small_add_carry": {"ED_REDUCE_CARRY", "ED_REDUCE_TOP", "ED_ADD_CARRY", "ED_SUB_BORROW", "ED_MUL_EXC"},
}


def test_field_forcing_vectors_light_their_counters(emu):
    """Counter sanity: each family of forcing_vectors.json lights its own counters through he_field_op, and no other
    curve's; random canonical operands light none."""
    cnt = Counters(emu)
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "forcing_vectors.json")))["cases"]
    out = np.zeros(4, dtype=np.uint64)
    lit = {}
    for c in cases:
        a = np.array(c["a"], dtype=np.uint64)
        b = np.array(c["b"], dtype=np.uint64) if c["b"] is not None else None
        before = cnt.snap()
        cnt.emu.he_field_op(c["curve"], OPS[c["op"]], _p(a), _p(b), _p(out))
        lit.setdefault(c["family"], set()).update(cnt.lit(before, cnt.snap()))
    for fam, want in FIELD_FAMILY_LEGS.items():
        assert want <= lit[fam], (fam, want - lit[fam])
        prefix = next(iter(want)).split("_")[0]
        assert all(n.startswith(prefix) for n in lit[fam]), (fam, lit[fam])
    for curve in range(3):
        a, b = V.field_elements(3000, curve, 71), V.field_elements(3000, curve, 72)
        before = cnt.snap()
        for i in range(a.shape[0]):
            ai, bi = np.ascontiguousarray(a[i]), np.ascontiguousarray(b[i])
            for op in OPS.values():
                cnt.emu.he_field_op(curve, op, _p(ai), _p(bi), _p(out))
        assert not cnt.lit(before, cnt.snap()), curve


def test_kernel_forcing_cases_reach_their_legs(emu):
    """he_multiply (and the Ed25519 table walk for the bases) lights every case's legs and returns the expectation."""
    cnt = Counters(emu)
    for c in FORCING["cases"]:
        before = cnt.snap()
        got = _multiply(emu, c["curve"], c["point"], c["scalar"])
        assert set(c["legs"]) <= cnt.lit(before, cnt.snap()), (c["family"], c["legs"])
        assert got.tolist() == c["expect"], c["family"]
    for b in FORCING["bases"]:
        for k, want in zip(b["scalars"], b["expect"]):
            before = cnt.snap()
            got = _multiply(emu, b["curve"], b["point"], k, fixed=True)
            assert set(b["legs"]) <= cnt.lit(before, cnt.snap()), (b["family"], b["legs"])
            assert got.tolist() == want, b["family"]


def test_kernel_forcing_expectations_match_c_oracle(oracle):
    for c in FORCING["cases"]:
        got = oracle.multiply(c["curve"], np.array(c["point"], dtype=np.uint64), np.array(c["scalar"], dtype=np.uint64))
        assert got.tolist() == c["expect"], c["family"]
    for b in FORCING["bases"]:
        for k, want in zip(b["scalars"], b["expect"]):
            got = oracle.multiply(b["curve"], np.array(b["point"], dtype=np.uint64), np.array(k, dtype=np.uint64))
            assert got.tolist() == want, b["family"]


def test_random_cases_do_not_reach_forced_legs(emu):
    """The forcing is needed: as many random canonical (scalar, point) pairs per curve reach none of the forced legs,
    while the legs the census calls routine are taken by them."""
    cnt = Counters(emu)
    forced = {leg["counter"] for leg in CENSUS["legs"].values() if leg["status"] == "forced"}
    routine = {leg["counter"] for leg in CENSUS["legs"].values() if leg["status"] == "routine"}
    seen = set()
    for curve in range(3):
        n = sum(1 for c in FORCING["cases"] if c["curve"] == curve)
        pts, ks = V.points(n, curve, 81), V.scalars(n, curve, 82)
        for i in range(n):
            before = cnt.snap()
            _multiply(emu, curve, pts[i], ks[i])
            lit = cnt.lit(before, cnt.snap())
            assert not lit & forced, (curve, lit & forced)
            seen |= lit
    assert routine <= seen, routine - seen
