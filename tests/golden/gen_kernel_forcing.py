"""
Generates tests/golden/kernel_forcing_vectors.json: (scalar, point) pairs built so that a named rare leg of the device
field / point arithmetic fires in an operation whose result the multiply kernels KEEP, with expected products from the
independent Python model oracle/py_model.py (restatement-derived, not reference-executed -- same provenance as
golden_vectors.json).  Each case records the reach counters (limbs.hpp FEC_RARE_LEGS, census tests/rare_legs.json) that
the host build of the same headers (tools/host_emul.cpp) must light on it; the generator keeps a candidate only if it
does, so the fixture cannot drift away from its legs.

  python tests/golden/gen_kernel_forcing.py

The first kept operations that consume the raw input:
  secp256k1  the ladder's step 0 keeps double(r1) = double(P) when bit 7 of the scalar's byte 0 is set (2655-2659)
  P-256      MSB first: at the first set bit result = 0 + P = P, the next step doubles P and adds P to it (2120-2156)
  Ed25519    LSB first: step 0 doubles the raw addend P (2062-2097)
"""
import ctypes
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from oracle import py_model as M  # noqa: E402
import vectors as V  # noqa: E402

W = 1 << 256
L = V.limbs_of
PER_FAMILY = 4          # crafted points per family (and one fixed-base base per family)
FIXED_SCALARS = 3       # scalars per fixed-base base
SEARCH_CANDIDATES = 1 << 30  # per leg and operand: about 20 s on 16 cores
SEARCH_THREADS = 16
SEARCH_SEED = 0x5EA4C4
# legs every multiplication takes (its first addition has the identity as an operand): not recorded per case
ROUTINE = {"SECP_PDOUBLE_ID", "SECP_PADD_EARLY", "P256_PADD_EARLY", "ED_PADD_EARLY"}


def host_emul():
    so = os.path.join(ROOT, "tools", "libhost_emul.so")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so,
                           os.path.join(ROOT, "tools", "host_emul.cpp")])
    return ctypes.CDLL(so)


class Reach:
    """he_multiply / he_ed_multiply_fixed with the rare-leg counters read around the call"""

    def __init__(self, emu):
        self.emu = emu
        emu.he_rare_leg_name.restype = ctypes.c_char_p
        self.n = emu.he_rare_leg_count()
        self.names = [emu.he_rare_leg_name(i).decode() for i in range(self.n)]
        self.buf = (ctypes.c_ulong * self.n)()

    def snap(self):
        self.emu.he_rare_legs(self.buf)
        return list(self.buf)

    def legs(self, curve, point, scalar, fixed=False):
        p = np.ascontiguousarray(np.array(point, dtype=np.uint64).reshape(-1))
        k = np.ascontiguousarray(np.array(scalar, dtype=np.uint64))
        out = np.zeros(p.size, dtype=np.uint64)
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        before = self.snap()
        if fixed and curve == 2:
            self.emu.he_ed_multiply_fixed(ptr(p), ptr(k), ptr(out))
        else:
            self.emu.he_multiply(curve, ptr(p), ptr(k), ptr(out))
        after = self.snap()
        return {self.names[i] for i in range(self.n) if after[i] > before[i]}, [int(v) for v in out]


def flat(pt):
    return [int(w) for c in pt for w in c]


def main():
    rng = random.Random(0x4B46C0DE)
    reach = Reach(host_emul())
    out = {"provenance": "restatement-derived by oracle/py_model.py; not reference-executed",
           "point_limbs": {str(c): V.POINT_LIMBS[c] for c in range(3)}, "cases": [], "bases": []}
    fixtures = json.load(open(os.path.join(HERE, "forcing_vectors.json")))["cases"]
    ripple = json.load(open(os.path.join(HERE, "secp256k1_sqr_ripple_operands.json")))["operands"]

    def rnd(curve):
        return rng.randrange(1, V.PRIME[curve])

    def scalar(curve, setbits=()):
        k = rng.getrandbits(256) % V.ORDER[curve]
        for b in setbits:
            k |= 1 << b
        return L(k)

    def keep(curve, family, legs, cands, k_of):
        """the first PER_FAMILY candidate points on which every leg of `legs` fires, with their scalar; a case records
        every non-routine leg it lights"""
        F = M.CURVES[curve]
        got = 0
        for pt in cands:
            k = k_of()
            lit, _ = reach.legs(curve, flat(pt), k)
            if not set(legs) <= lit:
                continue
            want = F.multiply(tuple(list(c) for c in pt), k)
            out["cases"].append({"curve": curve, "family": family, "legs": sorted(lit - ROUTINE), "scalar": [int(v) for v in k],
                                 "point": flat(pt), "expect": flat(want)})
            if got == 0:
                base_case(curve, family, legs, pt)
            got += 1
            if got == PER_FAMILY:
                return
        if got == 0:
            raise RuntimeError("family %s: no candidate reaches %s" % (family, legs))

    def base_case(curve, family, legs, pt):
        """the family's first point as a fixed base: FIXED_SCALARS scalars whose first kept step consumes it"""
        F = M.CURVES[curve]
        ks, exp = [], []
        for _ in range(FIXED_SCALARS):
            k = k_first(curve)
            ks.append([int(v) for v in k])
            exp.append(flat(F.multiply(tuple(list(c) for c in pt), k)))
        lit = reach.legs(curve, flat(pt), ks[0], fixed=True)[0]
        assert set(legs) <= lit, (family, legs, lit)
        out["bases"].append({"curve": curve, "family": family, "legs": sorted(legs), "point": flat(pt),
                             "scalars": ks, "expect": exp})

    def k_first(curve):
        if curve == 0:
            return scalar(0, (7,))            # ladder bit 0: step 0 keeps double(P)
        if curve == 1:
            return scalar(1, (255 - 8, 255 - 9))  # a set bit early enough that P is doubled and added on
        return scalar(2, (0,))                # Ed25519 doubles P at step 0 whatever the bit

    # ---------------- secp256k1 ----------------
    F0 = M.Secp
    for fam, leg in (("secp_sqr_cross_ripple", "SECP_SQR_RIPPLE"), ("secp_sqr_fold_ripple", "SECP_SQR_FOLD_RIPPLE"),
                     ("secp_sqr_fold_general", "SECP_SQR_FOLD_GENERAL")):
        try:
            keep(0, fam, ["SECP_SQR_EXC", leg], ((a, L(rnd(0)), L(rnd(0))) for a in ripple), lambda: k_first(0))
        except RuntimeError as e:
            print(e)
    borrow = [(c["a"], c["b"]) for c in fixtures if c["family"] == "secp_mul_borrow"]
    keep(0, "secp_mul_borrow", ["SECP_MUL_BW"], ((L(rnd(0)), a, b) for a, b in borrow), lambda: k_first(0))
    gep = [(c["a"], c["b"]) for c in fixtures if c["family"] == "secp_mul_ge_p" and c["op"] == "mul"]
    keep(0, "secp_mul_ge_p", ["SECP_CSUB_P"], ((L(rnd(0)), a, b) for a, b in gep), lambda: k_first(0))

    def add_top():  # x + sqr(y) with an all-ones top word: pdouble's add(p.x, b)
        while True:
            y = L(rnd(0))
            b = sum(v << (64 * i) for i, v in enumerate(F0.sqr(y)))
            s = (0xFFFFFFFF << 224) | rng.getrandbits(224)
            yield (L((s - b) % W), y, L(rnd(0)))
    keep(0, "secp_add_top", ["SECP_ADD_TOP"], add_top(), lambda: k_first(0))

    def add_carry():  # x + sqr(y) >= 2^256 with low 64 bits >= 2^64 - c: the short + c chain carries past word 1
        while True:
            y = L(rnd(0))
            b = sum(v << (64 * i) for i, v in enumerate(F0.sqr(y)))
            s = (rng.getrandbits(190) << 64) | ((1 << 64) - 1 - rng.randrange(1 << 20))
            if s < b:
                yield (L(W + s - b), y, L(rnd(0)))
    keep(0, "secp_add_carry", ["SECP_ADD_CARRY"], add_carry(), lambda: k_first(0))

    def x_zero():  # X = 0 stays 0 under doubling: the next ladder addition meets u1 = u2 = 0 on two finite points
        while True:
            yield (L(0), L(rnd(0)), L(rnd(0)))
    keep(0, "secp_x_zero", ["SECP_PADD_UEQ"], x_zero(), lambda: k_first(0))

    # ---------------- P-256 ----------------
    p1 = V.PRIME[1]
    nc = [p1, p1 + 1, p1 + 2, W - 1, W - 2, (0xFFFFFFFF << 224) | rng.getrandbits(224), W - (1 << 224),
          W - (1 << 96), (0xFFFFFFFF << 224) | rng.getrandbits(224)]

    def p256_noncanon(coord):
        for v in nc:
            pt = [L(rnd(1)), L(rnd(1)), L(rnd(1))]
            pt[coord] = L(v)
            yield tuple(pt)
    keep(1, "p256_noncanonical_x", ["P256_ADD_GENERAL"], p256_noncanon(0), lambda: k_first(1))
    keep(1, "p256_noncanonical_y", ["P256_ADD_GENERAL"], p256_noncanon(1), lambda: k_first(1))

    def x_ge_p():  # x in [p, 2p): the products canonicalise it, so the addition of P to 2P can meet u1 == u2
        while True:
            yield (L(p1 + rng.randrange(3)), L(rnd(1)), L(rnd(1)))
    keep(1, "p256_x_ge_p_ueq", ["P256_PADD_UEQ"], x_ge_p(), lambda: k_first(1))

    def zlow():
        for z in [1 << 32, (1 << 32) + 1, 1 << 64, (1 << 128) + 1, (rng.getrandbits(224) << 32), (rng.getrandbits(224) << 32) | 1]:
            yield (L(rnd(1)), L(rnd(1)), L(z))
    keep(1, "p256_z_low_word", ["P256_PDBL_ZLOW"], zlow(), lambda: k_first(1))

    # ---------------- Ed25519 ----------------
    p2 = V.PRIME[2]
    near = [p2 - 1, p2, p2 + 1, p2 + 18, (1 << 255) - 1, W - 1, W - 19, W - 20, (0x7FFFFFFF << 224) | rng.getrandbits(224),
            (0xFFFFFFFF << 224) | rng.getrandbits(224), (0x80000000 << 224) | rng.getrandbits(224)]

    def ed_near(coord):
        for v in near * 2:
            pt = [L(rnd(2)) for _ in range(4)]
            pt[coord] = L(v)
            yield tuple(pt)
    keep(2, "ed_near_p_x", ["ED_ADD_CARRY"], ed_near(0), lambda: k_first(2))
    keep(2, "ed_near_p_y", ["ED_REDUCE_TOP"], ed_near(1), lambda: k_first(2))
    small = [c["a"] for c in fixtures if c["family"] == "ed_small_add_carry" and c["op"] in ("mul", "sqr")]

    def ed_small(coord):
        for a in small:
            pt = [L(rnd(2)) for _ in range(4)]
            pt[coord] = a
            yield tuple(pt)
    keep(2, "ed_small_add_carry", ["ED_MUL_EXC"], ed_small(2), lambda: k_first(2))

    def ed_x_zero():  # x == -x: the doubling's `opposite` early-out returns the identity
        while True:
            yield (L(0), L(rnd(2)), L(rnd(2)), L(rnd(2)))
    keep(2, "ed_x_zero", ["ED_PDBL_OPPOSITE"], ed_x_zero(), lambda: k_first(2))

    # ---------------- secp256k1 with z = 1: batch_ecdh's keys are affine ----------------
    one = L(1)
    for fam, leg in (("secp_sqr_cross_ripple", "SECP_SQR_RIPPLE"), ("secp_sqr_fold_ripple", "SECP_SQR_FOLD_RIPPLE")):
        keep(0, fam + "_affine", ["SECP_SQR_EXC", leg], ((a, L(rnd(0)), one) for a in ripple), lambda: k_first(0))
    keep(0, "secp_mul_borrow_affine", ["SECP_MUL_BW"], ((L(rnd(0)), a, one) for a, _ in borrow), lambda: k_first(0))
    keep(0, "secp_mul_ge_p_affine", ["SECP_CSUB_P"], ((L(rnd(0)), a, one) for a, _ in gep), lambda: k_first(0))
    keep(0, "secp_add_top_affine", ["SECP_ADD_TOP"], ((x, y, one) for x, y, _ in add_top()), lambda: k_first(0))
    keep(0, "secp_add_carry_affine", ["SECP_ADD_CARRY"], ((x, y, one) for x, y, _ in add_carry()), lambda: k_first(0))
    keep(0, "secp_x_zero_affine", ["SECP_PADD_UEQ"], ((x, y, one) for x, y, _ in x_zero()), lambda: k_first(0))

    # ---------------- bounded searches: mul_small_k's legs on the first doubling's operands ----------------
    # The operand is square(x) (K = 3) or square(square(y)) (K = 8) of the raw coordinate; the reference's secp256k1
    # square is not a field square, so no operand can be constructed and the search runs forward, in C, on the counters.
    out["searches"] = []
    h = np.zeros(4, dtype=np.uint64)
    reach.emu.he_search_mulk.restype = ctypes.c_ulong
    for curve, leg in ((0, "SECP_MULK_EXC"), (0, "SECP_MULK_BW"), (1, "P256_MULK_EXC")):
        for which, operand in ((0, "mul_small(sqr(x), 3)"), (1, "mul_small(sqr(sqr(y)), 8)")):
            hits = reach.emu.he_search_mulk(curve, which, reach.names.index(leg), ctypes.c_uint64(SEARCH_SEED + which),
                                            ctypes.c_ulong(SEARCH_CANDIDATES), SEARCH_THREADS, ctypes.c_void_p(h.ctypes.data))
            out["searches"].append({"curve": curve, "leg": leg, "operand": operand, "candidates": SEARCH_CANDIDATES,
                                    "hits": int(hits)})
            if hits:
                pt = [L(rnd(curve)) for _ in range(3)]
                pt[which] = [int(v) for v in h]
                keep(curve, "%s_search_%s" % (leg.lower(), "xy"[which]), [leg], iter([tuple(pt)]), lambda: k_first(curve))

    with open(os.path.join(HERE, "kernel_forcing_vectors.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(len(out["cases"]), "cases,", len(out["bases"]), "bases")


if __name__ == "__main__":
    main()
