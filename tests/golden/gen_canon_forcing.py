"""
Writes tests/golden/canon_forcing_vectors.json: operands and points on which the rare legs of canonical mode
(forge_ec_amd/csrc/canon_curves.hpp, census in tests/rare_legs.json) are taken, with a fixed seed:

    python tests/golden/gen_canon_forcing.py [--search-log2 30]

Every case is CONFIRMED by the reach counters of the host emulation (tools/host_emul.cpp, limbs.hpp FEC_RARE_LEGS): a
candidate is kept only when exactly the legs of its family fire.  Every EXPECTED value is a big-integer result of
oracle/canon_model.py (tests/canon_msg_ref.py for the encodings); the emulation's own output is compared with it here and
never written.  Integers are 64 hex digits, points x then y, null for infinity.

"families": name -> curve (0 secp256k1, 1 P-256, 2 Ed25519), op, legs, and what the window is.
"field":    family, curve, op, a, b (null for sqr), t = the product modulo p that was aimed at (null for add / sub), expect.
            mul cases are (a, b = t / a) with a random, sqr cases a = +-sqrt(t): sqr_wide is another multiplier than mul_wide.
"points":   on-curve points whose coordinate fires the family's legs inside on_curve (x = sqrt(t); Ed25519: y = sqrt(t)),
            their encodings, and what the entry points must answer for them: k * P, u1 G + u2 P, a valid ECDSA (z, r, s),
            BIP-340 (r, s, e) and EdDSA (r, s, h) under P as the key, built from the model without a secret key.
"edge_scalars": k * P and k * G with the scalars that make the mixed / windowed additions meet infinity or their own
            operand (canon_curves.hpp jadd_affine, jadd_window).
"glv":      the bound that makes glv_secp::mul_window's top window dead, and the structured search for a scalar beyond it.
"searches": candidates tried and kept per family, and the 2^30 random scalars of the GLV search.
"""
import argparse
import ctypes
import json
import math
import os
import random
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), ROOT]

import canon_msg_ref as R  # noqa: E402
from oracle import canon_model as M  # noqa: E402

SEED = 0xCA11F0
SO = os.path.join(ROOT, "tools", "libhost_emul.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "inv": 5}
CURVES = [M.SECP256K1, M.P256, M.ED25519]
PS = [C.P for C in CURVES]
C_SECP = 2**32 + 977
NEGP256 = 2**256 - M.P256.P
FIELD_CASES, SEARCHED_CASES, POINT_CASES = 4, 2, 2
SEARCH_THREADS = 8   # part of the search's definition: thread t draws its own splitmix64 stream

# GLV basis of secp256k1 (Guide to ECC, Alg. 3.74): a_i + b_i lambda = 0 (mod n)
GLV_LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
GLV_A1 = 0x3086D221A7D46BCDE86C90E49284EB15
GLV_B1 = -0xE4437ED6010E88286F547FA90ABFE4C3
GLV_A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
GLV_B2 = GLV_A1
GLV_G1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031   # round(2^384 b2 / n)
GLV_G2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71   # round(2^384 (-b1) / n)


def hx(v):
    return "%064x" % v


def pt_hex(pt):
    return None if pt is M.INF else hx(pt[0]) + hx(pt[1])


class Emu:
    """the host emulation and its reach counters"""

    def __init__(self):
        src = os.path.join(ROOT, "tools", "host_emul.cpp")
        subprocess.check_call([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, src])
        self.lib = ctypes.CDLL(SO)
        self.lib.he_rare_leg_name.restype = ctypes.c_char_p
        self.lib.he_search_glv_top.restype = ctypes.c_ulong
        self.names = [self.lib.he_rare_leg_name(i).decode() for i in range(self.lib.he_rare_leg_count())]
        self.buf = (ctypes.c_ulong * len(self.names))()

    def snap(self):
        self.lib.he_rare_legs(self.buf)
        return list(self.buf)

    def run(self, fn, *args):
        """-> (return value, names of the counters that moved)"""
        keep = [np.array(M.limbs(a), dtype=np.uint64) if isinstance(a, int) and a >= 0 and not isinstance(a, bool) else a for a in args]
        ptrs = [ctypes.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in keep]
        before = self.snap()
        ret = getattr(self.lib, fn)(*ptrs)
        after = self.snap()
        return ret, {self.names[i] for i in range(len(after)) if after[i] > before[i]}

    def field_op(self, cid, op, a, b):
        out = np.zeros(4, dtype=np.uint64)
        _, lit = self.run("he_canon_field_op", ctypes.c_int(cid), ctypes.c_int(OPS[op]), a, 0 if b is None else b, out)
        return M.unlimbs(out), lit


def sqrt_mod(cid, a):
    P = PS[cid]
    if cid < 2:
        r = pow(a, (P + 1) // 4, P)
    else:
        r = pow(a, (P + 3) // 8, P)
        if r * r % P != a % P:
            r = r * pow(2, (P - 1) // 4, P) % P
    return r if r * r % P == a % P else None


def hi_words_max(v):
    return max((v >> (32 * k)) & 0xFFFFFFFF for k in range(8, 16))


# ---- field families ------------------------------------------------------------------------------------------------
def product_family(name, cid, legs, lo, hi, what, need_high_word=None):
    """mul and sqr families aiming at a product t in [lo, hi) modulo p; need_high_word: True / False = the 512-bit product
    must (not) have a word of its high half >= 0xFFFFF000 (secp256k1's general reduction)"""
    P = PS[cid]

    def high_ok(v):
        return need_high_word is None or (hi_words_max(v) >= 0xFFFFF000) == need_high_word

    def mul(rng):
        t, a = rng.randrange(lo, hi), rng.randrange(1, P)
        b = t * pow(a, -1, P) % P
        return (a, b, t) if high_ok(a * b) else None

    def sqr(rng):
        t = rng.randrange(lo, hi)
        a = sqrt_mod(cid, t)
        if a is None:
            return None
        a = P - a if rng.random() < 0.5 and a else a
        return (a, None, t) if high_ok(a * a) else None

    n = SEARCHED_CASES if need_high_word else FIELD_CASES   # one hit in ~2^16 candidates
    return [dict(name=name + "_mul", curve=cid, op="mul", legs=legs, what=what, draw=mul, n=n),
            dict(name=name + "_sqr", curve=cid, op="sqr", legs=legs, what=what, draw=sqr, n=n)]


def secp_general_family(name, legs, top, what):
    """products through reduce512_general: top = operands within 2^235 of 2^256 (the product's top word is all ones), else
    operands built so that word 9, 10 or 11 of the product is all ones and its top word is ordinary"""
    P = PS[0]

    def target(rng):
        k = rng.randrange(9, 12)
        v = rng.randrange(2**479, 2**508)
        return v | (0xFFFFFFFF << (32 * k)) | (1 << (32 * k - 1))      # the bit below keeps a borrow from the low half out

    def mul(rng):
        if top:
            return (rng.randrange(2**256 - 2**235, P), rng.randrange(2**256 - 2**235, P), None)
        a = rng.randrange(2**255, P)
        b = target(rng) // a
        return (a, b, None) if b < P and hi_words_max(a * b) >= 0xFFFFF000 and (a * b) >> 480 < 0xFFFFF000 else None

    def sqr(rng):
        if top:
            return (rng.randrange(2**256 - 2**235, P), None, None)
        a = math.isqrt(target(rng))
        return (a, None, None) if a < P and hi_words_max(a * a) >= 0xFFFFF000 and (a * a) >> 480 < 0xFFFFF000 else None

    return [dict(name=name + "_mul", curve=0, op="mul", legs=legs, what=what, draw=mul),
            dict(name=name + "_sqr", curve=0, op="sqr", legs=legs, what=what, draw=sqr)]


def sum_family(name, cid, op, legs, what, draw):
    return [dict(name=name, curve=cid, op=op, legs=legs, what=what, draw=draw)]


def add_with_sum(cid, lo, hi, keep=lambda a, b: True):
    """canonical a, b with a + b (as integers) in [lo, hi)"""
    P = PS[cid]

    def draw(rng):
        s = rng.randrange(lo, hi)
        a = rng.randrange(max(0, s - P + 1), min(P, s + 1))
        b = s - a
        return (a, b, None) if 0 <= b < P and keep(a, b) else None
    return draw


def sub_with_difference(cid, low_bits, below):
    """canonical a < b whose difference a - b modulo 2^256 has its low `low_bits` bits below `below`"""
    P = PS[cid]

    def draw(rng):
        d = (rng.randrange(1, 2**(256 - low_bits)) << low_bits) | rng.randrange(below)
        b = rng.randrange(P)
        a = b + d - 2**256
        return (a, b, None) if 0 <= a < b else None
    return draw


def field_families():
    P0, P1, P2 = PS
    top1 = lambda v: v >> 224 == 0xFFFFFFFF   # noqa: E731
    f = []
    # secp256k1: the value before the last step is t or t + p; it passes 2^256 exactly for t >= c = 2^32 + 977
    f += product_family("csecp_fast_wrap", 0, ["CSECP_FAST_WRAP"], C_SECP, 2**34, "t in [c, 2^34), fast path: t + p wraps, c is added again; csub_p not entered", False)
    f += product_family("csecp_csub_below_c", 0, ["SECP_CSUB_P"], 0, C_SECP, "t in [0, c): t + p < 2^256, csub_p entered and p subtracted", False)
    f += product_family("csecp_csub_near_p", 0, ["SECP_CSUB_P"], P0 - 2**34, P0, "t in [p - 2^34, p): csub_p entered, nothing subtracted", False)
    f += secp_general_family("csecp_general_top", ["CSECP_GENERAL"], True, "operands within 2^235 of 2^256: the product's top word sends it to reduce512_general")
    f += secp_general_family("csecp_general_mid", ["CSECP_GENERAL"], False, "word 9, 10 or 11 of the product all ones, its top word ordinary")
    f += product_family("csecp_general_wrap", 0, ["CSECP_GENERAL", "CSECP_GENERAL_WRAP"], C_SECP, 2**34, "t in [c, 2^34) and a high word >= 0xFFFFF000: reduce512_general's own wrap", True)
    f += product_family("csecp_general_csub", 0, ["CSECP_GENERAL", "SECP_CSUB_P"], 0, C_SECP, "t in [0, c) and a high word >= 0xFFFFF000: reduce512_general ends in csub_p, p subtracted", True)
    # borrowed from secp256k1.hpp
    f += sum_family("csecp_add_top_ge_p", 0, "add", ["SECP_ADD_TOP"], "a + b in [p, 2^256): top word all ones, p subtracted", add_with_sum(0, P0, 2**256))
    f += sum_family("csecp_add_top_lt_p", 0, "add", ["SECP_ADD_TOP"], "a + b in [2^256 - 2^224, p): leg entered, nothing subtracted", add_with_sum(0, 2**256 - 2**224, P0))
    f += sum_family("csecp_add_carry", 0, "add", ["SECP_ADD_CARRY"], "a + b = 2^256 + s with the low 64 bits of s within c of 2^64: the + c carries past word 1",
                    _secp_add_carry)
    f += sum_family("csecp_sub_borrow", 0, "sub", ["SECP_SUB_BORROW"], "a < b with the low 64 bits of a - b below c: the - c borrows past word 1", sub_with_difference(0, 64, C_SECP))
    # P-256: the value before the last step is t or t + p; t + p passes 2^256 exactly for t >= 2^256 - p = 2^224 - 2^192 - 2^96 + 1
    f += product_family("cp256_wrap", 1, ["CP256_WRAP"], NEGP256, NEGP256 + 2**34, "t in [2^256 - p, 2^256 - p + 2^34): t + p wraps, 2^256 - p is added again")
    f += product_family("cp256_wrap_2_224", 1, ["CP256_WRAP"], 2**224, 2**224 + 2**200, "t in [2^224, 2^224 + 2^200): the same wrap, further in")
    f += product_family("cp256_csub_below_wrap", 1, ["CP256_CSUB_P"], NEGP256 - 2**34, NEGP256, "t in [2^256 - p - 2^34, 2^256 - p): t + p just below 2^256, csub_p_unlikely entered and p subtracted")
    f += product_family("cp256_csub_small", 1, ["CP256_CSUB_P"], 0, 2**34, "t in [0, 2^34): t + p, csub_p_unlikely entered and p subtracted")
    f += product_family("cp256_csub_near_p", 1, ["CP256_CSUB_P"], P1 - 2**34, P1, "t in [p - 2^34, p): csub_p_unlikely entered, nothing subtracted")
    # borrowed from p256.hpp
    f += sum_family("cp256_add_operand_top", 1, "add", ["P256_ADD_GENERAL"], "a in [0xFFFFFFFF 2^224, p): an operand's top word is all ones",
                    lambda rng: (rng.randrange(0xFFFFFFFF << 224, P1), rng.randrange(2**200), None))
    f += sum_family("cp256_add_sum_ge_p", 1, "add", ["P256_ADD_GENERAL"], "a + b in [p, 2^256), neither top word all ones: p subtracted",
                    add_with_sum(1, P1, 2**256, lambda a, b: not top1(a) and not top1(b)))
    f += sum_family("cp256_add_sum_lt_p", 1, "add", ["P256_ADD_GENERAL"], "a + b in [0xFFFFFFFF 2^224, p), neither top word all ones: nothing subtracted",
                    add_with_sum(1, 0xFFFFFFFF << 224, P1, lambda a, b: not top1(a) and not top1(b)))
    # Ed25519: the value before the finish is t or t + p; it is t + p for few small t, and t has words 1..6 all ones for t >= 2^255 - 2^32
    f += product_family("ced_finish_small", 2, ["CED_FINISH"], 19, 2**11, "t in [19, 2^11) where the fold left t + p >= 2^255: ed::reduce subtracts p")
    f += product_family("ced_finish_below_19", 2, ["CED_FINISH", "ED_REDUCE_TOP"], 0, 19, "t in [0, 19) where the fold left t + p < 2^255: words 1..6 all ones, ed::reduce's exact comparison, p subtracted")
    f += product_family("ced_finish_near_p", 2, ["CED_FINISH", "ED_REDUCE_TOP"], P2 - 2**32, P2, "t in [p - 2^32, p): both legs entered, nothing subtracted")
    # borrowed from ed25519.hpp
    f += sum_family("ced_add_reduce_carry", 2, "add", ["ED_REDUCE_CARRY"], "a + b = 2^255 + s with the low word of s within 19 of 2^32: the + 19 leaves word 0",
                    _ed_add_carry)
    f += sum_family("ced_add_reduce_top_ge_p", 2, "add", ["ED_REDUCE_TOP"], "a + b in [p, 2^255): p subtracted", add_with_sum(2, P2, 2**255))
    f += sum_family("ced_add_reduce_top_lt_p", 2, "add", ["ED_REDUCE_TOP"], "a + b in [2^255 - 2^224, p): leg entered, nothing subtracted", add_with_sum(2, 2**255 - 2**224, P2))
    f += sum_family("ced_sub_borrow", 2, "sub", ["ED_SUB_BORROW"], "a < b with the low word of a - b below 19: the - 19 borrows past word 0", sub_with_difference(2, 32, 19))
    return f


def _ed_add_carry(rng):
    P = PS[2]
    s = 2**255 + ((rng.randrange(2**221) << 32) | rng.randrange(2**32 - 19, 2**32))
    a = rng.randrange(s - P + 1, P)
    return (a, s - a, None)


def _secp_add_carry(rng):
    P = PS[0]
    s = 2**256 + ((rng.randrange(2**190) << 64) | rng.randrange(2**64 - C_SECP, 2**64))
    a = rng.randrange(s - P + 1, P)
    return (a, s - a, None)


def build_field(emu, rng, searches):
    families, cases = {}, []
    for fam in field_families():
        cid, op, legs = fam["curve"], fam["op"], set(fam["legs"])
        C = CURVES[cid]
        tried = kept = 0
        while kept < fam.get("n", FIELD_CASES):
            tried += 1
            assert tried < 5_000_000, fam["name"]
            c = fam["draw"](rng)
            if c is None:
                continue
            a, b, t = c
            got, lit = emu.field_op(cid, op, a, b)
            want = C.field_op(op, a, b or 0)
            assert got == want and (t is None or want == t), (fam["name"], hx(a), b and hx(b))   # the emulation is right on the host
            if lit != legs:
                continue
            kept += 1
            cases.append(dict(family=fam["name"], curve=cid, op=op, a=hx(a), b=None if b is None else hx(b), t=None if t is None else hx(t), expect=hx(want)))
        families[fam["name"]] = dict(curve=cid, op=op, legs=sorted(legs), what=fam["what"])
        searches.append(dict(family=fam["name"], legs=sorted(legs), candidates=tried, hits=kept))
        print("%-28s %8d candidates" % (fam["name"], tried), file=sys.stderr, flush=True)
    return families, cases


# ---- points --------------------------------------------------------------------------------------------------------
def point_families():
    P0, P1, P2 = PS
    return [
        dict(name="csecp_point_fast_wrap", curve=0, legs=["CSECP_FAST_WRAP"], window=(C_SECP, 2**34), high=False),
        dict(name="csecp_point_general_top", curve=0, legs=["CSECP_GENERAL"], window=None, high=True),
        dict(name="csecp_point_general_wrap", curve=0, legs=["CSECP_GENERAL", "CSECP_GENERAL_WRAP"], window=(C_SECP, 2**34), high=True),
        dict(name="csecp_point_csub_below_c", curve=0, legs=["SECP_CSUB_P"], window=(0, C_SECP), high=False),
        dict(name="cp256_point_wrap", curve=1, legs=["CP256_WRAP"], window=(NEGP256, NEGP256 + 2**34), high=None),
        dict(name="cp256_point_csub_small", curve=1, legs=["CP256_CSUB_P"], window=(0, 2**34), high=None),
        dict(name="cp256_point_csub_near_p", curve=1, legs=["CP256_CSUB_P"], window=(P1 - 2**34, P1), high=None),
        dict(name="ced_point_finish_small", curve=2, legs=["CED_FINISH"], window=(19, 2**11), high=None),
        dict(name="ced_point_finish_near_p", curve=2, legs=["CED_FINISH", "ED_REDUCE_TOP"], window=(P2 - 2**32, P2), high=None),
    ]


def draw_point(fam, rng):
    """an on-curve point whose x (Ed25519: y) squares to a t of the window, or None"""
    cid = fam["curve"]
    P, C = PS[cid], CURVES[cid]
    if fam["window"] is None:
        v = rng.randrange(2**256 - 2**235, P)
    else:
        v = sqrt_mod(cid, rng.randrange(*fam["window"]))
        if v is None:
            return None
        v = P - v if rng.random() < 0.5 and v else v
    if fam["high"] is not None and (hi_words_max(v * v) >= 0xFFFFF000) != fam["high"]:
        return None
    if cid == 2:
        pt = R.ed_decode(v.to_bytes(32, "little"))
        return pt if pt and pt[0] else None
    w = sqrt_mod(cid, (v * v * v + C.A * v + C.B) % P)
    return (v, w) if w else None


def forge_signatures(cid, Q, rng):
    """valid (z, r, s) / (r, s, e) / (r, s, h) under the key Q, from the model and without a secret key"""
    C = CURVES[cid]
    n = C.N
    out = {}
    if cid == 2:
        S, h = rng.randrange(n), rng.randrange(n)
        Rp = C.add(C.mul(S, C.G), C.mul(h, C.neg(Q)))
        out["eddsa"] = dict(r=hx(int.from_bytes(C.encode(Rp), "little")), s=hx(S), h=hx(h))
        return out
    u1, u2 = rng.randrange(1, n), rng.randrange(1, n)
    Rp = C.add(C.mul(u1, C.G), C.mul(u2, Q))
    r = Rp[0] % n
    s = r * pow(u2, -1, n) % n
    out["ecdsa"] = dict(z=hx(u1 * s % n), r=hx(r), s=hx(s))
    assert r and s
    if cid == 0 and Q[1] % 2 == 0:
        while True:
            s, e = rng.randrange(n), rng.randrange(n)
            Rp = C.add(C.mul(s, C.G), C.mul((n - e) % n, Q))
            if Rp is not M.INF and Rp[1] % 2 == 0:
                break
        out["bip340"] = dict(r=hx(Rp[0]), s=hx(s), e=hx(e))
    return out


def build_points(emu, rng, searches):
    points = []
    xy = np.zeros(8, dtype=np.uint64)
    for fam in point_families():
        cid, legs = fam["curve"], set(fam["legs"])
        C = CURVES[cid]
        tried = kept = 0
        while kept < POINT_CASES:
            tried += 1
            assert tried < 5_000_000, fam["name"]
            pt = draw_point(fam, rng)
            if pt is None:
                continue
            if cid == 0 and kept == 0 and pt[1] % 2:       # the first point of a secp256k1 family has an even y: BIP-340 takes it
                pt = (pt[0], C.P - pt[1])
            assert C.on_curve(pt)
            pin = np.array(M.limbs(pt[0]) + M.limbs(pt[1]), dtype=np.uint64)
            ok, lit = emu.run("he_canon_on_curve", ctypes.c_int(cid), pin)
            assert ok == 1, fam["name"]
            if not legs <= lit:
                continue
            via = {}
            st, via["he_ced_mul" if cid == 2 else "he_canon_mul"] = emu.run("he_ced_mul", 1, pin, xy) if cid == 2 else emu.run("he_canon_mul", ctypes.c_int(cid), 1, pin, xy)
            assert st == 0 and (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == pt, fam["name"]
            enc = {}
            if cid == 2:
                enc["ed"] = C.encode(pt).hex()
                ok, via["he_ed_decode"] = emu.run("he_ed_decode", int.from_bytes(C.encode(pt), "little"), xy)
                assert ok == 1 and (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == pt
            else:
                enc["sec1_33"], enc["sec1_65"] = R.sec1_encode(pt).hex(), R.sec1_encode(pt, compressed=False).hex()
                assert R.sec1_decode(C, bytes.fromhex(enc["sec1_33"])) == pt
                if cid == 0 and pt[1] % 2 == 0:
                    enc["x_only"] = hx(pt[0])
                    assert R.lift_x(pt[0]) == pt
            assert all(legs <= v for v in via.values()), (fam["name"], via)
            kept += 1
            n = C.N
            ks = [1, 2, n - 1, rng.randrange(2**256)]
            u1, u2 = rng.randrange(1, n), rng.randrange(1, n)
            rec = dict(family=fam["name"], curve=cid, legs=sorted(legs), via=sorted(via), x=hx(pt[0]), y=hx(pt[1]), **enc,
                       mul=[dict(k=hx(k), out=pt_hex(C.mul(k % n if cid < 2 else k, pt))) for k in ks],
                       dm=dict(u1=hx(u1), u2=hx(u2), out=pt_hex(C.add(C.mul(u1, C.G), C.mul(u2, pt)))), **forge_signatures(cid, pt, rng))
            points.append(rec)
        searches.append(dict(family=fam["name"], legs=sorted(legs), candidates=tried, hits=kept))
        print("%-28s %8d candidates" % (fam["name"], tried), file=sys.stderr, flush=True)
    return points


# ---- the additions' exceptional legs -----------------------------------------------------------------------------------
def build_edge_scalars(emu, rng):
    out = []
    xy = np.zeros(8, dtype=np.uint64)
    for cid in (0, 1):
        C = CURVES[cid]
        n = C.N
        Q = C.mul(rng.randrange(1, n), C.G)
        for fn, pt, ks in (("mul", Q, [0, 1, n - 1, n, n + 1]), ("mul", C.G, [n]), ("mul_base", None, [0, 1, n - 1, n, 2**256 - 1])):
            for k in ks:
                want = C.mul(k % n, pt or C.G)
                if fn == "mul":
                    pin = np.array(M.xy_limbs(pt), dtype=np.uint64)
                    st, lit = emu.run("he_canon_mul", ctypes.c_int(cid), k, pin, xy)
                    if cid == 0:   # the kernel's ladder for secp256k1
                        st2, lit2 = emu.run("he_glv_mul", k, pin, xy)
                        assert st2 == (1 if want is M.INF else 0)
                else:
                    st, lit = emu.run("he_canon_mul_base", ctypes.c_int(cid), k, xy)
                    st8, lit8 = emu.run("he_canon_mul_base8", ctypes.c_int(cid), k, xy)
                    assert st8 == st
                    lit &= lit8
                assert st == (1 if want is M.INF else 0) and (want is M.INF or (M.unlimbs(xy[:4]), M.unlimbs(xy[4:])) == want)
                legs = sorted(l for l in lit if l.startswith("CWEI_"))
                out.append(dict(family="c%s_edge_%s" % (C.name, fn), curve=cid, fn=fn, k=hx(k), point=None if pt is None else pt_hex(pt), out=pt_hex(want), legs=legs))
    return out


# ---- GLV: the top window -----------------------------------------------------------------------------------------------
def glv_model(k):
    """the decomposition as glv_secp::decompose computes it, with big integers: signed (k1, k2)"""
    n = M.SECP256K1.N
    k %= n
    c1, c2 = (k * GLV_G1 + 2**383) >> 384, (k * GLV_G2 + 2**383) >> 384
    k2 = (c1 * -GLV_B1 + c2 * -GLV_B2) % n
    k1 = (k - k2 * GLV_LAMBDA) % n
    return (k1 - n if k1 > n // 2 else k1), (k2 - n if k2 > n // 2 else k2)


def convergents(num, den):
    h0, h1, k0, k1 = 0, 1, 1, 0
    while den:
        q = num // den
        num, den = den, num - q * den
        h0, h1, k0, k1 = h1, q * h1 + h0, k1, q * k1 + k0
        yield h1, k1


def build_glv(emu, rng, searches, search_log2):
    n = M.SECP256K1.N
    assert (GLV_A1 + GLV_B1 * GLV_LAMBDA) % n == 0 and (GLV_A2 + GLV_B2 * GLV_LAMBDA) % n == 0
    assert GLV_A1 * GLV_B2 - GLV_A2 * GLV_B1 == n
    # (k, 0) = beta1 v1 + beta2 v2 with beta1 = b2 k / n, beta2 = -b1 k / n; c_i = beta_i + e_i.  g_i = 2^384 |b| / n within
    # 1/2, k < 2^256, so k g_i / 2^384 is within 2^-129 of beta_i and rounding adds at most 1/2:  |e_i| <= 1/2 + 2^-129.
    # (k1, k2) = (k, 0) - c1 v1 - c2 v2 = -e1 v1 - e2 v2:  |k1| <= (|a1| + |a2|) (1/2 + 2^-129), |k2| <= (|b1| + |b2|) (1/2 + 2^-129)
    bound1 = (abs(GLV_A1) + abs(GLV_A2)) // 2 + 2
    bound2 = (abs(GLV_B1) + abs(GLV_B2)) // 2 + 2
    assert max(bound1, bound2) < 2**128
    cands = []
    for den in (GLV_B2, -GLV_B1):                     # rounding boundaries of c1 and c2: b k / n = m + 1/2
        for _ in range(20000):
            m = rng.randrange(den)
            cands += [((2 * m + 1) * n // (2 * den) + d) % n for d in range(-2, 3)]
    for _ in range(20000):                            # around lattice vectors and their half sums (the corners of the cell)
        i, j = rng.randrange(-2**127, 2**127), rng.randrange(-2**127, 2**127)
        base = i * GLV_A1 + j * GLV_A2
        cands += [(base + d) % n for d in range(-2, 3)] + [((base + GLV_A1 + GLV_A2) // 2 + d) % n for d in range(-2, 3)]
    for h, q in convergents(GLV_B2, -GLV_B1):         # j b1 + i b2 nearly 0: (j a1 + i a2) / 2 is nearly a corner for odd i, j
        for t in range(1, 64, 2):
            base = t * (h * GLV_A1 + q * GLV_A2)
            cands += [((base + s * GLV_A1 + u * GLV_A2) // 2 + d) % n for s in (0, 1) for u in (0, 1) for d in range(-3, 4)]
    cands += [0, 1, n - 1, n, 2**256 - 1, GLV_LAMBDA, n - GLV_LAMBDA, 2**128, 2**128 - 1, (n - 1) // 2, (n + 1) // 2]
    k1, k2 = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    hits, biggest = [], 0
    for k in cands:
        signs, _ = emu.run("he_glv_decompose", k, k1, k2)
        a, b = M.unlimbs(k1), M.unlimbs(k2)
        assert (-a if signs & 1 else a, -b if signs & 2 else b) == glv_model(k), hx(k)
        biggest = max(biggest, a, b)
        if max(a, b) >= 2**128:
            hits.append(hx(k))
    hit, top = (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
    count = 1 << search_log2
    found = emu.lib.he_search_glv_top(ctypes.c_uint64(SEED), ctypes.c_ulong(count), SEARCH_THREADS, hit, ctypes.byref(top))
    searches.append(dict(leg="CGLV_TOP_WINDOW", operand="random 256-bit scalars through glv_secp::decompose, |k1| or |k2| >= 2^128",
                         candidates=count, hits=int(found), largest_bits_96_159=hx(top.value)[-16:]))
    if found:
        hits.append(hx(M.unlimbs(list(hit))))
    return dict(bound_k1=hx(bound1), bound_k2=hx(bound2), structured=dict(candidates=len(cands), hits=len(hits), largest=hx(biggest)), scalars=hits,
                reason="|k1| <= (|a1| + |a2|) (1/2 + 2^-129) and |k2| <= (|b1| + |b2|) (1/2 + 2^-129), both below 2^128: bits 128..131 are clear")


def build(search_log2=30):
    emu = Emu()
    rng = random.Random(SEED)
    searches = []
    families, field = build_field(emu, rng, searches)
    points = build_points(emu, rng, searches)
    edge = build_edge_scalars(emu, rng)
    glv = build_glv(emu, rng, searches, search_log2)
    note = ("Forcing vectors of canonical mode, written by tests/golden/gen_canon_forcing.py (seed %#x): confirmed by the host emulation's reach "
            "counters, expected values from oracle/canon_model.py." % SEED)
    return dict(note=note, families=families, field=field, points=points, edge_scalars=edge, glv=glv, searches=searches)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--search-log2", type=int, default=30)
    args = ap.parse_args()
    fix = build(args.search_log2)
    out = os.path.join(HERE, "canon_forcing_vectors.json")
    line = lambda c: json.dumps(c, sort_keys=True, separators=(",", ":"))   # noqa: E731
    with open(out, "w") as f:   # one case per line
        f.write('{"note": %s,\n"families": {\n%s\n}' % (json.dumps(fix["note"]), ",\n".join("%s: %s" % (json.dumps(k), line(v)) for k, v in fix["families"].items())))
        for name in ("field", "points", "edge_scalars", "searches"):
            f.write(',\n"%s": [\n%s\n]' % (name, ",\n".join(line(c) for c in fix[name])))
        f.write(',\n"glv": %s}\n' % line(fix["glv"]))
    print(out, {k: len(v) for k, v in fix.items() if isinstance(v, (list, dict))})
