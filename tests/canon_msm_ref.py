"""
Reference for canonical mode's multi-scalar multiplication (fec_canon_msm): expected sums from oracle/canon_model.py, never
from the library.

Cheap expected values: every test point is a known multiple of the generator, P_i = a_i G, so a sum of any size costs one
model multiplication, sum k_i P_i = (sum k_i a_i mod N) G.  On Ed25519 P_i = a_i B + j_i T with T of order 8 (scalars are NOT
reduced modulo l by the call, and the torsion part tells k from k mod l): the sum is (sum k_i a_i mod l) B + (sum k_i j_i
mod 8) T.  msm_direct is the sum of model multiplications the shortcut is checked against (tests/test_canon_msm_model.py).

A point reference `r` of a case: an int i >= 0 is pool[i], i < 0 is -pool[-i - 1]; on Ed25519 "t<j>" is j T and "id" is (0, 1).
tests/golden/canon_msm_vectors.json (gen_canon_msm.py) holds the pool of 64 points per curve with their logarithms and the
explicit cases; the large cases are drawn from the pool by draw(), a seeded rule, and never stored.
"""
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import canon_model as CM  # noqa: E402

MODELS = {"secp256k1": CM.SECP256K1, "p256": CM.P256, "ed25519": CM.ED25519}
CURVE_ID = {"secp256k1": 0, "p256": 1, "ed25519": 2}
WINDOWS = (2, 4, 5, 8, 13, 16)
FINITE, INFINITY, BAD_POINT = 0, 1, 2
TOP = 2**256 - 1


def is_ed(name):
    return name == "ed25519"


def identity(name):
    return (0, 1) if is_ed(name) else CM.INF


def steering_scalars(name, windows=WINDOWS):
    """the scalars that steer the recoding, for every window width in `windows`"""
    N = MODELS[name].N
    ks = {0, 1, N - 1, N, N + 1, 2**255, TOP}
    for c in windows:
        ks |= {2**(c - 1) - 1, 2**(c - 1), 2**(c - 1) + 1, 2**c - 1, 2**c}
    return sorted(ks)


def msm_direct(name, ks, pts):
    """sum k_i P_i, one model multiplication per element"""
    C = MODELS[name]
    acc = identity(name)
    for k, p in zip(ks, pts):
        acc = C.add(acc, C.mul(k, p))
    return acc


def msm_by_logs(name, ks, logs, js=None, T=None):
    """the same sum from the logarithms: (sum k a mod N) G [+ (sum k j mod 8) T]"""
    C = MODELS[name]
    s = C.mul(sum(k * a for k, a in zip(ks, logs)) % C.N, C.G)
    if is_ed(name):
        s = C.add(s, C.mul(sum(k * j for k, j in zip(ks, js)) % 8, T))
    return s


def result(name, pt):
    """(xy as 8 limbs, status) as the call returns a sum"""
    if pt is CM.INF:
        return [0] * 8, INFINITY
    return CM.limbs(pt[0]) + CM.limbs(pt[1]), FINITE


class Fixture:
    def __init__(self, path):
        self.raw = json.load(open(path))
        self.curves = {}
        for name, d in self.raw["curves"].items():
            pool = [(int(e["a"], 16), e["j"], (int(e["x"], 16), int(e["y"], 16))) for e in d["pool"]]
            T = tuple(int(v, 16) for v in d["T"]) if "T" in d else None
            self.curves[name] = {"pool": pool, "T": T, "cases": d["cases"]}

    def pool(self, name):
        return self.curves[name]["pool"]

    def T(self, name):
        return self.curves[name]["T"]

    def cases(self, name):
        return self.curves[name]["cases"]

    def resolve(self, name, ref):
        """(point, a, j) of a point reference"""
        C, pool, T = MODELS[name], self.pool(name), self.T(name)
        if isinstance(ref, str):
            if ref == "id":
                return (0, 1), 0, 0
            j = int(ref[1:])
            return C.mul(j, T), 0, j
        if ref >= 0:
            a, j, p = pool[ref]
            return p, a, j
        a, j, p = pool[-ref - 1]
        return C.neg(p), (-a) % C.N, (-j) % 8

    def expected(self, name, ks, refs):
        """the model's sum for scalars ks and point references refs, by the logarithms"""
        res = [self.resolve(name, r) for r in refs]
        return msm_by_logs(name, ks, [a for _, a, _ in res], [j for _, _, j in res], self.T(name))

    def points(self, name, refs):
        return [self.resolve(name, r)[0] for r in refs]


def load_fixture(path=None):
    return Fixture(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canon_msm_vectors.json"))


def draw(name, n, seed):
    """the seeded rule of the large cases: n scalars below 2^256 and n pool references"""
    rng = random.Random("canon-msm/%s/%d/%d" % (name, n, seed))
    ks = [rng.getrandbits(256) for _ in range(n)]
    refs = [rng.randrange(64) for _ in range(n)]
    return ks, refs


def pack(ks, pts):
    """(scalars (n, 4) uint64, points (n, 8) uint64)"""
    k = np.array([CM.limbs(v) for v in ks], dtype=np.uint64).reshape(-1, 4)
    p = np.array([CM.xy_limbs(q) for q in pts], dtype=np.uint64).reshape(-1, 8)
    return k, p


def chain(name, n, a0, T=None):
    """n DISTINCT points for one model addition each: P_i = (a0 + i) G [+ (i mod 8) T]; returns (points, logs, js)"""
    C = MODELS[name]
    step = C.add(C.G, T) if is_ed(name) else C.G
    p, pts = C.mul(a0, C.G), []
    for _ in range(n):
        pts.append(p)
        p = C.add(p, step)
    return pts, [(a0 + i) % C.N for i in range(n)], [i % 8 for i in range(n)]
