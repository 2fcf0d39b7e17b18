"""
The crafted (scalar, point) pairs of tests/golden/kernel_forcing_vectors.json -- every case forces a named rare leg of a
multiply-family kernel in an operation whose result the kernel keeps (census: tests/rare_legs.json) -- as arrays, and
placed among random elements.  Shared by tests/test_gpu_kernel_forcing.py and tests/test_gpu_sched_geometry.py.
"""
import json
import os

import numpy as np

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCING = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_forcing_vectors.json")))


def cases(curve, affine=False):
    """the curve's cases, interleaved across families (case j of every family, then case j + 1): any run of as many
    positions as there are families holds one case of each"""
    cs = [c for c in FORCING["cases"] if c["curve"] == curve and (not affine or c["point"][8:12] == [1, 0, 0, 0])]
    fams = list(dict.fromkeys(c["family"] for c in cs))
    rank = {}
    for c in cs:
        rank[id(c)] = (sum(1 for d in cs[:cs.index(c)] if d["family"] == c["family"]), fams.index(c["family"]))
    cs.sort(key=lambda c: rank[id(c)])
    k = np.array([c["scalar"] for c in cs], dtype=np.uint64)
    p = np.array([c["point"] for c in cs], dtype=np.uint64)
    e = np.array([c["expect"] for c in cs], dtype=np.uint64)
    return k, p, e, [c["family"] for c in cs]


def mixed(curve, n, at, stream):
    """n random canonical (scalar, point) pairs with the crafted cases placed at the indices `at`, cycling over the
    interleaved cases: every family sits at some index once `at` has as many entries as the curve has families"""
    k, p, e, fam = cases(curve)
    at = sorted(set(at))
    assert len(at) >= len(set(fam)), "too few positions to place every family"
    ks, ps = V.scalars(n, curve, stream), V.points(n, curve, stream + 1)
    idx = np.arange(len(at)) % k.shape[0]
    ks[at], ps[at] = k[idx], p[idx]
    return ks, ps, (np.asarray(at), e[idx])
