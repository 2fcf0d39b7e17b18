"""Emit tests/golden/secp256k1_rare_carry_operands.json: operands on which the carries that the secp256k1 fast step
does not compute (tests/test_secp_rare_carry_model.py) fire, and near misses.  Found by search against that model.

    python tests/golden/gen_secp_rare_carry.py
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_secp_rare_carry_model as M  # noqa: E402

P = (1 << 256) - (1 << 32) - 977
ONES = 0xFFFFFFFF


def limbs(words):
    return [int(words[2 * i]) | (int(words[2 * i + 1]) << 32) for i in range(4)]


def value(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def mul_rows():
    rng = np.random.default_rng(20)
    n = 20000
    near = lambda: np.uint64(1 << 32) - rng.integers(1, 10, size=(n, 8), dtype=np.uint64)
    a, b = near(), near()
    # some uniform words, so that the rows are not all alike; canonical values
    for x in (a, b):
        u = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64)
        x[:] = np.where(rng.integers(0, 4, size=(n, 8)) == 0, u, x)
    _, fired = M.mul_scan(a, b, drop=False)
    rows, have = [], set()
    for r in range(n):
        cols = [k for k in range(15) if fired[r, k]]
        if cols and not set(cols) <= have and value(a[r]) < P and value(b[r]) < P:
            have |= set(cols)
            rows.append(("fires", a[r], b[r]))
    assert have == set(range(3, 14)), have  # column 2 cannot fire: a_0 b_2 + C_1 <= 2^64 - 2
    full = np.full(8, ONES, dtype=np.uint64)
    for kind, a0, b7 in (("below", 0xFFFFFFEF, 0xFFFFFFEF), ("threshold", 0xFFFFFFF0, 0xFFFFFFEF), ("threshold", 0xFFFFFFEF, 0xFFFFFFF0),
                         ("threshold", 0xFFFFFFF0, 0xFFFFFFF0)):
        x, y = full.copy(), full.copy()
        x[0], x[7], y[7] = a0, 0xFFFFFFFE, b7
        rows.append((kind, x, y))
    out = []
    for kind, x, y in rows:
        assert value(x) < P and value(y) < P
        _, f = M.mul_scan(x[None, :], y[None, :], drop=False)
        out.append({"kind": kind, "a": limbs(x), "b": limbs(y), "columns": [k for k in range(15) if f[0, k]],
                    "flagged": bool(M.mul_flag(x[None, :], y[None, :])[0])})
    return out


def limb_with_square_word2(target, rng):
    """a 64-bit x with bits 64..95 of x^2 equal to target"""
    while True:
        h = int(rng.integers(1 << 20, 1 << 30))
        x0 = math.isqrt((h << 96) | (target << 64) | (1 << 63))
        for x in range(x0 - 4, x0 + 5):
            if 0 < x < (1 << 64) and ((x * x) >> 64) & ONES == target:
                return x


def sqr_rows():
    rng = np.random.default_rng(21)
    out = []

    def search(limb_index, target, want, kind):
        """operands whose limb `limb_index` squares to word 2 == target, until the model's fired limbs == want"""
        for _ in range(20000):
            l = [int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63) for _ in range(4)]
            l[3] &= (1 << 63) - 1
            l[limb_index] = limb_with_square_word2(target, rng)
            if l[3] >> 63:
                continue
            a = M.words_of([l])
            _, fired, left = M.sqr_cross(a, drop=False)
            got = sorted(i + j + 2 for (i, j) in M.PLUS_ONE if fired[(i, j)][0])
            words = [int(left[k][0]) for k in (6, 10, 14)]
            if got == want and sum(w >= 0xFFFFFFEF for w in words) == 1:
                out.append({"kind": kind, "a": l, "limbs": got, "flagged": bool(M.sqr_flag(left)[0])})
                return
        raise SystemExit("no row for %s" % kind)

    for rep in range(2):
        search(1, ONES, [3], "fires")
        search(2, ONES, [5], "fires")
        search(3, ONES, [7], "fires")
        search(2, 0xFFFFFFFE, [5], "both_plus_ones")
    for li in (1, 2, 3):
        search(li, 0xFFFFFFEF, [], "below")
        search(li, 0xFFFFFFF0, [], "threshold")
    search(2, 0xFFFFFFFE, [], "threshold")  # one +1 only: 0xFFFFFFFE does not wrap
    return out


def main():
    doc = {"note": "secp256k1 field elements (64-bit limbs, least significant first) for the carries the ladder's fast step does not "
                   "compute: Mul rows (a, b) with the columns whose first product carries, square rows with the limbs whose +1 "
                   "ripples inside the limb; kinds: fires, both_plus_ones (L = 5 from 0xFFFFFFFE), below (a deciding word of "
                   "0xFFFFFFEF: unflagged), threshold (flagged, nothing fires).  Emitted by tests/golden/gen_secp_rare_carry.py",
           "mul": mul_rows(), "sqr": sqr_rows()}
    path = os.path.join(ROOT, "tests", "golden", "secp256k1_rare_carry_operands.json")
    with open(path, "w") as f:
        json.dump(doc, f)
        f.write("\n")
    print("wrote %s: %d mul rows, %d sqr rows" % (path, len(doc["mul"]), len(doc["sqr"])))


if __name__ == "__main__":
    main()
