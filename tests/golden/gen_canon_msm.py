"""
Writes tests/golden/canon_msm_vectors.json: per curve a pool of 64 points made by oracle/canon_model.py with their logarithms
(P = a G; on Ed25519 P = a B + j T, T of order 8, stored too) and the explicit cases of fec_canon_msm with n <= 200, each with
the model's sum.  Point references are those of tests/canon_msm_ref.py.  Deterministic: python tests/golden/gen_canon_msm.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import canon_msm_ref as R  # noqa: E402
from oracle import canon_model as CM  # noqa: E402


def torsion_generator():
    """a point of order exactly 8: l * Q for decodable y, until 4 (l Q) is not the identity"""
    E = CM.ED25519
    y = 2
    while True:
        y += 1
        try:
            Q = CM.ed25519_decode(y.to_bytes(32, "little"))
        except (AssertionError, ValueError):
            continue
        T = E.mul(E.N, Q)
        if E.mul(4, T) != E.IDENTITY:
            assert E.mul(8, T) == E.IDENTITY and E.on_curve(T)
            return T


def main():
    out = {"_generated_by": "tests/golden/gen_canon_msm.py from oracle/canon_model.py", "curves": {}}
    for name, C in R.MODELS.items():
        rng = random.Random("canon-msm-fixture/" + name)
        ed = R.is_ed(name)
        T = torsion_generator() if ed else None
        pool = []
        for i in range(64):
            a, j = rng.randrange(1, C.N), (i % 8 if ed else 0)
            p = C.mul(a, C.G)
            if ed:
                p = C.add(p, C.mul(j, T))
            assert C.on_curve(p)
            pool.append({"a": "%x" % a, "j": j, "x": "%064x" % p[0], "y": "%064x" % p[1]})
        d = {"pool": pool, "cases": []}
        if ed:
            d["T"] = ["%064x" % T[0], "%064x" % T[1]]
        out["curves"][name] = d

    path = os.path.join(HERE, "canon_msm_vectors.json")
    json.dump(out, open(path, "w"))
    fx = R.load_fixture(path)
    for name, C in R.MODELS.items():
        rng = random.Random("canon-msm-cases/" + name)
        ed = R.is_ed(name)
        big = lambda: rng.getrandbits(256)  # noqa: E731
        cases = [("empty", [], []), ("single", [big()], [3]),
                 ("random-40", [big() for _ in range(40)], [rng.randrange(64) for _ in range(40)]),
                 ("random-200", [big() for _ in range(200)], [rng.randrange(64) for _ in range(200)])]
        k = big()
        cases.append(("equal-scalars-64", [k] * 64, list(range(64))))
        cases.append(("one-point-50", [big() for _ in range(50)], [7] * 50))
        ks = [big() for _ in range(10)]
        cases.append(("k-P-and-k-minus-P", [v for v in ks for _ in (0, 1)], [r for i in range(10) for r in (i, -i - 1)]))
        ks = [rng.randrange(1, C.N) for _ in range(10)]
        cases.append(("k-P-and-N-minus-k-P", [v for q in ks for v in (q, C.N - q)], [i for i in range(10) for _ in (0, 1)]))
        cases.append(("zeros-20", [0] * 20, list(range(20))))
        cases.append(("all-ones-20", [R.TOP] * 20, list(range(20))))
        cases.append(("top-bucket-2^255", [2**255] * 20, list(range(20, 40))))
        cases.append(("steering", R.steering_scalars(name), [i % 64 for i in range(len(R.steering_scalars(name)))]))
        if ed:
            tk = [1, 7, 8, C.N, C.N + 1, R.TOP]
            cases.append(("torsion-inputs", [q for q in tk for _ in range(8)], ["t%d" % j for _ in tk for j in range(8)]))
            cases.append(("identity-among", [big() for _ in range(9)], [0, 1, "id", 2, 3, "id", 4, 5, 6]))
        for cname, ks, refs in cases:
            assert len(ks) == len(refs) <= 200
            want = fx.expected(name, ks, refs)
            assert want == R.msm_direct(name, ks, fx.points(name, refs)), (name, cname)
            xy, st = R.result(name, want)
            out["curves"][name]["cases"].append({"name": cname, "k": ["%x" % v for v in ks], "p": refs,
                                                 "x": "%064x" % CM.unlimbs(xy[:4]), "y": "%064x" % CM.unlimbs(xy[4:]), "status": st})
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
