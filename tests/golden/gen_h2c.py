"""
Generates tests/golden/h2c_vectors.json: HashToCurve fixtures from the restatement tests/h2c_ref.py over hashlib and
oracle/py_model.py (restatement-derived; not reference-executed; the two "k1" entries are RFC 9380 K.1 values).

  python tests/golden/gen_h2c.py

{"k1": [msg hex, out hex] under K1_DST, 32 bytes -- RFC 9380 K.1,
 "pool": 160 seeded bytes; an expander case uses its first msg_len bytes,
 "xmd": [msg_len, dst_len, out_len, out hex] over XMD_MSG_LENS x XMD_DST_LENS x XMD_OUT_LENS (dst = h2c_ref.dst_of(dst_len)),
   plus one case at out_len 8160, the longest the u8 block counter allows,
 "field": [curve, dst_len, count, msgs hex list, u] -- hash_to_field,
 "curve": per curve and dst_len: msgs (h2c_ref.messages), then hash / encode (projective limbs, cand, legs) and the trait
   method (xy, inf); the trait method also under an empty dst,
 "map": [curve, note, u, xy, cand, legs] -- map_to_curve on planted limbs: zero, one, limbs not below p, small and seeded
   values that give both outcomes of the sign comparison on each curve}.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import h2c_ref as R  # noqa: E402

XMD_MSG_LENS = (0, 1, 31, 64, 119)
XMD_DST_LENS = (0, 1, 21, 22, 255)
XMD_OUT_LENS = (0, 1, 32, 33, 96)
CURVE_DST_LENS = (1, 21, 22, 255)
N_MSGS = 10


def flat(*fes):
    return [int(v) for f in fes for v in f]


def limbs_of(v):
    return [(v >> (64 * i)) & R.M.M64 for i in range(4)]


def planted(curve, rng):
    p_limbs = ([0xFFFFFFFEFFFFFC2F, R.M.M64, R.M.M64, R.M.M64] if curve == R.SECP else list(R.M.P256c.P))
    cases = [("zero", [0, 0, 0, 0]), ("one", [1, 0, 0, 0]), ("two", [2, 0, 0, 0]), ("three", [3, 0, 0, 0]), ("p", p_limbs),
             ("p plus one", limbs_of(sum(l << (64 * i) for i, l in enumerate(p_limbs)) + 1)), ("all ones", [R.M.M64] * 4)]
    cases += [("seeded %d" % k, [rng.getrandbits(64) for _ in range(4)]) for k in range(4)]
    return cases


def main():
    rng = random.Random(0x483243)
    pool = bytes(rng.getrandbits(8) for _ in range(160))
    out = {"provenance": "restatement-derived by tests/h2c_ref.py over hashlib and oracle/py_model.py; not reference-executed; "
                         "k1 holds RFC 9380 K.1 values",
           "k1": [], "pool": pool.hex(), "xmd": [], "field": [], "curve": [], "map": []}
    for msg, want in R.K1:
        got = R.expand_message_xmd(msg, R.K1_DST, 32).hex()
        assert got == want
        out["k1"].append([msg.hex(), got])
    grid = [(m, d, o) for m in XMD_MSG_LENS for d in XMD_DST_LENS for o in XMD_OUT_LENS] + [(33, 22, R.MAX_OUT)]
    for m, d, o in grid:
        out["xmd"].append([m, d, o, R.expand_message_xmd(pool[:m], R.dst_of(d), o).hex()])
    for curve in (R.SECP, R.P256):
        for d, count in ((1, 1), (21, 2), (22, 3), (255, 5)):
            msgs = R.messages(6, 100 + d, d)
            u = [flat(*R.hash_to_field(curve, m, R.dst_of(d), count)[0]) for m in msgs]
            out["field"].append([curve, d, count, [m.hex() for m in msgs], u])
        for d in (0,) + CURVE_DST_LENS:
            msgs = R.messages(N_MSGS, 200 + d, d)
            dst = R.dst_of(d)
            case = {"curve": curve, "dst_len": d, "msgs": [m.hex() for m in msgs], "trait": []}
            for m in msgs:
                x, y, inf = R.curve_hash_to_curve(curve, m, dst)
                case["trait"].append([flat(x, y), int(inf)])
            if d:
                for name, encode in (("hash", False), ("encode", True)):
                    rows = []
                    for m in msgs:
                        p, cand, legs = R.hash_to_curve(curve, m, dst, encode)
                        rows.append([R.flat_proj(p), [flat(*c) for c in cand], legs])
                    case[name] = rows
            out["curve"].append(case)
        for note, u in planted(curve, rng):
            pt, cand, legs = R.map_to_curve(curve, u)
            out["map"].append([curve, note, [int(v) for v in u], flat(*pt), flat(*cand), legs])
    path = os.path.join(HERE, "h2c_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(len(out["xmd"]), "xmd,", len(out["field"]), "field,", len(out["curve"]), "curve,", len(out["map"]), "map cases,",
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
