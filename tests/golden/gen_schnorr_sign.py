"""
Generates tests/golden/schnorr_sign_vectors.json: Schnorr::<C, Sha256>::sign from the message for secp256k1 and P-256,
its challenge and C::Scalar::from_bytes_reduced for the three curves.  Restatement-derived: tests/schnorr_sign_ref.py over
oracle/py_model.py (not reference-executed); tests/test_schnorr_sign_model.py checks every entry against the C oracle too.

  python tests/golden/gen_schnorr_sign.py

"sign": per curve, keys {0, 1, N-1, N, 2^256-1, random} x message lengths {0, 1, 2, 53, 54, 61, 62, 63, 117, 118, 126, 200}
-- around the block edges of the 66-byte prefix: the padding moves to a further block at 54 and 118, 62 and 126 end exactly
on a block -- plus b"test message", as {"curve", "key" (its class), "sk", "msg" (hex), "status", "r_xy", "r_inf", "s",
"sig_bytes" (hex), "k", "e", "leg"} (k, e, leg null for the message case).
"reduced": per curve, at least 8 crafted 32-byte strings per reachable leg of from_bytes_reduced and 16 random ones, as
{"curve", "bytes" (hex), "out", "leg"}.
"challenge": per curve, finite and infinite R and P in all four combinations x message lengths {0, 1, 54, 62, 118, 200},
as {"curve", "r", "r_inf", "pk", "pk_inf", "msg" (hex), "e", "leg"} with r and pk indices into "points"[curve], the two
affine points (8 limbs each) every entry of that curve uses (schnorr_sign_ref.load_fixture puts "r_xy" / "pk_xy" back).
The file is written compactly, one entry per line.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import schnorr_sign_ref as S  # noqa: E402

LENGTHS = (0, 1, 2, 53, 54, 61, 62, 63, 117, 118, 126, 200)
CHALLENGE_LENGTHS = (0, 1, 54, 62, 118, 200)
KEY_CLASSES = ("0", "1", "N-1", "N", "2^256-1", "random")
FF = b"\xff"


def crafted(curve, rng):
    """[(32 bytes, the leg they are built for)]: 8 per reachable leg."""
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    nbe = S.trait_to_bytes(S.N[curve])
    out = []
    if curve == 0:
        out += [(bytes(32), "direct"), (bytes(31) + b"\x01", "direct"), ((S.val(S.N[0]) - 1).to_bytes(32, "big"), "direct")]
        out += [(bytes([rng.randrange(255)]) + rb(31), "direct") for _ in range(5)]
        # not below N big-endian (b[0..8] = FF); little-endian top limb below N[3] and its byte swap too
        out += [(FF * 8 + rb(16) + bytes([rng.randrange(255)]) + rb(6) + bytes([rng.randrange(255)]), "nosub") for _ in range(8)]
        # ... byte swap of the little-endian top limb = N[3], limb 2 = N[2], limb 1 above N[1]: None -> zero
        out += [(FF * 8 + bytes([0xBB + rng.randrange(0x45)]) + rb(7) + FF * 15 + b"\xfe", "nosub_zero") for _ in range(7)]
        out += [(FF * 31 + b"\xfe", "nosub_zero")]
        # little-endian top limb all ones: one subtraction
        out += [(FF * 7 + bytes([0xFE + (i & 1)]) + (FF * 8 + bytes([0xBB + rng.randrange(0x45)]) + rb(7) if not i & 1 else rb(16)) + FF * 8, "sub")
                for i in range(7)]
        out += [(FF * 32, "sub"), (nbe, None)]
    elif curve == 1:
        out += [(bytes(32), "direct"), (bytes(31) + b"\x01", "direct"), ((S.val(S.N[1]) - 1).to_bytes(32, "big"), "direct")]
        out += [(bytes([rng.randrange(255)]) + rb(31), "direct") for _ in range(5)]
        out += [(FF * 4 + bytes([1 + rng.randrange(255)]) + rb(27), "reduce_wide") for _ in range(6)]
        out += [(FF * 32, "reduce_wide"), (nbe, "reduce_wide")]
    else:
        out += [(bytes(32), "direct"), (FF * 32, "direct"), (nbe, "direct"), ((S.val(S.N[2]) - 1).to_bytes(32, "big"), "direct"),
                (S.val(S.N[2]).to_bytes(32, "little"), "direct")]
        out += [(FF * 8 + rb(24), "direct") for _ in range(3)]
    return out


def dumps(out):
    """Compact JSON, one entry of each list per line."""
    row = lambda v: json.dumps(v, separators=(",", ":"))
    parts = []
    for key, v in out.items():
        body = "[\n" + ",\n".join(row(x) for x in v) + "\n]" if isinstance(v, list) else row(v)
        parts.append(row(key) + ":" + body)
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main():
    rng = random.Random(0x5C4E)
    be = S.PyBackend()
    out = {"provenance": "tests/schnorr_sign_ref.py over oracle/py_model.py (hashlib, tests/rfc6979_ref.py): restatement-derived, "
                         "not reference-executed", "sign": [], "reduced": [], "points": {}, "challenge": []}
    for curve in (0, 1):
        nv = S.val(S.N[curve])
        keys = {"0": 0, "1": 1, "N-1": nv - 1, "N": nv, "2^256-1": (1 << 256) - 1}
        for name in KEY_CLASSES:
            for ln in LENGTHS + (None,):
                sk = S.limbs(keys[name] if name in keys else rng.randrange(1, nv))
                msg = b"test message" if ln is None else bytes(rng.randrange(256) for _ in range(ln))
                r = S.sign(be, curve, sk, msg)
                out["sign"].append({"curve": curve, "key": name, "sk": sk, "msg": msg.hex(), "status": r["status"], "r_xy": r["r_xy"],
                                    "r_inf": int(r["r_inf"]), "s": r["s"], "sig_bytes": r["sig_bytes"].hex(), "k": r["k"], "e": r["e"],
                                    "leg": r["leg"]})
    for curve in (0, 1, 2):
        rows = crafted(curve, rng) + [(bytes(rng.randrange(256) for _ in range(32)), None) for _ in range(16)]
        for b, want in rows:
            v, leg = S.from_bytes_reduced(curve, b)
            assert want is None or leg == want, (curve, b.hex(), leg, want)
            out["reduced"].append({"curve": curve, "bytes": b.hex(), "out": v, "leg": leg})
        legs = [r["leg"] for r in out["reduced"] if r["curve"] == curve]
        assert all(legs.count(l) >= 8 for l in S.REACHABLE[curve]) and set(legs) == set(S.REACHABLE[curve]), legs
        pts = [be.mul_g_affine(curve, S.limbs(rng.randrange(1, 1 << 64))) for _ in range(2)]
        out["points"][str(curve)] = [p[0] for p in pts]
        for i, ln in enumerate(CHALLENGE_LENGTHS):
            for f in range(4):
                r_inf, pk_inf = bool(f & 1), bool(f >> 1)
                msg = bytes(rng.randrange(256) for _ in range(ln))
                r_xy, pk_xy = pts[i & 1][0], pts[1 - (i & 1)][0]   # an infinite point keeps its limbs: only the flag counts
                e, leg = S.challenge(be, curve, r_xy, r_inf, pk_xy, pk_inf, msg)
                out["challenge"].append({"curve": curve, "r": i & 1, "r_inf": int(r_inf), "pk": 1 - (i & 1), "pk_inf": int(pk_inf),
                                         "msg": msg.hex(), "e": e, "leg": leg})
    with open(os.path.join(HERE, "schnorr_sign_vectors.json"), "w") as f:
        f.write(dumps(out))


if __name__ == "__main__":
    main()
