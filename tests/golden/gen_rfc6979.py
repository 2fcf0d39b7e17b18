"""
Generates tests/golden/rfc6979_vectors.json: Rfc6979::<C, Sha256>::generate_k and Ecdsa::<C, Sha256>::sign from the
message for secp256k1 and P-256.

  python tests/golden/gen_rfc6979.py

"recorded": the three nonces the reference's own test module records (forge-ec-rng/src/rfc6979.rs:191-204) as
{"msg" (hex), "sk" (limbs), "k" (limbs)}.  That test builds its key with the INHERENT little-endian Scalar::from_bytes
of 00..01, so the key is 1 << 248, and prints k with the inherent little-endian to_bytes: the recorded hex strings are
the byte-reversed big-endian values, kept here as "k_hex_recorded".
"cases": per curve, keys {0, 1, N-1, N, 2^256-1, random} x message lengths {0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120,
200}, plus b"test message" (no special case: rfc6979.rs and ecdsa.rs:98-211 do not look for it), as {"curve", "key"
(its class), "sk", "msg" (hex), "k" = generate_k(sk, msg) by tests/rfc6979_ref.py -- for every key, checked or not --,
"status", "r", "s" = rfc6979_ref.sign_msg over oracle/py_model.py (restatement-derived; not reference-executed)}.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import rfc6979_ref as R  # noqa: E402

LENGTHS = (0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 200)
KEY_CLASSES = ("0", "1", "N-1", "N", "2^256-1", "random")
RECORDED = ((bytes(32), "b2db5ea141944ef800a3a2401fbd178f5f806e5e6cd5ee64dad254cccc246702"),
            (b"sample", "03bc06786fe6b69d9269897046326f1ac330ec7c6df97a37cc02ef88c55962d1"),
            (b"test", "690c6e711fc81b139252c4fa8f12e177666e689dc2ac156bbf44bd7e1ee6e018"))


def main():
    rng = random.Random(0x6979)
    out = {"provenance": "k: tests/rfc6979_ref.py (hashlib / hmac); r, s, status: oracle/py_model.py, restatement-derived; "
                         "recorded: forge-ec-rng/src/rfc6979.rs:191-204, reference-recorded", "recorded": [], "cases": []}
    for msg, hexk in RECORDED:
        out["recorded"].append({"msg": msg.hex(), "sk": [0, 0, 0, 1 << 56], "k_hex_recorded": hexk,
                                "k": R.E._limbs(int.from_bytes(bytes.fromhex(hexk), "little"))})
    for curve in (0, 1):
        nv = R.ORDER[curve]
        keys = {"0": 0, "1": 1, "N-1": nv - 1, "N": nv, "2^256-1": (1 << 256) - 1}
        rows = []
        for name in KEY_CLASSES:
            for ln in LENGTHS + (None,):
                sk = keys[name] if name in keys else rng.randrange(1, nv)
                msg = b"test message" if ln is None else bytes(rng.randrange(256) for _ in range(ln))
                rows.append((name, R.E._limbs(sk), msg))
        r, s, st, _ = R.sign_msg(None, curve, [x[1] for x in rows], [x[2] for x in rows])
        for i, (name, sk, msg) in enumerate(rows):
            k, retries = R.generate_k(sk, msg, nv)
            assert retries == 0
            out["cases"].append({"curve": curve, "key": name, "sk": sk, "msg": msg.hex(), "k": R.E._limbs(k), "status": int(st[i]),
                                 "r": [int(v) for v in r[i]], "s": [int(v) for v in s[i]]})
    with open(os.path.join(HERE, "rfc6979_vectors.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
