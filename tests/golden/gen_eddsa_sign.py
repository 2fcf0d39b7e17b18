"""
Emits tests/golden/eddsa_sign_vectors.json: the reference's Ed25519Signature::sign, derive_public_key and
EdDsa::<Ed25519, Sha512>::sign (forge-ec-signature/src/eddsa.rs) through tests/eddsa_sign_ref.py over
oracle/py_model.py.  Covers both special cases of each function and their near misses, the SHA-512 padding
boundaries of all three hashes (message lengths 0, 1, 111, 112, 127, 128, 239, 240, 1000, and where the 32-byte
nonce prefix and the 66-byte R33 || A33 prefix cross them), and elements with the debug-build-panic status set and
clear.

    python tests/golden/gen_eddsa_sign.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import eddsa_sign_ref as R  # noqa: E402

OUT = os.path.join(HERE, "eddsa_sign_vectors.json")
LENGTHS = [0, 1, 111, 112, 127, 128, 239, 240, 1000,
           79, 80, 95, 96, 207, 208,          # 32 + len crosses 111/112, 127/128, 239/240
           45, 46, 61, 62, 173, 174]          # 66 + len likewise


def cases(seed=20261016):
    rnd = random.Random(seed)
    key = lambda first=None: bytes([first if first is not None else rnd.getrandbits(8)]) + bytes(rnd.getrandbits(8) for _ in range(31))
    msg = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    sign = [(key(), msg(n)) for n in LENGTHS]
    sign += [(key(), b"test message"), (key(0x9D), b"test message"), (key(), b"test messagf"), (key(), b"Test message"),
             (key(0x9D), b""), (key(0x9C), b""), (key(0x9D), b"\x00"), (key(), b"test message ")]
    sign += [(key(), msg(rnd.randrange(0, 300))) for _ in range(8)]
    derive = [key() for _ in range(6)] + [key(0x9D), key(0x9D), key(0x9C), key(0x9E)]
    sk = lambda top=None: [rnd.getrandbits(64) for _ in range(3)] + [((top << 56) | rnd.getrandbits(56)) if top is not None else rnd.getrandbits(64)]
    generic = [(sk(), msg(n)) for n in (0, 1, 64, 112, 128, 240)]
    generic += [(sk(), b"test message"), (sk(0x9D), b""), (sk(0x9C), b""), (sk(0x9D), b"x"), (sk(), b"test messagf"),
                ([0, 0, 0, 0], b"abc"), ([1, 0, 0, 0], b"")]
    return sign, derive, generic


def main():
    sign, derive, generic = cases()
    be = R.PyBackend()
    out = {"sign": [], "derive": [], "generic": []}
    for (k, m), (sig, st) in zip(sign, R.sign_batch([k for k, _ in sign], [m for _, m in sign], be)):
        out["sign"].append({"key": k.hex(), "msg": m.hex(), "sig": sig.hex(), "status": st})
    for k, (pk, st) in zip(derive, R.derive_batch(derive, be)):
        out["derive"].append({"key": k.hex(), "pk": pk.hex(), "status": st})
    for (k, m), (rx, ry, rinf, s, st) in zip(generic, R.eddsa_sign_batch([k for k, _ in generic], [m for _, m in generic], be)):
        out["generic"].append({"sk": [f"{v:016x}" for v in k], "msg": m.hex(), "r_xy": [f"{int(v):016x}" for v in list(rx) + list(ry)],
                               "r_inf": int(rinf), "s": [f"{int(v):016x}" for v in s], "status": st})
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(OUT, {k: len(v) for k, v in out.items()}, "status", sorted({c["status"] for c in out["sign"]}))


if __name__ == "__main__":
    main()
