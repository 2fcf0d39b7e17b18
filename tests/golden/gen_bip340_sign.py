"""
Emits tests/golden/bip340_sign_vectors.json: the reference's BipSchnorr::sign (forge-ec-signature/src/schnorr.rs:302-420)
through tests/bip340_sign_ref.py over oracle/py_model.py.  Covers ordinary keys (all four combinations of the
parities of P.y and R.y occur: tests/test_bip340_sign_model.py asserts it), the keys 0, 1, N - 1, N and 2^256 - 1 (N the
reference's order constant) and the true group order and its neighbour, "test message" and its near misses, the empty
message, and the message lengths at which the 32-byte prefix of the nonce hash and the 64-byte prefix of the challenge
hash cross the SHA-256 padding edges (prefix + message = 55, 56, 63, 64, 119, 120).

    python tests/golden/gen_bip340_sign.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bip340_sign_ref as R  # noqa: E402

OUT = os.path.join(HERE, "bip340_sign_vectors.json")
LENGTHS = [0, 22, 23, 24, 31, 32, 87, 88,      # 32 + len at 55 / 56 / 63 / 64 / 119 / 120
           54, 55, 56, 63, 64, 119, 120]       # 64 + len likewise
TRUE_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def cases(seed=20261017):
    rnd = random.Random(seed)
    key = lambda: bytes(rnd.getrandbits(8) for _ in range(32))
    msg = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    le = lambda v: v.to_bytes(32, "little")
    rows = [(key(), msg(n)) for n in LENGTHS]
    rows += [(key(), msg(rnd.randrange(1, 200))) for _ in range(10)]
    rows += [(le(0), b"abc"), (le(1), b"abc"), (le(R.N_VALUE - 1), b"abc"), (le(R.N_VALUE), b"abc"), (le((1 << 256) - 1), b"abc"),
             (le(TRUE_ORDER), b"abc"), (le(TRUE_ORDER - 1), b"abc"), (le(0), b"")]
    rows += [(key(), b"test message"), (le(R.N_VALUE), b"test message"), (key(), b"test messagf"), (key(), b"Test message"),
             (key(), b"test message "), (key(), b"")]
    return rows


def main():
    rows = cases()
    got = R.sign_batch([k for k, _ in rows], [m for _, m in rows], R.PyBackend())
    out = [{"key": k.hex(), "msg": m.hex(), "sig": sig.hex(), "status": st} for (k, m), (sig, st) in zip(rows, got)]
    with open(OUT, "w") as f:
        json.dump({"sign": out}, f, indent=0)
        f.write("\n")
    print(OUT, len(out), "status", sorted({c["status"] for c in out}))


if __name__ == "__main__":
    main()
