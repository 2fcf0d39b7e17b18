"""Rates of ECDH with the key derivation behind it, 32-byte keys, info of 0 and 32 bytes, everything resident in HBM,
device events on one stream, the calls of a row alternating after a warm-up, the median of REPS rounds and the spread
(max - min) of each side reported.  One JSON line per row, curve, n and info length:

  ecdh_derive_key  fec_ecdh_derive_key_dev against its own parts in the same process: fec_batch_ecdh_dev on the same keys
                   and fec_derive_key_dev on the secrets it wrote.  kdf_in_fused_ms = fused - batch_ecdh is what the key
                   derivation costs inside the finishing kernel; the yardstick is derive_key alone, with the sum of the
                   three spreads as slack (within_parts).
  ecdh_exchange    fec_ecdh_exchange_dev against fec_batch_mul_fixed_dev(n) + fec_batch_ecdh_dev(n) + fec_derive_key_dev(n),
                   the same way.  Those parts leave the public key in Jacobian form; fec_batch_to_affine_dev on it, the
                   inversion the exchange also runs, is timed beside them and reported as a column of its own.

    python tools/ecdh_kdf_perf.py       # FEC_KDF_LOG2=16,18,20  FEC_KDF_REPS=7  FEC_KDF_OUT=32
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import forge_ec_amd as F  # noqa: E402

P256_P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
P256_B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def peers(curve, n, rng):
    """n public keys.  secp256k1 validates nothing: arbitrary coordinates.  P-256: 4096 true curve points, repeated --
    the reference's validation accepts about half of them (the statuses are reported with every row); the private keys
    differ per element, so the products do too."""
    if curve == 0:
        return rng.integers(0, 1 << 64, size=(n, 8), dtype=np.uint64)
    import random
    r = random.Random(int(rng.integers(1 << 30)))
    limbs = lambda v: [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
    pts = []
    while len(pts) < min(n, 4096):
        x = r.randrange(P256_P)
        rhs = (x * x * x - 3 * x + P256_B) % P256_P
        y = pow(rhs, (P256_P + 1) // 4, P256_P)
        if y * y % P256_P == rhs:
            pts.append(limbs(x) + limbs(y))
    return np.resize(np.array(pts, dtype=np.uint64), (n, 8))


def main():
    logs = [int(v) for v in os.environ.get("FEC_KDF_LOG2", "16,18,20").split(",")]
    reps = int(os.environ.get("FEC_KDF_REPS", "7"))
    out_len = int(os.environ.get("FEC_KDF_OUT", "32"))
    ctx = F.Context(0)
    for curve in (0, 1):
        ctx.build_fixed_prefix(curve)                                   # a *_dev call only takes a table that exists
    st_ = torch.cuda.Stream()
    s = st_.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st_)
        fn()
        e1.record(st_)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def race(runs):
        for _ in range(2):
            for fn in runs:
                timed(fn)
        t = [[] for _ in runs]
        for _ in range(reps):
            for j, fn in enumerate(runs):
                t[j].append(timed(fn))
        return t

    def stats(v):
        return {"ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "all_ms": [round(x, 3) for x in v]}

    empty = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for logn in logs:
        n = 1 << logn
        rng = np.random.default_rng(170 + logn)
        for curve, name in ((0, "secp256k1"), (1, "p256")):
            d_sk = dev(rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64))
            d_pk = dev(peers(curve, n, rng))
            g = ctx.generator_dev(curve)
            secrets, keys, keys2, keys3 = empty(n * 32), empty(n * out_len), empty(n * out_len), empty(n * out_len)
            st0, st1, st2 = empty(n), empty(n), empty(n)
            pts, pub, pinf, aff, ainf = empty(n * 96), empty(n * 64), empty(n), empty(n * 64), empty(n)
            for info_len in (0, 32):
                info = bytes(range(info_len)) or None

                def run_fused():
                    ctx.ecdh_derive_key_dev(curve, d_sk.data_ptr(), d_pk.data_ptr(), None, info, out_len, keys.data_ptr(), st0.data_ptr(), n, s)

                def run_ecdh():
                    ctx.batch_ecdh_dev(curve, d_sk.data_ptr(), d_pk.data_ptr(), None, secrets.data_ptr(), st1.data_ptr(), n, s)

                def run_kdf():
                    ctx.derive_key_dev(curve, secrets.data_ptr(), 32, info, out_len, keys2.data_ptr(), n, s)

                def run_mul():
                    ctx.batch_mul_fixed_dev(curve, d_sk.data_ptr(), g, pts.data_ptr(), n, s)

                def run_exchange():
                    ctx.ecdh_exchange_dev(curve, d_sk.data_ptr(), d_pk.data_ptr(), None, info, out_len, pub.data_ptr(), pinf.data_ptr(),
                                          keys3.data_ptr(), st2.data_ptr(), n, s)

                def run_affine():
                    ctx.batch_to_affine_dev(curve, pts.data_ptr(), aff.data_ptr(), ainf.data_ptr(), n, s)

                run_ecdh()
                run_mul()
                t = race((run_fused, run_ecdh, run_kdf, run_exchange, run_mul, run_affine))
                fused, ecdh, kdf, exch, mul, affine = (stats(v) for v in t)
                torch.cuda.synchronize()
                ok = st1.cpu().numpy() == 0
                same = bool((keys.cpu().numpy().reshape(n, out_len)[ok] == keys2.cpu().numpy().reshape(n, out_len)[ok]).all())
                slack = round(fused["spread_ms"] + ecdh["spread_ms"] + kdf["spread_ms"], 3)
                inside = round(fused["ms"] - ecdh["ms"], 3)
                print(json.dumps({"row": "ecdh_derive_key", "curve": name, "n": n, "info_bytes": info_len, "key_bytes": out_len, "fused": fused,
                                  "batch_ecdh": ecdh, "derive_key": kdf, "kdf_in_fused_ms": inside, "spreads_ms": slack,
                                  "within_parts": inside <= kdf["ms"] + slack, "over_parts_ms": round(inside - kdf["ms"], 3),
                                  "keys_per_s": round(n / fused["ms"] * 1e3), "fused_equals_parts": same,
                                  "status_counts": np.bincount(st0.cpu().numpy(), minlength=3).tolist()}), flush=True)
                parts = round(mul["ms"] + ecdh["ms"] + kdf["ms"], 3)
                slack = round(exch["spread_ms"] + mul["spread_ms"] + ecdh["spread_ms"] + kdf["spread_ms"], 3)
                print(json.dumps({"row": "ecdh_exchange", "curve": name, "n": n, "info_bytes": info_len, "key_bytes": out_len, "exchange": exch,
                                  "mul_fixed": mul, "batch_ecdh": ecdh, "derive_key": kdf, "parts_ms": parts, "spreads_ms": slack,
                                  "within_parts": exch["ms"] <= parts + slack, "over_parts_ms": round(exch["ms"] - parts, 3),
                                  "to_affine": affine, "over_parts_and_to_affine_ms": round(exch["ms"] - parts - affine["ms"], 3),
                                  "exchanges_per_s": round(n / exch["ms"] * 1e3),
                                  "status_counts": np.bincount(st2.cpu().numpy(), minlength=3).tolist(),
                                  "prefix_bits": ctx.fixed_prefix_bits(curve)}), flush=True)
    ctx.check()
    ctx.close()


main()
