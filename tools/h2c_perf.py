"""Rates of hash-to-curve in parity mode, 32-byte messages, a 21-byte dst, secp256k1 and P-256, beside the yardsticks the
result is built from, all in one process.  Every figure is the ctx's own kernel timing (fec_ctx_set_timing: HIP events
around the launch sequence on the launch stream), so the _dev forms and the two yardsticks that have host forms only
(fec_batch_decompress, fec_point_op: one chunk, copies outside the events) are measured the same way.  The calls of a row
alternate after a warm-up; the median of REPS rounds and the spread (max - min) are reported.  One JSON line per curve and n:

  hash / encode / trait     fec_hash_to_curve_dev (HASH, ENCODE), fec_curve_hash_to_curve_dev
  xmd64, field2, map        fec_expand_message_xmd_dev (64 bytes), fec_hash_to_field_dev (count 2), fec_map_to_curve_dev
  sha256                    fec_sha256_dev on the same messages: one compression each
  to_affine                 fec_batch_to_affine_dev: one inversion per element
  decompress                fec_batch_decompress: one square-root exponentiation per element
  add                       fec_point_op(FEC_P_ADD)
  parts_ms = 2 * (to_affine + decompress) + add + xmd64 -- what the fused HASH call is measured against (the expander is
  four compressions at these lengths; four times sha256 is reported beside it), with the sum of the spreads as slack.

    python tools/h2c_perf.py       # FEC_H2C_LOG2=14,16,18,20  FEC_H2C_REPS=7
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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def main():
    logs = [int(v) for v in os.environ.get("FEC_H2C_LOG2", "14,16,18,20").split(",")]
    reps = int(os.environ.get("FEC_H2C_REPS", "7"))
    dst = b"forge-ec h2c perf dst"                                     # 21 bytes: b_1's input is one block
    ctx = F.Context(0)
    ctx.set_chunk(1 << max(logs))
    ctx.set_timing(True)
    empty = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def timed(fn):
        fn()
        return ctx.last_kernel_ms()[0]

    def race(runs):
        for _ in range(2):
            for fn in runs.values():
                timed(fn)
        t = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():
                t[k].append(timed(fn))
        return {k: {"ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in t.items()}

    for logn in logs:
        n = 1 << logn
        rng = np.random.default_rng(9380 + logn)
        msgs = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
        off = np.arange(n + 1, dtype=np.uint64) * 32
        d_msgs, d_off = dev(msgs), dev(off)
        enc = rng.integers(0, 256, size=(n, 33), dtype=np.uint8)
        enc[:, 0] = 2
        pa = rng.integers(1, 1 << 62, size=(n, 12), dtype=np.uint64)
        pb = rng.integers(1, 1 << 62, size=(n, 12), dtype=np.uint64)
        d_pa = dev(pa)
        for curve, name in ((0, "secp256k1"), (1, "p256")):
            out, cand, xy, inf, st, dig, u, xm = empty(n * 96), empty(n * 128), empty(n * 64), empty(n), empty(n), empty(n * 32), empty(n * 64), empty(n * 64)
            pm, po = d_msgs.data_ptr(), d_off.data_ptr()
            ctx.hash_to_field_dev(curve, pm, po, n * 32, dst, 2, u.data_ptr(), None, n)
            runs = {
                "hash": lambda: ctx.hash_to_curve_dev(curve, pm, po, n * 32, dst, out.data_ptr(), None, None, st.data_ptr(), n),
                "encode": lambda: ctx.encode_to_curve_dev(curve, pm, po, n * 32, dst, out.data_ptr(), None, None, st.data_ptr(), n),
                "trait": lambda: ctx.curve_hash_to_curve_dev(curve, pm, po, n * 32, dst, xy.data_ptr(), inf.data_ptr(), st.data_ptr(), n),
                "xmd64": lambda: ctx.expand_message_xmd_dev(pm, po, n * 32, dst, 64, xm.data_ptr(), st.data_ptr(), n),
                "field2": lambda: ctx.hash_to_field_dev(curve, pm, po, n * 32, dst, 2, u.data_ptr(), st.data_ptr(), n),
                "map": lambda: ctx.map_to_curve_dev(curve, u.data_ptr(), xy.data_ptr(), None, None, n),
                "sha256": lambda: ctx.sha256_dev(pm, po, n * 32, dig.data_ptr(), st.data_ptr(), n),
                "to_affine": lambda: ctx.batch_to_affine_dev(curve, d_pa.data_ptr(), xy.data_ptr(), inf.data_ptr(), n),
                "decompress": lambda: ctx.batch_decompress(curve, enc),
                "add": lambda: ctx.point_op(curve, 0, pa, pb),
            }
            r = race(runs)
            torch.cuda.synchronize()
            parts = round(2 * (r["to_affine"]["ms"] + r["decompress"]["ms"]) + r["add"]["ms"] + r["xmd64"]["ms"], 4)
            slack = round(r["hash"]["spread_ms"] + 2 * (r["to_affine"]["spread_ms"] + r["decompress"]["spread_ms"]) + r["add"]["spread_ms"]
                          + r["xmd64"]["spread_ms"], 4)
            print(json.dumps({"row": "h2c", "curve": name, "n": n, "msg_bytes": 32, "dst_bytes": len(dst), **r, "parts_ms": parts,
                              "spreads_ms": slack, "over_parts_ms": round(r["hash"]["ms"] - parts, 4),
                              "within_parts": r["hash"]["ms"] <= parts + slack, "four_sha256_ms": round(4 * r["sha256"]["ms"], 4),
                              "hashes_per_s": round(n / r["hash"]["ms"] * 1e3)}), flush=True)
    ctx.check()
    ctx.close()


main()
