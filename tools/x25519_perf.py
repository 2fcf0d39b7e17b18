"""Rate of the reference's x25519 (fec_x25519_dev) and Curve25519::multiply (fec_curve25519_mul_dev) on one GPU, inputs
resident in HBM, timed with device events on one stream after two warm-up calls; the median of REPS calls is reported.
The roofline fraction uses BASELINE.md's convention: MAD32 per element over the peak MAD32/s the ctx measures
(fec_measure_peak_mad32).  x25519's MAD32 count is derived in DESIGN.md section 11: 2 820 field Mul (255 ladder steps of
10, 269 in invert, 1 final) of 72 MAD32 each (64 for the 256 x 256 product, 8 for the fold by 19).  One JSON line per
(call, n) on stdout; with --out PREFIX also PREFIX.jsonl.

    python tools/x25519_perf.py [--out profiles/x25519_r06]      # FEC_X25519_LOG2=14,17,20  FEC_X25519_REPS=5
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

MULS_X25519 = 255 * 10 + 269 + 1
MAD32_PER_MUL = 72
MAD32_X25519 = MULS_X25519 * MAD32_PER_MUL
MAD32_MULTIPLY = MAD32_X25519 + (269 + 1) * MAD32_PER_MUL  # to_affine adds one invert and one Mul


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def main():
    logs = [int(v) for v in os.environ.get("FEC_X25519_LOG2", "14,17,20").split(",")]
    reps = int(os.environ.get("FEC_X25519_REPS", "5"))
    out_prefix = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    ctx = F.Context(0)
    peak = ctx.measure_peak_mad32()
    s = torch.cuda.Stream()
    lines = []
    for logn in logs:
        n = 1 << logn
        rng = np.random.default_rng(logn)
        sc = dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
        u = dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
        k = dev(rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 3)
        pts = dev(rng.integers(0, 1 << 63, size=(n, 8), dtype=np.uint64) * 3)
        out = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        calls = {"x25519": (lambda: ctx.x25519_dev(sc.data_ptr(), u.data_ptr(), out.data_ptr(), n, s.cuda_stream),
                            MAD32_X25519),
                 "curve25519_mul": (lambda: ctx.curve25519_mul_dev(k.data_ptr(), pts.data_ptr(), out.data_ptr(), n,
                                                                   s.cuda_stream), MAD32_MULTIPLY)}
        for name, (fn, mad32) in calls.items():
            def timed():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1)
            for _ in range(2):
                timed()
            ts = [timed() for _ in range(reps)]
            ms = statistics.median(ts)
            rate = n / ms * 1e3
            rec = {"row": name, "n": n, "kernel_ms": round(ms, 3), "per_s": round(rate), "ms_all": [round(v, 3) for v in ts],
                   "mad32_per_element": mad32, "peak_mad32_per_s": peak, "roofline": round(rate * mad32 / peak, 4)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del sc, u, k, pts, out
    ctx.close()
    if out_prefix:
        with open(out_prefix + ".jsonl", "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


main()
