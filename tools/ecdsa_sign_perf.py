"""Rate of batched Ecdsa::sign (fec_ecdsa_sign_dev) against the fixed-base product it is built on
(fec_batch_mul_fixed_dev on the ctx's generator), on the same seeded nonces k, inputs resident in HBM.  The two calls
alternate after a warm-up and are timed with device events on one stream; the median of REPS pairs is reported.
Both run on one default ctx, so both see the same prefix-table state (a *_dev call builds none).  One JSON line per
(curve, n), with ratio = sign rate / mul_fixed rate.

    python tools/ecdsa_sign_perf.py            # FEC_SIGN_LOG2=16,17,18,19,20  FEC_SIGN_REPS=7
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
from forge_ec_amd import synth  # noqa: E402

NAMES = {0: "secp256k1", 1: "p256"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def main():
    logs = [int(v) for v in os.environ.get("FEC_SIGN_LOG2", "16,17,18,19,20").split(",")]
    reps = int(os.environ.get("FEC_SIGN_REPS", "7"))
    ctx = F.Context(0)
    s = torch.cuda.Stream()
    for c in (0, 1):
        for logn in logs:
            n = 1 << logn
            k = dev(synth.scalars(n, c, 31))
            sk = dev(synth.scalars(n, c, 32))
            dg = dev(np.random.default_rng(33).integers(0, 256, size=(n, 32), dtype=np.uint8))
            sig = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            st = torch.empty(n, dtype=torch.uint8, device="cuda")
            out = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
            g = ctx.generator_dev(c)

            def run_sign():
                ctx.ecdsa_sign_dev(c, sk.data_ptr(), dg.data_ptr(), k.data_ptr(), sig.data_ptr(), st.data_ptr(), n, s.cuda_stream)

            def run_mul():
                ctx.batch_mul_fixed_dev(c, k.data_ptr(), g, out.data_ptr(), n, s.cuda_stream)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1)

            for _ in range(2):
                timed(run_sign)
                timed(run_mul)
            ts, tm = [], []
            for _ in range(reps):
                ts.append(timed(run_sign))
                tm.append(timed(run_mul))
            ms_s, ms_m = statistics.median(ts), statistics.median(tm)
            ok = int((st == 0).sum().item())
            print(json.dumps({"row": "ecdsa_sign", "curve": NAMES[c], "n": n, "sign_ms": round(ms_s, 3),
                              "mul_fixed_ms": round(ms_m, 3), "sign_per_s": round(n / ms_s * 1e3),
                              "mul_fixed_per_s": round(n / ms_m * 1e3), "ratio": round(ms_m / ms_s, 4),
                              "sign_ms_all": [round(v, 3) for v in ts], "mul_fixed_ms_all": [round(v, 3) for v in tm],
                              "status_ok": ok, "prefix_bits": ctx.fixed_prefix_bits(c)}),
                  flush=True)
            del k, sk, dg, sig, st, out
    ctx.close()


main()
