"""Rate of the parity-mode Ed25519 signer (fec_ed25519_sign_dev, SHA-512 included) against the fixed-base product it is
built on (fec_batch_mul_fixed_dev on the ctx's generator, full-width random scalars), and of fec_sha512_dev alone, with
64-byte messages, inputs resident in HBM.  The calls alternate after a warm-up and are timed with device events on one
stream; the median of REPS rounds is reported.  All run on one default ctx, so all see the same prefix-table state (a
*_dev call builds none).  One JSON line per n: ratio = sign rate / mul_fixed rate (at most 0.5: two products per
signature).

    python tools/eddsa_sign_perf.py            # FEC_SIGN_LOG2=16,18,20  FEC_SIGN_REPS=7  FEC_SIGN_MSG=64
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
    logs = [int(v) for v in os.environ.get("FEC_SIGN_LOG2", "16,18,20").split(",")]
    reps = int(os.environ.get("FEC_SIGN_REPS", "7"))
    mlen = int(os.environ.get("FEC_SIGN_MSG", "64"))
    ctx = F.Context(0)
    s = torch.cuda.Stream()
    for logn in logs:
        n = 1 << logn
        rng = np.random.default_rng(40 + logn)
        keys = dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
        msgs = dev(rng.integers(0, 256, size=n * mlen, dtype=np.uint8))
        off = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(mlen))
        k = dev(rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1))
        sig = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        st = torch.empty(n, dtype=torch.uint8, device="cuda")
        dg = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        out = torch.empty(n * 128, dtype=torch.uint8, device="cuda")
        g = ctx.generator_dev(2)

        def run_sign():
            ctx.ed25519_sign_dev(keys.data_ptr(), msgs.data_ptr(), off.data_ptr(), n * mlen, sig.data_ptr(), st.data_ptr(), n,
                                 s.cuda_stream)

        def run_mul():
            ctx.batch_mul_fixed_dev(2, k.data_ptr(), g, out.data_ptr(), n, s.cuda_stream)

        def run_sha():
            ctx.sha512_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, dg.data_ptr(), None, n, s.cuda_stream)

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
            timed(run_sha)
        ts, tm, th = [], [], []
        for _ in range(reps):
            ts.append(timed(run_sign))
            tm.append(timed(run_mul))
            th.append(timed(run_sha))
        ms_s, ms_m, ms_h = statistics.median(ts), statistics.median(tm), statistics.median(th)
        print(json.dumps({"row": "ed25519_sign", "n": n, "msg_bytes": mlen, "sign_ms": round(ms_s, 3),
                          "mul_fixed_ms": round(ms_m, 3), "sha512_ms": round(ms_h, 4), "sign_per_s": round(n / ms_s * 1e3),
                          "mul_fixed_per_s": round(n / ms_m * 1e3), "ratio": round(ms_m / ms_s, 4),
                          "sign_ms_all": [round(v, 3) for v in ts], "mul_fixed_ms_all": [round(v, 3) for v in tm],
                          "sha512_ms_all": [round(v, 4) for v in th], "status_counts": np.bincount(st.cpu().numpy(), minlength=3).tolist(),
                          "prefix_bits": ctx.fixed_prefix_bits(2)}), flush=True)
        del keys, msgs, off, k, sig, st, dg, out
    ctx.close()


main()
