"""Rates of Schnorr signing from the message and of its challenge, 64-byte messages, everything resident in HBM, device
events on one stream, the calls of a row alternating after a warm-up, the median of REPS rounds and the spread
(max - min) of each side reported.  One JSON line per row, curve and n:

  schnorr_sign_msg   fec_schnorr_sign_msg_dev against the sum of its own parts in the same process: fec_rfc6979_k_dev on
                     n, fec_batch_mul_fixed_dev on the 2n scalars k and sk.  What remains is the finishing pass
                     (finish_ms).  Beside it k_ecdsa_sign_finish from the same run (fec_ecdsa_sign_dev minus
                     fec_batch_mul_fixed_dev on n: two inversions as well) and estimate_ms = that kernel + 3 x the
                     per-message time of fec_sha256_dev on ONE-BLOCK (32-byte) messages: the compressions of the 66 + 64
                     byte challenge input.  within_estimate = finish <= estimate + the spreads of the terms.
  schnorr_challenge  fec_schnorr_challenge_dev beside fec_sha256_dev on messages of 66 + msg bytes: the difference is the
                     two encodings and the reduction.

    python tools/schnorr_sign_perf.py       # FEC_SCHNORR_LOG2=16,18,20  FEC_SCHNORR_REPS=7  FEC_SCHNORR_MSG=64
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
    logs = [int(v) for v in os.environ.get("FEC_SCHNORR_LOG2", "16,18,20").split(",")]
    reps = int(os.environ.get("FEC_SCHNORR_REPS", "7"))
    mlen = int(os.environ.get("FEC_SCHNORR_MSG", "64"))
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
        rng = np.random.default_rng(160 + logn)
        wide = 66 + mlen
        blob = rng.integers(0, 256, size=n * wide, dtype=np.uint8)
        d_msgs = dev(blob)
        d_off = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(mlen))
        d_off32 = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(32))        # one-block messages out of the same bytes
        d_offw = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(wide))       # messages as long as the challenge's input
        digests = empty(n * 32)
        ctx.sha256_dev(d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, digests.data_ptr(), None, n, s)
        scratch32 = empty(n * 32)
        t = race((lambda: ctx.sha256_dev(d_msgs.data_ptr(), d_off32.data_ptr(), n * 32, scratch32.data_ptr(), None, n, s),
                  lambda: ctx.sha256_dev(d_msgs.data_ptr(), d_offw.data_ptr(), n * wide, scratch32.data_ptr(), None, n, s)))
        one_block, sha_wide = stats(t[0]), stats(t[1])
        print(json.dumps({"row": "sha256", "n": n, "one_block_32_bytes": one_block, "bytes_%d" % wide: sha_wide}), flush=True)
        for curve, name in ((0, "secp256k1"), (1, "p256")):
            sk = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)         # below either order constant, not zero
            d_sk = dev(sk)
            g = ctx.generator_dev(curve)
            both = empty(2 * n * 32)                                            # k at [0, n), sk at [n, 2n)
            both[n * 32:] = d_sk
            kst, status, est = empty(n), empty(n), empty(n)
            pts2, pts1 = empty(2 * n * 96), empty(n * 96)
            r_xy, r_inf, sig_s, sig_b = empty(n * 64), empty(n), empty(n * 32), empty(n * 64)
            esig = empty(n * 64)

            def run_k():
                ctx.rfc6979_k_dev(curve, d_sk.data_ptr(), d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, both.data_ptr(), kst.data_ptr(), n, s)

            def run_mul2():
                ctx.batch_mul_fixed_dev(curve, both.data_ptr(), g, pts2.data_ptr(), 2 * n, s)

            def run_mul1():
                ctx.batch_mul_fixed_dev(curve, both.data_ptr(), g, pts1.data_ptr(), n, s)

            def run_fused():
                ctx.schnorr_sign_msg_dev(curve, d_sk.data_ptr(), d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, r_xy.data_ptr(), r_inf.data_ptr(),
                                         sig_s.data_ptr(), sig_b.data_ptr(), status.data_ptr(), n, s)

            def run_ecdsa():
                ctx.ecdsa_sign_dev(curve, d_sk.data_ptr(), digests.data_ptr(), both.data_ptr(), esig.data_ptr(), est.data_ptr(), n, s)

            run_k()
            t = race((run_fused, run_k, run_mul2, run_ecdsa, run_mul1))
            fused, k_, mul2, ecdsa, mul1 = (stats(v) for v in t)
            finish = round(fused["ms"] - k_["ms"] - mul2["ms"], 3)
            ecdsa_finish = round(ecdsa["ms"] - mul1["ms"], 3)
            estimate = round(ecdsa_finish + 3 * one_block["ms"], 3)
            slack = round(fused["spread_ms"] + k_["spread_ms"] + mul2["spread_ms"] + ecdsa["spread_ms"] + mul1["spread_ms"], 3)
            print(json.dumps({"row": "schnorr_sign_msg", "curve": name, "n": n, "msg_bytes": mlen, "from_message": fused, "rfc6979_k": k_,
                              "mul_fixed_2n": mul2, "finish_ms": finish, "ecdsa_sign": ecdsa, "mul_fixed_n": mul1,
                              "ecdsa_sign_finish_ms": ecdsa_finish, "estimate_ms": estimate, "spreads_ms": slack,
                              "within_estimate": finish <= estimate + slack, "signatures_per_s": round(n / fused["ms"] * 1e3),
                              "status_counts": np.bincount(status.cpu().numpy(), minlength=6).tolist(),
                              "prefix_bits": ctx.fixed_prefix_bits(curve)}), flush=True)
        for curve, name in ((0, "secp256k1"), (1, "p256"), (2, "ed25519")):
            k = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
            pts = empty(n * F.POINT_LIMBS[curve] * 8)
            d_k = dev(k)
            ctx.batch_mul_fixed_dev(curve, d_k.data_ptr(), ctx.generator_dev(curve), pts.data_ptr(), n, s)
            xy, inf, e, cst = empty(n * 64), empty(n), empty(n * 32), empty(n)
            ctx.batch_to_affine_dev(curve, pts.data_ptr(), xy.data_ptr(), inf.data_ptr(), n, s)
            t = race((lambda: ctx.schnorr_challenge_dev(curve, xy.data_ptr(), inf.data_ptr(), xy.data_ptr(), None, d_msgs.data_ptr(), d_off.data_ptr(),
                                                        n * mlen, e.data_ptr(), cst.data_ptr(), n, s),
                      lambda: ctx.sha256_dev(d_msgs.data_ptr(), d_offw.data_ptr(), n * wide, scratch32.data_ptr(), None, n, s)))
            ch, sh = stats(t[0]), stats(t[1])
            print(json.dumps({"row": "schnorr_challenge", "curve": name, "n": n, "msg_bytes": mlen, "challenge": ch, "sha256_%d_bytes" % wide: sh,
                              "difference_ms": round(ch["ms"] - sh["ms"], 3), "challenges_per_s": round(n / ch["ms"] * 1e3),
                              "status_nonzero": int(cst.count_nonzero())}), flush=True)
    ctx.check()
    ctx.close()


main()
