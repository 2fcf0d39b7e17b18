"""Rates of ECDSA signing from the message, 64-byte messages, everything resident in HBM, device events on one stream, the
calls of a row alternating after a warm-up, the median of REPS rounds and the spread (max - min) of each side reported.
One JSON line per row, curve and n:

  ecdsa_sign_msg  fec_ecdsa_sign_msg_dev against fec_ecdsa_sign_dev on the same keys with the digests and the nonces
                  computed beforehand (fec_sha256_dev, fec_rfc6979_k_dev) in the same process.  The difference is the
                  nonce pass.  estimate_ms = 18 x the per-message time of fec_sha256_dev on ONE-BLOCK (32-byte) messages
                  measured in the same run: the compressions the pass executes, two of them the 64-byte message's own
                  hash.  within_estimate = nonce pass <= estimate + the composition's spread.
  rfc6979_k       fec_rfc6979_k_dev alone: nonces per second.

    python tools/ecdsa_sign_msg_perf.py       # FEC_SIGNMSG_LOG2=16,18,20  FEC_SIGNMSG_REPS=7  FEC_SIGNMSG_MSG=64
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
    logs = [int(v) for v in os.environ.get("FEC_SIGNMSG_LOG2", "16,18,20").split(",")]
    reps = int(os.environ.get("FEC_SIGNMSG_REPS", "7"))
    mlen = int(os.environ.get("FEC_SIGNMSG_MSG", "64"))
    ctx = F.Context(0)
    for curve in (0, 1):
        ctx.build_fixed_prefix(curve)                                   # a *_dev call only takes a table that exists
    st_ = torch.cuda.Stream()

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

    for logn in logs:
        n = 1 << logn
        rng = np.random.default_rng(90 + logn)
        blob = rng.integers(0, 256, size=n * mlen, dtype=np.uint8)
        d_msgs, d_off = dev(blob), dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(mlen))
        d_off32 = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(32))      # one-block messages out of the same bytes
        digests = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        scratch32 = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        ctx.sha256_dev(d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, digests.data_ptr(), None, n, st_.cuda_stream)
        t = race((lambda: ctx.sha256_dev(d_msgs.data_ptr(), d_off32.data_ptr(), n * 32, scratch32.data_ptr(), None, n, st_.cuda_stream),))
        one_block = stats(t[0])
        print(json.dumps({"row": "sha256_one_block", "n": n, "msg_bytes": 32, "sha256": one_block}), flush=True)
        for curve, name in ((0, "secp256k1"), (1, "p256")):
            sk = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)         # below either order constant, not zero
            d_sk = dev(sk)
            nonces = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            kst = torch.empty(n, dtype=torch.uint8, device="cuda")
            sig = [torch.empty(n * 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
            status = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2)]

            def run_k():
                ctx.rfc6979_k_dev(curve, d_sk.data_ptr(), d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, nonces.data_ptr(), kst.data_ptr(), n,
                                  st_.cuda_stream)

            def run_fused():
                ctx.ecdsa_sign_msg_dev(curve, d_sk.data_ptr(), d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, sig[0].data_ptr(),
                                       status[0].data_ptr(), n, st_.cuda_stream)

            def run_parts():
                ctx.ecdsa_sign_dev(curve, d_sk.data_ptr(), digests.data_ptr(), nonces.data_ptr(), sig[1].data_ptr(), status[1].data_ptr(), n,
                                   st_.cuda_stream)

            k_alone = stats(race((run_k,))[0])
            print(json.dumps({"row": "rfc6979_k", "curve": name, "n": n, "msg_bytes": mlen, "rfc6979_k": k_alone,
                              "nonces_per_s": round(n / k_alone["ms"] * 1e3), "status_nonzero": int(kst.count_nonzero())}), flush=True)
            t = race((run_fused, run_parts))
            fused, parts = stats(t[0]), stats(t[1])
            nonce_pass = round(fused["ms"] - parts["ms"], 3)
            estimate = round(18 * one_block["ms"], 3)
            print(json.dumps({"row": "ecdsa_sign_msg", "curve": name, "n": n, "msg_bytes": mlen, "from_message": fused, "from_digest_and_nonce": parts,
                              "nonce_pass_ms": nonce_pass, "estimate_ms": estimate,
                              "within_estimate": nonce_pass <= estimate + parts["spread_ms"],
                              "signatures_per_s": round(n / fused["ms"] * 1e3),
                              "equal": bool(torch.equal(sig[0], sig[1]) and torch.equal(status[0], status[1])),
                              "status_counts": np.bincount(status[0].cpu().numpy(), minlength=6).tolist(),
                              "prefix_bits": ctx.fixed_prefix_bits(curve)}), flush=True)
    ctx.check()
    ctx.close()


main()
