"""Rate of the two parity-mode Ed25519 verifiers from the message (fec_ed25519_verify_dev, fec_eddsa_verify_ed25519_msg_dev:
decoding and SHA-512 included) against the verifier that starts after the hash (fec_eddsa_verify_ed25519_dev) on the SAME
decoded inputs, 64-byte messages, everything resident in HBM.  The byte form gets all-decoding inputs: under the
reference's sqrt that means x = 0 for R and for the public key (tests/golden/gen_eddsa_verify.py), so every lane goes
through both decompressions, the hash and the point computation; s and the messages are random.  The generic form and
the baseline get R = A = (0, 0) -- what those bytes decode to -- s as the byte form reads it, and for the baseline the k
that the byte form hashes.  The calls alternate after a warm-up and are timed with device events on one stream; the
median of REPS rounds is reported.  One JSON line per n: ratio = baseline time / new time.

    python tools/eddsa_verify_perf.py          # FEC_VERIFY_LOG2=16,18,20  FEC_VERIFY_REPS=7  FEC_VERIFY_MSG=64
"""
import hashlib
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
    logs = [int(v) for v in os.environ.get("FEC_VERIFY_LOG2", "16,18,20").split(",")]
    reps = int(os.environ.get("FEC_VERIFY_REPS", "7"))
    mlen = int(os.environ.get("FEC_VERIFY_MSG", "64"))
    ctx = F.Context(0)
    st_ = torch.cuda.Stream()
    for logn in logs:
        n = 1 << logn
        rng = np.random.default_rng(50 + logn)
        pk = np.zeros((n, 32), dtype=np.uint8)
        sig = np.zeros((n, 64), dtype=np.uint8)
        sig[:, 32:] = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        blob = rng.integers(0, 256, size=n * mlen, dtype=np.uint8)
        s_limbs = np.ascontiguousarray(sig[:, :31:-1]).view(np.uint64).reshape(n, 4)       # big-endian bytes -> limbs
        raw = blob.tobytes()
        k_limbs = np.array([np.frombuffer(hashlib.sha512(bytes(64) + raw[mlen * i:mlen * (i + 1)]).digest()[31::-1], dtype=np.uint64)
                            for i in range(n)])
        zero_xy = np.zeros((n, 8), dtype=np.uint64)
        d_pk, d_sig, d_msgs = dev(pk), dev(sig), dev(blob)
        d_off = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(mlen))
        d_xy, d_s, d_k = dev(zero_xy), dev(s_limbs), dev(k_limbs)
        out = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3)]

        def run_bytes():
            ctx.ed25519_verify_dev(d_pk.data_ptr(), d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, d_sig.data_ptr(), out[0].data_ptr(), n,
                                   st_.cuda_stream)

        def run_generic():
            ctx.eddsa_verify_ed25519_msg_dev(d_xy.data_ptr(), None, d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, d_xy.data_ptr(), None,
                                             d_s.data_ptr(), out[1].data_ptr(), n, st_.cuda_stream)

        def run_base():
            ctx.eddsa_verify_ed25519_dev(d_xy.data_ptr(), None, d_xy.data_ptr(), None, d_s.data_ptr(), d_k.data_ptr(), out[2].data_ptr(), n,
                                         st_.cuda_stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st_)
            fn()
            e1.record(st_)
            e1.synchronize()
            return e0.elapsed_time(e1)

        runs = (run_bytes, run_generic, run_base)
        for _ in range(2):
            for fn in runs:
                timed(fn)
        t = [[], [], []]
        for _ in range(reps):
            for j, fn in enumerate(runs):
                t[j].append(timed(fn))
        ms = [statistics.median(v) for v in t]
        same = bool(torch.equal(out[0], out[2]))   # the byte form and the baseline were given the same decoded inputs and k
        print(json.dumps({"row": "ed25519_verify_msg", "n": n, "msg_bytes": mlen, "bytes_ms": round(ms[0], 3), "generic_ms": round(ms[1], 3),
                          "from_points_ms": round(ms[2], 3), "bytes_per_s": round(n / ms[0] * 1e3), "generic_per_s": round(n / ms[1] * 1e3),
                          "from_points_per_s": round(n / ms[2] * 1e3), "ratio_bytes": round(ms[2] / ms[0], 4),
                          "ratio_generic": round(ms[2] / ms[1], 4), "bytes_ms_all": [round(v, 3) for v in t[0]],
                          "generic_ms_all": [round(v, 3) for v in t[1]], "from_points_ms_all": [round(v, 3) for v in t[2]],
                          "bytes_status_counts": np.bincount(out[0].cpu().numpy(), minlength=3).tolist(),
                          "bytes_equals_from_points": same, "prefix_bits": ctx.fixed_prefix_bits(2)}), flush=True)
    ctx.close()


main()
