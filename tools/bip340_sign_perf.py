"""Rates of the SHA-256 entry points, 64-byte messages, everything resident in HBM, device events on one stream, the calls
of a row alternating after a warm-up, the median of REPS rounds and the spread (max - min) of each side reported.
One JSON line per row and n:

  bip340_sign     fec_bip340_sign_dev against the COMPOSITION OF EXISTING CALLS on the same inputs in the same process:
                  two fec_batch_mul_fixed_dev (d * G, and a second scalar array in the place of k, which only the fused
                  call can compute) plus two fec_batch_to_affine_dev.  Keys have their top bit clear, so every lane
                  computes.  accept = fused median <= composition median + composition spread.
  sha256          fec_sha256_dev beside fec_sha512_dev on the same messages (ratio = sha512 time / sha256 time).
  ecdsa_verify_msg   fec_ecdsa_verify_msg_dev beside fec_ecdsa_verify_{secp256k1,p256}_dev on digests hashed beforehand
                  (random r, s and keys: both run the whole pipeline); the difference is the hash pass.

    python tools/bip340_sign_perf.py          # FEC_BIP340_LOG2=16,18,20  FEC_BIP340_REPS=7  FEC_BIP340_MSG=64
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
    logs = [int(v) for v in os.environ.get("FEC_BIP340_LOG2", "16,18,20").split(",")]
    reps = int(os.environ.get("FEC_BIP340_REPS", "7"))
    mlen = int(os.environ.get("FEC_BIP340_MSG", "64"))
    ctx = F.Context(0)
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
        rng = np.random.default_rng(70 + logn)
        keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        keys[:, 31] &= 0x7F                                             # little-endian: below the order constant
        k2 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        k2[:, 31] &= 0x7F
        blob = rng.integers(0, 256, size=n * mlen, dtype=np.uint8)
        d_keys, d_k2, d_msgs = dev(keys), dev(k2), dev(blob)
        d_off = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(mlen))
        sig = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        pts = [torch.empty(n * 96, dtype=torch.uint8, device="cuda") for _ in range(2)]
        xy = [torch.empty(n * 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
        inf = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2)]
        g = ctx.generator_dev(0)

        def run_fused():
            ctx.bip340_sign_dev(d_keys.data_ptr(), d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, sig.data_ptr(), status.data_ptr(), n,
                                st_.cuda_stream)

        def run_composed():
            for j, sc in enumerate((d_keys, d_k2)):
                ctx.batch_mul_fixed_dev(0, sc.data_ptr(), g, pts[j].data_ptr(), n, st_.cuda_stream)
                ctx.batch_to_affine_dev(0, pts[j].data_ptr(), xy[j].data_ptr(), inf[j].data_ptr(), n, st_.cuda_stream)

        t = race((run_fused, run_composed))
        fused, comp = stats(t[0]), stats(t[1])
        print(json.dumps({"row": "bip340_sign", "n": n, "msg_bytes": mlen, "fused": fused, "composition": comp,
                          "signatures_per_s": round(n / fused["ms"] * 1e3),
                          "accept": fused["ms"] <= comp["ms"] + comp["spread_ms"],
                          "status_counts": np.bincount(status.cpu().numpy(), minlength=5).tolist(),
                          "prefix_bits": ctx.fixed_prefix_bits(0)}), flush=True)

        d256 = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d512 = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        t = race((lambda: ctx.sha256_dev(d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, d256.data_ptr(), None, n, st_.cuda_stream),
                  lambda: ctx.sha512_dev(d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, d512.data_ptr(), None, n, st_.cuda_stream)))
        a, b = stats(t[0]), stats(t[1])
        print(json.dumps({"row": "sha256", "n": n, "msg_bytes": mlen, "sha256": a, "sha512": b,
                          "ratio_sha512_over_sha256": round(b["ms"] / a["ms"], 4)}), flush=True)

        for curve, name in ((0, "secp256k1"), (1, "p256")):
            r = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
            s = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
            pk = rng.integers(1, 1 << 62, size=(n, 8), dtype=np.uint64)
            d_r, d_s, d_pk = dev(r), dev(s), dev(pk)
            out = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2)]
            base = ctx.ecdsa_verify_secp256k1_dev if curve == 0 else ctx.ecdsa_verify_p256_dev
            t = race((lambda: ctx.ecdsa_verify_msg_dev(curve, d_msgs.data_ptr(), d_off.data_ptr(), n * mlen, d_r.data_ptr(), d_s.data_ptr(),
                                                       d_pk.data_ptr(), None, out[0].data_ptr(), n, st_.cuda_stream),
                      lambda: base(d256.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_pk.data_ptr(), None, out[1].data_ptr(), n,
                                   st_.cuda_stream)))
            a, b = stats(t[0]), stats(t[1])
            print(json.dumps({"row": "ecdsa_verify_msg", "curve": name, "n": n, "msg_bytes": mlen, "from_message": a, "from_digest": b,
                              "hash_pass_ms": round(a["ms"] - b["ms"], 3), "equal": bool(torch.equal(out[0], out[1]))}), flush=True)
    ctx.close()


main()
