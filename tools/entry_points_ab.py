"""Same-process A/B of the entry-point layer of two builds of the library (run on the GPU box):

    python tools/entry_points_ab.py <parent libfecgpu.so> <new libfecgpu.so> [log2 n = 20] [rounds = 3] [rows = all | base | msg] [swapped]

(a) the host-side cost of one enqueue-only *_dev call at n = 1: wall clock of a burst of calls divided by their number, the
    stream drained between bursts.  base: two canonical, two parity entry points; msg: the parity from-the-message family's
    fec_sha256_dev, fec_ecdsa_sign_msg_dev and fec_hash_to_curve_dev;
(b) the wall clock of one host-pointer call at 2^n elements.  base: fec_batch_mul, fec_canon_ecdsa_verify_msg,
    fec_canon_ecdsa_sign_digest, fec_canon_pubkey_tweak_add and fec_ecdsa_batch_verify; msg: fec_ecdsa_verify_msg and
    fec_ed25519_sign.
The parent library is measured alone first, `rounds` rounds; then new and parent alternate for `rounds` rounds.  The margin
is the larger of two spreads of the parent's round medians: alone, and while the two alternate (the first alone does not
resolve the effect of the order in which the libraries were loaded; `swapped` loads and prepares the new library first).
One JSON line per row.  Both libraries get the same
inputs, and the outputs of (b) are compared.
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from forge_ec_amd import synth as V

LOGN = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
ROWS = sys.argv[5] if len(sys.argv) > 5 else "all"
SWAPPED = len(sys.argv) > 6 and sys.argv[6] == "swapped"
N = 1 << LOGN
BURST, CALLS = 200, 5
vp = ctypes.c_void_p


class Lib:
    def __init__(self, path):
        self.name = os.path.basename(path)
        self.l = ctypes.CDLL(os.path.abspath(path))
        self.ctx = vp()
        assert self.l.fec_ctx_create(ctypes.byref(self.ctx), 0) == 0

    def __call__(self, fn, *args):
        f = getattr(self.l, fn)
        f.restype = ctypes.c_int
        rc = f(self.ctx, *[a if a is None or isinstance(a, ctypes._SimpleCData) else (vp(a.ctypes.data) if isinstance(a, np.ndarray) else ctypes.c_size_t(a)) for a in args])
        assert rc == 0, (fn, rc)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def ptr(t):
    return vp(t.data_ptr())


def rand(n, width, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, width), dtype=np.uint8)


def burst_us(call):
    """microseconds of host time per enqueue-only call"""
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(BURST):
        call()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt / BURST * 1e6


def call_ms(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def msg_rows_for(lib):
    """the parity from-the-message family"""
    c = ctypes.c_int
    dst = np.frombuffer(b"entry-points-ab", dtype=np.uint8).copy()
    one = {k: dev(v) for k, v in dict(sk=V.scalars(1, 0, 31), m=rand(1, 32, 32), off=np.array([0, 32], np.uint64), out=np.zeros(12, np.uint64),
                                      st=np.zeros(16, np.uint8)).items()}
    m1 = (ptr(one["m"]), ptr(one["off"]), 32)
    rows = [
        ("fec_sha256_dev n=1", "us", lambda: burst_us(lambda: lib("fec_sha256_dev", *m1, ptr(one["out"]), ptr(one["st"]), 1, None)), None),
        ("fec_ecdsa_sign_msg_dev n=1", "us", lambda: burst_us(lambda: lib("fec_ecdsa_sign_msg_dev", c(0), ptr(one["sk"]), *m1, ptr(one["out"]), ptr(one["st"]),
                                                                           1, None)), None),
        ("fec_hash_to_curve_dev n=1", "us", lambda: burst_us(lambda: lib("fec_hash_to_curve_dev", c(0), c(0), c(0), *m1, dst, len(dst), ptr(one["out"]), None,
                                                                          None, ptr(one["st"]), 1, None)), None),
    ]
    msgs, off = rand(N, 32, 33), np.arange(0, 32 * N + 1, 32, dtype=np.uint64)
    r, s = V.scalars(N, 0, 34), V.scalars(N, 0, 35)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(N, 0, 36), V.field_elements(N, 0, 37)], axis=1))
    vst = np.zeros(N, np.uint8)
    rows.append(("fec_ecdsa_verify_msg 2^%d" % LOGN, "ms",
                 lambda: call_ms(lambda: lib("fec_ecdsa_verify_msg", c(0), msgs, off, 32 * N, r, s, pk, None, vst, N)), vst))
    keys, sig, sst = rand(N, 32, 38), np.zeros((N, 64), np.uint8), np.zeros(N, np.uint8)
    rows.append(("fec_ed25519_sign 2^%d" % LOGN, "ms", lambda: call_ms(lambda: lib("fec_ed25519_sign", keys, msgs, off, 32 * N, sig, sst, N)), sig))
    return rows


def rows_for(lib):
    """[(row name, unit, one measurement, outputs to compare)]"""
    if ROWS == "msg":
        return msg_rows_for(lib)
    c = ctypes.c_int
    one = {k: dev(v) for k, v in dict(s=V.scalars(1, 0, 1), p=V.points(1, 0, 2), o=np.zeros(12, np.uint64), xy=np.zeros(8, np.uint64),
                                      st=np.zeros(16, np.uint8), pk=np.zeros(80, np.uint8), tw=rand(1, 32, 3), q=np.zeros(80, np.uint8)).items()}
    lib("fec_canon_public_key_dev", c(0), ptr(one["s"]), ptr(one["pk"]), 33, ptr(one["st"]), 1, None)
    torch.cuda.synchronize()
    rows = [
        ("fec_canon_mul_base_dev n=1", "us", lambda: burst_us(lambda: lib("fec_canon_mul_base_dev", c(0), ptr(one["s"]), ptr(one["xy"]), ptr(one["st"]), 1, None)), None),
        ("fec_canon_pubkey_tweak_add_dev n=1", "us", lambda: burst_us(lambda: lib("fec_canon_pubkey_tweak_add_dev", c(0), ptr(one["pk"]), 33, ptr(one["tw"]),
                                                                                   ptr(one["q"]), 33, ptr(one["st"]), 1, None)), None),
        ("fec_batch_mul_dev n=1", "us", lambda: burst_us(lambda: lib("fec_batch_mul_dev", c(0), ptr(one["s"]), ptr(one["p"]), ptr(one["o"]), 1, None)), None),
        ("fec_batch_validate_point_dev n=1", "us", lambda: burst_us(lambda: lib("fec_batch_validate_point_dev", c(0), ptr(one["xy"]), None, ptr(one["st"]), 1, None)), None),
    ]
    k, p = V.scalars(N, 0, 11), V.points(N, 0, 12)
    out = np.zeros((N, 12), np.uint64)
    rows.append(("fec_batch_mul 2^%d" % LOGN, "ms", lambda: call_ms(lambda: lib("fec_batch_mul", c(0), k, p, out, N)), out))
    keys, st = rand(N, 32, 13), np.zeros(N, np.uint8)
    keys[:, 0] &= 0x7F
    pks = np.zeros((N, 33), np.uint8)
    lib("fec_canon_public_key", c(0), keys, pks, 33, st, N)
    msgs, off, sigs, res = rand(N, 32, 14), np.arange(0, 32 * N + 1, 32, dtype=np.uint64), rand(N, 64, 15), np.zeros(N, np.uint8)
    rows.append(("fec_canon_ecdsa_verify_msg 2^%d" % LOGN, "ms",
                 lambda: call_ms(lambda: lib("fec_canon_ecdsa_verify_msg", c(0), msgs, off, 32 * N, sigs, pks, 33, res, N)), res))
    dg, sg, sst = rand(N, 32, 16), np.zeros((N, 64), np.uint8), np.zeros(N, np.uint8)
    rows.append(("fec_canon_ecdsa_sign_digest 2^%d" % LOGN, "ms",
                 lambda: call_ms(lambda: lib("fec_canon_ecdsa_sign_digest", c(0), dg, keys, ctypes.c_uint(1), sg, sst, N)), sg))
    tw, q, qst = rand(N, 32, 17), np.zeros((N, 33), np.uint8), np.zeros(N, np.uint8)
    rows.append(("fec_canon_pubkey_tweak_add 2^%d" % LOGN, "ms",
                 lambda: call_ms(lambda: lib("fec_canon_pubkey_tweak_add", c(0), pks, 33, tw, q, 33, qst, N)), q))
    bd = rand(N, 32, 18)
    bd[:, 0] &= 0x7F
    r, s, a = V.scalars(N, 0, 19), V.scalars(N, 0, 20), V.scalars(N, 0, 21)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(N, 0, 22), V.field_elements(N, 0, 23)], axis=1))
    bres, det = np.zeros(1, np.uint8), np.zeros(16, np.uint64)
    rows.append(("fec_ecdsa_batch_verify 2^%d" % LOGN, "ms",
                 lambda: call_ms(lambda: lib("fec_ecdsa_batch_verify", c(0), bd, r, s, pk, None, a, N, bres, det)), det))
    return rows + (msg_rows_for(lib) if ROWS == "all" else [])


def main():
    if SWAPPED:
        new, parent = Lib(sys.argv[2]), Lib(sys.argv[1])
        rn, rp = rows_for(new), rows_for(parent)
    else:
        parent, new = Lib(sys.argv[1]), Lib(sys.argv[2])
        rp, rn = rows_for(parent), rows_for(new)
    for (name, unit, mp, op), (_, _, mn, on) in zip(rp, rn):
        mp(), mn()   # warm-up: tables, staging, scratch
        equal = None if op is None else bool(np.array_equal(op, on))
        nonzero = None if op is None else int(np.count_nonzero(op))
        alone = [float(np.median([mp() for _ in range(CALLS)])) for _ in range(ROUNDS)]
        pa, ne = [], []
        for _ in range(ROUNDS):
            ne.append(float(np.median([mn() for _ in range(CALLS)])))
            pa.append(float(np.median([mp() for _ in range(CALLS)])))
        print(json.dumps({"row": name, "unit": unit, "loaded_first": "new" if SWAPPED else "parent", "parent_alone_rounds": [round(x, 4) for x in alone],
                          "margin": round(max(max(alone) - min(alone), max(pa) - min(pa)), 4), "margin_alone": round(max(alone) - min(alone), 4),
                          "margin_alternating": round(max(pa) - min(pa), 4), "new_rounds": [round(x, 4) for x in ne],
                          "parent_rounds": [round(x, 4) for x in pa], "new_minus_parent": round(float(np.median(ne) - np.median(pa)), 4),
                          "outputs_equal": equal, "output_bytes_nonzero": nonzero}), flush=True)


if __name__ == "__main__":
    main()
