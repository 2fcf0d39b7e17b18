"""Canonical-math mode timing probe (NOT the headline bench, NOT reference parity): kernel ms from
HIP events inside the library for secp256k1 key generation (k*G, comb) and ECDH (k*P, windowed),
inputs resident in HBM.  One JSON line per workload.

    python tools/canon_perf.py [log2_n] [reps] [curve,...]

From the message (fec_canon_*_verify_msg_dev) against the parts it replaces, one JSON line per row:

    python tools/canon_perf.py msg [log2_n] [reps] [out.jsonl]

The batch is resident on the device: n messages of 32 bytes, then of 256 bytes; keys are real (k*G from the comb,
encoded on the host), signatures are random bytes -- every lane does the full work and is rejected at the end.  Per
scheme, alternating in one process: the *_verify_msg_dev call; fec_sha256_dev / fec_sha512_dev over what a caller of
the after-the-hash verifier has to hash (the bare message for ECDSA, T || T || r || pk || msg for BIP-340, R || A || msg
for Ed25519) plus that verifier on limb arrays.  Wall clock around a device synchronise, median and spread (max - min) of
`reps` samples; the whole set of rows is measured twice (pass 0, pass 1), so the run-to-run spread shows.  Then
fec_canon_decompress_dev alone and the three host-pointer forms (32-byte messages, PCIe included).

The signing side (fec_canon_mul_base_secret_dev, the *_sign_*_dev calls), by the same method:

    python tools/canon_perf.py sign [log2_n] [reps] [out.jsonl]

"scan" rows: the secret comb against fec_canon_mul_base_dev on a ctx made with FEC_CANON_COMB4=1 (the same table, the same
64 additions: the difference is the scan and the branch-free addition) and against the default 8-bit comb.  "sign" rows:
each signer with 32- and 256-byte messages, alternating with its parts -- the secret comb pass(es) on as many scalars,
fec_sha256_dev / fec_sha512_dev over the bytes the signer hashes, for ECDSA the parity-mode RFC 6979 kernel (the same chain;
it hashes the message itself), and the fec_canon_scalar_op passes, which exist as host-pointer calls only and are reported
apart (PCIe included).  "verify-valid" rows: fec_canon_*_verify_msg_dev over the signatures the signers just made, all
of which must come out valid.  Last, one host-pointer row per signer.

X25519 (fec_canon_x25519_dev, fec_canon_x25519_base_dev), by the same method:

    python tools/canon_perf.py x25519 [log2_n] [reps] [out.jsonl]

"ladder" rows: fec_canon_x25519_dev on random u against fec_canon_mul_dev(FEC_ED25519) -- the same field, the windowed
Edwards multiplication -- and against parity mode's fec_x25519_dev.  "base" rows: fec_canon_x25519_base_dev against
fec_canon_mul_base_secret_dev(FEC_ED25519) (the difference is the clamp, the map's inversion and the encoding) and against
fec_canon_x25519_dev at u = 9, whose outputs must equal the base path's.  Last, one host-pointer row each.

Recovery, Keccak-256 and recoverable signing on secp256k1, by the same method:

    python tools/canon_perf.py recover [log2_n] [reps] [out.jsonl]

The signatures are real (fec_canon_ecdsa_sign_recoverable_digest_dev over random digests and keys) and every one must recover
to its key.  "recover" rows: fec_canon_ecdsa_recover_dev (out_len 64) against fec_canon_ecdsa_verify_msg_dev with 33-byte
keys and 32-byte messages -- one square root, one grouped inversion and u1 G + u2 Q each, the verifier with a SHA-256 on top.
"address" rows: out_len 20 against out_len 64, the cost of the Keccak in the finish pass.  "keccak" rows:
fec_canon_keccak256_dev against fec_sha256_dev on the same 64-byte messages.  "sign" rows: the recoverable signer against
fec_canon_ecdsa_sign_digest_dev, whose signatures must be the same bytes.  Last, one host-pointer row each.

EC tweak-add and BIP-32 derivation on secp256k1, by the same method:

    python tools/canon_perf.py bip32 [log2_n] [reps] [out.jsonl]

Before anything is timed: derive_priv -> public_key must equal derive_pub, chain codes included, and pubkey_tweak_add must equal
public_key(seckey_tweak_add).  "tweak" rows: fec_canon_pubkey_tweak_add_dev on 33-byte keys against fec_canon_decompress_dev(33)
followed by fec_canon_mul_base_dev on the same batch (its square root and its comb, without the addition and the encoding).
"tweak-emulation" rows: against the double_mul(t, 1, P) it replaces, with the decoding that emulation needs.  "derive-pub" rows:
fec_canon_bip32_derive_pub_dev with n parents against the tweak-add (the difference is the four compressions);
"derive-pub-shared": with one parent against fec_canon_mul_base_dev, the floor of that form.  "derive-priv":
fec_canon_bip32_derive_priv_dev on non-hardened indices against fec_canon_public_key_dev, the same secret comb;
"derive-priv-hardened": under FEC_CANON_BIP32_NO_COMB against fec_sha512_dev on 64-byte messages, four compressions against
one.  Last, one host-pointer row each.

RIPEMD-160 / HASH160, Taproot output keys and CKDpub along a path on secp256k1, by the same method:

    [FEC_AB_LIB=<another build of libfecgpu.so>] python tools/canon_perf.py wallet [log2_n] [reps] [out.jsonl]

Before anything is timed: the path call at depth 2 and 3 must equal as many chained fec_canon_bip32_derive_pub_dev calls, its
fingerprints and HASH160 must equal fec_canon_pubkey_hash160_dev of the chain's keys, and the Taproot call must equal
fec_canon_pubkey_tweak_add_dev fed tweaks that fec_sha256_dev computed from the tag prefix.  "path-depth2" / "path-depth3" rows:
fec_canon_bip32_derive_pub_path_dev with both optional outputs NULL against the chain -- the chain runs in the library named by
FEC_AB_LIB where that is set (the build of the parent commit, loaded beside this one with a ctx of its own: the same box, the
same process, alternating) and in this library otherwise; the row says which.  "path-optional" rows: the depth-2 call with
out_hash160, with out_fingerprints and with both against both NULL.  "hash" rows: fec_canon_ripemd160_dev and
fec_canon_hash160_dev against fec_sha256_dev (FEC_AB_LIB's where set) on the same 64-byte messages.  "taproot" rows:
fec_canon_taproot_output_key_dev with and without roots against fec_canon_pubkey_tweak_add_dev (pk_len 32, out_len 32) fed
precomputed tweaks.  Last, one host-pointer row each.

The bucket-method multi-scalar multiplication (fec_canon_msm_dev), by the same method:

    python tools/canon_perf.py msm [max_log2_n] [reps] [out.jsonl]

Inputs resident, wall clock around a device synchronise, median of `reps` (7); every MSM sample alternates in this process
with one of its comparator, fec_canon_mul_dev on the same n pairs -- what a caller had to run before summing the n points on
the CPU.  "size" rows: n = 2^10 .. 2^max in steps of 4x, random scalars, the automatic window.  "window" rows: n = 2^18 and 2^20 (or
max), every forced window 8 .. 16 -- the sweep the automatic rule is read from.  "skew" rows at the same n: all scalars equal,
and one point throughout, next to the random row.  Every row records the status byte the call left (0).

Batch signature verification (fec_canon_bip340_batch_verify_msg_dev, fec_canon_ed25519_batch_verify_msg_dev):

    python tools/canon_perf.py batch [max_log2_n] [reps] [out.jsonl]

Inputs resident -- 32-byte messages, signatures made by the library's own signers -- wall clock around a device synchronise,
median of `reps` (7); every batch sample alternates in this process with one of fec_canon_bip340_verify_msg_dev /
fec_canon_ed25519_verify_msg_dev over the same signatures.  "size" rows: n = 2^10 .. 2^20, and 2^max above that where the
signatures fit.  "all-refused" row: every s out of range, so the sum is 2 n + 1 times 0 * G.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import forge_ec_amd as F  # noqa: E402
from forge_ec_amd import synth  # noqa: E402
from forge_ec_amd.canon import CANON_CURVES  # noqa: E402

# field multiplications per unit (each = 64 MAD32 for the 512-bit product + 8 for the fold)
MULS = {"keygen": 64 * 11 + 274, "ecdh": 7 + 13 * 11 + 64 * (4 * 7 + 16) + 274 + 5}
MAD_PER_MUL = 72


def _timed(fn, reps):
    """median and spread (max - min) in ms of `reps` runs after one warm-up, wall clock around a device synchronise"""
    samples = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:
            samples.append((time.perf_counter() - t0) * 1e3)
    samples.sort()
    return samples[len(samples) // 2], samples[-1] - samples[0]


def _encoded_keys(ctx, n):
    """real keys as bytes: {("secp256k1", 33): (n,33) uint8, ..., ("bip340", 32), ("ed25519", 32)}"""
    out = {}
    k = synth.scalars(n, 0, 51)
    for cname in ("secp256k1", "p256", "ed25519"):
        xy, st = CANON_CURVES[cname](ctx).mul_base(k)
        assert not st.any()
        x = xy[:, :4].copy().view(np.uint8).reshape(n, 32)
        y = xy[:, 4:].copy().view(np.uint8).reshape(n, 32)
        if cname == "ed25519":
            enc = y.copy()
            enc[:, 31] |= (x[:, 0] & 1) << 7
            out[("ed25519", 32)] = enc
            continue
        xb, yb = x[:, ::-1], y[:, ::-1]   # big-endian
        out[(cname, 33)] = np.ascontiguousarray(np.concatenate([(2 + (y[:, :1] & 1)).astype(np.uint8), xb], axis=1))
        out[(cname, 65)] = np.ascontiguousarray(np.concatenate([np.full((n, 1), 4, dtype=np.uint8), xb, yb], axis=1))
        if cname == "secp256k1":
            out[("bip340", 32)] = np.ascontiguousarray(xb)
    return out


def main_msg():
    logn = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    n = 1 << logn
    ctx = F.Context(0)
    lib, h = ctx._lib, ctx._h
    rng = np.random.default_rng(16)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    keys = _encoded_keys(ctx, n)
    sigs_h = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    sigs_h[:, 0] &= 0x7F      # big-endian r and s below p and n; Ed25519's little-endian S below l
    sigs_h[:, 32] &= 0x7F
    sigs_h[:, 63] &= 0x0F
    sigs = dev(sigs_h)
    limbs = [torch.from_numpy(synth.scalars(n, 0, 60 + i).view(np.int64)).cuda() for i in range(4)]
    pub = torch.from_numpy(CANON_CURVES["secp256k1"](ctx).mul_base(synth.scalars(n, 0, 51))[0].view(np.int64)).cuda()
    pub_p256 = torch.from_numpy(CANON_CURVES["p256"](ctx).mul_base(synth.scalars(n, 0, 51))[0].view(np.int64)).cuda()
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    digests = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    xy = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    schemes = [("ecdsa-secp256k1-33", "secp256k1", ("secp256k1", 33), 0), ("ecdsa-secp256k1-65", "secp256k1", ("secp256k1", 65), 0),
               ("ecdsa-p256-33", "p256", ("p256", 33), 0), ("bip340", "secp256k1", ("bip340", 32), 128), ("ed25519", "ed25519", ("ed25519", 32), 64)]
    for npass in range(2):
        for mlen in (32, 256):
            msgs = dev(rng.integers(0, 256, size=n * mlen, dtype=np.uint8))
            off = dev(np.arange(n + 1, dtype=np.uint64) * mlen)
            for name, cname, kk, prefix in schemes:
                c = CANON_CURVES[cname](ctx)
                pk = dev(keys[kk])
                # what the parts approach hashes: the message behind its prefix
                pm = dev(rng.integers(0, 256, size=n * (prefix + mlen), dtype=np.uint8)) if prefix else msgs
                poff = dev(np.arange(n + 1, dtype=np.uint64) * (prefix + mlen)) if prefix else off
                if name.startswith("ecdsa"):
                    whole = lambda: c.ecdsa_verify_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, sigs.data_ptr(), pk.data_ptr(), kk[1], res.data_ptr(), n, st)  # noqa: E731
                    hash_ = lambda: ctx.sha256_dev(pm.data_ptr(), poff.data_ptr(), n * mlen, digests.data_ptr(), None, n, st)  # noqa: E731
                    p = pub if cname == "secp256k1" else pub_p256
                    verify = lambda: c.ecdsa_verify_dev(limbs[0].data_ptr(), limbs[1].data_ptr(), limbs[2].data_ptr(), p.data_ptr(), res.data_ptr(), n, st)  # noqa: E731
                elif name == "bip340":
                    whole = lambda: c.bip340_verify_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, sigs.data_ptr(), pk.data_ptr(), res.data_ptr(), n, st)  # noqa: E731
                    hash_ = lambda: ctx.sha256_dev(pm.data_ptr(), poff.data_ptr(), n * (prefix + mlen), digests.data_ptr(), None, n, st)  # noqa: E731
                    verify = lambda: c.bip340_verify_dev(pub.data_ptr(), limbs[1].data_ptr(), limbs[2].data_ptr(), limbs[3].data_ptr(), res.data_ptr(), n, st)  # noqa: E731
                else:
                    whole = lambda: c.ed25519_verify_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, sigs.data_ptr(), pk.data_ptr(), res.data_ptr(), n, st)  # noqa: E731
                    hash_ = lambda: ctx.sha512_dev(pm.data_ptr(), poff.data_ptr(), n * (prefix + mlen), digests.data_ptr(), None, n, st)  # noqa: E731
                    verify = lambda: c.eddsa_verify_dev(pk.data_ptr(), sigs.data_ptr(), limbs[2].data_ptr(), limbs[3].data_ptr(), res.data_ptr(), n, st)  # noqa: E731
                ws, hs, vs = [], [], []
                for _ in range(3):       # whole, parts, whole, parts, ...: alternating in one process
                    ws.append(_timed(whole, reps))
                    hs.append(_timed(hash_, reps))
                    vs.append(_timed(verify, reps))
                w, h_, v = (sorted(x)[1] for x in (ws, hs, vs))      # the middle round's (median, spread)
                emit({"row": name, "msg_bytes": mlen, "pass": npass, "n": n, "reps": reps,
                      "msg_dev_ms": round(w[0], 4), "msg_dev_spread_ms": round(max(x[1] for x in ws), 4),
                      "hash_dev_ms": round(h_[0], 4), "verify_dev_ms": round(v[0], 4), "parts_ms": round(h_[0] + v[0], 4),
                      "parts_spread_ms": round(max(x[1] for x in hs) + max(x[1] for x in vs), 4),
                      "msg_over_parts": round(w[0] / (h_[0] + v[0]), 4), "M_per_s": round(n / w[0] / 1e3, 3)})
        for cname, kl in (("secp256k1", 33), ("secp256k1", 65), ("p256", 33), ("p256", 65)):
            c = CANON_CURVES[cname](ctx)
            pk = dev(keys[(cname, kl)])
            ms, spread = _timed(lambda: c.decompress_dev(pk.data_ptr(), kl, xy.data_ptr(), res.data_ptr(), n, st), reps)
            emit({"row": "decompress-%s-%d" % (cname, kl), "pass": npass, "n": n, "reps": reps, "ms": round(ms, 4),
                  "spread_ms": round(spread, 4), "M_per_s": round(n / ms / 1e3, 3)})
    # host pointers: what a caller with arrays in host memory sees (PCIe: 64 + key + message bytes in, 1 byte out)
    mlen = 32
    msgs_h = rng.integers(0, 256, size=n * mlen, dtype=np.uint8)
    off_h = np.arange(n + 1, dtype=np.uint64) * mlen
    res_h = np.zeros(n, dtype=np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    for name, cid, kk in (("ecdsa-secp256k1-33", 0, ("secp256k1", 33)), ("bip340", None, ("bip340", 32)), ("ed25519", None, ("ed25519", 32))):
        pk = keys[kk]
        if cid is not None:
            fn = lambda: lib.fec_canon_ecdsa_verify_msg(h, cid, p(msgs_h), p(off_h), n * mlen, p(sigs_h), p(pk), kk[1], p(res_h), n)  # noqa: E731
        elif name == "bip340":
            fn = lambda: lib.fec_canon_bip340_verify_msg(h, p(msgs_h), p(off_h), n * mlen, p(sigs_h), p(pk), p(res_h), n)  # noqa: E731
        else:
            fn = lambda: lib.fec_canon_ed25519_verify_msg(h, p(msgs_h), p(off_h), n * mlen, p(sigs_h), p(pk), p(res_h), n)  # noqa: E731
        assert fn() == 0
        ms, spread = _timed(fn, reps)
        emit({"row": "host-" + name, "msg_bytes": mlen, "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4),
              "M_per_s": round(n / ms / 1e3, 3), "bytes_per_signature": 64 + kk[1] + mlen + 8 + 1})
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_sign():
    logn = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    n = 1 << logn
    ctx = F.Context(0)
    os.environ["FEC_CANON_COMB4"] = "1"
    ctx4 = F.Context(0)
    del os.environ["FEC_CANON_COMB4"]
    lib, h = ctx._lib, ctx._h
    rng = np.random.default_rng(17)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def rounds(fns):
        """each of fns three times, alternating; per fn the middle round's median and the largest spread"""
        got = [[] for _ in fns]
        for _ in range(3):
            for g, fn in zip(got, fns):
                g.append(_timed(fn, reps))
        return [(sorted(g)[1][0], max(x[1] for x in g)) for g in got]

    keys_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    keys_h[:, 0] &= 0x7F                     # big-endian keys below both orders, and not zero
    keys_h[:, 31] |= 1
    keys = dev(keys_h)
    aux = dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    k_limbs = torch.from_numpy(synth.scalars(n, 0, 71).view(np.int64)).cuda()
    k_limbs[:, 3] &= 0x0FFFFFFFFFFFFFFF      # below every order
    k2 = torch.cat([k_limbs, k_limbs])
    xy = torch.empty((2 * n, 8), dtype=torch.int64, device="cuda")
    stat = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    sigs = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    digests = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    pks = {33: torch.empty((n, 33), dtype=torch.uint8, device="cuda"), 32: torch.empty((n, 32), dtype=torch.uint8, device="cuda")}
    knonce = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    for npass in range(2):
        # ---- the price of the scan ----
        for cname in ("secp256k1", "p256", "ed25519"):
            c, c4 = CANON_CURVES[cname](ctx), CANON_CURVES[cname](ctx4)
            sec, pub4, pub8 = rounds([
                lambda: c.mul_base_secret_dev(k_limbs.data_ptr(), xy.data_ptr(), stat.data_ptr(), n, st),
                lambda: c4.mul_base_dev(k_limbs.data_ptr(), xy.data_ptr(), stat.data_ptr(), n, st),
                lambda: c.mul_base_dev(k_limbs.data_ptr(), xy.data_ptr(), stat.data_ptr(), n, st)])
            emit({"row": "scan-" + cname, "pass": npass, "n": n, "reps": reps, "secret_ms": round(sec[0], 4), "secret_spread_ms": round(sec[1], 4),
                  "comb4_ms": round(pub4[0], 4), "comb4_spread_ms": round(pub4[1], 4), "comb8_ms": round(pub8[0], 4),
                  "comb8_spread_ms": round(pub8[1], 4), "secret_over_comb4": round(sec[0] / pub4[0], 4),
                  "secret_over_comb8": round(sec[0] / pub8[0], 4), "M_per_s": round(n / sec[0] / 1e3, 3)})
        # ---- each signer against its parts, then the verifier on what it made ----
        for mlen in (32, 256):
            msgs = dev(rng.integers(0, 256, size=n * mlen, dtype=np.uint8))
            off = dev(np.arange(n + 1, dtype=np.uint64) * mlen)

            def hashed(fn, prefix):
                pm = dev(rng.integers(0, 256, size=n * (prefix + mlen), dtype=np.uint8))
                po = dev(np.arange(n + 1, dtype=np.uint64) * (prefix + mlen))
                return lambda: fn(pm.data_ptr(), po.data_ptr(), n * (prefix + mlen), digests.data_ptr(), None, n, st)

            for name, cname in (("ecdsa-secp256k1", "secp256k1"), ("ecdsa-p256", "p256"), ("bip340", "secp256k1"), ("ed25519", "ed25519")):
                c = CANON_CURVES[cname](ctx)
                comb1 = lambda: c.mul_base_secret_dev(k_limbs.data_ptr(), xy.data_ptr(), stat.data_ptr(), n, st)  # noqa: E731
                if name.startswith("ecdsa"):
                    cid = 0 if cname == "secp256k1" else 1
                    whole = lambda: c.ecdsa_sign_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, keys.data_ptr(), 1, sigs.data_ptr(), stat.data_ptr(), n, st)  # noqa: E731
                    parts = [comb1, lambda: ctx.rfc6979_k_dev(cid, k_limbs.data_ptr(), msgs.data_ptr(), off.data_ptr(), n * mlen, knonce.data_ptr(),
                                                              stat.data_ptr(), n, st)]
                    scalar_passes = 4      # x mod n, k^-1, r d + z, the product
                elif name == "bip340":
                    whole = lambda: c.bip340_sign_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, keys.data_ptr(), aux.data_ptr(), sigs.data_ptr(), stat.data_ptr(), n, st)  # noqa: E731
                    parts = [comb1, comb1, hashed(ctx.sha256_dev, 128), hashed(ctx.sha256_dev, 128)]    # nonce and challenge hashes (the 96-byte aux hash: not counted)
                    scalar_passes = 1
                else:
                    whole = lambda: c.ed25519_sign_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, keys.data_ptr(), sigs.data_ptr(), pks[32].data_ptr(), stat.data_ptr(), n, st)  # noqa: E731
                    parts = [lambda: c.mul_base_secret_dev(k2.data_ptr(), xy.data_ptr(), stat.data_ptr(), 2 * n, st),
                             hashed(ctx.sha512_dev, 32), hashed(ctx.sha512_dev, 64)]
                    scalar_passes = 1
                got = rounds([whole] + parts)
                w, ps = got[0], got[1:]
                parts_ms, parts_spread = sum(p[0] for p in ps), sum(p[1] for p in ps)
                emit({"row": "sign-" + name, "msg_bytes": mlen, "pass": npass, "n": n, "reps": reps, "sign_dev_ms": round(w[0], 4),
                      "sign_dev_spread_ms": round(w[1], 4), "parts_ms": round(parts_ms, 4), "parts_spread_ms": round(parts_spread, 4),
                      "parts_each_ms": [round(p[0], 4) for p in ps], "scalar_op_passes_not_included": scalar_passes,
                      "sign_over_parts": round(w[0] / parts_ms, 4), "M_per_s": round(n / w[0] / 1e3, 3)})
                # the verifier on these signatures: every one must be valid
                torch.cuda.synchronize()
                assert not bool(stat[:n].any()), name
                if name.startswith("ecdsa"):
                    c.public_key_dev(keys.data_ptr(), pks[33].data_ptr(), 33, stat.data_ptr(), n, st)
                    ver = lambda: c.ecdsa_verify_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, sigs.data_ptr(), pks[33].data_ptr(), 33, res.data_ptr(), n, st)  # noqa: E731
                elif name == "bip340":
                    c.public_key_dev(keys.data_ptr(), pks[32].data_ptr(), 32, stat.data_ptr(), n, st, scheme=3)
                    ver = lambda: c.bip340_verify_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, sigs.data_ptr(), pks[32].data_ptr(), res.data_ptr(), n, st)  # noqa: E731
                else:
                    ver = lambda: c.ed25519_verify_msg_dev(msgs.data_ptr(), off.data_ptr(), n * mlen, sigs.data_ptr(), pks[32].data_ptr(), res.data_ptr(), n, st)  # noqa: E731
                ms, spread = _timed(ver, reps)
                torch.cuda.synchronize()
                assert int(res.sum()) == n, (name, int(res.sum()))
                emit({"row": "verify-valid-" + name, "msg_bytes": mlen, "pass": npass, "n": n, "reps": reps, "ms": round(ms, 4),
                      "spread_ms": round(spread, 4), "M_per_s": round(n / ms / 1e3, 3), "valid": n})
    # ---- the scalar-field passes (host pointers only) and one host-pointer row per signer ----
    a_h = synth.scalars(n, 0, 72)
    for cname in ("secp256k1", "ed25519"):
        c = CANON_CURVES[cname](ctx)
        ms, spread = _timed(lambda: c.scalar_muladd(a_h, a_h, a_h), reps)
        emit({"row": "scalar-op-muladd-host-" + cname, "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4)})
    ms, spread = _timed(lambda: CANON_CURVES["secp256k1"](ctx).scalar_inv(a_h), reps)
    emit({"row": "scalar-op-inverse-host-secp256k1", "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4)})
    mlen = 32
    msgs_h = rng.integers(0, 256, size=n * mlen, dtype=np.uint8)
    off_h = np.arange(n + 1, dtype=np.uint64) * mlen
    sig_h, st_h, pk_h = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    aux_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    for name, fn in (("ecdsa-secp256k1", lambda: lib.fec_canon_ecdsa_sign_msg(h, 0, p(msgs_h), p(off_h), n * mlen, p(keys_h), 1, p(sig_h), p(st_h), n)),
                     ("bip340", lambda: lib.fec_canon_bip340_sign_msg(h, p(msgs_h), p(off_h), n * mlen, p(keys_h), p(aux_h), p(sig_h), p(st_h), n)),
                     ("ed25519", lambda: lib.fec_canon_ed25519_sign_msg(h, p(msgs_h), p(off_h), n * mlen, p(keys_h), p(sig_h), p(pk_h), p(st_h), n))):
        assert fn() == 0
        ms, spread = _timed(fn, reps)
        emit({"row": "host-sign-" + name, "msg_bytes": mlen, "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4),
              "M_per_s": round(n / ms / 1e3, 3)})
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_x25519():
    from forge_ec_amd.canon import CanonX25519
    logn = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    n = 1 << logn
    ctx = F.Context(0)
    lib, h = ctx._lib, ctx._h
    rng = np.random.default_rng(20)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def rounds(fns):
        """each of fns three times, alternating; per fn the middle round's median and the largest spread"""
        got = [[] for _ in fns]
        for _ in range(3):
            for g, fn in zip(got, fns):
                g.append(_timed(fn, reps))
        return [(sorted(g)[1][0], max(x[1] for x in g)) for g in got]

    x, ed = CanonX25519(ctx), CANON_CURVES["ed25519"](ctx)
    ks_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    us_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    nine_h = np.zeros((n, 32), dtype=np.uint8)
    nine_h[:, 0] = 9
    ks, us, nine = dev(ks_h), dev(us_h), dev(nine_h)
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    out9 = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    stat = torch.empty(n, dtype=torch.uint8, device="cuda")
    xy = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    pts = torch.from_numpy(ed.mul_base(synth.scalars(n, 0, 51))[0].view(np.int64)).cuda()     # points for the windowed multiplication
    for npass in range(2):
        lad, win, par = rounds([
            lambda: x.x25519_dev(ks.data_ptr(), us.data_ptr(), out.data_ptr(), stat.data_ptr(), n, st),
            lambda: ed.mul_dev(ks.data_ptr(), pts.data_ptr(), xy.data_ptr(), stat.data_ptr(), n, st),
            lambda: ctx.x25519_dev(ks.data_ptr(), us.data_ptr(), out.data_ptr(), n, st)])
        emit({"row": "ladder", "pass": npass, "n": n, "reps": reps, "x25519_dev_ms": round(lad[0], 4), "x25519_dev_spread_ms": round(lad[1], 4),
              "canon_mul_ed25519_ms": round(win[0], 4), "canon_mul_ed25519_spread_ms": round(win[1], 4),
              "parity_x25519_dev_ms": round(par[0], 4), "parity_x25519_dev_spread_ms": round(par[1], 4),
              "ladder_over_windowed": round(lad[0] / win[0], 4), "ladder_over_parity": round(lad[0] / par[0], 4),
              "M_per_s": round(n / lad[0] / 1e3, 3)})
        base, comb, lad9 = rounds([
            lambda: x.x25519_base_dev(ks.data_ptr(), out.data_ptr(), n, st),
            lambda: ed.mul_base_secret_dev(ks.data_ptr(), xy.data_ptr(), stat.data_ptr(), n, st),
            lambda: x.x25519_dev(ks.data_ptr(), nine.data_ptr(), out9.data_ptr(), stat.data_ptr(), n, st)])
        torch.cuda.synchronize()
        assert bool((out == out9).all()) and not bool(stat.any())
        emit({"row": "base", "pass": npass, "n": n, "reps": reps, "x25519_base_dev_ms": round(base[0], 4), "x25519_base_dev_spread_ms": round(base[1], 4),
              "mul_base_secret_ed25519_ms": round(comb[0], 4), "mul_base_secret_ed25519_spread_ms": round(comb[1], 4),
              "x25519_dev_at_9_ms": round(lad9[0], 4), "x25519_dev_at_9_spread_ms": round(lad9[1], 4),
              "base_over_secret_comb": round(base[0] / comb[0], 4), "base_over_ladder_at_9": round(base[0] / lad9[0], 4),
              "M_per_s": round(n / base[0] / 1e3, 3)})
    out_h, st_h = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    for name, fn in (("x25519", lambda: lib.fec_canon_x25519(h, p(ks_h), p(us_h), p(out_h), p(st_h), n)),
                     ("x25519_base", lambda: lib.fec_canon_x25519_base(h, p(ks_h), p(out_h), n))):
        assert fn() == 0
        ms, spread = _timed(fn, reps)
        emit({"row": "host-" + name, "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4), "M_per_s": round(n / ms / 1e3, 3)})
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_recover():
    from forge_ec_amd.canon import CanonKeccak
    logn = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    n = 1 << logn
    ctx = F.Context(0)
    lib, h = ctx._lib, ctx._h
    rng = np.random.default_rng(21)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def rounds(fns):
        """each of fns three times, alternating; per fn the middle round's median and the largest spread"""
        got = [[] for _ in fns]
        for _ in range(3):
            for g, fn in zip(got, fns):
                g.append(_timed(fn, reps))
        return [(sorted(g)[1][0], max(x[1] for x in g)) for g in got]

    def pair(row, npass, names, fns, **extra):
        a, b = rounds(fns)
        emit(dict({"row": row, "pass": npass, "n": n, "reps": reps, names[0] + "_ms": round(a[0], 4), names[0] + "_spread_ms": round(a[1], 4),
                   names[1] + "_ms": round(b[0], 4), names[1] + "_spread_ms": round(b[1], 4), "ratio": round(a[0] / b[0], 4),
                   "M_per_s": round(n / a[0] / 1e3, 3)}, **extra))

    cv, kk = CANON_CURVES["secp256k1"](ctx), CanonKeccak(ctx)
    keys_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    keys_h[:, 0] &= 0x7F      # big-endian keys below n ...
    keys_h[:, 31] |= 1        # ... and not zero
    dg_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    msg64_h = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    keys, dg, msg64 = dev(keys_h), dev(dg_h), dev(msg64_h)
    off32 = torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64, device="cuda")
    off64 = torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device="cuda")
    sigs, sigs2 = (torch.empty((n, 64), dtype=torch.uint8, device="cuda") for _ in range(2))
    rec, stat, stat2, res = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(4))
    pk33, out33 = (torch.empty((n, 33), dtype=torch.uint8, device="cuda") for _ in range(2))
    out64 = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    out20 = torch.empty((n, 20), dtype=torch.uint8, device="cuda")
    hash_k, hash_s = (torch.empty((n, 32), dtype=torch.uint8, device="cuda") for _ in range(2))
    # real signatures with their ids, and what they must recover to
    cv.ecdsa_sign_recoverable_digest_dev(dg.data_ptr(), keys.data_ptr(), 1, sigs.data_ptr(), rec.data_ptr(), stat.data_ptr(), n, st)
    cv.public_key_dev(keys.data_ptr(), pk33.data_ptr(), 33, stat2.data_ptr(), n, st)
    cv.ecdsa_recover_dev(dg.data_ptr(), sigs.data_ptr(), rec.data_ptr(), out33.data_ptr(), 33, res.data_ptr(), n, st)
    torch.cuda.synchronize()
    assert not bool(stat.any()) and not bool(stat2.any()) and not bool(res.any()) and bool((out33 == pk33).all())
    for npass in range(2):
        pair("recover", npass, ("ecdsa_recover_dev_64", "ecdsa_verify_msg_dev_33"), [
            lambda: cv.ecdsa_recover_dev(dg.data_ptr(), sigs.data_ptr(), rec.data_ptr(), out64.data_ptr(), 64, res.data_ptr(), n, st),
            lambda: cv.ecdsa_verify_msg_dev(dg.data_ptr(), off32.data_ptr(), 32 * n, sigs.data_ptr(), pk33.data_ptr(), 33, stat2.data_ptr(), n, st)])
        pair("address", npass, ("ecdsa_recover_dev_20", "ecdsa_recover_dev_64"), [
            lambda: cv.ecdsa_recover_dev(dg.data_ptr(), sigs.data_ptr(), rec.data_ptr(), out20.data_ptr(), 20, res.data_ptr(), n, st),
            lambda: cv.ecdsa_recover_dev(dg.data_ptr(), sigs.data_ptr(), rec.data_ptr(), out64.data_ptr(), 64, res.data_ptr(), n, st)])
        pair("keccak", npass, ("keccak256_dev_64B", "sha256_dev_64B"), [
            lambda: kk.keccak256_dev(msg64.data_ptr(), off64.data_ptr(), 64 * n, hash_k.data_ptr(), stat2.data_ptr(), n, st),
            lambda: lib.fec_sha256_dev(h, msg64.data_ptr(), off64.data_ptr(), 64 * n, hash_s.data_ptr(), stat2.data_ptr(), n, st)])
        pair("sign", npass, ("sign_recoverable_digest_dev", "sign_digest_dev"), [
            lambda: cv.ecdsa_sign_recoverable_digest_dev(dg.data_ptr(), keys.data_ptr(), 1, sigs2.data_ptr(), rec.data_ptr(), stat.data_ptr(), n, st),
            lambda: cv.ecdsa_sign_digest_dev(dg.data_ptr(), keys.data_ptr(), 1, sigs.data_ptr(), stat.data_ptr(), n, st)])
        torch.cuda.synchronize()
        assert bool((sigs == sigs2).all()) and not bool(res.any())
    # the address is the hash of the raw key
    kk.keccak256_dev(out64.data_ptr(), off64.data_ptr(), 64 * n, hash_k.data_ptr(), None, n, st)
    torch.cuda.synchronize()
    assert bool((hash_k[:, 12:] == out20).all())
    p = lambda a: a.ctypes.data  # noqa: E731
    sigs_h, rec_h = sigs.cpu().numpy(), rec.cpu().numpy()
    out_h, st_h, dig_h = np.zeros((n, 20), np.uint8), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    off_h = np.arange(0, 64 * (n + 1), 64, dtype=np.uint64)
    for name, fn in (("ecdsa_recover_20", lambda: lib.fec_canon_ecdsa_recover(h, 0, p(dg_h), p(sigs_h), p(rec_h), p(out_h), 20, p(st_h), n)),
                     ("keccak256_64B", lambda: lib.fec_canon_keccak256(h, p(msg64_h), p(off_h), 64 * n, p(dig_h), n))):
        assert fn() == 0
        ms, spread = _timed(fn, reps)
        emit({"row": "host-" + name, "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4), "M_per_s": round(n / ms / 1e3, 3)})
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_bip32():
    from forge_ec_amd.canon import CanonBip32
    from forge_ec_amd import _lib as L
    logn = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    n = 1 << logn
    ctx = F.Context(0)
    lib, h = ctx._lib, ctx._h
    rng = np.random.default_rng(22)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def rounds(fns):
        """each of fns three times, alternating; per fn the middle round's median and the largest spread"""
        got = [[] for _ in fns]
        for _ in range(3):
            for g, fn in zip(got, fns):
                g.append(_timed(fn, reps))
        return [(sorted(g)[1][0], max(x[1] for x in g)) for g in got]

    def pair(row, npass, names, fns, **extra):
        a, b = rounds(fns)
        emit(dict({"row": row, "pass": npass, "n": n, "reps": reps, names[0] + "_ms": round(a[0], 4), names[0] + "_spread_ms": round(a[1], 4),
                   names[1] + "_ms": round(b[0], 4), names[1] + "_spread_ms": round(b[1], 4), "ratio": round(a[0] / b[0], 4),
                   "M_per_s": round(n / a[0] / 1e3, 3)}, **extra))

    cv, hd = CANON_CURVES["secp256k1"](ctx), CanonBip32(ctx)
    keys_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    keys_h[:, 0] &= 0x7F      # big-endian keys and tweaks below n ...
    keys_h[:, 31] |= 1        # ... and not zero
    tw_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    tw_h[:, 0] &= 0x7F
    cc_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    idx_h = rng.integers(0, 1 << 31, size=n, dtype=np.uint32)
    msg64_h = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    keys, tw, cc, idx, msg64 = dev(keys_h), dev(tw_h), dev(cc_h), dev(idx_h), dev(msg64_h)
    hard = dev(idx_h | np.uint32(1 << 31))
    tw_limbs = dev(np.ascontiguousarray(tw_h[:, ::-1]))          # the same tweaks as little-endian limbs
    one = np.zeros((n, 4), dtype=np.uint64)
    one[:, 0] = 1
    one = dev(one)
    off64 = torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device="cuda")
    pk33, out33, out33b, child33 = (torch.empty((n, 33), dtype=torch.uint8, device="cuda") for _ in range(4))
    xy, xy2 = (torch.empty((n, 8), dtype=torch.int64, device="cuda") for _ in range(2))
    ck, occ, occ2, tk = (torch.empty((n, 32), dtype=torch.uint8, device="cuda") for _ in range(4))
    dg64 = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    s1, s2, s3 = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3))
    P = lambda t: t.data_ptr()  # noqa: E731
    # what the timed calls must agree on: derive_priv -> public_key == derive_pub; tweak-add == public_key(seckey_tweak_add)
    cv.public_key_dev(P(keys), P(pk33), 33, P(s1), n, st)
    hd.derive_priv_dev(P(keys), P(cc), n, P(idx), 0, P(ck), P(occ), P(s2), n, st)
    cv.public_key_dev(P(ck), P(child33), 33, P(s3), n, st)
    torch.cuda.synchronize()
    assert not bool(s1.any()) and not bool(s2.any()) and not bool(s3.any())
    hd.derive_pub_dev(P(pk33), P(cc), n, P(idx), P(out33), P(occ2), P(s1), n, st)
    cv.seckey_tweak_add_dev(P(keys), P(tw), P(tk), P(s2), n, st)
    cv.public_key_dev(P(tk), P(out33b), 33, P(s3), n, st)
    torch.cuda.synchronize()
    assert not bool(s1.any()) and bool((out33 == child33).all()) and bool((occ == occ2).all()) and not bool(s2.any()) and not bool(s3.any())
    cv.pubkey_tweak_add_dev(P(pk33), 33, P(tw), P(out33), 33, P(s1), n, st)
    torch.cuda.synchronize()
    assert not bool(s1.any()) and bool((out33 == out33b).all())

    def decompress_then(fn):
        def run():
            cv.decompress_dev(P(pk33), 33, P(xy), P(s2), n, st)
            fn()
        return run

    for npass in range(2):
        pair("tweak", npass, ("pubkey_tweak_add_dev_33", "decompress_dev_33+mul_base_dev"), [
            lambda: cv.pubkey_tweak_add_dev(P(pk33), 33, P(tw), P(out33), 33, P(s1), n, st),
            decompress_then(lambda: cv.mul_base_dev(P(tw_limbs), P(xy2), P(s3), n, st))])
        pair("tweak-emulation", npass, ("pubkey_tweak_add_dev_33", "decompress_dev_33+double_mul_dev(t,1,P)"), [
            lambda: cv.pubkey_tweak_add_dev(P(pk33), 33, P(tw), P(out33), 33, P(s1), n, st),
            decompress_then(lambda: cv.double_mul_dev(P(tw_limbs), P(one), P(xy), P(xy2), P(s3), n, st))])
        pair("derive-pub", npass, ("bip32_derive_pub_dev", "pubkey_tweak_add_dev_33"), [
            lambda: hd.derive_pub_dev(P(pk33), P(cc), n, P(idx), P(out33), P(occ2), P(s1), n, st),
            lambda: cv.pubkey_tweak_add_dev(P(pk33), 33, P(tw), P(out33b), 33, P(s3), n, st)])
        pair("derive-pub-shared", npass, ("bip32_derive_pub_dev_n_par_1", "mul_base_dev"), [
            lambda: hd.derive_pub_dev(P(pk33), P(cc), 1, P(idx), P(out33), P(occ2), P(s1), n, st),
            lambda: cv.mul_base_dev(P(tw_limbs), P(xy2), P(s3), n, st)])
        pair("derive-priv", npass, ("bip32_derive_priv_dev", "public_key_dev_33"), [
            lambda: hd.derive_priv_dev(P(keys), P(cc), n, P(idx), 0, P(ck), P(occ), P(s1), n, st),
            lambda: cv.public_key_dev(P(keys), P(out33b), 33, P(s3), n, st)])
        pair("derive-priv-hardened", npass, ("bip32_derive_priv_dev_no_comb", "sha512_dev_64B"), [
            lambda: hd.derive_priv_dev(P(keys), P(cc), n, P(hard), L.CANON_BIP32_NO_COMB, P(ck), P(occ), P(s1), n, st),
            lambda: lib.fec_sha512_dev(h, P(msg64), P(off64), 64 * n, P(dg64), P(s3), n, st)], compressions=(4, 1))
        torch.cuda.synchronize()
        assert not bool(s1.any()) and not bool(s3.any())
    p = lambda a: a.ctypes.data  # noqa: E731
    pk_h = pk33.cpu().numpy()
    o33, o32, occ_h, st_h = np.zeros((n, 33), np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    for name, fn in (("pubkey_tweak_add_33", lambda: lib.fec_canon_pubkey_tweak_add(h, 0, p(pk_h), 33, p(tw_h), p(o33), 33, p(st_h), n)),
                     ("bip32_derive_pub", lambda: lib.fec_canon_bip32_derive_pub(h, p(pk_h), p(cc_h), n, p(idx_h), p(o33), p(occ_h), p(st_h), n)),
                     ("bip32_derive_pub_n_par_1", lambda: lib.fec_canon_bip32_derive_pub(h, p(pk_h), p(cc_h), 1, p(idx_h), p(o33), p(occ_h), p(st_h), n)),
                     ("bip32_derive_priv", lambda: lib.fec_canon_bip32_derive_priv(h, p(keys_h), p(cc_h), n, p(idx_h), 0, p(o32), p(occ_h), p(st_h), n))):
        assert fn() == 0
        ms, spread = _timed(fn, reps)
        emit({"row": "host-" + name, "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4), "M_per_s": round(n / ms / 1e3, 3)})
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_wallet():
    from forge_ec_amd.canon import CanonBip32, CanonKeccak
    logn = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    n = 1 << logn
    ctx = F.Context(0)
    lib, h = ctx._lib, ctx._h
    rng = np.random.default_rng(23)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    # the comparator library: another build beside this one, with a ctx of its own
    base_lib, base_h, base_name = lib, h, "this build"
    if os.environ.get("FEC_AB_LIB"):
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        base_lib = ctypes.CDLL(os.path.abspath(os.environ["FEC_AB_LIB"]))
        base_lib.fec_ctx_create.argtypes = [ctypes.POINTER(vp), ci]
        base_lib.fec_ctx_destroy.argtypes = [vp]
        base_lib.fec_ctx_destroy.restype = None
        base_lib.fec_canon_bip32_derive_pub_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
        base_lib.fec_canon_pubkey_tweak_add_dev.argtypes = [vp, ci, vp, sz, vp, vp, sz, vp, sz, vp]
        base_lib.fec_sha256_dev.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp]
        hh = vp()
        assert base_lib.fec_ctx_create(ctypes.byref(hh), 0) == 0
        base_h, base_name = hh, os.path.basename(os.environ["FEC_AB_LIB"])

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def rounds(fns):
        """each of fns three times, alternating; per fn the middle round's median and the largest spread"""
        got = [[] for _ in fns]
        for _ in range(3):
            for g, fn in zip(got, fns):
                g.append(_timed(fn, reps))
        return [(sorted(g)[1][0], max(x[1] for x in g)) for g in got]

    def pair(row, npass, names, fns, **extra):
        a, b = rounds(fns)
        emit(dict({"row": row, "pass": npass, "n": n, "reps": reps, names[0] + "_ms": round(a[0], 4), names[0] + "_spread_ms": round(a[1], 4),
                   names[1] + "_ms": round(b[0], 4), names[1] + "_spread_ms": round(b[1], 4), "ratio": round(a[0] / b[0], 4),
                   "M_per_s": round(n / a[0] / 1e3, 3)}, **extra))

    cv, hd, hs = CANON_CURVES["secp256k1"](ctx), CanonBip32(ctx), CanonKeccak(ctx)
    keys_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    keys_h[:, 0] &= 0x7F
    keys_h[:, 31] |= 1
    cc_h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    idx_h = rng.integers(0, 1 << 31, size=(n, 3), dtype=np.uint32)
    msg64_h = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    keys, cc, msg64 = dev(keys_h), dev(cc_h), dev(msg64_h)
    idx3, idx2 = dev(idx_h), dev(idx_h[:, :2])
    col = [dev(idx_h[:, j]) for j in range(3)]
    off64 = torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device="cuda")
    pk33, ka, kb, out33 = (torch.empty((n, 33), dtype=torch.uint8, device="cuda") for _ in range(4))
    ca, cb, occ, x32, t32, q32, q32b, dg32 = (torch.empty((n, 32), dtype=torch.uint8, device="cuda") for _ in range(8))
    fp, fpb = (torch.empty((n, 4), dtype=torch.uint8, device="cuda") for _ in range(2))
    h20, h20b = (torch.empty((n, 20), dtype=torch.uint8, device="cuda") for _ in range(2))
    s1, s2, par = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3))
    P = lambda t: t.data_ptr()  # noqa: E731
    cv.public_key_dev(P(keys), P(pk33), 33, P(s1), n, st)
    torch.cuda.synchronize()
    assert not bool(s1.any())

    def chain(depth, L=None, hh=None):
        """depth chained derive_pub_dev calls: the last level's parent is left in ka or kb, the child in the other"""
        L, hh = L or lib, hh or h
        src, scc = (pk33, cc)
        bufs = [(ka, ca), (kb, cb)]
        for level in range(depth):
            dk, dc = bufs[level & 1]
            rc = L.fec_canon_bip32_derive_pub_dev(hh, P(src), P(scc), n, P(col[level]), P(dk), P(dc), P(s2), n, st)
            assert rc == 0
            src, scc = dk, dc
        return src, scc

    # what the timed calls must agree on
    for depth, ix in ((2, idx2), (3, idx3)):
        hd.derive_pub_path_dev(P(pk33), P(cc), n, P(ix), depth, P(out33), P(occ), P(fp), P(h20), P(s1), n, st)
        child, ccc = chain(depth)
        parent = kb if child is ka else ka
        hs.pubkey_hash160_dev(P(child), 33, P(h20b), n, st)
        torch.cuda.synchronize()
        assert not bool(s1.any()) and not bool(s2.any()) and bool((out33 == child).all()) and bool((occ == ccc).all()) and bool((h20 == h20b).all())
        hs.pubkey_hash160_dev(P(parent), 33, P(h20b), n, st)
        torch.cuda.synchronize()
        assert bool((fp == h20b[:, :4]).all())
    x32.copy_(pk33[:, 1:])
    tag = np.frombuffer(__import__("hashlib").sha256(b"TapTweak").digest() * 2, dtype=np.uint8)
    pre96 = torch.cat([torch.from_numpy(tag.copy()).cuda().expand(n, 64), x32], dim=1).contiguous()
    pre128 = torch.cat([pre96, cc.view(n, 32)], dim=1).contiguous()
    off96 = torch.arange(0, 96 * (n + 1), 96, dtype=torch.int64, device="cuda")
    off128 = torch.arange(0, 128 * (n + 1), 128, dtype=torch.int64, device="cuda")
    for roots, pre, off, width in ((None, pre96, off96, 96), (cc, pre128, off128, 128)):
        assert lib.fec_sha256_dev(h, P(pre), P(off), width * n, P(t32), P(s2), n, st) == 0
        cv.pubkey_tweak_add_dev(P(x32), 32, P(t32), P(q32b), 32, P(s2), n, st)
        cv.taproot_output_key_dev(P(x32), 32, P(roots) if roots is not None else None, P(q32), P(par), P(s1), n, st)
        torch.cuda.synchronize()
        assert not bool(s1.any()) and not bool(s2.any()) and bool((q32 == q32b).all())

    for npass in range(2):
        for depth, ix in ((2, idx2), (3, idx3)):
            pair("path-depth%d" % depth, npass, ("bip32_derive_pub_path_dev", "%d_chained_bip32_derive_pub_dev" % depth), [
                lambda: hd.derive_pub_path_dev(P(pk33), P(cc), n, P(ix), depth, P(out33), P(occ), None, None, P(s1), n, st),
                lambda: chain(depth, base_lib, base_h)], chain_library=base_name)
        both_null = lambda: hd.derive_pub_path_dev(P(pk33), P(cc), n, P(idx2), 2, P(out33), P(occ), None, None, P(s1), n, st)  # noqa: E731
        pair("path-optional", npass, ("path_dev_depth2_hash160", "path_dev_depth2_both_null"), [
            lambda: hd.derive_pub_path_dev(P(pk33), P(cc), n, P(idx2), 2, P(out33), P(occ), None, P(h20), P(s1), n, st), both_null])
        pair("path-optional", npass, ("path_dev_depth2_fingerprints", "path_dev_depth2_both_null"), [
            lambda: hd.derive_pub_path_dev(P(pk33), P(cc), n, P(idx2), 2, P(out33), P(occ), P(fp), None, P(s1), n, st), both_null])
        pair("path-optional", npass, ("path_dev_depth2_both", "path_dev_depth2_both_null"), [
            lambda: hd.derive_pub_path_dev(P(pk33), P(cc), n, P(idx2), 2, P(out33), P(occ), P(fp), P(h20), P(s1), n, st), both_null])
        sha = lambda: base_lib.fec_sha256_dev(base_h, P(msg64), P(off64), 64 * n, P(dg32), P(s2), n, st)  # noqa: E731
        pair("hash", npass, ("ripemd160_dev_64B", "sha256_dev_64B"), [
            lambda: hs.ripemd160_dev(P(msg64), P(off64), 64 * n, P(h20), P(s1), n, st), sha], sha256_library=base_name)
        pair("hash", npass, ("hash160_dev_64B", "sha256_dev_64B"), [
            lambda: hs.hash160_dev(P(msg64), P(off64), 64 * n, P(h20), P(s1), n, st), sha], sha256_library=base_name)
        pair("hash", npass, ("pubkey_hash160_dev_33", "sha256_dev_64B"), [
            lambda: hs.pubkey_hash160_dev(P(pk33), 33, P(h20), n, st), sha], sha256_library=base_name)
        tweak_add = lambda: base_lib.fec_canon_pubkey_tweak_add_dev(base_h, 0, P(x32), 32, P(t32), P(q32b), 32, P(s2), n, st)  # noqa: E731
        pair("taproot", npass, ("taproot_output_key_dev_roots", "pubkey_tweak_add_dev_32_32"), [
            lambda: cv.taproot_output_key_dev(P(x32), 32, P(cc), P(q32), P(par), P(s1), n, st), tweak_add], tweak_add_library=base_name)
        pair("taproot", npass, ("taproot_output_key_dev_no_roots", "pubkey_tweak_add_dev_32_32"), [
            lambda: cv.taproot_output_key_dev(P(x32), 32, None, P(q32), P(par), P(s1), n, st), tweak_add], tweak_add_library=base_name)
        torch.cuda.synchronize()
        assert not bool(s1.any()) and not bool(s2.any())
    p = lambda a: a.ctypes.data  # noqa: E731
    pk_h, x_h = pk33.cpu().numpy(), x32.cpu().numpy()
    off_h = np.arange(0, 64 * (n + 1), 64, dtype=np.uint64)
    o33, o32, o20, o4, st_h, par_h = (np.zeros((n, w), np.uint8) for w in (33, 32, 20, 4, 1, 1))
    for name, fn in (("ripemd160_64B", lambda: lib.fec_canon_ripemd160(h, p(msg64_h), p(off_h), 64 * n, p(o20), n)),
                     ("hash160_64B", lambda: lib.fec_canon_hash160(h, p(msg64_h), p(off_h), 64 * n, p(o20), n)),
                     ("pubkey_hash160_33", lambda: lib.fec_canon_pubkey_hash160(h, p(pk_h), 33, p(o20), n)),
                     ("taproot_output_key_roots", lambda: lib.fec_canon_taproot_output_key(h, p(x_h), 32, p(cc_h), p(o32), p(par_h), p(st_h), n)),
                     ("bip32_derive_pub_path_depth3_all_outputs",
                      lambda: lib.fec_canon_bip32_derive_pub_path(h, p(pk_h), p(cc_h), n, p(idx_h), 3, p(o33), p(o32), p(o4), p(o20), p(st_h), n))):
        assert fn() == 0
        ms, spread = _timed(fn, reps)
        emit({"row": "host-" + name, "n": n, "reps": reps, "ms": round(ms, 4), "spread_ms": round(spread, 4), "M_per_s": round(n / ms / 1e3, 3)})
    if base_lib is not lib:
        torch.cuda.synchronize()
        base_lib.fec_ctx_destroy(base_h)
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_msm():
    max_log = int(sys.argv[2]) if len(sys.argv) > 2 else 22
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    ctx = F.Context(0)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    nmax = 1 << max_log
    gen = torch.Generator(device="cuda")
    gen.manual_seed(28)
    rand = lambda m: torch.randint(-2**63, 2**63 - 1, (m, 4), dtype=torch.int64, device="cuda", generator=gen)  # noqa: E731

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def pair(c, k, p, n, window):
        """(msm median ms, comparator median ms, status): the two calls alternate sample by sample"""
        out1 = torch.empty(8, dtype=torch.int64, device="cuda")
        st1 = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
        outn = torch.empty((n, 8), dtype=torch.int64, device="cuda")
        stn = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctx.set_canon_msm_window(window)
        fns = (lambda: c.msm_dev(k.data_ptr(), p.data_ptr(), n, out1.data_ptr(), st1.data_ptr(), st),
               lambda: c.mul_dev(k.data_ptr(), p.data_ptr(), outn.data_ptr(), stn.data_ptr(), n, st))
        samples = ([], [])
        for i in range(reps + 1):
            for smp, fn in zip(samples, fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i:
                    smp.append((time.perf_counter() - t0) * 1e3)
        ctx.set_canon_msm_window(0)
        med = [sorted(x)[len(x) // 2] for x in samples]
        return med[0], med[1], int(st1.cpu()[0])

    for cname in CANON_CURVES:
        c = CANON_CURVES[cname](ctx)
        k = rand(nmax)
        p = torch.empty((nmax, 8), dtype=torch.int64, device="cuda")
        stat = torch.empty(nmax, dtype=torch.uint8, device="cuda")
        c.mul_base_dev(rand(nmax).data_ptr(), p.data_ptr(), stat.data_ptr(), nmax, st)
        torch.cuda.synchronize()
        for logn in range(10, max_log + 1, 2):
            n = 1 << logn
            m, cmp_, status = pair(c, k, p, n, 0)
            emit({"row": "size", "curve": cname, "n": n, "window": 0, "reps": reps, "msm_ms": round(m, 4), "canon_mul_ms": round(cmp_, 4),
                  "speedup": round(cmp_ / m, 3), "M_per_s": round(n / m / 1e3, 3), "status": status})
        for sweep_log in sorted({min(18, max_log), min(20, max_log)}):
            n = 1 << sweep_log
            for window in range(8, 17):
                m, cmp_, status = pair(c, k, p, n, window)
                emit({"row": "window", "curve": cname, "n": n, "window": window, "reps": reps, "msm_ms": round(m, 4),
                      "canon_mul_ms": round(cmp_, 4), "speedup": round(cmp_ / m, 3), "status": status})
        rand_ms = None
        m, cmp_, status = pair(c, k, p, n, 0)
        rand_ms = m
        emit({"row": "skew", "input": "random", "curve": cname, "n": n, "window": 0, "reps": reps, "msm_ms": round(m, 4), "canon_mul_ms": round(cmp_, 4),
              "status": status})
        keq = k[:1].repeat(n, 1).contiguous()
        m, cmp_, status = pair(c, keq, p, n, 0)
        emit({"row": "skew", "input": "all scalars equal", "curve": cname, "n": n, "window": 0, "reps": reps, "msm_ms": round(m, 4),
              "canon_mul_ms": round(cmp_, 4), "over_random": round(m / rand_ms, 3), "status": status})
        p1 = p[:1].repeat(n, 1).contiguous()
        m, cmp_, status = pair(c, k, p1, n, 0)
        emit({"row": "skew", "input": "one point", "curve": cname, "n": n, "window": 0, "reps": reps, "msm_ms": round(m, 4),
              "canon_mul_ms": round(cmp_, 4), "over_random": round(m / rand_ms, 3), "status": status})
        del k, p, stat, keq, p1
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_batch():
    max_log = int(sys.argv[2]) if len(sys.argv) > 2 else 22
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    ctx = F.Context(0)
    st = torch.cuda.current_stream().cuda_stream
    rows, mlen = [], 32
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    seed = bytes(range(32))

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for scheme, cname in (("bip340", "secp256k1"), ("ed25519", "ed25519")):
        c = CANON_CURVES[cname](ctx)
        batch = c.bip340_batch_verify_msg_dev if scheme == "bip340" else c.ed25519_batch_verify_msg_dev
        single = c.bip340_verify_msg_dev if scheme == "bip340" else c.ed25519_verify_msg_dev
        nmax = 1 << max_log
        try:     # 2^22 only where the signatures fit
            msgs = torch.randint(0, 256, (nmax * mlen,), dtype=torch.uint8, device="cuda", generator=gen)
            off = (torch.arange(nmax + 1, dtype=torch.int64, device="cuda") * mlen)
            keys = torch.randint(0, 256, (nmax, 32), dtype=torch.uint8, device="cuda", generator=gen)
            keys[:, 0] &= 0x7F        # a BIP-340 key below n
            keys[:, 31] |= 1          # ... and not zero
            sigs = torch.empty((nmax, 64), dtype=torch.uint8, device="cuda")
            pks = torch.empty((nmax, 32), dtype=torch.uint8, device="cuda")
            stat = torch.empty(nmax, dtype=torch.uint8, device="cuda")
            res = torch.empty(nmax, dtype=torch.uint8, device="cuda")
            verdict = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
            if scheme == "bip340":
                aux = torch.zeros((nmax, 32), dtype=torch.uint8, device="cuda")
                c.bip340_sign_msg_dev(msgs.data_ptr(), off.data_ptr(), nmax * mlen, keys.data_ptr(), aux.data_ptr(), sigs.data_ptr(), stat.data_ptr(), nmax, st)
                torch.cuda.synchronize()
                assert int(stat.count_nonzero()) == 0
                c.public_key_dev(keys.data_ptr(), pks.data_ptr(), 32, stat.data_ptr(), nmax, st, scheme=3)
            else:
                c.ed25519_sign_msg_dev(msgs.data_ptr(), off.data_ptr(), nmax * mlen, keys.data_ptr(), sigs.data_ptr(), pks.data_ptr(), stat.data_ptr(), nmax, st)
            torch.cuda.synchronize()
            assert int(stat.count_nonzero()) == 0
        except torch.cuda.OutOfMemoryError:
            emit({"row": "skipped", "scheme": scheme, "max_log": max_log, "why": "the signatures do not fit"})
            continue

        def pair(n, sg):
            """(batch median ms, per-signature median ms, spreads): the two calls alternate sample by sample"""
            fns = (lambda: batch(msgs.data_ptr(), off.data_ptr(), n * mlen, sg.data_ptr(), pks.data_ptr(), seed, stat.data_ptr(), verdict.data_ptr(), n, st),
                   lambda: single(msgs.data_ptr(), off.data_ptr(), n * mlen, sg.data_ptr(), pks.data_ptr(), res.data_ptr(), n, st))
            samples = ([], [])
            for i in range(reps + 1):
                for smp, fn in zip(samples, fns):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if i:
                        smp.append((time.perf_counter() - t0) * 1e3)
            srt = [sorted(x) for x in samples]
            return srt[0][len(srt[0]) // 2], srt[1][len(srt[1]) // 2], srt[0][-1] - srt[0][0], srt[1][-1] - srt[1][0]

        sizes = list(range(10, min(max_log, 20) + 1)) + ([max_log] if max_log > 20 else [])
        for logn in sizes:
            n = 1 << logn
            b, s, bs, ss = pair(n, sigs)
            ok = int(verdict.cpu()[0]) == 1 and int(stat[:n].count_nonzero()) == 0 and int(res[:n].sum()) == n
            emit({"row": "size", "scheme": scheme, "n": n, "msg_bytes": mlen, "reps": reps, "batch_ms": round(b, 4), "batch_spread_ms": round(bs, 4),
                  "single_ms": round(s, 4), "single_spread_ms": round(ss, 4), "single_over_batch": round(s / b, 3),
                  "batch_M_per_s": round(n / b / 1e3, 3), "single_M_per_s": round(n / s / 1e3, 3), "all_valid": ok})
        # every element refused (s = 2^256 - 1): what the batch call costs when the sum is 2 n + 1 times 0 * G
        n = 1 << min(max_log, 20)
        bad = sigs[:n].clone()
        bad[:, 32:] = 255
        b, s, bs, ss = pair(n, bad)
        emit({"row": "all-refused", "scheme": scheme, "n": n, "msg_bytes": mlen, "reps": reps, "batch_ms": round(b, 4), "batch_spread_ms": round(bs, 4),
              "single_ms": round(s, 4), "single_over_batch": round(s / b, 3), "verdict": int(verdict.cpu()[0]),
              "every_status_3": int((stat[:n] == 3).sum()) == n})
        del msgs, off, keys, sigs, pks, stat, res, bad
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main():
    logn = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    curves = sys.argv[3].split(",") if len(sys.argv) > 3 else list(CANON_CURVES)
    n = 1 << logn
    ctx = F.Context(0)
    ctx.set_timing(True)
    st = torch.cuda.current_stream().cuda_stream
    k = torch.from_numpy(synth.scalars(n, 0, 41).view(np.int64)).cuda()
    k2 = torch.from_numpy(synth.scalars(n, 0, 42).view(np.int64)).cuda()
    k3 = torch.from_numpy(synth.scalars(n, 0, 43).view(np.int64)).cuda()
    k4 = torch.from_numpy(synth.scalars(n, 0, 44).view(np.int64)).cuda()
    pub = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    for cname in curves:
        c = CANON_CURVES[cname](ctx)
        extra = {"secp256k1": ("ecdsa-verify", "bip340-verify"), "p256": ("ecdsa-verify",), "ed25519": ("eddsa-verify",)}[cname]
        for name in ("keygen", "ecdh", "double-mul") + extra:
            best = None
            for _ in range(reps + 1):
                if name == "keygen":
                    c.mul_base_dev(k.data_ptr(), pub.data_ptr(), status.data_ptr(), n, st)
                    ms, kern = ctx.last_kernel_ms()
                elif name == "ecdh":
                    c.mul_dev(k2.data_ptr(), pub.data_ptr(), out.data_ptr(), status.data_ptr(), n, st)
                    ms, kern = ctx.last_kernel_ms()
                elif name == "ecdsa-verify":  # scalars + comb + accumulate + normalise + compare, wall clock
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    c.ecdsa_verify_dev(k.data_ptr(), k2.data_ptr(), k3.data_ptr(), pub.data_ptr(), status.data_ptr(), n, st)
                    torch.cuda.synchronize()
                    ms, kern = (time.perf_counter() - t0) * 1e3, "k_canon_ecdsa_scalars + comb + accumulate + normalize + finish"
                elif name in ("bip340-verify", "eddsa-verify"):  # prepare (decode / lift_x) + double-mul + final test
                    fn = c.bip340_verify_dev if name == "bip340-verify" else c.eddsa_verify_dev
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(k.data_ptr(), k2.data_ptr(), k3.data_ptr(), k4.data_ptr(), status.data_ptr(), n, st)
                    torch.cuda.synchronize()
                    ms, kern = (time.perf_counter() - t0) * 1e3, "prepare + comb + accumulate + normalize + finish"
                else:  # u1*G + u2*P: three launches on the ctx stream; wall clock around a device sync
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    c.double_mul_dev(k.data_ptr(), k2.data_ptr(), pub.data_ptr(), out.data_ptr(), status.data_ptr(), n, st)
                    torch.cuda.synchronize()
                    ms, kern = (time.perf_counter() - t0) * 1e3, "k_canon_mul_base + k_canon_mul<accum> + k_canon_normalize"
                best = ms if best is None or ms < best else best
            torch.cuda.synchronize()
            assert name.endswith("-verify") or int(status.sum()) == 0
            rate = n / (best * 1e-3)
            print(json.dumps({"workload": "%s-canon-%s" % (cname, name), "mode": "canonical math, NOT reference parity",
                              "n": n, "kernel": kern, "ms": round(best, 4), "M_per_s": round(rate / 1e6, 3)}),
                  flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "msg":
    main_msg()
elif len(sys.argv) > 1 and sys.argv[1] == "sign":
    main_sign()
elif len(sys.argv) > 1 and sys.argv[1] == "x25519":
    main_x25519()
elif len(sys.argv) > 1 and sys.argv[1] == "recover":
    main_recover()
elif len(sys.argv) > 1 and sys.argv[1] == "bip32":
    main_bip32()
elif len(sys.argv) > 1 and sys.argv[1] == "wallet":
    main_wallet()
elif len(sys.argv) > 1 and sys.argv[1] == "msm":
    main_msm()
elif len(sys.argv) > 1 and sys.argv[1] == "batch":
    main_batch()
else:
    main()
