"""
GPU tests of parity mode's call order across streams: pairs and chains of *_dev calls of ONE ctx on two user streams (and
the ctx's own, stream = NULL) with no synchronisation between the calls, every output compared with the C restatement (the
`oracle` fixture) or with the compositions over it that the other GPU tests use (ecdsa_sign_ref, schnorr_sign_ref,
eddsa_sign_ref, eddsa_verify_ref, bip340_sign_ref, rfc6979_ref, ecdh_kdf_ref, h2c_ref, x25519_ref, hashlib), never with
another GPU run.  The construction of tests/test_gpu_canon_streams.py, for the other half of the library.

include/fecgpu.h promises that the launches of one ctx execute in call order whatever streams they name.  Parity mode
leans on the promise in four places: the Ed25519 addend table (ctx->d_ed_table) belongs to the ctx and is rebuilt for every
base of the caller's own; product_pair forks the fixed-base product of the verifiers, of double_mul and of ecdh_exchange
onto the ctx's one side stream (ctx->stream2); the device error word is shared; and a caller may feed one call's output
tensor to the next call on another stream.  tests/test_parity_launch_order.py holds the promise on the text of fecgpu.hip;
here two calls really are in flight, behind the gate of tests/stream_gate.py (its docstring says how the gate makes a
missing ordering deterministic).  launch_schnorr_sign copied the secret keys into its scratch AHEAD of its ordering: behind
a call on another stream that writes the key tensor (test_pipeline_reduced_bytes_to_schnorr_sign) the copy read the
sentinel, so P = multiply(G, sk) came from stale bytes while the nonce and the finishing pass read the real keys.

Families: (a) the users of the Ed25519 addend table behind and ahead of a rebuild for another base; (b) the calls that fork
onto ctx->stream2, on both user streams at once; (c) the calls whose scratch belongs to the stream, or that have none, on
both streams at once; (d) pipelines, every stage's output compared; (e) the first calls of a fresh ctx on user streams, a
stream = NULL call behind both user streams, and a fixture that leaves the session ctx's last launch on its own stream.
Not here: n >= 2^16 (the per-launch prefix table and the popcount sort: tests/test_gpu_size_regimes.py),
fec_ctx_set_fixed_prefix_bits from a gated call (its build synchronises the host, which the gate forbids), multi-device ctxs.

Inputs: n = 64 * 3 + 5 elements (three full wavefronts and a ragged one) cycling eight model-computed records per call;
call A starts the cycle at record 0 and call B at record 3, so their inputs and expected outputs differ at every element
(status bytes: wherever the eight records' statuses differ; the verifiers' records are picked from a pool so that they mix
what the reference accepts and rejects).  Messages have the eight lengths of the canonical module.  Outputs are pre-filled
with a sentinel.

Sizing of the gate, measured on an MI355X after warm-up (each run prints both figures under -s): the parity launchers do
more on the host than the canonical ones (a WorkArea request, the events of the side stream's fork and join), and still the
host issues a pair of calls in 0.02 - 0.20 ms (median 0.04 ms) and the three-call chains in 0.03 - 0.12 ms; the longest
issue seen in the module's 169 gated runs was 0.54 ms, once (batch_mul_dev -> batch_to_affine_dev -> batch_compress_dev,
0.03 ms in its other runs: a hiccup of the host).  FILL_STEPS = 64 matmuls of 2048^2 in fp32 take 7.7 - 9.9 ms: fourteen
times the longest issue and forty times the longest that repeats, so the canonical module's step count stands here.  The
two event assertions check the sizing on every run.  The module's 170 tests take about 7 s together, none more than 0.4 s
(the first one also pays for the session's ctx and the gate's streams).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import bip340_sign_ref as B340
import ecdh_kdf_ref as K
import ecdsa_sign_ref as ES
import eddsa_sign_ref as EdS
import eddsa_verify_ref as EdV
import h2c_ref as H
import rfc6979_ref as RF
import schnorr_sign_ref as SS
import vectors as V
import x25519_ref as X
from stream_gate import Call, Gate, ptr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = 64 * 3 + 5
NREC = 8
ROT_A, ROT_B = 0, 3
FILL_DIM, FILL_STEPS = 2048, 64
SECP, P256, ED = 0, 1, 2
NAMES = {SECP: "secp256k1", P256: "p256", ED: "ed25519"}
LENGTHS = [1, 31, 55, 64, 135, 136, 137, 200]   # message lengths of the eight records: either side of the hashes' block edges
INFO, DST = b"call order, 21 bytes.", H.dst_of(21)
FILL = 0xEE

GATE = Gate(FILL_DIM, FILL_STEPS)
_run = GATE.run

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- records and tensors -------------------------------------------------------------------------------------------------
def ix(rot):
    return (np.arange(N) + rot) % NREC


def cyc(a, rot):
    """the eight records `a` (an array, one row each) as the N rows of a call that starts the cycle at `rot`"""
    a = np.asarray(a)
    return np.ascontiguousarray(a[ix(rot)])


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def up_cyc(a, rot):
    return up(cyc(a, rot))


def messages(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=L_, dtype=np.uint8).tobytes() for L_ in LENGTHS]


def up_msgs(msgs, rot):
    msgs = [msgs[i] for i in ix(rot)]
    off = np.zeros(N + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return up(np.frombuffer(b"".join(msgs), dtype=np.uint8)), up(off), int(off[-1])


def out(width):
    """an output of `width` bytes per element, pre-filled with the sentinel"""
    import torch
    return torch.full((N, width), FILL, dtype=torch.uint8, device="cuda"), FILL


def status():
    import torch
    return torch.full((N, 1), 9, dtype=torch.uint8, device="cuda"), 9


def u8(rows_):
    return np.array([list(bytes(r)) for r in rows_], dtype=np.uint8)


def u64(a, w):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).reshape(-1, w)


def pick(st, what, one_status=False):
    """NREC indices into a pool whose model statuses are `st`: the statuses in turn, as even a mix as the pool allows.
    one_status: the reference is known to give this pool one answer (then the sentinel alone tells a written status)"""
    st = [int(v) for v in st]
    groups = {v: [i for i, s in enumerate(st) if s == v] for v in sorted(set(st), reverse=True)}
    assert one_status or len(groups) >= 2, "%s: the model gives one status for the whole pool" % what
    chosen = []
    while len(chosen) < NREC:
        for v in groups:
            if groups[v] and len(chosen) < NREC:
                chosen.append(groups[v].pop(0))
    return np.array(chosen)


def scalars_below_order(c, seed):
    """keys the signers accept: [1, n) and below 2^255"""
    k = V.scalars(NREC, c, seed)
    k[:, 3] >>= np.uint64(1)
    k[:, 0] |= np.uint64(1)
    return k


def true_points(oracle, c, seed):
    """affine multiples of the generator under the reference's own arithmetic"""
    xy, inf = oracle.batch_to_affine(c, oracle.batch_mul_fixed(c, V.scalars(NREC, c, seed), oracle.generator(c)))
    assert not inf.any()
    return xy


def p256_curve_points(n, seed):
    import random
    rng = random.Random(seed)
    rows_ = []
    while len(rows_) < n:
        x = rng.randrange(K.P256_P)
        rhs = (x * x * x - 3 * x + K.P256_B) % K.P256_P
        y = pow(rhs, (K.P256_P + 1) // 4, K.P256_P)
        if y * y % K.P256_P == rhs:
            rows_.append(K.limbs(x) + K.limbs(y))
    return np.array(rows_, dtype=np.uint64)


# ---- the calls: each f(ctx, oracle, rot, ...) -> Call ----------------------------------------------------------------------
def c_mul(ctx, oracle, rot, c):
    k, p = V.scalars(NREC, c, 3101), V.points(NREC, c, 3102)
    want = cached(("mul", c), lambda: oracle.batch_mul(c, k, p))
    dk, dp, o = up_cyc(k, rot), up_cyc(p, rot), out(8 * V.POINT_LIMBS[c])
    return Call("batch_mul_dev " + NAMES[c], lambda st: ctx.batch_mul_dev(c, dk.data_ptr(), dp.data_ptr(), o[0].data_ptr(), N, ptr(st)),
                [o], [cyc(want, rot)])


def c_mul_fixed(ctx, oracle, rot, c, base):
    """base: "G" (the ctx's generator) or the name of a base of the caller's own"""
    seed = 3110 + sum(map(ord, base))
    k = V.scalars(NREC, c, seed)
    b = oracle.generator(c) if base == "G" else V.points(1, c, seed + 1)[0]
    want = cached(("mul_fixed", c, base), lambda: oracle.batch_mul_fixed(c, k, b))
    dk, o = up_cyc(k, rot), out(8 * V.POINT_LIMBS[c])
    db = None if base == "G" else up(b)
    at = ctx.generator_dev(c) if base == "G" else db.data_ptr()
    call = Call("batch_mul_fixed_dev %s base %s" % (NAMES[c], base), lambda st: ctx.batch_mul_fixed_dev(c, dk.data_ptr(), at, o[0].data_ptr(), N, ptr(st)),
                [o], [cyc(want, rot)])
    call.keep = db
    return call


def c_double_mul(ctx, oracle, rot, c):
    u1, u2, q = V.scalars(NREC, c, 3121), V.scalars(NREC, c, 3122), V.points(NREC, c, 3123)
    want = cached(("double_mul", c), lambda: oracle.batch_double_mul(c, u1, u2, q))
    a, b, dq, o = up_cyc(u1, rot), up_cyc(u2, rot), up_cyc(q, rot), out(8 * V.POINT_LIMBS[c])
    return Call("batch_double_mul_dev " + NAMES[c],
                lambda st: ctx.batch_double_mul_dev(c, a.data_ptr(), b.data_ptr(), dq.data_ptr(), o[0].data_ptr(), N, ptr(st)), [o], [cyc(want, rot)])


def c_to_affine(ctx, oracle, rot, c):
    p = cached(("to_affine in", c), lambda: oracle.batch_mul(c, V.scalars(NREC, c, 3131), V.points(NREC, c, 3132)))
    wxy, winf = cached(("to_affine", c), lambda: oracle.batch_to_affine(c, p))
    dp, xy, inf = up_cyc(p, rot), out(64), out(1)
    return Call("batch_to_affine_dev " + NAMES[c], lambda st: ctx.batch_to_affine_dev(c, dp.data_ptr(), xy[0].data_ptr(), inf[0].data_ptr(), N, ptr(st)),
                [xy, inf], [cyc(wxy, rot), cyc(winf, rot)])


def c_compress(ctx, oracle, rot, c):
    xy = V.field_elements(2 * NREC, c, 3141).reshape(NREC, 8)
    inf = np.array([0, 0, 1, 0, 0, 0, 0, 1], dtype=np.uint8)
    want = cached(("compress", c), lambda: oracle.batch_compress(c, xy, inf))
    dxy, dinf, o = up_cyc(xy, rot), up_cyc(inf, rot), out(33)
    return Call("batch_compress_dev " + NAMES[c], lambda st: ctx.batch_compress_dev(c, dxy.data_ptr(), dinf.data_ptr(), o[0].data_ptr(), N, ptr(st)),
                [o], [cyc(want, rot)])


def _validate_records(oracle, c):
    pool = 32
    xy = np.ascontiguousarray(np.concatenate([V.field_elements(pool, c, 3151), V.field_elements(pool, c, 3152)], axis=1))
    if c == P256:
        xy[:24] = p256_curve_points(24, 3153)            # about half pass the reference's is_on_curve
    if c == SECP:
        xy[:16] = true_points(oracle, c, 3154).repeat(2, axis=0)
    if c == ED:                                            # (0, 1) is on the curve and of order 1; so is the generator
        xy[:8, :4] = 0
        xy[:4, 4:] = np.array([1, 0, 0, 0], dtype=np.uint64)
        xy[8:16] = true_points(oracle, c, 3155)
    inf = np.zeros(pool, dtype=np.uint8)
    inf[5::7] = 1
    ok = oracle.batch_validate_point(c, xy, inf, nthreads=8)
    at = pick(ok, "validate_point " + NAMES[c])
    return xy[at], inf[at], ok[at]


def c_validate(ctx, oracle, rot, c):
    xy, inf, ok = cached(("validate", c), lambda: _validate_records(oracle, c))
    dxy, dinf, o = up_cyc(xy, rot), up_cyc(inf, rot), status()
    return Call("batch_validate_point_dev " + NAMES[c],
                lambda st: ctx.batch_validate_point_dev(c, dxy.data_ptr(), dinf.data_ptr(), o[0].data_ptr(), N, ptr(st)), [o], [cyc(ok, rot)])


def _ecdh_records(oracle, c):
    sk, pk, inf = K.planted_batch(c, n=32, seed=0x57EA)
    sk[3] = 0
    sec, st = oracle.batch_ecdh(c, sk, pk, inf, nthreads=8)
    at = pick(st, "ecdh " + NAMES[c])
    return sk[at], pk[at], inf[at]


def c_ecdh(ctx, oracle, rot, c):
    sk, pk, inf = cached(("ecdh in", c), lambda: _ecdh_records(oracle, c))
    wsec, wst = cached(("ecdh", c), lambda: oracle.batch_ecdh(c, sk, pk, inf))
    a, b, f, sec, st_ = up_cyc(sk, rot), up_cyc(pk, rot), up_cyc(inf, rot), out(32), status()
    return Call("batch_ecdh_dev " + NAMES[c],
                lambda st: ctx.batch_ecdh_dev(c, a.data_ptr(), b.data_ptr(), f.data_ptr(), sec[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [sec, st_], [cyc(wsec, rot), cyc(wst, rot)])


def c_ecdh_derive_key(ctx, oracle, rot, c):
    sk, pk, inf = cached(("ecdh in", c), lambda: _ecdh_records(oracle, c))
    wk, wst = cached(("ecdh_derive_key", c), lambda: K.ecdh_derive_key(oracle, c, sk, pk, inf, INFO, 33))
    a, b, f, keys, st_ = up_cyc(sk, rot), up_cyc(pk, rot), up_cyc(inf, rot), out(33), status()
    return Call("ecdh_derive_key_dev " + NAMES[c],
                lambda st: ctx.ecdh_derive_key_dev(c, a.data_ptr(), b.data_ptr(), f.data_ptr(), INFO, 33, keys[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [keys, st_], [cyc(wk, rot), cyc(wst, rot)])


def c_ecdh_exchange(ctx, oracle, rot, c):
    sk, pk, inf = cached(("ecdh in", c), lambda: _ecdh_records(oracle, c))
    wxy, winf, wk, wst = cached(("ecdh_exchange", c), lambda: K.exchange(oracle, c, sk, pk, inf, INFO, 33))
    a, b, f = up_cyc(sk, rot), up_cyc(pk, rot), up_cyc(inf, rot)
    pub, pinf, keys, st_ = out(64), out(1), out(33), status()
    return Call("ecdh_exchange_dev " + NAMES[c],
                lambda st: ctx.ecdh_exchange_dev(c, a.data_ptr(), b.data_ptr(), f.data_ptr(), INFO, 33, pub[0].data_ptr(), pinf[0].data_ptr(),
                                                 keys[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [pub, pinf, keys, st_], [cyc(wxy, rot), cyc(winf, rot), cyc(wk, rot), cyc(wst, rot)])


def c_derive_key(ctx, oracle, rot, c):
    sec = np.random.default_rng(3161 + c).integers(0, 256, size=(NREC, 32), dtype=np.uint8)
    want = cached(("derive_key", c), lambda: u8([K.derive_key(c, bytes(s), INFO, 33) for s in sec]))
    a, keys = up_cyc(sec, rot), out(33)
    return Call("derive_key_dev " + NAMES[c], lambda st: ctx.derive_key_dev(c, a.data_ptr(), 32, INFO, 33, keys[0].data_ptr(), N, ptr(st)),
                [keys], [cyc(want, rot)])


def c_ecdsa_sign(ctx, oracle, rot, c):
    sk, k = scalars_below_order(c, 3171), scalars_below_order(c, 3172)
    d = np.random.default_rng(3173 + c).integers(0, 256, size=(NREC, 32), dtype=np.uint8)
    d[5] = 0xFF                                            # a digest >= n
    sk[6] = 0                                              # Err(InvalidPrivateKey)
    r, s, wst = cached(("ecdsa_sign", c), lambda: ES.sign(oracle, c, sk, d, k))
    a, b, e, sig, st_ = up_cyc(sk, rot), up_cyc(d, rot), up_cyc(k, rot), out(64), status()
    return Call("ecdsa_sign_dev " + NAMES[c],
                lambda st: ctx.ecdsa_sign_dev(c, a.data_ptr(), b.data_ptr(), e.data_ptr(), sig[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [sig, st_], [cyc(np.concatenate([r, s], axis=1), rot), cyc(wst, rot)])


def c_ecdsa_sign_msg(ctx, oracle, rot, c):
    sk, msgs = scalars_below_order(c, 3181), messages(3182 + c)
    r, s, wst, _ = cached(("ecdsa_sign_msg", c), lambda: RF.sign_msg(oracle, c, sk, msgs))
    a, (m, off, total), sig, st_ = up_cyc(sk, rot), up_msgs(msgs, rot), out(64), status()
    return Call("ecdsa_sign_msg_dev " + NAMES[c],
                lambda st: ctx.ecdsa_sign_msg_dev(c, a.data_ptr(), m.data_ptr(), off.data_ptr(), total, sig[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [sig, st_], [cyc(np.concatenate([r, s], axis=1), rot), cyc(wst, rot)])


def c_rfc6979(ctx, oracle, rot, c):
    sk, msgs = np.random.default_rng(3191 + c).integers(0, 1 << 64, size=(NREC, 4), dtype=np.uint64), messages(3192 + c)
    want = cached(("rfc6979", c), lambda: RF.nonces(c, sk, msgs)[0])
    a, (m, off, total), k, st_ = up_cyc(sk, rot), up_msgs(msgs, rot), out(32), status()
    return Call("rfc6979_k_dev " + NAMES[c],
                lambda st: ctx.rfc6979_k_dev(c, a.data_ptr(), m.data_ptr(), off.data_ptr(), total, k[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [k, st_], [cyc(want, rot), np.zeros(N, dtype=np.uint8)])


def c_bip340_sign(ctx, oracle, rot):
    keys, msgs = np.random.default_rng(3201).integers(0, 256, size=(NREC, 32), dtype=np.uint8), messages(3202)
    keys[6] = 0xFF                                         # d >= N
    want = cached(("bip340",), lambda: B340.sign_batch(keys, msgs, B340.CBackend(8)))
    a, (m, off, total), sig, st_ = up_cyc(keys, rot), up_msgs(msgs, rot), out(64), status()
    return Call("bip340_sign_dev",
                lambda st: ctx.bip340_sign_dev(a.data_ptr(), m.data_ptr(), off.data_ptr(), total, sig[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [sig, st_], [cyc(u8([w[0] for w in want]), rot), cyc(np.array([w[1] for w in want], dtype=np.uint8), rot)])


def schnorr_sign_call(ctx, c, d_sk, msgs, rot, want):
    """fec_schnorr_sign_msg_dev on the key tensor d_sk; want: schnorr_sign_ref.sign_many of the eight records"""
    (m, off, total), r, rinf, s, sb, st_ = up_msgs(msgs, rot), out(64), out(1), out(32), out(64), status()
    call = Call("schnorr_sign_msg_dev " + NAMES[c],
                lambda st: ctx.schnorr_sign_msg_dev(c, d_sk.data_ptr(), m.data_ptr(), off.data_ptr(), total, r[0].data_ptr(), rinf[0].data_ptr(),
                                                    s[0].data_ptr(), sb[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [r, rinf, s, sb, st_], [cyc(want[k], rot) for k in ("r_xy", "r_inf", "s", "sig_bytes", "status")])
    call.names = ("r_xy", "r_inf", "s", "sig_bytes", "status")
    return call


def c_schnorr_sign(ctx, oracle, rot, c):
    sk, msgs = np.random.default_rng(3211 + c).integers(0, 1 << 64, size=(NREC, 4), dtype=np.uint64), messages(3212 + c)
    want = cached(("schnorr_sign", c), lambda: SS.sign_many(c, sk, msgs))
    return schnorr_sign_call(ctx, c, up_cyc(sk, rot), msgs, rot, want)


def _challenge(oracle, c, r_xy, r_inf, pk_xy, pk_inf, msgs):
    be = SS.CBackend()
    er, ep = oracle.batch_compress(c, r_xy, r_inf), oracle.batch_compress(c, pk_xy, pk_inf)
    return u64([SS.from_bytes_reduced(c, hashlib.sha256(bytes(er[i]) + bytes(ep[i]) + msgs[i]).digest(), be.reduce_wide)[0] for i in range(len(msgs))], 4)


def c_schnorr_challenge(ctx, oracle, rot, c):
    r_xy, pk_xy, msgs = true_points(oracle, c, 3221), true_points(oracle, c, 3222), messages(3223 + c)
    r_inf, pk_inf = np.array([0, 1, 0, 0, 0, 0, 0, 0], dtype=np.uint8), np.array([0, 0, 0, 0, 1, 0, 0, 0], dtype=np.uint8)
    want = cached(("schnorr_challenge", c), lambda: _challenge(oracle, c, r_xy, r_inf, pk_xy, pk_inf, msgs))
    a, af, b, bf, (m, off, total), e, st_ = up_cyc(r_xy, rot), up_cyc(r_inf, rot), up_cyc(pk_xy, rot), up_cyc(pk_inf, rot), up_msgs(msgs, rot), out(32), status()
    return Call("schnorr_challenge_dev " + NAMES[c],
                lambda st: ctx.schnorr_challenge_dev(c, a.data_ptr(), af.data_ptr(), b.data_ptr(), bf.data_ptr(), m.data_ptr(), off.data_ptr(), total,
                                                     e[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [e, st_], [cyc(want, rot), np.zeros(N, dtype=np.uint8)])


def reduced_bytes(c):
    """eight 32-byte strings for from_bytes_reduced: random, with values at and above the order among them"""
    b = np.random.default_rng(3231 + c).integers(0, 256, size=(NREC, 32), dtype=np.uint8)
    b[1, :8] = 0xFF
    b[4] = 0xFF
    b[6, :16] = 0
    return b


def _reduced(c, b):
    be = SS.CBackend()
    return u64([SS.from_bytes_reduced(c, bytes(x), be.reduce_wide)[0] for x in b], 4)


def c_from_bytes_reduced(ctx, oracle, rot, c):
    b = reduced_bytes(c)
    want = cached(("reduced", c), lambda: _reduced(c, b))
    a, o = up_cyc(b, rot), out(32)
    return Call("scalar_from_bytes_reduced_dev " + NAMES[c], lambda st: ctx.scalar_from_bytes_reduced_dev(c, a.data_ptr(), o[0].data_ptr(), N, ptr(st)),
                [o], [cyc(want, rot)])


def c_sha(ctx, oracle, rot, bits):
    msgs = messages(3241 + bits)
    fn, h = (ctx.sha256_dev, hashlib.sha256) if bits == 256 else (ctx.sha512_dev, hashlib.sha512)
    (m, off, total), o, st_ = up_msgs(msgs, rot), out(bits // 8), status()
    return Call("sha%d_dev" % bits, lambda st: fn(m.data_ptr(), off.data_ptr(), total, o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [cyc(u8([h(x).digest() for x in msgs]), rot), np.zeros(N, dtype=np.uint8)])


def c_x25519(ctx, oracle, rot):
    rng = np.random.default_rng(3251)
    s, u = rng.integers(0, 256, size=(NREC, 32), dtype=np.uint8), rng.integers(0, 256, size=(NREC, 32), dtype=np.uint8)
    s[2] = 0
    s[2, 0] = 2                                            # the special scalar
    u[5] = 0                                               # the final z is zero
    want = cached(("x25519",), lambda: u8([X.x25519(bytes(a), bytes(b)) for a, b in zip(s, u)]))
    a, b, o = up_cyc(s, rot), up_cyc(u, rot), out(32)
    return Call("x25519_dev", lambda st: ctx.x25519_dev(a.data_ptr(), b.data_ptr(), o[0].data_ptr(), N, ptr(st)), [o], [cyc(want, rot)])


def c_curve25519_mul(ctx, oracle, rot):
    rng = np.random.default_rng(3261)
    k = rng.integers(0, 1 << 63, size=(NREC, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(NREC, 4), dtype=np.uint64)
    p = rng.integers(0, 1 << 63, size=(NREC, 8), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(NREC, 8), dtype=np.uint64)
    k[3] = [2, 0, 0, 0]
    p[6, 4:] = 0
    want = cached(("curve25519_mul",), lambda: u64([sum(X.multiply(p[i, :4], p[i, 4:], k[i]), []) for i in range(NREC)], 8))
    a, b, o = up_cyc(k, rot), up_cyc(p, rot), out(64)
    return Call("curve25519_mul_dev", lambda st: ctx.curve25519_mul_dev(a.data_ptr(), b.data_ptr(), o[0].data_ptr(), N, ptr(st)), [o], [cyc(want, rot)])


def c_xmd(ctx, oracle, rot):
    msgs = messages(3271)
    want = cached(("xmd",), lambda: u8([H.expand_message_xmd(m, DST, 96) for m in msgs]))
    (m, off, total), o, st_ = up_msgs(msgs, rot), out(96), status()
    return Call("expand_message_xmd_dev",
                lambda st: ctx.expand_message_xmd_dev(m.data_ptr(), off.data_ptr(), total, DST, 96, o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [cyc(want, rot), np.zeros(N, dtype=np.uint8)])


def _field(c, msgs, count):
    return np.array([H.hash_to_field(c, m, DST, count)[0] for m in msgs], dtype=np.uint64).reshape(len(msgs), count * 4)


def c_hash_to_field(ctx, oracle, rot, c):
    msgs = messages(3281 + c)
    want = cached(("hash_to_field", c), lambda: _field(c, msgs, 2))
    (m, off, total), o, st_ = up_msgs(msgs, rot), out(64), status()
    return Call("hash_to_field_dev " + NAMES[c],
                lambda st: ctx.hash_to_field_dev(c, m.data_ptr(), off.data_ptr(), total, DST, 2, o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [cyc(want, rot), np.zeros(N, dtype=np.uint8)])


def _maps(c, us):
    """h2c_ref.map_to_curve per element -> xy (n,8), cand (n,8), legs (n,)"""
    r = [H.map_to_curve(c, u) for u in us]
    return (u64([list(x[0][0]) + list(x[0][1]) for x in r], 8), u64([list(x[1][0]) + list(x[1][1]) for x in r], 8),
            np.array([x[2] for x in r], dtype=np.uint8))


def map_call(ctx, c, d_u, want, rot):
    xy, cand, legs = out(64), out(64), out(1)
    return Call("map_to_curve_dev " + NAMES[c],
                lambda st: ctx.map_to_curve_dev(c, d_u.data_ptr(), xy[0].data_ptr(), cand[0].data_ptr(), legs[0].data_ptr(), N, ptr(st)),
                [xy, cand, legs], [cyc(w, rot) for w in want])


def c_map_to_curve(ctx, oracle, rot, c):
    u = V.field_elements(NREC, c, 3291)
    u[4] = 0
    want = cached(("map", c), lambda: _maps(c, u))
    return map_call(ctx, c, up_cyc(u, rot), want, rot)


def _h2c(c, msgs):
    r = [H.hash_to_curve(c, m, DST) for m in msgs]
    return (u64([H.flat_proj(x[0]) for x in r], 12), u64([[v for cd in x[1] for part in cd for v in part] for x in r], 16),
            np.array([x[2] for x in r], dtype=np.uint8).reshape(len(msgs), 2))


def c_hash_to_curve(ctx, oracle, rot, c):
    msgs = messages(3301 + c)
    want = cached(("h2c", c), lambda: _h2c(c, msgs))
    (m, off, total), o, cand, legs, st_ = up_msgs(msgs, rot), out(96), out(128), out(2), status()
    return Call("hash_to_curve_dev " + NAMES[c],
                lambda st: ctx.hash_to_curve_dev(c, m.data_ptr(), off.data_ptr(), total, DST, o[0].data_ptr(), cand[0].data_ptr(), legs[0].data_ptr(),
                                                 st_[0].data_ptr(), N, ptr(st)),
                [o, cand, legs, st_], [cyc(w, rot) for w in want] + [np.zeros(N, dtype=np.uint8)])


# -- the verifiers: records picked from a pool so that the eight mix what the reference accepts and rejects
def _ecdsa_pool(oracle, c, dg, seed):
    """r, s, pk, inf for the digests dg: the even rows accept (the key at infinity, r = x of multiply(G, h * s^-1) as the
    reference derives it, where its s^-1 is not zero), the odd rows are random"""
    n = dg.shape[0]
    r, s = V.scalars(n, c, seed), V.scalars(n, c, seed + 1)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, c, seed + 2), V.field_elements(n, c, seed + 3)], axis=1))
    inf = np.zeros(n, dtype=np.uint8)
    op = oracle.secp256k1_scalar_op if c == SECP else oracle.p256_scalar_op
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    for i in range(0, n, 2):
        h = np.array(K.limbs(int.from_bytes(dg[i].tobytes(), "big")), dtype=np.uint64)
        s_inv, ok = op("inv", s[i])
        u1 = op("mul", h, s_inv)[0] if ok else np.zeros(4, dtype=np.uint64)
        xy, is_inf = oracle.to_affine(c, oracle.multiply(c, oracle.generator(c), u1))
        inf[i] = 1
        r[i] = oracle.field_op(0, "mul", xy[:4], one) if c == SECP else xy[:4]
    return r, s, pk, inf


def _ecdsa_verify(oracle, c, dg, r, s, pk, inf):
    return (oracle.batch_secp256k1_ecdsa_verify if c == SECP else oracle.batch_p256_ecdsa_verify)(dg, r, s, pk, inf)


def _ecdsa_verify_records(oracle, c, msgs=None):
    """the eight records of the ECDSA verifiers: on random digests, or (msgs: a pool of 32) on SHA-256 of the messages"""
    pool = 32
    dg = np.random.default_rng(3311 + c).integers(0, 256, size=(pool, 32), dtype=np.uint8) if msgs is None else u8([hashlib.sha256(m).digest() for m in msgs])
    if msgs is None:
        dg[:, 0] &= 0x7F
        dg[7] = 0xFF                                       # digest >= n: the reference panics
    r, s, pk, inf = _ecdsa_pool(oracle, c, dg, 3320 + 10 * c)
    want = _ecdsa_verify(oracle, c, dg, r, s, pk, inf)
    at = pick(want, "ecdsa_verify " + NAMES[c])
    assert 1 in want[at] and 0 in want[at]
    return at, dg[at], r[at], s[at], pk[at], inf[at], want[at]


def ecdsa_verify_call(ctx, c, d_dg, rec, rot):
    _, _, r, s, pk, inf, want = rec
    a, b, e, f, o = up_cyc(r, rot), up_cyc(s, rot), up_cyc(pk, rot), up_cyc(inf, rot), status()
    fn = ctx.ecdsa_verify_secp256k1_dev if c == SECP else ctx.ecdsa_verify_p256_dev
    return Call("ecdsa_verify_%s_dev" % NAMES[c], lambda st: fn(d_dg.data_ptr(), a.data_ptr(), b.data_ptr(), e.data_ptr(), f.data_ptr(), o[0].data_ptr(), N, ptr(st)),
                [o], [cyc(want, rot)])


def c_ecdsa_verify(ctx, oracle, rot, c):
    rec = cached(("ecdsa_verify", c), lambda: _ecdsa_verify_records(oracle, c))
    return ecdsa_verify_call(ctx, c, up_cyc(rec[1], rot), rec, rot)


def pool_messages(seed):
    """32 messages, the eight lengths four times over"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=LENGTHS[i % NREC], dtype=np.uint8).tobytes() for i in range(32)]


def ecdsa_msg_records(oracle, c):
    """(the eight messages, the records) of the ECDSA verifiers from the message"""
    def make():
        msgs = pool_messages(3331 + c)
        rec = _ecdsa_verify_records(oracle, c, msgs)
        return [msgs[i] for i in rec[0]], rec
    return cached(("ecdsa_verify_msg", c), make)


def c_ecdsa_verify_msg(ctx, oracle, rot, c):
    msgs, (_, _, r, s, pk, inf, want) = ecdsa_msg_records(oracle, c)
    (m, off, total), a, b, e, f, o = up_msgs(msgs, rot), up_cyc(r, rot), up_cyc(s, rot), up_cyc(pk, rot), up_cyc(inf, rot), status()
    return Call("ecdsa_verify_msg_dev " + NAMES[c],
                lambda st: ctx.ecdsa_verify_msg_dev(c, m.data_ptr(), off.data_ptr(), total, a.data_ptr(), b.data_ptr(), e.data_ptr(), f.data_ptr(),
                                                    o[0].data_ptr(), N, ptr(st)), [o], [cyc(want, rot)])


def _eddsa_verify_records(oracle):
    n = 24
    s, k = V.scalars(n, ED, 3341), V.scalars(n, ED, 3342)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, ED, 3343), V.field_elements(n, ED, 3344)], axis=1))
    r = np.ascontiguousarray(np.concatenate([V.field_elements(n, ED, 3345), V.field_elements(n, ED, 3346)], axis=1))
    pinf, rinf = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    axy, _ = oracle.batch_to_affine(ED, oracle.batch_mul_fixed(ED, s[:12], oracle.generator(ED)))
    for j in range(12):                                    # R = to_affine(s * G) with A at infinity or k = 0: these verify
        r[j] = axy[j]
        if j % 2:
            pinf[j] = 1
        else:
            k[j] = 0
    rinf[13] = 1
    want = oracle.batch_ed25519_eddsa_verify(r, rinf, pk, pinf, s, k)
    at = pick(want, "eddsa_verify")
    return r[at], rinf[at], pk[at], pinf[at], s[at], k[at], want[at]


def c_eddsa_verify(ctx, oracle, rot):
    rec = cached(("eddsa_verify",), lambda: _eddsa_verify_records(oracle))
    t = [up_cyc(a, rot) for a in rec[:6]]
    o = status()
    return Call("eddsa_verify_ed25519_dev",
                lambda st: ctx.eddsa_verify_ed25519_dev(*[x.data_ptr() for x in t], o[0].data_ptr(), N, ptr(st)), [o], [cyc(rec[6], rot)])


def _ed25519_verify_records(oracle):
    """the byte form: R and A drawn so that most decode, s = 0 where such a lane can verify (tests/test_gpu_eddsa_verify.py)"""
    n = 64
    rng = np.random.default_rng(3351)
    cand = rng.integers(0, 256, size=(64, 33), dtype=np.uint8)
    cand[:, 0] = 2
    cand[::2, 1:] = 0
    ok = oracle.batch_decompress(ED, cand)[2].astype(bool)
    good, bad = cand[ok][:, 1:], cand[~ok][:, 1:]
    assert len(good) and len(bad)
    keep = rng.integers(0, 4, size=(n, 2)) != 0
    pk = np.where(keep[:, :1], good[rng.integers(0, len(good), n)], bad[rng.integers(0, len(bad), n)])
    r = np.where(keep[:, 1:], good[rng.integers(0, len(good), n)], bad[rng.integers(0, len(bad), n)])
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[rng.integers(0, 3, n) == 0] = 0
    pk, sig = np.ascontiguousarray(pk), np.ascontiguousarray(np.concatenate([r, s], axis=1))
    msgs = [rng.integers(0, 256, size=LENGTHS[i % NREC], dtype=np.uint8).tobytes() for i in range(n)]
    want = np.array(EdV.verify_batch(pk, msgs, sig, EdV.CBackend(8)), dtype=np.uint8)
    at = pick(want, "ed25519_verify")
    return pk[at], [msgs[i] for i in at], sig[at], want[at]


def ed25519_verify_call(ctx, d_pk, msgs, sig, want, rot):
    (m, off, total), b, o = up_msgs(msgs, rot), up_cyc(sig, rot), status()
    return Call("ed25519_verify_dev",
                lambda st: ctx.ed25519_verify_dev(d_pk.data_ptr(), m.data_ptr(), off.data_ptr(), total, b.data_ptr(), o[0].data_ptr(), N, ptr(st)),
                [o], [cyc(want, rot)])


def c_ed25519_verify(ctx, oracle, rot):
    pk, msgs, sig, want = cached(("ed25519_verify",), lambda: _ed25519_verify_records(oracle))
    return ed25519_verify_call(ctx, up_cyc(pk, rot), msgs, sig, want, rot)


def _eddsa_verify_msg_records(oracle):
    """the generic form: arbitrary limbs, and constructed verifying signatures (the key at infinity, R = to_affine(s * G))"""
    n = 24
    rng = np.random.default_rng(3361)
    f = lambda w: rng.integers(0, 1 << 63, size=(n, w), dtype=np.uint64)
    pk, r, s = f(8), f(8), f(4)
    pinf, rinf = (rng.integers(0, 8, n) == 0).astype(np.uint8), (rng.integers(0, 8, n) == 1).astype(np.uint8)
    cs = rng.integers(1, 1 << 60, size=(12, 4), dtype=np.uint64)
    cr, cinf = oracle.batch_to_affine(ED, oracle.batch_mul_fixed(ED, cs, oracle.generator(ED)))
    assert not cinf.any()
    r[:12], rinf[:12], s[:12], pinf[:12] = cr, 0, cs, 1
    msgs = [rng.integers(0, 256, size=LENGTHS[i % NREC], dtype=np.uint8).tobytes() for i in range(n)]
    want = np.array(EdV.eddsa_verify_batch(pk, pinf, msgs, r, rinf, s, EdV.CBackend(8)), dtype=np.uint8)
    at = pick(want, "eddsa_verify_msg")
    return pk[at], pinf[at], [msgs[i] for i in at], r[at], rinf[at], s[at], want[at]


def c_eddsa_verify_msg(ctx, oracle, rot):
    pk, pinf, msgs, r, rinf, s, want = cached(("eddsa_verify_msg",), lambda: _eddsa_verify_msg_records(oracle))
    a, af, (m, off, total), b, bf, e, o = up_cyc(pk, rot), up_cyc(pinf, rot), up_msgs(msgs, rot), up_cyc(r, rot), up_cyc(rinf, rot), up_cyc(s, rot), status()
    return Call("eddsa_verify_ed25519_msg_dev",
                lambda st: ctx.eddsa_verify_ed25519_msg_dev(a.data_ptr(), af.data_ptr(), m.data_ptr(), off.data_ptr(), total, b.data_ptr(), bf.data_ptr(),
                                                            e.data_ptr(), o[0].data_ptr(), N, ptr(st)), [o], [cyc(want, rot)])


def _schnorr_verify_records(oracle, c):
    """the fixture's cases (for P-256 signatures that VERIFY under the reference's arithmetic among them) and random rows"""
    with open(os.path.join(HERE, "golden", "schnorr_vectors.json")) as f:
        fx = [x for x in json.load(f)["verify"] if x["curve"] == c]
    n = len(fx) + 8
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, c, 3371), V.field_elements(n, c, 3372)], axis=1))
    r = np.ascontiguousarray(np.concatenate([V.field_elements(n, c, 3373), V.field_elements(n, c, 3374)], axis=1))
    s, e = V.scalars(n, c, 3375), V.scalars(n, c, 3376)
    pinf, rinf = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for i, x in enumerate(fx):
        pk[i], r[i], s[i], e[i], pinf[i], rinf[i] = x["pk"], x["r"], x["s"], x["e"], x["pk_inf"], x["r_inf"]
    want = oracle.batch_schnorr_verify(c, pk, pinf, r, rinf, s, e)
    # (Schnorr::verify answers false to whatever Ed25519 and secp256k1 input the fixture and its generator found: new(x, -y))
    at = pick(want, "schnorr_verify " + NAMES[c], one_status=c != P256)
    return pk[at], pinf[at], r[at], rinf[at], s[at], e[at], want[at]


def c_schnorr_verify(ctx, oracle, rot, c):
    rec = cached(("schnorr_verify", c), lambda: _schnorr_verify_records(oracle, c))
    t = [up_cyc(a, rot) for a in rec[:6]]
    o = status()
    return Call("schnorr_verify_dev " + NAMES[c],
                lambda st: ctx.schnorr_verify_dev(c, *[x.data_ptr() for x in t], o[0].data_ptr(), N, ptr(st)), [o], [cyc(rec[6], rot)])


# -- the Ed25519 signers
def ed_keys():
    keys = np.random.default_rng(3381).integers(0, 256, size=(NREC, 32), dtype=np.uint8)
    keys[4, 0] = 0x9D                                      # the key of the reference's RFC 8032 special case (not its message)
    return keys


def c_ed25519_sign(ctx, oracle, rot):
    keys, msgs = ed_keys(), messages(3382)
    want = cached(("ed25519_sign",), lambda: EdS.sign_batch(keys, msgs, EdS.CBackend(8)))
    a, (m, off, total), sig, st_ = up_cyc(keys, rot), up_msgs(msgs, rot), out(64), status()
    return Call("ed25519_sign_dev",
                lambda st: ctx.ed25519_sign_dev(a.data_ptr(), m.data_ptr(), off.data_ptr(), total, sig[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [sig, st_], [cyc(u8([w[0] for w in want]), rot), cyc(np.array([w[1] for w in want], dtype=np.uint8), rot)])


def c_eddsa_sign(ctx, oracle, rot):
    sk, msgs = np.random.default_rng(3391).integers(0, 1 << 63, size=(NREC, 4), dtype=np.uint64) * np.uint64(2), messages(3392)
    want = cached(("eddsa_sign",), lambda: EdS.eddsa_sign_batch(sk, msgs, EdS.CBackend(8)))
    a, (m, off, total), r, rinf, s, st_ = up_cyc(sk, rot), up_msgs(msgs, rot), out(64), out(1), out(32), status()
    return Call("eddsa_sign_ed25519_dev",
                lambda st: ctx.eddsa_sign_ed25519_dev(a.data_ptr(), m.data_ptr(), off.data_ptr(), total, r[0].data_ptr(), rinf[0].data_ptr(), s[0].data_ptr(),
                                                      st_[0].data_ptr(), N, ptr(st)),
                [r, rinf, s, st_], [cyc(u64([list(w[0]) + list(w[1]) for w in want], 8), rot), cyc(np.array([int(w[2]) for w in want], dtype=np.uint8), rot),
                                    cyc(u64([w[3] for w in want], 4), rot), cyc(np.array([w[4] for w in want], dtype=np.uint8), rot)])


def _derived(keys):
    return cached(("ed25519_derive",), lambda: EdS.derive_batch(keys, EdS.CBackend(8)))


def c_ed25519_derive(ctx, oracle, rot):
    keys = ed_keys()
    want = _derived(keys)
    a, pk, st_ = up_cyc(keys, rot), out(32), status()
    return Call("ed25519_derive_public_key_dev", lambda st: ctx.ed25519_derive_public_key_dev(a.data_ptr(), pk[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [pk, st_], [cyc(u8([w[0] for w in want]), rot), cyc(np.array([w[1] for w in want], dtype=np.uint8), rot)])


ASSIGN = {"A on s1, B on s2": ("s1", "s2"), "A on s2, B on s1": ("s2", "s1")}


@pytest.fixture(scope="module", autouse=True)
def _leave_the_ctx_on_its_own_stream(gpu_ctx, oracle):
    """whatever subset of the module ran: the ctx's last launch names its own stream afterwards, and has finished"""
    yield
    import torch
    if GATE.geared:
        c = c_sha(gpu_ctx, oracle, ROT_A, 256)
        c.run(None)
        torch.cuda.synchronize()
        assert not c.bad()
        if GATE.timings:
            print("\n" + GATE.summary())


# ---- a. the users of the Ed25519 addend table behind and ahead of a rebuild ----------------------------------------------
TABLE_USERS = {
    "batch_mul_fixed own base X": (c_mul_fixed, (ED, "X")),
    "batch_mul_fixed generator": (c_mul_fixed, (ED, "G")),
    "batch_double_mul": (c_double_mul, (ED,)),
    "eddsa_verify_ed25519": (c_eddsa_verify, ()),
    "ed25519_verify": (c_ed25519_verify, ()),
    "eddsa_verify_ed25519_msg": (c_eddsa_verify_msg, ()),
    "schnorr_verify": (c_schnorr_verify, (ED,)),
    "ed25519_sign": (c_ed25519_sign, ()),
    "eddsa_sign_ed25519": (c_eddsa_sign, ()),
    "ed25519_derive_public_key": (c_ed25519_derive, ()),
}


@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("where", ["behind the rebuild", "ahead of the rebuild"])
@pytest.mark.parametrize("b", list(TABLE_USERS))
def test_ed25519_table_users_in_call_order(gpu_ctx, oracle, b, where, assign):
    """batch_mul_fixed_dev on a base Y of the caller's own always rebuilds ctx->d_ed_table: the user behind it must read its
    own base's table (the rebuild for G or X waits for Y's reader), the user ahead of it must have left the table"""
    f, args = TABLE_USERS[b]
    if where == "behind the rebuild":
        calls = [c_mul_fixed(gpu_ctx, oracle, ROT_A, ED, "Y"), f(gpu_ctx, oracle, ROT_B, *args)]
    else:
        calls = [f(gpu_ctx, oracle, ROT_A, *args), c_mul_fixed(gpu_ctx, oracle, ROT_B, ED, "Y")]
    _run(calls, ASSIGN[assign])


# ---- b. the calls that fork onto ctx->stream2, on both user streams at once -----------------------------------------------
FORKERS = {
    "batch_double_mul secp256k1": (c_double_mul, (SECP,)),
    "batch_double_mul p256": (c_double_mul, (P256,)),
    "batch_double_mul ed25519": (c_double_mul, (ED,)),
    "ecdsa_verify_secp256k1": (c_ecdsa_verify, (SECP,)),
    "ecdsa_verify_p256": (c_ecdsa_verify, (P256,)),
    "ecdsa_verify_msg secp256k1": (c_ecdsa_verify_msg, (SECP,)),
    "ecdsa_verify_msg p256": (c_ecdsa_verify_msg, (P256,)),
    "schnorr_verify secp256k1": (c_schnorr_verify, (SECP,)),
    "schnorr_verify p256": (c_schnorr_verify, (P256,)),
    "ecdh_exchange secp256k1": (c_ecdh_exchange, (SECP,)),
    "ecdh_exchange p256": (c_ecdh_exchange, (P256,)),
}


@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("ahead", ["itself", "another kind"])
@pytest.mark.parametrize("b", list(FORKERS))
def test_side_stream_users_on_both_streams(gpu_ctx, oracle, b, ahead, assign):
    """the fixed-base product of B goes to the one ctx->stream2 that A's went to: it must wait for A's join.  "another kind":
    ecdh_derive_key_dev for P-256, the scheduler on a work area of the stream's own and no fork"""
    f, args = FORKERS[b]
    a = f(gpu_ctx, oracle, ROT_A, *args) if ahead == "itself" else c_ecdh_derive_key(gpu_ctx, oracle, ROT_A, P256)
    _run([a, f(gpu_ctx, oracle, ROT_B, *args)], ASSIGN[assign])


# ---- c. the per-stream-scratch and no-scratch family on both streams at once ----------------------------------------------
PER_STREAM = {
    "batch_mul secp256k1": (c_mul, (SECP,)),
    "batch_mul p256": (c_mul, (P256,)),
    "batch_mul ed25519": (c_mul, (ED,)),
    "batch_mul_fixed generator secp256k1": (c_mul_fixed, (SECP, "G")),
    "batch_mul_fixed generator p256": (c_mul_fixed, (P256, "G")),
    "batch_to_affine": (c_to_affine, (SECP,)),
    "batch_compress": (c_compress, (ED,)),
    "batch_validate_point secp256k1": (c_validate, (SECP,)),
    "batch_validate_point p256": (c_validate, (P256,)),
    "batch_validate_point ed25519": (c_validate, (ED,)),
    "batch_ecdh": (c_ecdh, (SECP,)),
    "ecdh_derive_key": (c_ecdh_derive_key, (P256,)),
    "derive_key": (c_derive_key, (SECP,)),
    "ecdsa_sign": (c_ecdsa_sign, (SECP,)),
    "ecdsa_sign_msg": (c_ecdsa_sign_msg, (P256,)),
    "rfc6979_k": (c_rfc6979, (SECP,)),
    "bip340_sign": (c_bip340_sign, ()),
    "schnorr_sign_msg": (c_schnorr_sign, (P256,)),
    "schnorr_challenge": (c_schnorr_challenge, (ED,)),
    "scalar_from_bytes_reduced": (c_from_bytes_reduced, (SECP,)),
    "sha256": (c_sha, (256,)),
    "sha512": (c_sha, (512,)),
    "x25519": (c_x25519, ()),
    "curve25519_mul": (c_curve25519_mul, ()),
    "expand_message_xmd": (c_xmd, ()),
    "hash_to_field": (c_hash_to_field, (SECP,)),
    "map_to_curve": (c_map_to_curve, (P256,)),
    "hash_to_curve p256": (c_hash_to_curve, (P256,)),
}


@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("b", list(PER_STREAM))
def test_per_stream_family_on_both_streams(gpu_ctx, oracle, b, assign):
    """the same call on both streams, rotations A and B: scratch per stream (or none); the prefix tables, the error word and
    last_stream shared"""
    f, args = PER_STREAM[b]
    _run([f(gpu_ctx, oracle, ROT_A, *args), f(gpu_ctx, oracle, ROT_B, *args)], ASSIGN[assign])


# ---- d. pipelines: one call's output tensor is the next call's input on the other stream ------------------------------------
def alternate(first, k):
    second = "s2" if first == "s1" else "s1"
    return tuple((first, second)[i & 1] for i in range(k))


def reduced_to_schnorr_sign(ctx, c):
    """[scalar_from_bytes_reduced_dev, schnorr_sign_msg_dev(sk = that output)] and what the model says of both"""
    b, msgs = reduced_bytes(c), messages(3401 + c)
    sk = cached(("reduced", c), lambda: _reduced(c, b))
    want = cached(("reduced -> schnorr_sign", c), lambda: SS.sign_many(c, sk, msgs))
    a, d_sk = up_cyc(b, ROT_B), out(32)
    reduce_ = Call("scalar_from_bytes_reduced_dev " + NAMES[c], lambda st: ctx.scalar_from_bytes_reduced_dev(c, a.data_ptr(), d_sk[0].data_ptr(), N, ptr(st)),
                   [d_sk], [cyc(sk, ROT_B)])
    return [reduce_, schnorr_sign_call(ctx, c, d_sk[0], msgs, ROT_B, want)]


@pytest.mark.parametrize("first", ["s1", "s2"])
@pytest.mark.parametrize("c", [SECP, P256], ids=["secp256k1", "p256"])
def test_pipeline_reduced_bytes_to_schnorr_sign(gpu_ctx, oracle, c, first):
    """scalar_from_bytes_reduced_dev -> schnorr_sign_msg_dev with sk = that output.  The signer's copy of sk into its scratch
    was enqueued ahead of its ordering: it read the sentinel, P = multiply(G, sk) came from stale bytes, and s and
    sig_bytes (computed from the real sk behind the ordering, and a challenge over the stale P) were not the model's"""
    _run(reduced_to_schnorr_sign(gpu_ctx, c), alternate(first, 2))


@pytest.mark.parametrize("first", ["s1", "s2"])
@pytest.mark.parametrize("c", [SECP, P256], ids=["secp256k1", "p256"])
def test_pipeline_sha256_to_ecdsa_verify(gpu_ctx, oracle, c, first):
    """sha256_dev -> ecdsa_verify_secp256k1_dev / ecdsa_verify_p256_dev on the digests of that output"""
    msgs, rec = ecdsa_msg_records(oracle, c)
    (m, off, total), dg, st_ = up_msgs(msgs, ROT_B), out(32), status()
    sha = Call("sha256_dev", lambda st: gpu_ctx.sha256_dev(m.data_ptr(), off.data_ptr(), total, dg[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
               [dg, st_], [cyc(rec[1], ROT_B), np.zeros(N, dtype=np.uint8)])
    _run([sha, ecdsa_verify_call(gpu_ctx, c, dg[0], rec, ROT_B)], alternate(first, 2))


@pytest.mark.parametrize("first", ["s1", "s2"])
@pytest.mark.parametrize("c", [SECP, P256], ids=["secp256k1", "p256"])
def test_pipeline_sha256_and_rfc6979_to_ecdsa_sign(gpu_ctx, oracle, c, first):
    """sha256_dev, rfc6979_k_dev -> ecdsa_sign_dev on both outputs: what ecdsa_sign_msg gives in the model"""
    sk, msgs = scalars_below_order(c, 3411), messages(3412 + c)
    r, s, wst, k = cached(("sha, rfc6979 -> ecdsa_sign", c), lambda: RF.sign_msg(oracle, c, sk, msgs))
    assert not (wst == 1).any()                            # every key passes the signer's check, so every element drew a nonce
    d_sk, (m, off, total) = up_cyc(sk, ROT_B), up_msgs(msgs, ROT_B)
    dg, st1, dk, st2, sig, st3 = out(32), status(), out(32), status(), out(64), status()
    zeros = np.zeros(N, dtype=np.uint8)
    calls = [
        Call("sha256_dev", lambda st: gpu_ctx.sha256_dev(m.data_ptr(), off.data_ptr(), total, dg[0].data_ptr(), st1[0].data_ptr(), N, ptr(st)),
             [dg, st1], [cyc(u8([hashlib.sha256(x).digest() for x in msgs]), ROT_B), zeros]),
        Call("rfc6979_k_dev", lambda st: gpu_ctx.rfc6979_k_dev(c, d_sk.data_ptr(), m.data_ptr(), off.data_ptr(), total, dk[0].data_ptr(), st2[0].data_ptr(), N, ptr(st)),
             [dk, st2], [cyc(k, ROT_B), zeros]),
        Call("ecdsa_sign_dev", lambda st: gpu_ctx.ecdsa_sign_dev(c, d_sk.data_ptr(), dg[0].data_ptr(), dk[0].data_ptr(), sig[0].data_ptr(), st3[0].data_ptr(), N, ptr(st)),
             [sig, st3], [cyc(np.concatenate([r, s], axis=1), ROT_B), cyc(wst, ROT_B)]),
    ]
    _run(calls, alternate(first, 3))


@pytest.mark.parametrize("first", ["s1", "s2"])
@pytest.mark.parametrize("c", [SECP, P256, ED], ids=["secp256k1", "p256", "ed25519"])
def test_pipeline_mul_to_affine_compress(gpu_ctx, oracle, c, first):
    """batch_mul_dev -> batch_to_affine_dev -> batch_compress_dev"""
    mul = c_mul(gpu_ctx, oracle, ROT_B, c)
    wxy, winf = cached(("mul -> to_affine", c), lambda: oracle.batch_to_affine(c, _cache["mul", c]))
    w33 = cached(("mul -> compress", c), lambda: oracle.batch_compress(c, wxy, winf))
    p, xy, inf, o = mul.outs[0][0], out(64), out(1), out(33)
    calls = [
        mul,
        Call("batch_to_affine_dev", lambda st: gpu_ctx.batch_to_affine_dev(c, p.data_ptr(), xy[0].data_ptr(), inf[0].data_ptr(), N, ptr(st)),
             [xy, inf], [cyc(wxy, ROT_B), cyc(winf, ROT_B)]),
        Call("batch_compress_dev", lambda st: gpu_ctx.batch_compress_dev(c, xy[0].data_ptr(), inf[0].data_ptr(), o[0].data_ptr(), N, ptr(st)),
             [o], [cyc(w33, ROT_B)]),
    ]
    _run(calls, alternate(first, 3))


@pytest.mark.parametrize("first", ["s1", "s2"])
def test_pipeline_ed25519_derive_public_key_to_verify(gpu_ctx, oracle, first):
    """ed25519_derive_public_key_dev -> ed25519_verify_dev on the produced keys, the signatures made by the model's signer
    (the odd records' messages changed afterwards); the model's verifier says what each is worth"""
    keys, msgs = ed_keys(), messages(3421)
    derive = c_ed25519_derive(gpu_ctx, oracle, ROT_B)

    def make():
        sig = u8([w[0] for w in EdS.sign_batch(keys, msgs, EdS.CBackend(8))])
        other = [m if i % 2 == 0 else m[:-1] + bytes([m[-1] ^ 1]) for i, m in enumerate(msgs)]
        pk = u8([w[0] for w in _derived(keys)])
        return sig, other, np.array(EdV.verify_batch(pk, other, sig, EdV.CBackend(8)), dtype=np.uint8)
    sig, other, want = cached(("derive -> verify",), make)
    _run([derive, ed25519_verify_call(gpu_ctx, derive.outs[0][0], other, sig, want, ROT_B)], alternate(first, 2))


@pytest.mark.parametrize("first", ["s1", "s2"])
@pytest.mark.parametrize("c", [SECP, P256], ids=["secp256k1", "p256"])
def test_pipeline_ecdh_to_derive_key(gpu_ctx, oracle, c, first):
    """batch_ecdh_dev -> derive_key_dev on the produced secrets, whatever their status"""
    ecdh = c_ecdh(gpu_ctx, oracle, ROT_B, c)
    want = cached(("ecdh -> derive_key", c), lambda: u8([K.derive_key(c, bytes(s), INFO, 33) for s in _cache["ecdh", c][0]]))
    sec, keys = ecdh.outs[0][0], out(33)
    kdf = Call("derive_key_dev", lambda st: gpu_ctx.derive_key_dev(c, sec.data_ptr(), 32, INFO, 33, keys[0].data_ptr(), N, ptr(st)), [keys], [cyc(want, ROT_B)])
    _run([ecdh, kdf], alternate(first, 2))


@pytest.mark.parametrize("first", ["s1", "s2"])
@pytest.mark.parametrize("c", [SECP, P256], ids=["secp256k1", "p256"])
def test_pipeline_hash_to_field_to_map_to_curve(gpu_ctx, oracle, c, first):
    """hash_to_field_dev (count 1) -> map_to_curve_dev on the produced field elements"""
    msgs = messages(3431 + c)
    u = cached(("hash_to_field 1", c), lambda: _field(c, msgs, 1))
    want = cached(("hash_to_field -> map", c), lambda: _maps(c, u))
    (m, off, total), d_u, st_ = up_msgs(msgs, ROT_B), out(32), status()
    field = Call("hash_to_field_dev", lambda st: gpu_ctx.hash_to_field_dev(c, m.data_ptr(), off.data_ptr(), total, DST, 1, d_u[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                 [d_u, st_], [cyc(u, ROT_B), np.zeros(N, dtype=np.uint8)])
    _run([field, map_call(gpu_ctx, c, d_u[0], want, ROT_B)], alternate(first, 2))


# ---- e. the edges the canonical module also has -----------------------------------------------------------------------------
def test_first_calls_of_a_ctx_on_user_streams(oracle):
    """a fresh ctx: an Ed25519 composed call on s1 (the addend table of G is built on first use, on a user stream), then a
    P-256 composed call on s2, then the Ed25519 one's reader of the table again.  Nothing is warmed up -- the streams' scratch
    is allocated here -- so there is no gate either: the results must be the model's"""
    import torch
    import forge_ec_amd as F
    g = GATE.gear()
    ctx = F.Context(0)
    try:
        calls = [c_ed25519_sign(ctx, oracle, ROT_A), c_ecdsa_verify(ctx, oracle, ROT_B, P256), c_eddsa_verify(ctx, oracle, ROT_B)]
        torch.cuda.synchronize()
        for call, k in zip(calls, ("s1", "s2", "s1")):
            call.run(g[k])
        torch.cuda.synchronize()
        assert not any(call.bad() for call in calls), [call.bad() for call in calls]
        ctx.check()
    finally:
        ctx.close()


def test_null_stream_call_behind_the_user_streams(gpu_ctx, oracle):
    """calls on s1 and s2, then one on the ctx's own stream (NULL) that reads the addend table the second one rebuilt over:
    ordered like any other chain, and the ctx's last launch no longer names a stream of this module"""
    _run([c_double_mul(gpu_ctx, oracle, ROT_A, P256), c_mul_fixed(gpu_ctx, oracle, ROT_B, ED, "Y"), c_mul_fixed(gpu_ctx, oracle, ROT_A, ED, "G")],
         ("s1", "s2", None))
    gpu_ctx.check()
