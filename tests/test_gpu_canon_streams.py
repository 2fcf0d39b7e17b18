"""
GPU tests of canonical mode's call order across streams: pairs and chains of *_dev calls of ONE ctx on two user streams
(and the ctx's own, stream = NULL) with no synchronisation between the calls, every output compared with the big-integer
model (oracle/canon_model.py and the canon_*_ref.py modules beside this file), never with another GPU run.

include/fecgpu.h promises that the launches of one ctx execute in call order whatever streams they name: the verifiers,
recovery, tweak-add and CKDpub lay their work areas out over the same ctx->d_verify, every multiplication shares d_zbuf / d_tbuf /
d_win_scratch, the secret family shares the comb tables and the error word, and a caller may feed one call's output tensor
to the next call on another stream.  tests/test_canon_launch_order.py holds the promise on the text of canon.hip; here two
calls really are in flight.

The gate (tests/stream_gate.py, shared with tests/test_gpu_parity_streams.py; _run here) makes a missing ordering
deterministic instead of hoped-for.  After a warm-up of the same calls on the same
streams (growth of a work area, the first build of a comb table and the first allocation of a stream's scratch all
synchronise, and would hide a race), a chain of fp32 matmuls is queued on the stream of call A and event e_fill behind it;
a trivial op and event e_probe go to the other stream and the host waits for e_probe.  Then A, B, ... are issued back to
back and e_fill is polled.  The test FAILS unless (1) e_probe completed while e_fill had not -- the two streams run side by
side -- and (2) e_fill was still pending after the last call was issued -- none of A's kernels had started when B's first
one became runnable.  Under both, a first kernel of B that is not ordered behind A runs before all of A and the rest of B
after all of A: B computes on A's scratch, or reads inputs that A has not written yet.  That is how launch_canon_ecdsa_verify
and launch_canon_sig_verify (fec_canon_ecdsa_verify_dev, fec_canon_bip340_verify_dev, fec_canon_eddsa_verify_dev) failed
before they ordered their stream ahead of their first kernel.

Sizing, measured on an MI355X after warm-up (time.perf_counter round the issue loop, event timing round the filler; each
run prints both under -s): the host issues a pair of calls in 0.03 - 0.11 ms and the longest chain here, four calls with
the tensor unpacking between them, in 0.19 ms.  FILL_STEPS = 64 matmuls of 2048^2 in fp32 take 7.7 - 9.0 ms: forty times
the longest issue (ten times would leave 2 ms, no more than one hiccup of the host; one such hiccup, an issue of 0.54 ms, is
on record: still a fourteenth of the filler), and the 147 gated runs of the module take about 7 s together.  The two event assertions check the sizing on every run.

The streams: HIP spreads a process's streams over a few hardware queues (four by default) by the
number of users each queue has, and two streams that share a queue run one after the other -- two torch streams created
one after the other did exactly that here, and every gated test failed on its first condition.  So gear() creates six,
takes the first as s1 and as s2 the first of the others that the device demonstrably runs beside s1 (the gate's own
probe), and keeps all six for the life of the module.  Which queue the ctx's own stream (NULL) shares cannot be seen from
here; in the chains that end on it the gate's conditions are still checked between s1 and s2.

Inputs: n = 64 * 3 + 5 elements (three full wavefronts and a ragged one) cycling eight model-computed records per curve;
call A starts the cycle at record 0 and call B at record 3, so their inputs and expected outputs differ at every element.
Verifier batches are all valid (the model says so), so a mix-up shows as rejects.  Outputs are pre-filled with a sentinel.
"""
import random

import numpy as np
import pytest

import canon_bip32_ref as B32
import canon_msg_ref as R
import canon_recover_ref as RV
import canon_sign_ref as S
import canon_x25519_ref as X
import canon_wallet_ref as W
from oracle import canon_model as M
from stream_gate import Call, Gate, ptr

pytestmark = pytest.mark.gpu

N = 64 * 3 + 5
NREC = 8
ROT_A, ROT_B = 0, 3
FILL_DIM, FILL_STEPS = 2048, 64
NAMES = ["secp256k1", "p256", "ed25519"]
MODEL = dict(zip(NAMES, [M.SECP256K1, M.P256, M.ED25519]))
LENGTHS = [1, 31, 55, 64, 135, 136, 137, 200]   # message lengths of the eight records: either side of the hashes' block edges


# ---- model records, computed once --------------------------------------------------------------------------------------
_records = {}


def _weierstrass_records(curve):
    C = MODEL[curve]
    rng = random.Random(0x57A3 + NAMES.index(curve))
    out = []
    for j in range(NREC):
        d = rng.randrange(1, C.N)
        Q = C.mul(d, C.G)
        key = d.to_bytes(32, "big")
        digest, msg = rng.randbytes(32), rng.randbytes(LENGTHS[j])
        rsig, recid, st = RV.sign_recoverable_digest(C, d, digest, S.LOW_S)
        assert st == 0 and RV.verify_digest(C, digest, rsig, Q) and RV.recover_point(C, digest, rsig, recid) == Q
        msig, st = S.ecdsa_sign_msg(C, d, msg)
        pk33, pk65 = R.sec1_encode(Q), R.sec1_encode(Q, compressed=False)
        assert st == 0 and R.ecdsa_verify(C, msg, msig, pk33) == 1 and R.ecdsa_verify(C, msg, msig, pk65) == 1
        tweak = rng.randrange(1, C.N).to_bytes(32, "big")
        tw33, st1 = B32.pubkey_tweak_add(C, pk33, tweak, 33)
        sktw, st2 = B32.seckey_tweak_add(C, key, tweak)
        assert st1 == 0 and st2 == 0
        k, kb, u1, u2 = rng.randrange(2**256), rng.randrange(1, C.N), rng.randrange(1, C.N), rng.randrange(1, C.N)
        rec = dict(d=d, key=key, Q=Q, pk33=pk33, pk65=pk65, digest=digest, msg=msg, rsig=rsig, recid=recid, msig=msig,
                   z=int.from_bytes(digest, "big"), r=int.from_bytes(rsig[:32], "big"), s=int.from_bytes(rsig[32:], "big"),
                   tweak=tweak, tw33=tw33, sktw=sktw, k=k, kp=C.mul(k % C.N, Q), kb=kb, kg=C.mul(kb, C.G), u1=u1, u2=u2,
                   dm=C.add(C.mul(u1, C.G), C.mul(u2, Q)))
        if curve == "secp256k1":
            aux = rng.randbytes(32)
            bsig, st = S.bip340_sign(d, msg, aux)
            bpk = R.bip340_pubkey(d)
            assert st == 0 and R.bip340_verify(msg, bsig, bpk) == 1
            cc, idx = rng.randbytes(32), rng.randrange(B32.HARDENED)
            rec.update(aux=aux, bsig=bsig, bpk=bpk, e=R.bip340_challenge(bsig[:32], bpk, msg), eth=RV.encode(Q, 20), cc=cc, idx=idx,
                       hidx=B32.HARDENED | rng.randrange(B32.HARDENED), pub=B32.ckd_pub(pk33, cc, idx), priv=B32.ckd_priv(key, cc, idx))
            rec["hard"] = B32.ckd_priv(key, cc, rec["hidx"], B32.NO_COMB)
            assert rec["pub"][2] == 0 and rec["priv"][2] == 0 and rec["hard"][2] == 0
            assert S.public_key(0, rec["priv"][0], 33) == (rec["pub"][0], 0)
        out.append(rec)
    return out


def _ed_records():
    C = M.ED25519
    rng = random.Random(0x57A5)
    out = []
    for j in range(NREC):
        seed, msg = rng.randbytes(32), rng.randbytes(LENGTHS[j])
        sig, pk = S.ed25519_sign(seed, msg)
        assert R.ed25519_verify(msg, sig, pk) == 1
        Q = R.ed_decode(pk)
        k, kb, u1, u2 = rng.randrange(2**256), rng.randrange(1, C.N), rng.randrange(1, C.N), rng.randrange(1, C.N)
        xk, xu = rng.randbytes(32), rng.randbytes(32)
        out.append(dict(seed=seed, msg=msg, sig=sig, pk=pk, Q=Q, a_enc=int.from_bytes(pk, "little"), r_enc=int.from_bytes(sig[:32], "little"),
                        s=int.from_bytes(sig[32:], "little"), h=R.ed25519_challenge(sig[:32], pk, msg), k=k, kp=C.mul(k, Q), kb=kb,
                        kg=C.mul(kb, C.G), u1=u1, u2=u2, dm=C.add(C.mul(u1, C.G), C.mul(u2, Q)), xk=xk, xu=xu, x=X.x25519_status(xk, xu),
                        xbase=X.x25519_base(xk), keccak=RV.keccak256(msg)))
    return out


def recs(curve):
    if curve not in _records:
        _records[curve] = _ed_records() if curve == "ed25519" else _weierstrass_records(curve)
    return _records[curve]


_shared = {}


def shared_child(parent, j):
    """CKDpub of record `parent`'s key and chain code at record j's index"""
    if (parent, j) not in _shared:
        rs = recs("secp256k1")
        _shared[(parent, j)] = B32.ckd_pub(rs[parent]["pk33"], rs[parent]["cc"], rs[j]["idx"])
        assert _shared[(parent, j)][2] == 0
    return _shared[(parent, j)]


# ---- tensors ----------------------------------------------------------------------------------------------------------
def cyc(curve, rot, f):
    rs = recs(curve)
    return [f(rs[(i + rot) % NREC]) for i in range(N)]


def words(vals):
    return np.array([M.limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def xy(pts):
    return np.array([M.xy_limbs(p) for p in pts], dtype=np.uint64).reshape(len(pts), 8)


def rows(bs):
    return np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(len(bs), -1).copy()


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def up_msgs(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return up(np.frombuffer(b"".join(msgs), dtype=np.uint8)), up(off), int(off[-1])


def out_xy():
    import torch
    return torch.full((N, 8), -1, dtype=torch.int64, device="cuda"), -1


def out_bytes(width=None, fill=0xEE):
    import torch
    return torch.full((N,) if width is None else (N, width), fill, dtype=torch.uint8, device="cuda"), fill


def out_status():
    return out_bytes(None, 9)


ZEROS, ONES = np.zeros(N, dtype=np.uint8), np.ones(N, dtype=np.uint8)


# ---- the calls ----------------------------------------------------------------------------------------------------------
def _canon(ctx, curve):
    from forge_ec_amd.canon import CANON_CURVES
    return CANON_CURVES[curve](ctx)


def c_ecdsa_verify(ctx, rot, curve):
    dev = _canon(ctx, curve)
    z, r, s = (up(words(cyc(curve, rot, lambda e, k=k: e[k]))) for k in "zrs")
    pk = up(xy(cyc(curve, rot, lambda e: e["Q"])))
    res = out_status()
    return Call("ecdsa_verify_dev " + curve,
                lambda st: dev.ecdsa_verify_dev(z.data_ptr(), r.data_ptr(), s.data_ptr(), pk.data_ptr(), res[0].data_ptr(), N, ptr(st)), [res], [ONES])


def c_bip340_verify(ctx, rot):
    dev = _canon(ctx, "secp256k1")
    cols = [lambda e: int.from_bytes(e["bpk"], "big"), lambda e: int.from_bytes(e["bsig"][:32], "big"),
            lambda e: int.from_bytes(e["bsig"][32:], "big"), lambda e: e["e"]]
    a, b, c, d = (up(words(cyc("secp256k1", rot, f))) for f in cols)
    res = out_status()
    return Call("bip340_verify_dev",
                lambda st: dev.bip340_verify_dev(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), res[0].data_ptr(), N, ptr(st)), [res], [ONES])


def c_eddsa_verify(ctx, rot):
    dev = _canon(ctx, "ed25519")
    a, b, c, d = (up(words(cyc("ed25519", rot, lambda e, k=k: e[k]))) for k in ("a_enc", "r_enc", "s", "h"))
    res = out_status()
    return Call("eddsa_verify_dev",
                lambda st: dev.eddsa_verify_dev(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), res[0].data_ptr(), N, ptr(st)), [res], [ONES])


def c_ecdsa_verify_msg(ctx, rot, curve, pk_len):
    dev = _canon(ctx, curve)
    m, off, total = up_msgs(cyc(curve, rot, lambda e: e["msg"]))
    sg, pk = up(rows(cyc(curve, rot, lambda e: e["msig"]))), up(rows(cyc(curve, rot, lambda e: e["pk%d" % pk_len])))
    res = out_status()
    return Call("ecdsa_verify_msg_dev %s %d" % (curve, pk_len),
                lambda st: dev.ecdsa_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), pk_len, res[0].data_ptr(), N,
                                                    ptr(st)), [res], [ONES])


def c_bip340_verify_msg(ctx, rot):
    dev = _canon(ctx, "secp256k1")
    m, off, total = up_msgs(cyc("secp256k1", rot, lambda e: e["msg"]))
    sg, pk = up(rows(cyc("secp256k1", rot, lambda e: e["bsig"]))), up(rows(cyc("secp256k1", rot, lambda e: e["bpk"])))
    res = out_status()
    return Call("bip340_verify_msg_dev",
                lambda st: dev.bip340_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), res[0].data_ptr(), N, ptr(st)),
                [res], [ONES])


def c_ed25519_verify_msg(ctx, rot):
    dev = _canon(ctx, "ed25519")
    m, off, total = up_msgs(cyc("ed25519", rot, lambda e: e["msg"]))
    sg, pk = up(rows(cyc("ed25519", rot, lambda e: e["sig"]))), up(rows(cyc("ed25519", rot, lambda e: e["pk"])))
    res = out_status()
    return Call("ed25519_verify_msg_dev",
                lambda st: dev.ed25519_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), res[0].data_ptr(), N, ptr(st)),
                [res], [ONES])


def c_recover(ctx, rot, curve, out_len):
    dev = _canon(ctx, curve)
    dg, sg = up(rows(cyc(curve, rot, lambda e: e["digest"]))), up(rows(cyc(curve, rot, lambda e: e["rsig"])))
    rc = up(np.array(cyc(curve, rot, lambda e: e["recid"]), dtype=np.uint8))
    out, st_ = out_bytes(out_len), out_status()
    want = rows(cyc(curve, rot, lambda e: RV.encode(e["Q"], out_len)))
    return Call("ecdsa_recover_dev %s %d" % (curve, out_len),
                lambda st: dev.ecdsa_recover_dev(dg.data_ptr(), sg.data_ptr(), rc.data_ptr(), out[0].data_ptr(), out_len, st_[0].data_ptr(), N, ptr(st)),
                [out, st_], [want, ZEROS])


def c_pubkey_tweak_add(ctx, rot, curve):
    dev = _canon(ctx, curve)
    pk, tw = up(rows(cyc(curve, rot, lambda e: e["pk33"]))), up(rows(cyc(curve, rot, lambda e: e["tweak"])))
    out, st_ = out_bytes(33), out_status()
    return Call("pubkey_tweak_add_dev " + curve,
                lambda st: dev.pubkey_tweak_add_dev(pk.data_ptr(), 33, tw.data_ptr(), out[0].data_ptr(), 33, st_[0].data_ptr(), N, ptr(st)),
                [out, st_], [rows(cyc(curve, rot, lambda e: e["tw33"])), ZEROS])


def c_derive_pub(ctx, rot, shared):
    from forge_ec_amd.canon import CanonBip32
    dev = CanonBip32(ctx)
    rs = recs("secp256k1")
    idx = up(np.array(cyc("secp256k1", rot, lambda e: e["idx"]), dtype=np.uint32))
    if shared:
        par = rot % NREC
        pk, cc = up(rows([rs[par]["pk33"]])), up(rows([rs[par]["cc"]]))
        want = [shared_child(par, (i + rot) % NREC) for i in range(N)]
    else:
        pk, cc = up(rows(cyc("secp256k1", rot, lambda e: e["pk33"]))), up(rows(cyc("secp256k1", rot, lambda e: e["cc"])))
        want = cyc("secp256k1", rot, lambda e: e["pub"])
    out, occ, st_ = out_bytes(33), out_bytes(32), out_status()
    return Call("derive_pub_dev " + ("shared parent" if shared else "a parent each"),
                lambda st: dev.derive_pub_dev(pk.data_ptr(), cc.data_ptr(), 1 if shared else N, idx.data_ptr(), out[0].data_ptr(), occ[0].data_ptr(),
                                              st_[0].data_ptr(), N, ptr(st)),
                [out, occ, st_], [rows([w[0] for w in want]), rows([w[1] for w in want]), ZEROS])


def c_mul_base(ctx, rot, curve):
    dev = _canon(ctx, curve)
    k = up(words(cyc(curve, rot, lambda e: e["kb"])))
    o, st_ = out_xy(), out_status()
    return Call("mul_base_dev " + curve, lambda st: dev.mul_base_dev(k.data_ptr(), o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [xy(cyc(curve, rot, lambda e: e["kg"])), ZEROS])


def c_mul(ctx, rot, curve):
    dev = _canon(ctx, curve)
    k, p = up(words(cyc(curve, rot, lambda e: e["k"]))), up(xy(cyc(curve, rot, lambda e: e["Q"])))
    o, st_ = out_xy(), out_status()
    return Call("mul_dev " + curve, lambda st: dev.mul_dev(k.data_ptr(), p.data_ptr(), o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [xy(cyc(curve, rot, lambda e: e["kp"])), ZEROS])


def c_double_mul(ctx, rot, curve):
    dev = _canon(ctx, curve)
    a, b = up(words(cyc(curve, rot, lambda e: e["u1"]))), up(words(cyc(curve, rot, lambda e: e["u2"])))
    p = up(xy(cyc(curve, rot, lambda e: e["Q"])))
    o, st_ = out_xy(), out_status()
    return Call("double_mul_dev " + curve,
                lambda st: dev.double_mul_dev(a.data_ptr(), b.data_ptr(), p.data_ptr(), o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [xy(cyc(curve, rot, lambda e: e["dm"])), ZEROS])


def c_mul_base_secret(ctx, rot, curve):
    dev = _canon(ctx, curve)
    k = up(words(cyc(curve, rot, lambda e: e["kb"])))
    o, st_ = out_xy(), out_status()
    return Call("mul_base_secret_dev " + curve, lambda st: dev.mul_base_secret_dev(k.data_ptr(), o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [xy(cyc(curve, rot, lambda e: e["kg"])), ZEROS])


def c_public_key(ctx, rot, curve, out_len, scheme=None):
    dev = _canon(ctx, curve)
    sid = R.CURVE_IDS[curve] if scheme is None else scheme
    keys = cyc(curve, rot, lambda e: e["seed"] if curve == "ed25519" else e["key"])
    want = [S.public_key(sid, k, out_len) for k in keys[:NREC]]
    assert all(w[1] == 0 for w in want)
    k = up(rows(keys))
    out, st_ = out_bytes(out_len), out_status()
    return Call("public_key_dev %s %d" % (curve, out_len),
                lambda st: dev.public_key_dev(k.data_ptr(), out[0].data_ptr(), out_len, st_[0].data_ptr(), N, ptr(st), scheme=sid),
                [out, st_], [rows([want[i % NREC][0] for i in range(N)]), ZEROS])


def c_ecdsa_sign_digest(ctx, rot, curve, recoverable):
    dev = _canon(ctx, curve)
    dg, k = up(rows(cyc(curve, rot, lambda e: e["digest"]))), up(rows(cyc(curve, rot, lambda e: e["key"])))
    sg, st_ = out_bytes(64), out_status()
    want = rows(cyc(curve, rot, lambda e: e["rsig"]))
    if not recoverable:
        return Call("ecdsa_sign_digest_dev " + curve,
                    lambda st: dev.ecdsa_sign_digest_dev(dg.data_ptr(), k.data_ptr(), S.LOW_S, sg[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                    [sg, st_], [want, ZEROS])
    rc = out_status()
    return Call("ecdsa_sign_recoverable_digest_dev " + curve,
                lambda st: dev.ecdsa_sign_recoverable_digest_dev(dg.data_ptr(), k.data_ptr(), S.LOW_S, sg[0].data_ptr(), rc[0].data_ptr(), st_[0].data_ptr(), N,
                                                                 ptr(st)),
                [sg, rc, st_], [want, np.array(cyc(curve, rot, lambda e: e["recid"]), dtype=np.uint8), ZEROS])


def c_ecdsa_sign_msg(ctx, rot, curve):
    dev = _canon(ctx, curve)
    m, off, total = up_msgs(cyc(curve, rot, lambda e: e["msg"]))
    k = up(rows(cyc(curve, rot, lambda e: e["key"])))
    sg, st_ = out_bytes(64), out_status()
    return Call("ecdsa_sign_msg_dev " + curve,
                lambda st: dev.ecdsa_sign_msg_dev(m.data_ptr(), off.data_ptr(), total, k.data_ptr(), 0, sg[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [sg, st_], [rows(cyc(curve, rot, lambda e: e["msig"])), ZEROS])


def c_bip340_sign_msg(ctx, rot):
    dev = _canon(ctx, "secp256k1")
    m, off, total = up_msgs(cyc("secp256k1", rot, lambda e: e["msg"]))
    k, a = up(rows(cyc("secp256k1", rot, lambda e: e["key"]))), up(rows(cyc("secp256k1", rot, lambda e: e["aux"])))
    sg, st_ = out_bytes(64), out_status()
    return Call("bip340_sign_msg_dev",
                lambda st: dev.bip340_sign_msg_dev(m.data_ptr(), off.data_ptr(), total, k.data_ptr(), a.data_ptr(), sg[0].data_ptr(), st_[0].data_ptr(), N,
                                                   ptr(st)),
                [sg, st_], [rows(cyc("secp256k1", rot, lambda e: e["bsig"])), ZEROS])


def c_ed25519_sign_msg(ctx, rot):
    dev = _canon(ctx, "ed25519")
    m, off, total = up_msgs(cyc("ed25519", rot, lambda e: e["msg"]))
    k = up(rows(cyc("ed25519", rot, lambda e: e["seed"])))
    sg, pk, st_ = out_bytes(64), out_bytes(32), out_status()
    return Call("ed25519_sign_msg_dev",
                lambda st: dev.ed25519_sign_msg_dev(m.data_ptr(), off.data_ptr(), total, k.data_ptr(), sg[0].data_ptr(), pk[0].data_ptr(), st_[0].data_ptr(),
                                                    N, ptr(st)),
                [sg, pk, st_], [rows(cyc("ed25519", rot, lambda e: e["sig"])), rows(cyc("ed25519", rot, lambda e: e["pk"])), ZEROS])


def c_x25519(ctx, rot):
    from forge_ec_amd.canon import CanonX25519
    dev = CanonX25519(ctx)
    k, u = up(rows(cyc("ed25519", rot, lambda e: e["xk"]))), up(rows(cyc("ed25519", rot, lambda e: e["xu"])))
    out, st_ = out_bytes(32), out_status()
    return Call("x25519_dev", lambda st: dev.x25519_dev(k.data_ptr(), u.data_ptr(), out[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [out, st_], [rows(cyc("ed25519", rot, lambda e: e["x"][0])), np.array(cyc("ed25519", rot, lambda e: e["x"][1]), dtype=np.uint8)])


def c_x25519_base(ctx, rot):
    from forge_ec_amd.canon import CanonX25519
    dev = CanonX25519(ctx)
    k = up(rows(cyc("ed25519", rot, lambda e: e["xk"])))
    out = out_bytes(32)
    return Call("x25519_base_dev", lambda st: dev.x25519_base_dev(k.data_ptr(), out[0].data_ptr(), N, ptr(st)),
                [out], [rows(cyc("ed25519", rot, lambda e: e["xbase"]))])


def c_derive_priv(ctx, rot, hardened):
    from forge_ec_amd.canon import CanonBip32
    dev = CanonBip32(ctx)
    k, cc = up(rows(cyc("secp256k1", rot, lambda e: e["key"]))), up(rows(cyc("secp256k1", rot, lambda e: e["cc"])))
    idx = up(np.array(cyc("secp256k1", rot, lambda e: e["hidx" if hardened else "idx"]), dtype=np.uint32))
    want = cyc("secp256k1", rot, lambda e: e["hard" if hardened else "priv"])
    flags = B32.NO_COMB if hardened else 0
    out, occ, st_ = out_bytes(32), out_bytes(32), out_status()
    return Call("derive_priv_dev " + ("hardened, no comb" if hardened else "with the comb"),
                lambda st: dev.derive_priv_dev(k.data_ptr(), cc.data_ptr(), N, idx.data_ptr(), flags, out[0].data_ptr(), occ[0].data_ptr(), st_[0].data_ptr(),
                                               N, ptr(st)),
                [out, occ, st_], [rows([w[0] for w in want]), rows([w[1] for w in want]), ZEROS])


def c_seckey_tweak_add(ctx, rot, curve):
    dev = _canon(ctx, curve)
    k, t = up(rows(cyc(curve, rot, lambda e: e["key"]))), up(rows(cyc(curve, rot, lambda e: e["tweak"])))
    out, st_ = out_bytes(32), out_status()
    return Call("seckey_tweak_add_dev " + curve,
                lambda st: dev.seckey_tweak_add_dev(k.data_ptr(), t.data_ptr(), out[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [out, st_], [rows(cyc(curve, rot, lambda e: e["sktw"])), ZEROS])


def c_keccak256(ctx, rot):
    from forge_ec_amd.canon import CanonKeccak
    dev = CanonKeccak(ctx)
    m, off, total = up_msgs(cyc("ed25519", rot, lambda e: e["msg"]))
    out, st_ = out_bytes(32), out_status()
    return Call("keccak256_dev", lambda st: dev.keccak256_dev(m.data_ptr(), off.data_ptr(), total, out[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [out, st_], [rows(cyc("ed25519", rot, lambda e: e["keccak"])), ZEROS])


def c_decompress(ctx, rot, curve, pk_len):
    dev = _canon(ctx, curve)
    k = up(rows(cyc(curve, rot, lambda e: e["pk%d" % pk_len])))
    o, st_ = out_xy(), out_status()
    return Call("decompress_dev %s %d" % (curve, pk_len),
                lambda st: dev.decompress_dev(k.data_ptr(), pk_len, o[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [o, st_], [xy(cyc(curve, rot, lambda e: e["Q"])), ZEROS])


_wallet = {}


def wallet_recs():
    """per secp256k1 record: a Merkle root and the Taproot output key of the x-only key; a depth-3 path and its CKDpub"""
    if not _wallet:
        rng = random.Random(0x57A7)
        out = []
        for e in recs("secp256k1"):
            root = rng.randbytes(32)
            path = [rng.randrange(B32.HARDENED) for _ in range(3)]
            tap, child = W.taproot_output_key(e["bpk"], root), W.derive_pub_path(e["pk33"], e["cc"], path)
            assert tap[2] == 0 and child[4] == 0
            out.append(dict(root=root, path=path, tap=tap, child=child))
        _wallet["recs"] = out
    return _wallet["recs"]


def wcyc(rot, f):
    ws = wallet_recs()
    return [f(ws[(i + rot) % NREC]) for i in range(N)]


def c_taproot_output_key(ctx, rot):
    dev = _canon(ctx, "secp256k1")
    pk, rt = up(rows(cyc("secp256k1", rot, lambda e: e["bpk"]))), up(rows(wcyc(rot, lambda w: w["root"])))
    out, par, st_ = out_bytes(32), out_status(), out_status()
    return Call("taproot_output_key_dev",
                lambda st: dev.taproot_output_key_dev(pk.data_ptr(), 32, rt.data_ptr(), out[0].data_ptr(), par[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [out, par, st_], [rows(wcyc(rot, lambda w: w["tap"][0])), np.array(wcyc(rot, lambda w: w["tap"][1]), dtype=np.uint8), ZEROS])


def c_derive_pub_path(ctx, rot):
    from forge_ec_amd.canon import CanonBip32
    dev = CanonBip32(ctx)
    pk, cc = up(rows(cyc("secp256k1", rot, lambda e: e["pk33"]))), up(rows(cyc("secp256k1", rot, lambda e: e["cc"])))
    idx = up(np.array(wcyc(rot, lambda w: w["path"]), dtype=np.uint32))
    out, occ, fp, h160, st_ = out_bytes(33), out_bytes(32), out_bytes(4), out_bytes(20), out_status()
    return Call("derive_pub_path_dev depth 3",
                lambda st: dev.derive_pub_path_dev(pk.data_ptr(), cc.data_ptr(), N, idx.data_ptr(), 3, out[0].data_ptr(), occ[0].data_ptr(),
                                                   fp[0].data_ptr(), h160[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [out, occ, fp, h160, st_], [rows(wcyc(rot, lambda w, k=k: w["child"][k])) for k in range(4)] + [ZEROS])


def c_digest20(ctx, rot, which):
    from forge_ec_amd.canon import CanonKeccak
    dev = CanonKeccak(ctx)
    m, off, total = up_msgs(cyc("secp256k1", rot, lambda e: e["msg"]))
    out, st_ = out_bytes(20), out_status()
    fn, model = (dev.ripemd160_dev, W.ripemd160) if which == "ripemd160" else (dev.hash160_dev, W.hash160)
    return Call(which + "_dev", lambda st: fn(m.data_ptr(), off.data_ptr(), total, out[0].data_ptr(), st_[0].data_ptr(), N, ptr(st)),
                [out, st_], [rows(cyc("secp256k1", rot, lambda e: model(e["msg"]))), ZEROS])


def c_pubkey_hash160(ctx, rot):
    from forge_ec_amd.canon import CanonKeccak
    dev = CanonKeccak(ctx)
    pk = up(rows(cyc("secp256k1", rot, lambda e: e["pk33"])))
    out = out_bytes(20)
    return Call("pubkey_hash160_dev 33", lambda st: dev.pubkey_hash160_dev(pk.data_ptr(), 33, out[0].data_ptr(), N, ptr(st)),
                [out], [rows(cyc("secp256k1", rot, lambda e: W.hash160(e["pk33"])))])


# every user of ctx->d_verify, by the layout it gives the buffer
VERIFY_USERS = {
    "ecdsa_verify secp256k1": (c_ecdsa_verify, ("secp256k1",), "ecdsa"),
    "ecdsa_verify p256": (c_ecdsa_verify, ("p256",), "ecdsa"),
    "bip340_verify": (c_bip340_verify, (), "sig"),
    "eddsa_verify": (c_eddsa_verify, (), "sig"),
    "ecdsa_verify_msg secp256k1 33": (c_ecdsa_verify_msg, ("secp256k1", 33), "ecdsa"),
    "ecdsa_verify_msg secp256k1 65": (c_ecdsa_verify_msg, ("secp256k1", 65), "ecdsa"),
    "ecdsa_verify_msg p256 33": (c_ecdsa_verify_msg, ("p256", 33), "ecdsa"),
    "ecdsa_verify_msg p256 65": (c_ecdsa_verify_msg, ("p256", 65), "ecdsa"),
    "bip340_verify_msg": (c_bip340_verify_msg, (), "sig"),
    "ed25519_verify_msg": (c_ed25519_verify_msg, (), "sig"),
    "ecdsa_recover secp256k1 address": (c_recover, ("secp256k1", 20), "recover"),
    "ecdsa_recover secp256k1 key": (c_recover, ("secp256k1", 65), "recover"),
    "ecdsa_recover p256 key": (c_recover, ("p256", 65), "recover"),
    "pubkey_tweak_add secp256k1": (c_pubkey_tweak_add, ("secp256k1",), "tweak"),
    "pubkey_tweak_add p256": (c_pubkey_tweak_add, ("p256",), "tweak"),
    "derive_pub shared": (c_derive_pub, (True,), "tweak"),
    "derive_pub each": (c_derive_pub, (False,), "tweak"),
    "taproot_output_key": (c_taproot_output_key, (), "tweak"),
    "derive_pub_path depth 3": (c_derive_pub_path, (), "tweak"),
}
# the call that goes ahead of a user of each layout: a user of another one
OTHER_LAYOUT = {"ecdsa": "bip340_verify_msg", "sig": "ecdsa_recover secp256k1 key", "recover": "derive_pub each", "tweak": "ecdsa_verify_msg p256 33"}

# the calls whose scratch belongs to the stream (or that have none): they share the comb tables, the error word and last_stream
PER_STREAM = {
    "mul_base_secret secp256k1": (c_mul_base_secret, ("secp256k1",)),
    "mul_base_secret ed25519": (c_mul_base_secret, ("ed25519",)),
    "public_key secp256k1 33": (c_public_key, ("secp256k1", 33)),
    "public_key p256 65": (c_public_key, ("p256", 65)),
    "public_key bip340": (c_public_key, ("secp256k1", 32, S.SCHEME_BIP340)),
    "public_key ed25519": (c_public_key, ("ed25519", 32)),
    "ecdsa_sign_digest secp256k1": (c_ecdsa_sign_digest, ("secp256k1", False)),
    "ecdsa_sign_recoverable_digest p256": (c_ecdsa_sign_digest, ("p256", True)),
    "ecdsa_sign_msg p256": (c_ecdsa_sign_msg, ("p256",)),
    "bip340_sign_msg": (c_bip340_sign_msg, ()),
    "ed25519_sign_msg": (c_ed25519_sign_msg, ()),
    "x25519": (c_x25519, ()),
    "x25519_base": (c_x25519_base, ()),
    "derive_priv comb": (c_derive_priv, (False,)),
    "derive_priv hardened": (c_derive_priv, (True,)),
    "seckey_tweak_add secp256k1": (c_seckey_tweak_add, ("secp256k1",)),
    "keccak256": (c_keccak256, ()),
    "decompress p256 33": (c_decompress, ("p256", 33)),
    "ripemd160": (c_digest20, ("ripemd160",)),
    "hash160": (c_digest20, ("hash160",)),
    "pubkey_hash160 33": (c_pubkey_hash160, ()),
}


# ---- the gate (tests/stream_gate.py), with this module's filler ------------------------------------------------------------
GATE = Gate(FILL_DIM, FILL_STEPS)
gear, _run, TIMINGS = GATE.gear, GATE.run, GATE.timings


ASSIGN = {"A on s1, B on s2": ("s1", "s2"), "A on s2, B on s1": ("s2", "s1")}


@pytest.fixture(scope="module", autouse=True)
def _leave_the_ctx_on_its_own_stream(gpu_ctx):
    """whatever subset of the module ran: the ctx's last launch names its own stream afterwards, and has finished"""
    yield
    import torch
    if GATE.geared:
        c = c_keccak256(gpu_ctx, ROT_A)
        c.run(None)
        torch.cuda.synchronize()
        assert not c.bad()
        if TIMINGS:
            print("\n" + GATE.summary())


# ---- 1. every user of d_verify behind another one ------------------------------------------------------------------------
@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("ahead", ["another layout", "the same call"])
@pytest.mark.parametrize("b", list(VERIFY_USERS))
def test_verify_area_users_in_call_order(gpu_ctx, b, ahead, assign):
    """B's kernels must not touch d_verify before A's last one has left it, whichever layout A gave it"""
    fb, argb, layout = VERIFY_USERS[b]
    fa, arga, _ = VERIFY_USERS[OTHER_LAYOUT[layout]] if ahead == "another layout" else VERIFY_USERS[b]
    _run([fa(gpu_ctx, ROT_A, *arga), fb(gpu_ctx, ROT_B, *argb)], ASSIGN[assign])


# ---- 2. the multiplications behind a verifier ----------------------------------------------------------------------------
@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("curve", NAMES)
@pytest.mark.parametrize("b", ["mul_base", "mul", "double_mul"])
def test_multiplications_behind_a_verifier(gpu_ctx, b, curve, assign):
    """d_zbuf, d_tbuf and d_win_scratch: the verifier's comb and ladder leave Z (and T) there for their own last kernels"""
    a = c_eddsa_verify(gpu_ctx, ROT_A) if curve == "ed25519" else c_ecdsa_verify(gpu_ctx, ROT_A, curve)
    fb = dict(mul_base=c_mul_base, mul=c_mul, double_mul=c_double_mul)[b]
    _run([a, fb(gpu_ctx, ROT_B, curve)], ASSIGN[assign])


# ---- 3. the per-stream family on both streams at once --------------------------------------------------------------------
@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("b", list(PER_STREAM))
def test_per_stream_family_on_both_streams(gpu_ctx, b, assign):
    """each behind its predecessor in the list: scratch per stream, the comb tables, the error word and last_stream shared"""
    names = list(PER_STREAM)
    fa, arga = PER_STREAM[names[names.index(b) - 1]]
    fb, argb = PER_STREAM[b]
    _run([fa(gpu_ctx, ROT_A, *arga), fb(gpu_ctx, ROT_B, *argb)], ASSIGN[assign])


# ---- 4. pipelines: one call's output tensor is the next call's input -----------------------------------------------------
def _le(dst, src, stream):
    """dst = the big-endian 32-byte rows of src as little-endian ones (the limbs of the same integers), on `stream`"""
    import torch
    with torch.cuda.stream(stream):
        dst.copy_(src.flip(1))


@pytest.mark.parametrize("first", ["s1", "s2"])
@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_pipeline_key_sign_verify_recover(gpu_ctx, curve, first):
    """public_key_dev -> ecdsa_sign_recoverable_digest_dev -> ecdsa_verify_dev on the produced key and r, s (unpacked to
    limbs by torch on the producing streams) -> ecdsa_recover_dev on the produced signature and ids"""
    import torch
    dev = _canon(gpu_ctx, curve)
    rot = ROT_B
    dg, keys = up(rows(cyc(curve, rot, lambda e: e["digest"]))), up(rows(cyc(curve, rot, lambda e: e["key"])))
    z = up(words(cyc(curve, rot, lambda e: e["z"])))
    pk65, st1 = out_bytes(65), out_status()
    pkxy = torch.full((N, 64), 0xEE, dtype=torch.uint8, device="cuda")
    sg, rc, st2 = out_bytes(64), out_status(), out_status()
    r_le, s_le = (torch.full((N, 32), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
    res = out_status()
    rec, st4 = out_bytes(65), out_status()

    def key(st):
        dev.public_key_dev(keys.data_ptr(), pk65[0].data_ptr(), 65, st1[0].data_ptr(), N, ptr(st))
        _le(pkxy[:, :32], pk65[0][:, 1:33], st)
        _le(pkxy[:, 32:], pk65[0][:, 33:], st)

    def sign(st):
        dev.ecdsa_sign_recoverable_digest_dev(dg.data_ptr(), keys.data_ptr(), S.LOW_S, sg[0].data_ptr(), rc[0].data_ptr(), st2[0].data_ptr(), N, ptr(st))
        _le(r_le, sg[0][:, :32], st)
        _le(s_le, sg[0][:, 32:], st)

    want_pk, want_sig = rows(cyc(curve, rot, lambda e: e["pk65"])), rows(cyc(curve, rot, lambda e: e["rsig"]))
    want_rc = np.array(cyc(curve, rot, lambda e: e["recid"]), dtype=np.uint8)
    calls = [
        Call("public_key_dev", key, [pk65, st1, (pkxy, 0xEE)], [want_pk, ZEROS, xy(cyc(curve, rot, lambda e: e["Q"]))]),
        Call("ecdsa_sign_recoverable_digest_dev", sign, [sg, rc, st2, (r_le, 0xEE), (s_le, 0xEE)],
             [want_sig, want_rc, ZEROS, words(cyc(curve, rot, lambda e: e["r"])), words(cyc(curve, rot, lambda e: e["s"]))]),
        Call("ecdsa_verify_dev", lambda st: dev.ecdsa_verify_dev(z.data_ptr(), r_le.data_ptr(), s_le.data_ptr(), pkxy.data_ptr(), res[0].data_ptr(), N, ptr(st)),
             [res], [ONES]),
        Call("ecdsa_recover_dev", lambda st: dev.ecdsa_recover_dev(dg.data_ptr(), sg[0].data_ptr(), rc[0].data_ptr(), rec[0].data_ptr(), 65, st4[0].data_ptr(), N, ptr(st)),
             [rec, st4], [want_pk, ZEROS]),
    ]
    second = "s2" if first == "s1" else "s1"
    _run(calls, (first, second, None, first))


@pytest.mark.parametrize("order", [("s1", "s2"), ("s2", None)], ids=["s1 s2", "s2 NULL"])
def test_pipeline_ed25519_sign_verify(gpu_ctx, order):
    """ed25519_sign_msg_dev -> ed25519_verify_msg_dev on the produced signatures and keys"""
    dev = _canon(gpu_ctx, "ed25519")
    sign = c_ed25519_sign_msg(gpu_ctx, ROT_B)
    m, off, total = up_msgs(cyc("ed25519", ROT_B, lambda e: e["msg"]))
    sg, pk = sign.outs[0][0], sign.outs[1][0]
    res = out_status()
    verify = Call("ed25519_verify_msg_dev",
                  lambda st: dev.ed25519_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), res[0].data_ptr(), N, ptr(st)),
                  [res], [ONES])
    _run([sign, verify], order)


@pytest.mark.parametrize("order", [("s1", "s2", None), ("s2", None, "s1")], ids=["s1 s2 NULL", "s2 NULL s1"])
def test_pipeline_bip340_key_sign_verify(gpu_ctx, order):
    """public_key_dev (x-only) -> bip340_sign_msg_dev -> bip340_verify_msg_dev on the produced keys and signatures"""
    dev = _canon(gpu_ctx, "secp256k1")
    key = c_public_key(gpu_ctx, ROT_B, "secp256k1", 32, S.SCHEME_BIP340)
    sign = c_bip340_sign_msg(gpu_ctx, ROT_B)
    m, off, total = up_msgs(cyc("secp256k1", ROT_B, lambda e: e["msg"]))
    pk, sg = key.outs[0][0], sign.outs[0][0]
    res = out_status()
    verify = Call("bip340_verify_msg_dev",
                  lambda st: dev.bip340_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), res[0].data_ptr(), N, ptr(st)),
                  [res], [ONES])
    _run([key, sign, verify], order)


@pytest.mark.parametrize("order", [("s1", "s2", None), ("s2", None, "s1")], ids=["s1 s2 NULL", "s2 NULL s1"])
def test_pipeline_derive_priv_public_key_derive_pub(gpu_ctx, order):
    """derive_priv_dev -> public_key_dev of the produced child keys, and derive_pub_dev of the parents' public keys: the
    model says that both give the same children"""
    dev = _canon(gpu_ctx, "secp256k1")
    priv = c_derive_priv(gpu_ctx, ROT_B, False)
    child = priv.outs[0][0]
    out, st_ = out_bytes(33), out_status()
    want = rows(cyc("secp256k1", ROT_B, lambda e: e["pub"][0]))
    pub_of_child = Call("public_key_dev", lambda st: dev.public_key_dev(child.data_ptr(), out[0].data_ptr(), 33, st_[0].data_ptr(), N, ptr(st)),
                        [out, st_], [want, ZEROS])
    derive_pub = c_derive_pub(gpu_ctx, ROT_B, False)
    assert np.array_equal(derive_pub.want[0], want)
    _run([priv, pub_of_child, derive_pub], order)


# ---- 5. a ctx whose first canonical calls name user streams --------------------------------------------------------------
@pytest.mark.parametrize("curve", NAMES)
def test_first_calls_of_a_ctx_on_user_streams(curve):
    """a fresh ctx: k * G on s1, then a signer on s2.  Both comb tables are built on first use, on a user stream, and the
    work areas grow; nothing is warmed up, so there is no gate either: the results must be the model's"""
    import torch
    import forge_ec_amd as F
    g = gear()
    ctx = F.Context(0)
    try:
        a = c_mul_base(ctx, ROT_A, curve)
        b = c_ed25519_sign_msg(ctx, ROT_B) if curve == "ed25519" else c_ecdsa_sign_digest(ctx, ROT_B, curve, False)
        torch.cuda.synchronize()
        a.run(g["s1"])
        b.run(g["s2"])
        torch.cuda.synchronize()
        assert not a.bad() and not b.bad(), (a.bad(), b.bad())
        ctx.check()
    finally:
        ctx.close()


# ---- the module's last call names the ctx's own stream -------------------------------------------------------------------
def test_null_stream_call_behind_the_user_streams(gpu_ctx):
    """a call on s2, then one on the ctx's own stream (NULL): ordered like any other pair, and the ctx's last launch no
    longer names a stream of this module"""
    _run([c_x25519_base(gpu_ctx, ROT_A), c_mul_base(gpu_ctx, ROT_B, "p256")], ("s2", None))
    gpu_ctx.check()
