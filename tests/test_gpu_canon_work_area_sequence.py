"""
GPU test of canonical mode's work areas in ctx->d_verify, met in sequence by ONE fresh ctx.

Every verifier, recovery, tweak-add, CKDpub and the Taproot call lays its regions out in ctx->d_verify, a grow-only buffer of
the ctx (ensure_owned in forge_ec_amd/csrc/canon.hip).  The other GPU tests run on one long-lived ctx whose buffer has long
grown to its largest size; here a new Context(0) makes eight *_dev calls on the ctx's own stream, each one's area meeting a
buffer whose size another, mostly smaller, call has set, and then the same eight in reverse order, when nothing grows any
more and every area sits in a larger buffer:

  1. ecdsa_verify_msg_dev, secp256k1, n = 9          5. ed25519_verify_msg_dev, n = 7
  2. bip340_verify_msg_dev, n = 65                   6. ecdsa_verify_dev (after the hash), P-256, n = 64
  3. ecdsa_recover_dev, P-256, out_len 33, n = 8     7. bip32 derive_pub_path_dev, depth 2, one shared parent, n = 9
  4. pubkey_tweak_add_dev, secp256k1, n = 257        8. taproot_output_key_dev, n = 1

The sizes are the small ones at which a group of eight (NORM_GROUP), a wavefront and a block are full, one over or one
under.  The sixteen calls are issued back to back with no synchronisation between them; every output is then compared with
the big-integer models (oracle/canon_model.py and the canon_*_ref.py modules beside this file), never with another GPU run.

Inputs: eight seeded records per call, cycled over the batch; the forward pass starts the cycle at record 0 and the
reverse pass at record 3, so the two passes differ at every element.  Records 2, 3, 5 and 7 are refused ones (a changed
message, a scalar out of range, an undecodable key, a hardened index, ...), so every batch but the single Taproot key mixes
valid and invalid elements; that one is valid in the forward pass and refused in the reverse pass.  Outputs are pre-filled
with a sentinel.
"""
import functools
import random

import numpy as np
import pytest

import canon_bip32_ref as B32
import canon_msg_ref as R
import canon_recover_ref as RV
import canon_sign_ref as S
import canon_wallet_ref as W
from oracle import canon_model as M

pytestmark = pytest.mark.gpu

NREC = 8
ROT_FORWARD, ROT_REVERSE = 0, 3
SENTINEL = 0xEE
SECP, P256, ED = M.SECP256K1, M.P256, M.ED25519


def _keys(C, rng):
    d = rng.randrange(1, C.N)
    return d, C.mul(d, C.G)


def _flip(b, at=0):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def _unliftable_x(rng):
    while True:
        x = rng.randrange(SECP.P)
        if R.lift_x(x) is None:
            return x.to_bytes(32, "big")


# ---- the eight records of every call, computed once: the inputs and what the model says comes out ------------------------
@functools.lru_cache(maxsize=None)
def ecdsa_msg_records():
    rng, out = random.Random(0x5E01), []
    for j in range(NREC):
        d, Q = _keys(SECP, rng)
        msg = rng.randbytes((1, 55, 56, 64, 119, 120, 200, 31)[j])
        sig, st = S.ecdsa_sign_msg(SECP, d, msg)
        assert st == 0
        pk = R.sec1_encode(Q)
        if j == 2:
            msg = _flip(msg)
        elif j == 3:
            sig = sig[:32] + SECP.N.to_bytes(32, "big")
        elif j == 5:
            pk = b"\x05" + pk[1:]
        elif j == 7:
            sig = bytes(32) + sig[32:]
        out.append(dict(msg=msg, sig=sig, pk=pk, want=R.ecdsa_verify(SECP, msg, sig, pk)))
    return out


@functools.lru_cache(maxsize=None)
def bip340_msg_records():
    rng, out = random.Random(0x5E02), []
    for j in range(NREC):
        d, _ = _keys(SECP, rng)
        msg = rng.randbytes((1, 32, 55, 56, 64, 2, 137, 33)[j])
        sig, st = S.bip340_sign(d, msg, rng.randbytes(32))
        assert st == 0
        pk = R.bip340_pubkey(d)
        if j == 2:
            msg = msg + b"\x00"
        elif j == 3:
            sig = SECP.P.to_bytes(32, "big") + sig[32:]
        elif j == 5:
            pk = _unliftable_x(rng)
        elif j == 7:
            sig = sig[:32] + SECP.N.to_bytes(32, "big")
        out.append(dict(msg=msg, sig=sig, pk=pk, want=R.bip340_verify(msg, sig, pk)))
    return out


@functools.lru_cache(maxsize=None)
def recover_records():
    rng, out = random.Random(0x5E03), []
    for j in range(NREC):
        d, Q = _keys(P256, rng)
        digest = rng.randbytes(32)
        sig, recid, st = RV.sign_recoverable_digest(P256, d, digest, S.LOW_S)
        assert st == 0 and RV.recover_point(P256, digest, sig, recid) == Q
        if j == 2:
            recid = 4
        elif j == 3:
            sig = bytes(32) + sig[32:]
        elif j == 5:
            sig = sig[:32] + P256.N.to_bytes(32, "big")
        elif j == 7:
            recid |= 2          # x = r + n: not below p for a random r
        key, status = RV.recover(P256, digest, sig, recid, 33)
        out.append(dict(digest=digest, sig=sig, recid=recid, key=key, status=status))
    return out


@functools.lru_cache(maxsize=None)
def tweak_records():
    rng, out = random.Random(0x5E04), []
    for j in range(NREC):
        d, Q = _keys(SECP, rng)
        pk, tweak = R.sec1_encode(Q), rng.randrange(1, SECP.N).to_bytes(32, "big")
        if j == 2:
            tweak = SECP.N.to_bytes(32, "big")
        elif j == 3:
            pk = b"\x04" + pk[1:]
        elif j == 5:
            tweak = (SECP.N - d).to_bytes(32, "big")      # P + t G at infinity
        elif j == 7:
            pk = pk[:1] + _unliftable_x(rng)
        key, status = B32.pubkey_tweak_add(SECP, pk, tweak, 33)
        out.append(dict(pk=pk, tweak=tweak, key=key, status=status))
    return out


@functools.lru_cache(maxsize=None)
def ed25519_msg_records():
    rng, out = random.Random(0x5E05), []
    for j in range(NREC):
        seed, msg = rng.randbytes(32), rng.randbytes((0, 1, 47, 48, 111, 112, 175, 300)[j])
        sig, pk = S.ed25519_sign(seed, msg)
        if j == 2:
            msg = _flip(msg, len(msg) - 1)
        elif j == 3:
            sig = sig[:32] + ED.N.to_bytes(32, "little")
        elif j == 5:
            pk = b"\xff" * 31 + b"\x7f"                   # y >= p
        elif j == 7:
            sig = _flip(sig, 31)
        out.append(dict(msg=msg, sig=sig, pk=pk, want=R.ed25519_verify(msg, sig, pk)))
    return out


@functools.lru_cache(maxsize=None)
def ecdsa_records():
    rng, out = random.Random(0x5E06), []
    for j in range(NREC):
        d, Q = _keys(P256, rng)
        digest = rng.randbytes(32)
        sig, st = S.ecdsa_sign_digest(P256, d, digest)
        assert st == 0
        if j == 2:
            digest = _flip(digest, 31)
        elif j == 3:
            sig = sig[:32] + bytes(32)
        elif j == 5:
            sig = P256.N.to_bytes(32, "big") + sig[32:]
        elif j == 7:
            Q = P256.add(Q, P256.G)
        z, r, s = (int.from_bytes(b, "big") for b in (digest, sig[:32], sig[32:]))
        out.append(dict(z=z, r=r, s=s, Q=Q, want=1 if RV.verify_digest(P256, digest, sig, Q) else 0))
    return out


@functools.lru_cache(maxsize=None)
def path_records():
    """one parent for the batch, two indices per element"""
    rng, out = random.Random(0x5E07), []
    d, Q = _keys(SECP, rng)
    pk, cc = R.sec1_encode(Q), rng.randbytes(32)
    for j in range(NREC):
        path = [rng.randrange(B32.HARDENED), rng.randrange(B32.HARDENED)]
        if j in (2, 5):
            path[0] |= B32.HARDENED
        elif j in (3, 7):
            path[1] |= B32.HARDENED
        out.append(dict(path=path, want=W.derive_pub_path(pk, cc, path)))
    return pk, cc, out


@functools.lru_cache(maxsize=None)
def taproot_records():
    rng, out = random.Random(0x5E08), []
    for j in range(NREC):
        d, _ = _keys(SECP, rng)
        x, root = (_unliftable_x(rng) if j in (2, 3, 5, 7) else R.bip340_pubkey(d)), rng.randbytes(32)
        out.append(dict(x=x, root=root, want=W.taproot_output_key(x, root)))
    return out


# ---- tensors ------------------------------------------------------------------------------------------------------------
def cyc(records, rot, n, f):
    return [f(records[(i + rot) % NREC]) for i in range(n)]


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def rows(bs):
    return np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(len(bs), -1).copy()


def words(vals):
    return np.array([M.limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def up_msgs(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return up(np.frombuffer(b"".join(msgs) + b"\x00", dtype=np.uint8)), up(off), int(off[-1])


def out(n, width=1):
    import torch
    return torch.full((n, width), SENTINEL, dtype=torch.uint8, device="cuda")


class Call:
    """one *_dev call on tensors of its own: run() issues it on the ctx's own stream; outs: its output tensors; want: what
    the model says each holds afterwards, one row per element"""

    def __init__(self, name, n, run, outs, want):
        self.name, self.n, self.run, self.outs = name, n, run, outs
        self.want = [np.ascontiguousarray(w).view(np.uint8).reshape(n, -1) for w in want]
        assert len(outs) == len(want)

    def bad(self):
        wrong = set()
        for t, w in zip(self.outs, self.want):
            got = t.cpu().numpy().reshape(self.n, -1)
            wrong.update(int(i) for i in np.nonzero((got != w).any(axis=1))[0])
        return sorted(wrong)


def flags(vals):
    return np.array(vals, dtype=np.uint8)


def mixed(vals, good):
    """the batch holds accepted and refused elements"""
    ok = sum(1 for v in vals if v == good)
    return 0 < ok < len(vals)


# ---- the eight calls ------------------------------------------------------------------------------------------------------
def c_ecdsa_verify_msg(ctx, rot, n=9):
    from forge_ec_amd.canon import CanonSecp256k1
    dev, rs = CanonSecp256k1(ctx), ecdsa_msg_records()
    m, off, total = up_msgs(cyc(rs, rot, n, lambda e: e["msg"]))
    sg, pk, res = up(rows(cyc(rs, rot, n, lambda e: e["sig"]))), up(rows(cyc(rs, rot, n, lambda e: e["pk"]))), out(n)
    want = cyc(rs, rot, n, lambda e: e["want"])
    assert mixed(want, 1)
    return Call("ecdsa_verify_msg_dev secp256k1", n,
                lambda: dev.ecdsa_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), 33, res.data_ptr(), n),
                [res], [flags(want)])


def c_bip340_verify_msg(ctx, rot, n=65):
    from forge_ec_amd.canon import CanonSecp256k1
    dev, rs = CanonSecp256k1(ctx), bip340_msg_records()
    m, off, total = up_msgs(cyc(rs, rot, n, lambda e: e["msg"]))
    sg, pk, res = up(rows(cyc(rs, rot, n, lambda e: e["sig"]))), up(rows(cyc(rs, rot, n, lambda e: e["pk"]))), out(n)
    want = cyc(rs, rot, n, lambda e: e["want"])
    assert mixed(want, 1)
    return Call("bip340_verify_msg_dev", n,
                lambda: dev.bip340_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), res.data_ptr(), n),
                [res], [flags(want)])


def c_recover(ctx, rot, n=8):
    from forge_ec_amd.canon import CanonP256
    dev, rs = CanonP256(ctx), recover_records()
    dg, sg = up(rows(cyc(rs, rot, n, lambda e: e["digest"]))), up(rows(cyc(rs, rot, n, lambda e: e["sig"])))
    rc, key, st = up(flags(cyc(rs, rot, n, lambda e: e["recid"]))), out(n, 33), out(n)
    want = cyc(rs, rot, n, lambda e: e["status"])
    assert mixed(want, 0)
    return Call("ecdsa_recover_dev p256 33", n,
                lambda: dev.ecdsa_recover_dev(dg.data_ptr(), sg.data_ptr(), rc.data_ptr(), key.data_ptr(), 33, st.data_ptr(), n),
                [key, st], [rows(cyc(rs, rot, n, lambda e: e["key"])), flags(want)])


def c_pubkey_tweak_add(ctx, rot, n=257):
    from forge_ec_amd.canon import CanonSecp256k1
    dev, rs = CanonSecp256k1(ctx), tweak_records()
    pk, tw = up(rows(cyc(rs, rot, n, lambda e: e["pk"]))), up(rows(cyc(rs, rot, n, lambda e: e["tweak"])))
    key, st = out(n, 33), out(n)
    want = cyc(rs, rot, n, lambda e: e["status"])
    assert mixed(want, 0)
    return Call("pubkey_tweak_add_dev secp256k1", n,
                lambda: dev.pubkey_tweak_add_dev(pk.data_ptr(), 33, tw.data_ptr(), key.data_ptr(), 33, st.data_ptr(), n),
                [key, st], [rows(cyc(rs, rot, n, lambda e: e["key"])), flags(want)])


def c_ed25519_verify_msg(ctx, rot, n=7):
    from forge_ec_amd.canon import CanonEd25519
    dev, rs = CanonEd25519(ctx), ed25519_msg_records()
    m, off, total = up_msgs(cyc(rs, rot, n, lambda e: e["msg"]))
    sg, pk, res = up(rows(cyc(rs, rot, n, lambda e: e["sig"]))), up(rows(cyc(rs, rot, n, lambda e: e["pk"]))), out(n)
    want = cyc(rs, rot, n, lambda e: e["want"])
    assert mixed(want, 1)
    return Call("ed25519_verify_msg_dev", n,
                lambda: dev.ed25519_verify_msg_dev(m.data_ptr(), off.data_ptr(), total, sg.data_ptr(), pk.data_ptr(), res.data_ptr(), n),
                [res], [flags(want)])


def c_ecdsa_verify(ctx, rot, n=64):
    from forge_ec_amd.canon import CanonP256
    dev, rs = CanonP256(ctx), ecdsa_records()
    z, r, s = (up(words(cyc(rs, rot, n, lambda e, k=k: e[k]))) for k in "zrs")
    pk = up(np.array(cyc(rs, rot, n, lambda e: M.xy_limbs(e["Q"])), dtype=np.uint64).reshape(n, 8))
    res = out(n)
    want = cyc(rs, rot, n, lambda e: e["want"])
    assert mixed(want, 1)
    return Call("ecdsa_verify_dev p256", n,
                lambda: dev.ecdsa_verify_dev(z.data_ptr(), r.data_ptr(), s.data_ptr(), pk.data_ptr(), res.data_ptr(), n), [res], [flags(want)])


def c_derive_pub_path(ctx, rot, n=9):
    from forge_ec_amd.canon import CanonBip32
    dev = CanonBip32(ctx)
    ppk, pcc, rs = path_records()
    pk, cc = up(rows([ppk])), up(rows([pcc]))
    idx = up(np.array(cyc(rs, rot, n, lambda e: e["path"]), dtype=np.uint32).reshape(n, 2))
    key, occ, fp, h160, st = out(n, 33), out(n, 32), out(n, 4), out(n, 20), out(n)
    want = cyc(rs, rot, n, lambda e: e["want"])
    assert mixed([w[4] for w in want], 0)
    return Call("bip32 derive_pub_path_dev depth 2, shared parent", n,
                lambda: dev.derive_pub_path_dev(pk.data_ptr(), cc.data_ptr(), 1, idx.data_ptr(), 2, key.data_ptr(), occ.data_ptr(), fp.data_ptr(),
                                                h160.data_ptr(), st.data_ptr(), n),
                [key, occ, fp, h160, st], [rows([w[k] for w in want]) for k in range(4)] + [flags([w[4] for w in want])])


def c_taproot(ctx, rot, n=1):
    from forge_ec_amd.canon import CanonSecp256k1
    dev, rs = CanonSecp256k1(ctx), taproot_records()
    x, root = up(rows(cyc(rs, rot, n, lambda e: e["x"]))), up(rows(cyc(rs, rot, n, lambda e: e["root"])))
    key, par, st = out(n, 32), out(n), out(n)
    want = cyc(rs, rot, n, lambda e: e["want"])
    return Call("taproot_output_key_dev", n,
                lambda: dev.taproot_output_key_dev(x.data_ptr(), 32, root.data_ptr(), key.data_ptr(), par.data_ptr(), st.data_ptr(), n),
                [key, par, st], [rows([w[0] for w in want]), flags([w[1] for w in want]), flags([w[2] for w in want])])


SEQUENCE = [c_ecdsa_verify_msg, c_bip340_verify_msg, c_recover, c_pubkey_tweak_add, c_ed25519_verify_msg, c_ecdsa_verify, c_derive_pub_path,
            c_taproot]


def test_eight_work_areas_in_sequence_and_in_reverse_on_a_fresh_ctx():
    import torch
    import forge_ec_amd as F
    taproot = [r["want"][2] for r in taproot_records()]
    assert taproot[ROT_FORWARD] == 0 and taproot[ROT_REVERSE] != 0    # the single key: accepted going up, refused coming down
    with F.Context(0) as ctx:
        calls = [make(ctx, ROT_FORWARD) for make in SEQUENCE] + [make(ctx, ROT_REVERSE) for make in reversed(SEQUENCE)]
        assert [c.n for c in calls[:8]] == [9, 65, 8, 257, 7, 64, 9, 1]
        torch.cuda.synchronize()
        for c in calls:       # back to back: the library's own ordering is all that separates one area from the next
            c.run()
        torch.cuda.synchronize()
        for k, c in enumerate(calls):
            assert c.bad() == [], "call %d of 16, %s: elements that differ from the model" % (k + 1, c.name)
        ctx.check()
