"""
GPU tests of the canonical-mode tweak-add and BIP-32 derivation (include/fecgpu_canon.h: fec_canon_pubkey_tweak_add,
fec_canon_seckey_tweak_add, fec_canon_bip32_derive_pub, fec_canon_bip32_derive_priv and their *_dev forms) against the fixture
tests/golden/canon_bip32_vectors.json, which the model tests/canon_bip32_ref.py wrote and tests/test_canon_bip32_model.py pins
by BIP-32 test vector 1.  Every comparison is byte-exact, status included.  Also: the batch sizes at the edges of the
eight-element normalisation groups and of a wavefront, each refused and each exceptional case alone among ordinary elements,
one shared parent against the parent replicated, derive_priv -> public_key == derive_pub round trips, the tweak-add against the
double multiplication it replaces, vector 1's chain on the device, chunks, shard workers, refused arguments.
"""
import os
import random

import numpy as np
import pytest

import canon_bip32_ref as B

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = B.load_fixture(os.path.join(HERE, "golden", "canon_bip32_vectors.json"))
CURVES = sorted(B.CURVES)
COUNTS = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513]
ARG, UNSUPPORTED = -1, -5
AMONG = 64 * 3 + 5
LANES = (0, 31, 32, 63, AMONG - 1)
SECP = B.SECP256K1
H = B.HARDENED


def forms(curve):
    return (33, 65, 32) if curve == "secp256k1" else (33, 65)


def _cv(ctx, curve):
    from forge_ec_amd.canon import CANON_CURVES
    return CANON_CURVES[curve](ctx)


def _hd(ctx):
    from forge_ec_amd.canon import CanonBip32
    return CanonBip32(ctx)


_POINTS = {}


def expected(case, out_len):
    """the record of one tweak case in one output form, from its out33"""
    if case["status"]:
        return bytes(out_len)
    key = (case["curve"], case["out33"])
    if key not in _POINTS:
        _POINTS[key] = B.decode(B.CURVES[case["curve"]], bytes.fromhex(case["out33"]))
    return B.encode(_POINTS[key], out_len)


def _rows(hexes, width):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), dtype=np.uint8).reshape(len(hexes), width).copy()


def _brows(items, width):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), width).copy()


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _dev_out(n, width, fill=0xEE):
    import torch
    return torch.full((n, width) if width > 1 else (n,), fill, dtype=torch.uint8, device="cuda")


# ---- the four calls, host and *_dev forms alike: numpy in, numpy out ------------------------------------------------------
def tweak(ctx, curve, pks, tw, pk_len, out_len, dev):
    import torch
    if not dev:
        return _cv(ctx, curve).pubkey_tweak_add(pks, tw, pk_len, out_len)
    n = pks.shape[0]
    tp, tt, out, st = _to_dev(pks), _to_dev(tw), _dev_out(n, out_len), _dev_out(n, 1, 77)
    _cv(ctx, curve).pubkey_tweak_add_dev(tp.data_ptr(), pk_len, tt.data_ptr(), out.data_ptr(), out_len, st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def sectweak(ctx, curve, keys, tw, dev):
    import torch
    if not dev:
        return _cv(ctx, curve).seckey_tweak_add(keys, tw)
    n = keys.shape[0]
    tk, tt, out, st = _to_dev(keys), _to_dev(tw), _dev_out(n, 32), _dev_out(n, 1, 77)
    _cv(ctx, curve).seckey_tweak_add_dev(tk.data_ptr(), tt.data_ptr(), out.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def derive_pub(ctx, pks, ccs, idx, dev):
    import torch
    idx = np.asarray(idx, dtype=np.uint32)
    if not dev:
        return _hd(ctx).derive_pub(pks, ccs, idx)
    n = idx.shape[0]
    tp, tc, ti = _to_dev(pks), _to_dev(ccs), _to_dev(idx)
    out, occ, st = _dev_out(n, 33), _dev_out(n, 32), _dev_out(n, 1, 77)
    _hd(ctx).derive_pub_dev(tp.data_ptr(), tc.data_ptr(), pks.shape[0], ti.data_ptr(), out.data_ptr(), occ.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), occ.cpu().numpy(), st.cpu().numpy()


def derive_priv(ctx, keys, ccs, idx, flags, dev):
    import torch
    idx = np.asarray(idx, dtype=np.uint32)
    if not dev:
        return _hd(ctx).derive_priv(keys, ccs, idx, flags)
    n = idx.shape[0]
    tk, tc, ti = _to_dev(keys), _to_dev(ccs), _to_dev(idx)
    out, occ, st = _dev_out(n, 32), _dev_out(n, 32), _dev_out(n, 1, 77)
    _hd(ctx).derive_priv_dev(tk.data_ptr(), tc.data_ptr(), keys.shape[0], ti.data_ptr(), flags, out.data_ptr(), occ.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), occ.cpu().numpy(), st.cpu().numpy()


def _tweak_inputs(pick, pk_len):
    return _rows([c["key"] for c in pick], pk_len), _rows([c["tweak"] for c in pick], 32), np.array([c["status"] for c in pick], dtype=np.uint8)


def _tweak_want(pick, out_len):
    return _brows([expected(c, out_len) for c in pick], out_len)


def _pub_inputs(pick):
    return (_rows([c["pk"] for c in pick], 33), _rows([c["cc"] for c in pick], 32), np.array([c["index"] for c in pick], dtype=np.uint32),
            _rows([c["child"] for c in pick], 33), _rows([c["child_cc"] for c in pick], 32), np.array([c["status"] for c in pick], dtype=np.uint8))


def _priv_inputs(pick):
    return (_rows([c["key"] for c in pick], 32), _rows([c["cc"] for c in pick], 32), np.array([c["index"] for c in pick], dtype=np.uint32),
            _rows([c["child"] for c in pick], 32), _rows([c["child_cc"] for c in pick], 32), np.array([c["status"] for c in pick], dtype=np.uint8))


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_every_tweak_case_every_form(gpu_ctx, curve):
    cases = [c for c in FIXTURE["tweak"] if c["curve"] == curve]
    for pk_len in forms(curve):
        pick = [c for c in cases if len(c["key"]) == 2 * pk_len]
        pks, tw, wst = _tweak_inputs(pick, pk_len)
        assert {2, 3, 8} <= set(wst.tolist()) and (wst == 0).sum() >= 64 + 4
        for out_len in forms(curve):
            want = _tweak_want(pick, out_len)
            for dev in (False, True):
                out, st = tweak(gpu_ctx, curve, pks, tw, pk_len, out_len, dev)
                bad = [i for i in range(len(pick)) if st[i] != wst[i] or bytes(out[i]) != bytes(want[i])]
                assert not bad, [(pk_len, out_len, dev, pick[i]["class"], pick[i]["name"], int(st[i])) for i in bad]
    pick = [c for c in FIXTURE["seckey"] if c["curve"] == curve]
    keys, tw = _rows([c["key"] for c in pick], 32), _rows([c["tweak"] for c in pick], 32)
    want, wst = _rows([c["out"] for c in pick], 32), np.array([c["status"] for c in pick], dtype=np.uint8)
    assert {3, 6, 8} <= set(wst.tolist())
    for dev in (False, True):
        assert _same(sectweak(gpu_ctx, curve, keys, tw, dev), (want, wst)), dev
    gpu_ctx.check()


def test_every_bip32_case(gpu_ctx):
    pk, cc, idx, child, ccc, wst = _pub_inputs(FIXTURE["bip32_pub"])
    assert {2, 9} <= set(wst.tolist()) and (wst == 0).sum() >= 128
    for dev in (False, True):
        out, occ, st = derive_pub(gpu_ctx, pk, cc, idx, dev)
        bad = [i for i in range(len(idx)) if st[i] != wst[i] or bytes(out[i]) != bytes(child[i]) or bytes(occ[i]) != bytes(ccc[i])]
        assert not bad, [(dev, FIXTURE["bip32_pub"][i]["name"], int(st[i])) for i in bad]
    for flags in (0, B.NO_COMB):
        pick = [c for c in FIXTURE["bip32_priv"] if c["flags"] == flags]
        key, cc, idx, child, ccc, wst = _priv_inputs(pick)
        assert {6, 9} <= set(wst.tolist()) if flags else 6 in wst
        for dev in (False, True):
            out, occ, st = derive_priv(gpu_ctx, key, cc, idx, flags, dev)
            bad = [i for i in range(len(idx)) if st[i] != wst[i] or bytes(out[i]) != bytes(child[i]) or bytes(occ[i]) != bytes(ccc[i])]
            assert not bad, [(dev, flags, pick[i]["name"], int(st[i])) for i in bad]
    gpu_ctx.check()


@pytest.mark.parametrize("curve", CURVES)
def test_element_counts(gpu_ctx, curve):
    """n cases at the edges of the eight-element groups and of a wavefront, cycling from the refused cases on, so that n = 1 is
    not an ordinary case; forms and host / *_dev take turns"""
    cases = [c for c in FIXTURE["tweak"] if c["curve"] == curve and len(c["key"]) == 66]
    start = next(i for i, c in enumerate(cases) if c["status"])
    scases = [c for c in FIXTURE["seckey"] if c["curve"] == curve]
    sstart = next(i for i, c in enumerate(scases) if c["status"])
    fs = forms(curve)
    for j, n in enumerate(COUNTS):
        pick = [cases[(start + i) % len(cases)] for i in range(n)]
        pks, tw, wst = _tweak_inputs(pick, 33)
        out_len = fs[j % len(fs)]
        assert _same(tweak(gpu_ctx, curve, pks, tw, 33, out_len, j % 2 == 0), (_tweak_want(pick, out_len), wst)), (n, out_len)
        pick = [scases[(sstart + i) % len(scases)] for i in range(n)]
        got = sectweak(gpu_ctx, curve, _rows([c["key"] for c in pick], 32), _rows([c["tweak"] for c in pick], 32), j % 2 == 1)
        assert _same(got, (_rows([c["out"] for c in pick], 32), np.array([c["status"] for c in pick], dtype=np.uint8))), n
    gpu_ctx.check()


def test_element_counts_bip32(gpu_ctx):
    pub, priv = FIXTURE["bip32_pub"], [c for c in FIXTURE["bip32_priv"] if c["flags"] == 0]
    pstart = next(i for i, c in enumerate(pub) if c["status"])
    vstart = next(i for i, c in enumerate(priv) if c["status"])
    for j, n in enumerate(COUNTS):
        pk, cc, idx, child, ccc, wst = _pub_inputs([pub[(pstart + i) % len(pub)] for i in range(n)])
        assert _same(derive_pub(gpu_ctx, pk, cc, idx, j % 2 == 0), (child, ccc, wst)), n
        key, cc, idx, child, ccc, wst = _priv_inputs([priv[(vstart + i) % len(priv)] for i in range(n)])
        assert _same(derive_priv(gpu_ctx, key, cc, idx, 0, j % 2 == 1), (child, ccc, wst)), n
    gpu_ctx.check()


@pytest.mark.parametrize("curve", CURVES)
def test_refused_and_exceptional_tweaks_alone_among_ordinary_ones(gpu_ctx, curve):
    """each refused case, and each exceptional addition (t = 0, the doubling, the sum at infinity), alone at lanes 0, 31, 32, 63
    and at the last of 197 ordinary elements, every one of which must still be exact"""
    for pk_len in (33, 65):
        cases = [c for c in FIXTURE["tweak"] if c["curve"] == curve and len(c["key"]) == 2 * pk_len]
        ordinary = [c for c in cases if c["class"] == "random"]
        ordinary = [ordinary[i % len(ordinary)] for i in range(AMONG)]
        special = [c for c in cases if c["status"] or c["class"] in ("doubling", "tweak")]
        assert len(special) >= 9 and {c["class"] for c in special} >= {"doubling", "infinity", "tweak"}
        pk0, tw0, st0 = _tweak_inputs(ordinary, pk_len)
        want0 = _tweak_want(ordinary, 33)
        for j, c in enumerate(special):
            cp, ct, cst = _tweak_inputs([c], pk_len)
            cw = _tweak_want([c], 33)
            for lane in LANES:
                pks, tw, want, wst = pk0.copy(), tw0.copy(), want0.copy(), st0.copy()
                pks[lane], tw[lane], want[lane], wst[lane] = cp[0], ct[0], cw[0], cst[0]
                assert _same(tweak(gpu_ctx, curve, pks, tw, pk_len, 33, (j + lane) % 2 == 0), (want, wst)), (c["name"], lane)
    gpu_ctx.check()


def test_refused_derivations_alone_among_ordinary_ones(gpu_ctx):
    pub = FIXTURE["bip32_pub"]
    ordinary = [c for c in pub if c["class"] == "random"]
    ordinary = [ordinary[i % len(ordinary)] for i in range(AMONG)]
    base = _pub_inputs(ordinary)
    for j, c in enumerate([c for c in pub if c["status"]]):
        one = _pub_inputs([c])
        for lane in LANES:
            a = [x.copy() for x in base]
            for x, y in zip(a, one):
                x[lane] = y[0]
            assert _same(derive_pub(gpu_ctx, a[0], a[1], a[2], (j + lane) % 2 == 0), a[3:]), (c["name"], lane)
    priv = FIXTURE["bip32_priv"]
    for flags in (0, B.NO_COMB):
        ordinary = [c for c in priv if c["class"] == "random" and (c["index"] >= H or not flags)]
        ordinary = [ordinary[i % len(ordinary)] for i in range(AMONG)]
        base = _priv_inputs(ordinary)
        refused = [c for c in priv if c["status"] and c["flags"] == flags]
        assert refused
        for j, c in enumerate(refused):
            one = _priv_inputs([c])
            for lane in LANES:
                a = [x.copy() for x in base]
                for x, y in zip(a, one):
                    x[lane] = y[0]
                assert _same(derive_priv(gpu_ctx, a[0], a[1], a[2], flags, (j + lane) % 2 == 0), a[3:]), (c["name"], lane, flags)
    gpu_ctx.check()


# ---- properties at n = 513 ------------------------------------------------------------------------------------------------------
def _random_parents(rng, n):
    keys = _brows([B.b32(rng.randrange(1, SECP.N)) for _ in range(n)], 32)
    ccs = np.frombuffer(bytes(rng.randrange(256) for _ in range(32 * n)), dtype=np.uint8).reshape(n, 32).copy()
    return keys, ccs


def test_shared_parent_equals_the_replicated_parent(gpu_ctx):
    rng = random.Random(0x5131)
    n = 513
    keys, ccs = _random_parents(rng, 1)
    pk, pst = _cv(gpu_ctx, "secp256k1").public_key(keys, 33)
    idx = np.array([rng.randrange(H) for _ in range(n)], dtype=np.uint32)
    idx[7], idx[64], idx[512] = H, 2**32 - 1, 0
    for dev in (False, True):
        one = derive_pub(gpu_ctx, pk, ccs, idx, dev)
        rep = derive_pub(gpu_ctx, np.repeat(pk, n, axis=0), np.repeat(ccs, n, axis=0), idx, dev)
        assert _same(one, rep) and one[2][7] == one[2][64] == 9 and (one[2] != 0).sum() == 2, dev
        for i in (0, 8, 63, 511, 512):
            assert (bytes(one[0][i]), bytes(one[1][i]), int(one[2][i])) == B.ckd_pub(bytes(pk[0]), bytes(ccs[0]), int(idx[i])), i
    # a bytes parent is the shared-parent case too; so is one bad parent, which refuses every element
    assert _same(_hd(gpu_ctx).derive_pub(bytes(pk[0]), bytes(ccs[0]), idx), one)
    bad = derive_pub(gpu_ctx, _brows([b"\x05" + bytes(pk[0][1:])], 33), ccs, idx[:70], True)
    assert (bad[2] == 2).all() and not bad[0].any() and not bad[1].any()
    idx[::3] |= H
    for dev in (False, True):
        one = derive_priv(gpu_ctx, keys, ccs, idx, 0, dev)
        rep = derive_priv(gpu_ctx, np.repeat(keys, n, axis=0), np.repeat(ccs, n, axis=0), idx, 0, dev)
        assert _same(one, rep) and not one[2].any(), dev
        for i in (0, 1, 8, 512):
            assert (bytes(one[0][i]), bytes(one[1][i]), 0) == B.ckd_priv(bytes(keys[0]), bytes(ccs[0]), int(idx[i])), i
    gpu_ctx.check()


def test_derive_priv_then_public_key_is_derive_pub(gpu_ctx):
    rng = random.Random(0x5132)
    n = 513
    cv = _cv(gpu_ctx, "secp256k1")
    keys, ccs = _random_parents(rng, n)
    keys[5] = 0
    idx = np.array([rng.randrange(H) for _ in range(n)], dtype=np.uint32)
    ck, ccc, st = derive_priv(gpu_ctx, keys, ccs, idx, 0, False)
    pk, pst = cv.public_key(keys, 33)
    cp, pcc, st2 = derive_pub(gpu_ctx, pk, ccs, idx, True)
    pub_of_child, st3 = cv.public_key(ck, 33)
    ok = np.arange(n) != 5
    assert st[5] == 6 and st2[5] == 2 and st3[5] == 6 and not st[ok].any() and not st2[ok].any() and not st3[ok].any()
    assert np.array_equal(pub_of_child, cp) and np.array_equal(ccc, pcc) and not cp[5].any() and not ccc[5].any() and not ck[5].any()
    # mixed hardened and non-hardened lanes in one call; NO_COMB gives the same child keys on the hardened ones
    mixed = idx.copy()
    mixed[1::2] |= H
    a = derive_priv(gpu_ctx, keys, ccs, mixed, 0, True)
    b = derive_priv(gpu_ctx, keys, ccs, mixed, B.NO_COMB, True)
    hard = (mixed >= H) & ok
    assert np.array_equal(a[0][~hard & ok], ck[~hard & ok]) and not a[2][ok].any()
    assert _same([x[hard] for x in a], [x[hard] for x in b]) and (b[2][~hard & ok] == 9).all() and not b[0][~hard].any() and not b[1][~hard].any()
    assert b[2][5] == 6
    for i in (1, 3, 511):
        assert (bytes(a[0][i]), bytes(a[1][i]), 0) == B.ckd_priv(bytes(keys[i]), bytes(ccs[i]), int(mixed[i])), i
    gpu_ctx.check()


def _limbs(rows):
    """(n,32) big-endian bytes -> (n,4) uint64 little-endian limbs"""
    return np.ascontiguousarray(rows[:, ::-1]).view("<u8").reshape(-1, 4).copy()


@pytest.mark.parametrize("curve", CURVES)
def test_tweak_add_is_the_double_mul_it_replaces(gpu_ctx, curve):
    """pubkey_tweak_add(P, t) == fec_canon_double_mul(t, 1, P) re-encoded, t = 0, the doubling and the sum at infinity among them;
    and == public_key(seckey_tweak_add(d, t))"""
    C = B.CURVES[curve]
    rng = random.Random(0x5133)
    n = 513
    cv = _cv(gpu_ctx, curve)
    ds = [rng.randrange(1, C.N) for _ in range(n)]
    ts = [rng.randrange(C.N) for _ in range(n)]
    ts[3], ts[64], ts[200], ts[512] = 0, ds[64], C.N - ds[200], 1
    keys, tw = _brows([B.b32(d) for d in ds], 32), _brows([B.b32(t) for t in ts], 32)
    pk, pst = cv.public_key(keys, 65)
    assert not pst.any()
    out, st = tweak(gpu_ctx, curve, pk, tw, 65, 65, True)
    xy, dst = cv.decompress(pk, 65)
    one = np.zeros((n, 4), dtype=np.uint64)
    one[:, 0] = 1
    sxy, sst = cv.double_mul(_limbs(tw), one, xy)
    assert sst[200] == 1 and st[200] == 8 and not out[200].any() and (sst[np.arange(n) != 200] == 0).all() and not st[np.arange(n) != 200].any()
    x_be = np.ascontiguousarray(sxy[:, :4]).view(np.uint8).reshape(n, 32)[:, ::-1]
    y_be = np.ascontiguousarray(sxy[:, 4:]).view(np.uint8).reshape(n, 32)[:, ::-1]
    ok = np.arange(n) != 200
    assert (out[ok, 0] == 4).all() and np.array_equal(out[ok, 1:33], x_be[ok]) and np.array_equal(out[ok, 33:], y_be[ok])
    assert np.array_equal(out[3], pk[3]) and bytes(out[64]) == B.encode(C.mul(2 * ds[64], C.G), 65)
    sk, sst2 = sectweak(gpu_ctx, curve, keys, tw, True)
    assert sst2[200] == 8 and not sst2[ok].any()
    pk2, _ = cv.public_key(sk, 65)
    assert np.array_equal(pk2[ok], out[ok])
    gpu_ctx.check()


def test_vector_1_chain_on_the_device(gpu_ctx):
    """m -> m/0' -> m/0'/1 through *_dev calls, no host copy between the levels; the last level again by CKDpub from the
    device-computed public key of m/0'"""
    import torch
    hd, cv = _hd(gpu_ctx), _cv(gpu_ctx, "secp256k1")
    v = [c for c in FIXTURE["bip32_priv"] if c["class"] == "vector1"]
    assert v[0]["child"] == "edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea"
    n = 3   # the same chain three times: the levels run as batches
    k0, c0 = _to_dev(_rows([v[0]["key"]] * n, 32)), _to_dev(_rows([v[0]["cc"]] * n, 32))
    i1, i2 = _to_dev(np.array([H] * n, dtype=np.uint32)), _to_dev(np.array([1] * n, dtype=np.uint32))
    k1, c1, k2, c2, c2p = (_dev_out(n, 32) for _ in range(5))
    p1, p2 = _dev_out(n, 33), _dev_out(n, 33)
    s = [_dev_out(n, 1, 77) for _ in range(4)]
    hd.derive_priv_dev(k0.data_ptr(), c0.data_ptr(), n, i1.data_ptr(), 0, k1.data_ptr(), c1.data_ptr(), s[0].data_ptr(), n)
    hd.derive_priv_dev(k1.data_ptr(), c1.data_ptr(), n, i2.data_ptr(), 0, k2.data_ptr(), c2.data_ptr(), s[1].data_ptr(), n)
    cv.public_key_dev(k1.data_ptr(), p1.data_ptr(), 33, s[2].data_ptr(), n)
    hd.derive_pub_dev(p1.data_ptr(), c1.data_ptr(), n, i2.data_ptr(), p2.data_ptr(), c2p.data_ptr(), s[3].data_ptr(), n)
    torch.cuda.synchronize()
    assert not any(x.cpu().numpy().any() for x in s)
    for i in range(n):
        assert bytes(k1.cpu().numpy()[i]).hex() == "edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea"
        assert bytes(c1.cpu().numpy()[i]).hex() == "47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141"
        assert bytes(p1.cpu().numpy()[i]).hex() == "035a784662a4a20a65bf6aab9ae98a6c068a81c52e4b032c0fb5400c706cfccc56"
        assert bytes(k2.cpu().numpy()[i]).hex() == "3c6cb8d0f6a264c91ea8b5030fadaa8e538b020f0a387421a12de9319dc93368"
        assert bytes(c2.cpu().numpy()[i]).hex() == bytes(c2p.cpu().numpy()[i]).hex() == "2a7857631386ba23dacac34180dd1983734e444fdbf774041578e9b6adb37c19"
        assert bytes(p2.cpu().numpy()[i]).hex() == "03501e454bf00751f24b1b489aa925215d66af2234e3891c3b21a52bedb3cd711c"
    gpu_ctx.check()


def test_chunks_and_a_multi_device_ctx(gpu_ctx):
    """n = 200 in chunks of 64; two shard workers on one GPU; the shared parent crosses chunks and shards"""
    import forge_ec_amd as F
    n = 200
    cases = [c for c in FIXTURE["tweak"] if c["curve"] == "secp256k1" and len(c["key"]) == 66]
    pick = [cases[(40 + i) % len(cases)] for i in range(n)]
    pks, tw, wst = _tweak_inputs(pick, 33)
    want = _tweak_want(pick, 65)
    sc = [c for c in FIXTURE["seckey"] if c["curve"] == "p256"]
    sc = [sc[i % len(sc)] for i in range(n)]
    pub = [FIXTURE["bip32_pub"][(100 + i) % len(FIXTURE["bip32_pub"])] for i in range(n)]
    priv = [c for c in FIXTURE["bip32_priv"] if c["flags"] == 0]
    priv = [priv[(100 + i) % len(priv)] for i in range(n)]
    pi, vi = _pub_inputs(pub), _priv_inputs(priv)
    rng = random.Random(0x5134)
    skey, scc = _random_parents(rng, 1)
    sidx = np.array([rng.randrange(2**32) for _ in range(n)], dtype=np.uint32)
    swant = [B.ckd_priv(bytes(skey[0]), bytes(scc[0]), int(i)) for i in sidx]
    spk = _brows([B.public_key(SECP, bytes(skey[0]))], 33)
    pwant = [B.ckd_pub(bytes(spk[0]), bytes(scc[0]), int(i)) for i in sidx]

    def run(ctx):
        assert _same(tweak(ctx, "secp256k1", pks, tw, 33, 65, False), (want, wst)) and (wst != 0).sum() >= 10
        got = sectweak(ctx, "p256", _rows([c["key"] for c in sc], 32), _rows([c["tweak"] for c in sc], 32), False)
        assert _same(got, (_rows([c["out"] for c in sc], 32), np.array([c["status"] for c in sc], dtype=np.uint8)))
        assert _same(derive_pub(ctx, pi[0], pi[1], pi[2], False), pi[3:]) and pi[5].any()
        assert _same(derive_priv(ctx, vi[0], vi[1], vi[2], 0, False), vi[3:]) and vi[5].any()
        out, occ, st = derive_priv(ctx, skey, scc, sidx, 0, False)
        assert [(bytes(out[i]), bytes(occ[i]), int(st[i])) for i in range(n)] == swant
        out, occ, st = derive_pub(ctx, spk, scc, sidx, False)
        assert [(bytes(out[i]), bytes(occ[i]), int(st[i])) for i in range(n)] == pwant and 9 in st and 0 in st

    gpu_ctx.set_chunk(64)
    try:
        run(gpu_ctx)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    with F.Context(devices=[0, 0]) as multi:
        run(multi)
    gpu_ctx.check()


def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    assert (L.CANON_BAD_POINT, L.CANON_BAD_SCALAR, L.CANON_BAD_KEY, L.CANON_NO_KEY, L.CANON_BAD_INDEX, L.CANON_BIP32_INVALID, L.CANON_BIP32_NO_COMB) == \
        (B.BAD_POINT, B.BAD_SCALAR, B.BAD_KEY, B.NO_KEY, B.BAD_INDEX, B.BIP32_INVALID, B.NO_COMB) == (2, 3, 6, 8, 9, 10, 1)
    lib, h = L.lib(), gpu_ctx._h
    p = lambda a: a.ctypes.data   # noqa: E731
    S, P, ED = L.SECP256K1, L.P256, L.ED25519
    n = 4
    pick = [c for c in FIXTURE["tweak"] if c["curve"] == "secp256k1" and len(c["key"]) == 66][:n]
    pks, tw, wst = _tweak_inputs(pick, 33)
    out, st = np.zeros((n, 65), np.uint8), np.zeros(n, np.uint8)
    vi = _priv_inputs([c for c in FIXTURE["bip32_priv"] if c["flags"] == 0][:n])
    pi = _pub_inputs(FIXTURE["bip32_pub"][:n])
    o32, occ = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    # the host forms: a good call, n = 0 with nulls, each null, the curves, the lengths, n_par, the flags
    assert lib.fec_canon_pubkey_tweak_add(h, S, p(pks), 33, p(tw), p(out), 65, p(st), n) == 0 and np.array_equal(out, _tweak_want(pick, 65))
    assert lib.fec_canon_pubkey_tweak_add(h, S, None, 33, None, None, 33, None, 0) == 0
    assert lib.fec_canon_seckey_tweak_add(h, S, None, None, None, None, 0) == 0
    assert lib.fec_canon_bip32_derive_pub(h, None, None, 0, None, None, None, None, 0) == 0
    assert lib.fec_canon_bip32_derive_priv(h, None, None, 0, None, 0, None, None, None, 0) == 0
    good = [h, S, p(pks), 33, p(tw), p(out), 65, p(st), n]
    for i in (0, 2, 4, 5, 7):
        args = list(good)
        args[i] = None
        assert lib.fec_canon_pubkey_tweak_add(*args) == ARG, i
    for ln in (0, 1, 31, 34, 64, 66):
        assert lib.fec_canon_pubkey_tweak_add(h, S, p(pks), ln, p(tw), p(out), 33, p(st), n) == ARG, ln
        assert lib.fec_canon_pubkey_tweak_add(h, S, p(pks), 33, p(tw), p(out), ln, p(st), n) == ARG, ln
    assert lib.fec_canon_pubkey_tweak_add(h, P, p(pks), 32, p(tw), p(out), 33, p(st), n) == ARG
    assert lib.fec_canon_pubkey_tweak_add(h, P, p(pks), 33, p(tw), p(out), 32, p(st), n) == ARG
    assert lib.fec_canon_pubkey_tweak_add(h, S, p(pks), 33, p(tw), p(out), 32, p(st), n) == 0
    assert lib.fec_canon_pubkey_tweak_add(h, ED, p(pks), 33, p(tw), p(out), 33, p(st), n) == UNSUPPORTED
    assert lib.fec_canon_pubkey_tweak_add(h, 7, p(pks), 33, p(tw), p(out), 33, p(st), n) == ARG
    assert lib.fec_canon_seckey_tweak_add(h, ED, p(tw), p(tw), p(o32), p(st), n) == UNSUPPORTED
    assert lib.fec_canon_seckey_tweak_add(h, 7, p(tw), p(tw), p(o32), p(st), n) == ARG
    for i in (0, 2, 3, 4, 5):
        args = [h, S, p(tw), p(tw), p(o32), p(st), n]
        args[i] = None
        assert lib.fec_canon_seckey_tweak_add(*args) == ARG, i
    good = [h, p(pi[0]), p(pi[1]), n, p(pi[2]), p(out), p(occ), p(st), n]
    assert lib.fec_canon_bip32_derive_pub(*good) == 0
    for i in (0, 1, 2, 4, 5, 6, 7):
        args = list(good)
        args[i] = None
        assert lib.fec_canon_bip32_derive_pub(*args) == ARG, i
    for n_par in (0, 2, 3, 5):
        assert lib.fec_canon_bip32_derive_pub(h, p(pi[0]), p(pi[1]), n_par, p(pi[2]), p(out), p(occ), p(st), n) == ARG, n_par
        assert lib.fec_canon_bip32_derive_priv(h, p(vi[0]), p(vi[1]), n_par, p(vi[2]), 0, p(o32), p(occ), p(st), n) == ARG, n_par
    good = [h, p(vi[0]), p(vi[1]), n, p(vi[2]), 0, p(o32), p(occ), p(st), n]
    assert lib.fec_canon_bip32_derive_priv(*good) == 0 and np.array_equal(o32, vi[3]) and np.array_equal(occ, vi[4])
    for i in (0, 1, 2, 4, 6, 7, 8):
        args = list(good)
        args[i] = None
        assert lib.fec_canon_bip32_derive_priv(*args) == ARG, i
    for flags in (2, 3, 4, 0x80000000):
        assert lib.fec_canon_bip32_derive_priv(h, p(vi[0]), p(vi[1]), n, p(vi[2]), flags, p(o32), p(occ), p(st), n) == ARG, flags
    # the *_dev forms: good calls, n = 0, nulls, misalignment, a multi-device ctx
    pad = np.zeros(16, np.uint8)
    tp, tt, tk, tc = (_to_dev(np.concatenate([a.reshape(-1), pad])) for a in (pks, tw, vi[0], vi[1]))
    ti = _to_dev(np.concatenate([vi[2], np.zeros(4, np.uint32)]))
    to, tc2 = torch.zeros(n * 65 + 16, dtype=torch.uint8, device="cuda"), torch.zeros(n * 32 + 16, dtype=torch.uint8, device="cuda")
    tst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    PK, T, KY, CC, IX, O, OC, ST = (t.data_ptr() for t in (tp, tt, tk, tc, ti, to, tc2, tst))
    for ln in (33, 65, 32):
        assert lib.fec_canon_pubkey_tweak_add_dev(h, S, PK, 33, T, O, ln, ST, n, None) == 0
    assert lib.fec_canon_pubkey_tweak_add_dev(h, S, PK + 1, 33, T, O + 1, 33, ST, n, None) == 0     # SEC 1 records have no alignment
    assert lib.fec_canon_seckey_tweak_add_dev(h, S, KY, T, O, ST, n, None) == 0
    assert lib.fec_canon_bip32_derive_pub_dev(h, PK, CC, n, IX, O, OC, ST, n, None) == 0
    assert lib.fec_canon_bip32_derive_pub_dev(h, PK + 33, CC, 1, IX, O + 3, OC, ST, n, None) == 0
    assert lib.fec_canon_bip32_derive_priv_dev(h, KY, CC, n, IX, 0, O, OC, ST, n, None) == 0
    assert lib.fec_canon_bip32_derive_priv_dev(h, KY, CC, 1, IX, 1, O, OC, ST, n, None) == 0
    torch.cuda.synchronize()
    assert lib.fec_canon_pubkey_tweak_add_dev(h, S, None, 33, None, None, 33, None, 0, None) == 0
    assert lib.fec_canon_seckey_tweak_add_dev(h, S, None, None, None, None, 0, None) == 0
    assert lib.fec_canon_bip32_derive_pub_dev(h, None, None, 0, None, None, None, None, 0, None) == 0
    assert lib.fec_canon_bip32_derive_priv_dev(h, None, None, 0, None, 0, None, None, None, 0, None) == 0
    for args in ((None, S, PK, 33, T, O, 33, ST, n, None), (h, S, None, 33, T, O, 33, ST, n, None), (h, S, PK, 33, None, O, 33, ST, n, None),
                 (h, S, PK, 33, T, None, 33, ST, n, None), (h, S, PK, 33, T, O, 33, None, n, None), (h, S, PK, 33, T + 8, O, 33, ST, n, None),
                 (h, S, PK + 8, 32, T, O, 33, ST, n, None), (h, S, PK, 33, T, O + 8, 32, ST, n, None), (h, S, PK, 34, T, O, 33, ST, n, None),
                 (h, S, PK, 33, T, O, 64, ST, n, None), (h, P, PK, 32, T, O, 33, ST, n, None), (h, 7, PK, 33, T, O, 33, ST, n, None)):
        assert lib.fec_canon_pubkey_tweak_add_dev(*args) == ARG, args
    assert lib.fec_canon_pubkey_tweak_add_dev(h, ED, PK, 33, T, O, 33, ST, n, None) == UNSUPPORTED
    for args in ((None, S, KY, T, O, ST, n, None), (h, S, None, T, O, ST, n, None), (h, S, KY, None, O, ST, n, None), (h, S, KY, T, None, ST, n, None),
                 (h, S, KY, T, O, None, n, None), (h, S, KY + 8, T, O, ST, n, None), (h, S, KY, T + 4, O, ST, n, None), (h, S, KY, T, O + 8, ST, n, None),
                 (h, 7, KY, T, O, ST, n, None)):
        assert lib.fec_canon_seckey_tweak_add_dev(*args) == ARG, args
    assert lib.fec_canon_seckey_tweak_add_dev(h, ED, KY, T, O, ST, n, None) == UNSUPPORTED
    for args in ((None, PK, CC, n, IX, O, OC, ST, n, None), (h, None, CC, n, IX, O, OC, ST, n, None), (h, PK, None, n, IX, O, OC, ST, n, None),
                 (h, PK, CC, n, None, O, OC, ST, n, None), (h, PK, CC, n, IX, None, OC, ST, n, None), (h, PK, CC, n, IX, O, None, ST, n, None),
                 (h, PK, CC, n, IX, O, OC, None, n, None), (h, PK, CC, 2, IX, O, OC, ST, n, None), (h, PK, CC, 0, IX, O, OC, ST, n, None),
                 (h, PK, CC + 8, n, IX, O, OC, ST, n, None), (h, PK, CC, n, IX, O, OC + 8, ST, n, None), (h, PK, CC, n, IX + 2, O, OC, ST, n, None)):
        assert lib.fec_canon_bip32_derive_pub_dev(*args) == ARG, args
    for args in ((None, KY, CC, n, IX, 0, O, OC, ST, n, None), (h, None, CC, n, IX, 0, O, OC, ST, n, None), (h, KY, None, n, IX, 0, O, OC, ST, n, None),
                 (h, KY, CC, n, None, 0, O, OC, ST, n, None), (h, KY, CC, n, IX, 0, None, OC, ST, n, None), (h, KY, CC, n, IX, 0, O, None, ST, n, None),
                 (h, KY, CC, n, IX, 0, O, OC, None, n, None), (h, KY, CC, 3, IX, 0, O, OC, ST, n, None), (h, KY, CC, n, IX, 2, O, OC, ST, n, None),
                 (h, KY + 8, CC, n, IX, 0, O, OC, ST, n, None), (h, KY, CC + 4, n, IX, 0, O, OC, ST, n, None), (h, KY, CC, n, IX, 0, O + 8, OC, ST, n, None),
                 (h, KY, CC, n, IX, 0, O, OC + 8, ST, n, None), (h, KY, CC, n, IX + 1, 0, O, OC, ST, n, None)):
        assert lib.fec_canon_bip32_derive_priv_dev(*args) == ARG, args
    torch.cuda.synchronize()
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_canon_pubkey_tweak_add_dev(multi._h, S, PK, 33, T, O, 33, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_seckey_tweak_add_dev(multi._h, S, KY, T, O, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_bip32_derive_pub_dev(multi._h, PK, CC, n, IX, O, OC, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_bip32_derive_priv_dev(multi._h, KY, CC, n, IX, 0, O, OC, ST, n, None) == UNSUPPORTED
