"""
GPU tests of the canonical-mode RIPEMD-160 / HASH160 calls, the Taproot output key and CKDpub along a path
(include/fecgpu_canon.h: fec_canon_ripemd160, fec_canon_hash160, fec_canon_pubkey_hash160, fec_canon_taproot_output_key,
fec_canon_bip32_derive_pub_path and their *_dev forms) against the model tests/canon_wallet_ref.py, which
tests/test_canon_wallet_model.py pins by published vectors.  Every comparison is byte-exact, status included; host and *_dev
forms go through one helper each, output buffers pre-filled with a byte that is not zero.  The model is slow (15 ms a level),
so its results are computed once per module and shared; the largest batches are also held against the calls they replace on
the GPU -- chained derive_pub, pubkey_tweak_add fed the model's tweak -- which the existing suite holds against the model.
"""
import os
import random

import numpy as np
import pytest

import canon_bip32_ref as B
import canon_wallet_ref as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = W.load_fixture(os.path.join(HERE, "golden", "canon_wallet_vectors.json"))
LENGTHS = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 200)
HASH_COUNTS = [1, 63, 64, 65, 257]
COUNTS = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257]
ARG, UNSUPPORTED = -1, -5
AMONG = 64 * 3 + 5
LANES = (0, 31, 32, 63, AMONG - 1)
SECP = B.SECP256K1
H = B.HARDENED
FILL = 0xEE


def _secp(ctx):
    from forge_ec_amd.canon import CanonSecp256k1
    return CanonSecp256k1(ctx)


def _hd(ctx):
    from forge_ec_amd.canon import CanonBip32
    return CanonBip32(ctx)


def _hash(ctx):
    from forge_ec_amd.canon import CanonKeccak
    return CanonKeccak(ctx)


def _brows(items, width):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), width).copy()


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _dev_out(n, width, fill=FILL):
    import torch
    return torch.full((n, width) if width > 1 else (n,), fill, dtype=torch.uint8, device="cuda")


def _same(got, want):
    return len(got) == len(want) and all(g is None and w is None or np.array_equal(g, w) for g, w in zip(got, want))


# ---- the calls, host and *_dev forms alike: numpy in, numpy out -------------------------------------------------------------
def digests(ctx, which, msgs, dev, bad=()):
    """which: "ripemd160" / "hash160"; dev form: (digests, status), with the offsets of the elements in `bad` out of range"""
    import torch
    if not dev:
        return getattr(_hash(ctx), which)(msgs), np.zeros(len(msgs), np.uint8)
    n = len(msgs)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    total = int(off[n])
    for i in bad:
        off[i + 1] = total + 1 + i   # past the end: messages i and i + 1 are out of range or run backwards
    tb, to = _to_dev(np.frombuffer(b"".join(msgs) + bytes(8), dtype=np.uint8)), _to_dev(off)
    out, st = _dev_out(n, 20), _dev_out(n, 1, 77)
    getattr(_hash(ctx), which + "_dev")(tb.data_ptr(), to.data_ptr(), total, out.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def pubkey_hash160(ctx, pks, pk_len, dev):
    import torch
    if not dev:
        return _hash(ctx).pubkey_hash160(pks, pk_len)
    n = pks.shape[0]
    tp, out = _to_dev(pks), _dev_out(n, 20)
    _hash(ctx).pubkey_hash160_dev(tp.data_ptr(), pk_len, out.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def taproot(ctx, pks, roots, pk_len, dev):
    import torch
    if not dev:
        return _secp(ctx).taproot_output_key(pks, roots, pk_len)
    n = pks.shape[0]
    tp, tr = _to_dev(pks), (None if roots is None else _to_dev(roots))
    out, par, st = _dev_out(n, 32), _dev_out(n, 1), _dev_out(n, 1, 77)
    _secp(ctx).taproot_output_key_dev(tp.data_ptr(), pk_len, None if tr is None else tr.data_ptr(), out.data_ptr(), par.data_ptr(),
                                      st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), par.cpu().numpy(), st.cpu().numpy()


def path(ctx, pks, ccs, idx, dev, fp=True, h160=True):
    """(child keys, chain codes, fingerprints or None, HASH160 or None, status)"""
    import torch
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.uint32))
    if not dev:
        return _hd(ctx).derive_pub_path(pks, ccs, idx, fp, h160)
    n, depth = idx.shape
    tp, tc, ti = _to_dev(pks), _to_dev(ccs), _to_dev(idx)
    out, occ, st = _dev_out(n, 33), _dev_out(n, 32), _dev_out(n, 1, 77)
    tf, th = (_dev_out(n, 4) if fp else None), (_dev_out(n, 20) if h160 else None)
    _hd(ctx).derive_pub_path_dev(tp.data_ptr(), tc.data_ptr(), pks.shape[0], ti.data_ptr(), depth, out.data_ptr(), occ.data_ptr(),
                                 tf.data_ptr() if fp else None, th.data_ptr() if h160 else None, st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), occ.cpu().numpy(), tf.cpu().numpy() if fp else None, th.cpu().numpy() if h160 else None, st.cpu().numpy()


def derive_pub(ctx, pks, ccs, idx):
    return _hd(ctx).derive_pub(pks, ccs, np.asarray(idx, dtype=np.uint32))


# ---- the model's results, once ---------------------------------------------------------------------------------------------
_POOL = {}


def keys_pool():
    """257 public keys (33 bytes) and chain codes from a seed"""
    if "keys" not in _POOL:
        rng = random.Random(0x3201)
        _POOL["keys"] = [B.encode(SECP.mul(rng.randrange(1, SECP.N), SECP.G), 33) for _ in range(257)]
        _POOL["ccs"] = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(257)]
    return _POOL["keys"], _POOL["ccs"]


def taproot_pool():
    """257 x-only internal keys, roots, and the model's (output, parity, status) with a root and without"""
    if "tap" not in _POOL:
        keys, ccs = keys_pool()
        xs = [k[1:] for k in keys]
        rooted = [W.taproot_output_key(x, r) for x, r in zip(xs, ccs)]
        bare = [W.taproot_output_key(x) for x in xs]
        assert all(r[2] == 0 for r in rooted + bare)
        _POOL["tap"] = (xs, ccs, rooted, bare)
    return _POOL["tap"]


def path_pool():
    """65 parents walked three levels by the model, every level's result kept: (rows of 3 indices, per depth the list of
    (child, cc, fingerprint, hash160, status))"""
    if "path" not in _POOL:
        keys, ccs = keys_pool()
        rng = random.Random(0x3202)
        rows = [[rng.randrange(H) for _ in range(3)] for _ in range(65)]
        rows[0] = [0, H - 1, 1]
        by_depth = {1: [], 2: [], 3: []}
        for i in range(65):   # one walk per parent, every level kept
            k, c = keys[i], ccs[i]
            for d in (1, 2, 3):
                parent = k
                k, c, st = B.ckd_pub(k, c, rows[i][d - 1])
                assert st == 0
                by_depth[d].append((k, c, W.hash160(parent)[:4], W.hash160(k), 0))
        assert by_depth[2][:3] == [W.derive_pub_path(keys[i], ccs[i], rows[i][:2]) for i in range(3)]
        _POOL["path"] = (rows, by_depth)
    return _POOL["path"]


def _path_want(results, fp=True, h160=True):
    return (_brows([r[0] for r in results], 33), _brows([r[1] for r in results], 32), _brows([r[2] for r in results], 4) if fp else None,
            _brows([r[3] for r in results], 20) if h160 else None, np.array([r[4] for r in results], dtype=np.uint8))


# ---- hashes ----------------------------------------------------------------------------------------------------------------
def _messages(n, seed):
    """n messages whose lengths cycle through LENGTHS from a rotating start: neighbours in a wavefront differ in block count"""
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(LENGTHS[(i * 5 + seed) % len(LENGTHS)])) for i in range(n)]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("which", ["ripemd160", "hash160"])
def test_hashes_mixed_lengths(gpu_ctx, which, dev):
    model = getattr(W, which)
    fx = [bytes.fromhex(c["msg"]) for c in FIXTURE["hashes"]]
    got, st = digests(gpu_ctx, which, fx, dev)
    assert np.array_equal(got, _brows([bytes.fromhex(c[which]) for c in FIXTURE["hashes"]], 20)) and not st.any()
    for n in HASH_COUNTS:
        msgs = _messages(n, n)
        if n >= 63:
            assert {len(m) for m in msgs[:63]} == set(LENGTHS)
        got, st = digests(gpu_ctx, which, msgs, dev)
        assert np.array_equal(got, _brows([model(m) for m in msgs], 20)) and not st.any(), n
    gpu_ctx.check()


@pytest.mark.parametrize("which", ["ripemd160", "hash160"])
def test_hash_bad_range(gpu_ctx, which):
    """an offset past the end: the message that ends there and the one that starts there get status 4 and a zero digest"""
    import torch
    model = getattr(W, which)
    msgs = _messages(130, 7)
    got, st = digests(gpu_ctx, which, msgs, True, bad=(5, 64))
    want = _brows([model(m) for m in msgs], 20)
    wst = np.zeros(130, np.uint8)
    for i in (5, 6, 64, 65):
        want[i], wst[i] = 0, 4
    assert np.array_equal(got, want) and np.array_equal(st, wst)
    # no status array: the digests alone
    off = np.zeros(4, np.uint64)
    off[1:] = (3, 1 << 40, 6)
    tb, to, out = _to_dev(np.frombuffer(b"abcdef" + bytes(8), np.uint8)), _to_dev(off), _dev_out(3, 20)
    getattr(_hash(gpu_ctx), which + "_dev")(tb.data_ptr(), to.data_ptr(), 6, out.data_ptr(), None, 3)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _brows([model(b"abc"), bytes(20), bytes(20)], 20))
    gpu_ctx.check()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("pk_len", [33, 65])
def test_pubkey_hash160(gpu_ctx, pk_len, dev):
    keys, _ = keys_pool()
    recs = [k if pk_len == 33 else B.encode(B.decode(SECP, k), 65) for k in keys[:65]]
    recs[3] = bytes(pk_len)            # the bytes as they lie: nothing is decoded
    recs[4] = b"\xff" * pk_len
    want = _brows([W.hash160(r) for r in recs], 20)
    for n in (1, 63, 64, 65):
        assert np.array_equal(pubkey_hash160(gpu_ctx, _brows(recs[:n], pk_len), pk_len, dev), want[:n]), n
    gpu_ctx.check()


# ---- Taproot ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("pk_len", [32, 33])
def test_taproot_fixture(gpu_ctx, pk_len, dev):
    for rooted in (False, True):
        sel = [c for c in FIXTURE["taproot"] if len(c["pk"]) == 2 * pk_len and (c["root"] is not None) == rooted]
        if not sel:
            continue
        got = taproot(gpu_ctx, _brows([bytes.fromhex(c["pk"]) for c in sel], pk_len),
                      _brows([bytes.fromhex(c["root"]) for c in sel], 32) if rooted else None, pk_len, dev)
        want = (_brows([bytes.fromhex(c["out"]) for c in sel], 32), np.array([c["parity"] for c in sel], np.uint8),
                np.array([c["status"] for c in sel], np.uint8))
        assert _same(got, want), (pk_len, rooted)
    assert any(c["status"] for c in FIXTURE["taproot"] if len(c["pk"]) == 2 * pk_len)
    gpu_ctx.check()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("rooted", [False, True], ids=["bip86", "root"])
@pytest.mark.parametrize("pk_len", [32, 33])
def test_taproot_counts(gpu_ctx, pk_len, rooted, dev):
    xs, roots, with_root, bare = taproot_pool()
    results = with_root if rooted else bare
    recs = xs if pk_len == 32 else [bytes([2 + (i & 1)]) + x for i, x in enumerate(xs)]   # both tags: ignored
    for n in COUNTS:
        got = taproot(gpu_ctx, _brows(recs[:n], pk_len), _brows(roots[:n], 32) if rooted else None, pk_len, dev)
        want = (_brows([r[0] for r in results[:n]], 32), np.array([r[1] for r in results[:n]], np.uint8), np.zeros(n, np.uint8))
        assert _same(got, want), n
    assert {r[1] for r in results} == {0, 1}
    gpu_ctx.check()


@pytest.mark.parametrize("rooted", [False, True], ids=["bip86", "root"])
def test_taproot_is_the_tweak_add_of_the_model_tweak(gpu_ctx, rooted):
    """every count, against fec_canon_pubkey_tweak_add_dev (pk_len 32, out_len 32) fed H_TapTweak from hashlib"""
    import torch
    xs, roots, _, _ = taproot_pool()
    tweaks = [W.taptweak(x, r if rooted else None) for x, r in zip(xs, roots)]
    for n in COUNTS:
        out, par, st = taproot(gpu_ctx, _brows(xs[:n], 32), _brows(roots[:n], 32) if rooted else None, 32, True)
        tp, tt, o32, o33, s32, s33 = _to_dev(_brows(xs[:n], 32)), _to_dev(_brows(tweaks[:n], 32)), _dev_out(n, 32), _dev_out(n, 33), _dev_out(n, 1), _dev_out(n, 1)
        _secp(gpu_ctx).pubkey_tweak_add_dev(tp.data_ptr(), 32, tt.data_ptr(), o32.data_ptr(), 32, s32.data_ptr(), n)
        _secp(gpu_ctx).pubkey_tweak_add_dev(tp.data_ptr(), 32, tt.data_ptr(), o33.data_ptr(), 33, s33.data_ptr(), n)
        torch.cuda.synchronize()
        o33 = o33.cpu().numpy()
        assert np.array_equal(out, o32.cpu().numpy()) and np.array_equal(out, o33[:, 1:]) and np.array_equal(par, o33[:, 0] & 1), n
        assert not st.any() and not s32.cpu().numpy().any()
    gpu_ctx.check()


def _off_curve_x():
    return next(B.b32(v) for v in range(1, 50) if B.sqrt_mod(SECP, (v ** 3 + 7) % SECP.P) is None)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("refusal", ["x >= p", "off the curve", "tag 4"])
def test_taproot_one_refusal_among_ordinary(gpu_ctx, refusal, dev):
    xs, roots, with_root, _ = taproot_pool()
    pk_len = 33 if refusal == "tag 4" else 32
    base = [x if pk_len == 32 else b"\x02" + x for x in xs[:AMONG]]
    want = (_brows([r[0] for r in with_root[:AMONG]], 32), np.array([r[1] for r in with_root[:AMONG]], np.uint8), np.zeros(AMONG, np.uint8))
    for lane in LANES:
        recs = list(base)
        recs[lane] = {"x >= p": B.b32(SECP.P + lane), "off the curve": _off_curve_x(), "tag 4": b"\x04" + xs[lane]}[refusal]
        got = taproot(gpu_ctx, _brows(recs, pk_len), _brows(roots[:AMONG], 32), pk_len, dev)
        w = [a.copy() for a in want]
        w[0][lane], w[1][lane], w[2][lane] = 0, 0, W.BAD_POINT
        assert _same(got, w), lane
    gpu_ctx.check()


# ---- CKDpub along a path ---------------------------------------------------------------------------------------------------
def _chain(ctx, pks, ccs, idx):
    """depth chained fec_canon_bip32_derive_pub calls, fingerprints and HASH160 by fec_canon_pubkey_hash160: what the path call
    replaces.  The status is the first of the chain that is not 0, every output zero then."""
    idx = np.asarray(idx, dtype=np.uint32)
    n, depth = idx.shape
    k, c = (np.repeat(a, n, axis=0) if a.shape[0] != n else a for a in (pks, ccs))
    first = np.zeros(n, np.uint8)
    for level in range(depth):
        parent = k
        k, c, st = derive_pub(ctx, k, c, idx[:, level])
        first = np.where(first == 0, st, first)
    fp = pubkey_hash160(ctx, parent, 33, False)[:, :4].copy()
    h160 = pubkey_hash160(ctx, k, 33, False)
    for a in (k, c, fp, h160):
        a[first != 0] = 0
    return k, c, fp, h160, first


def test_path_vector_1_and_fixture(gpu_ctx):
    v1 = [c for c in FIXTURE["path"] if c["class"] == "vector1"][0]
    assert v1["child"] == "022a471424da5e657499d1ff51cb43c47481a03b1e77f951fe64cec9f5a48f7011" and v1["fingerprint"] == "d880d7d8"
    assert v1["hash160"] == "d69aa102255fed74378278c7812701ea641fdf32"
    for depth in sorted({len(c["indices"]) for c in FIXTURE["path"]}):
        sel = [c for c in FIXTURE["path"] if len(c["indices"]) == depth]
        want = _path_want([tuple(bytes.fromhex(c[k]) for k in ("child", "child_cc", "fingerprint", "hash160")) + (c["status"],) for c in sel])
        for dev in (False, True):
            got = path(gpu_ctx, _brows([bytes.fromhex(c["pk"]) for c in sel], 33), _brows([bytes.fromhex(c["cc"]) for c in sel], 32),
                       [c["indices"] for c in sel], dev)
            assert _same(got, want), (depth, dev)
    assert {c["status"] for c in FIXTURE["path"]} == {0, W.BAD_POINT, W.BAD_INDEX}
    gpu_ctx.check()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_path_against_the_model(gpu_ctx, depth, dev):
    keys, ccs = keys_pool()
    rows, by_depth = path_pool()
    for n in [c for c in COUNTS if c <= 65]:
        got = path(gpu_ctx, _brows(keys[:n], 33), _brows(ccs[:n], 32), [r[:depth] for r in rows[:n]], dev)
        assert _same(got, _path_want(by_depth[depth][:n])), n
    gpu_ctx.check()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_path_against_chained_calls_every_count(gpu_ctx, depth, dev):
    """n_par = n and n_par = 1, each against depth chained derive_pub calls on the GPU; a hardened index in the batch"""
    keys, ccs = keys_pool()
    rng = random.Random(0x3203 + depth)
    pks, cc = _brows(keys, 33), _brows(ccs, 32)
    for n in COUNTS:
        idx = np.array([[rng.randrange(H) for _ in range(depth)] for _ in range(n)], dtype=np.uint32)
        if n > 2:
            idx[n // 2, depth - 1] |= H
        want = _chain(gpu_ctx, pks[:n], cc[:n], idx)
        assert _same(path(gpu_ctx, pks[:n], cc[:n], idx, dev), want), n
        assert (want[4] != 0).sum() == (1 if n > 2 else 0) and want[0][0].any()
        shared = path(gpu_ctx, pks[5:6], cc[5:6], idx, dev)
        assert _same(shared, _chain(gpu_ctx, pks[5:6], cc[5:6], idx)), n
        assert _same(shared, path(gpu_ctx, np.repeat(pks[5:6], n, axis=0), np.repeat(cc[5:6], n, axis=0), idx, dev)), n
    gpu_ctx.check()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_path_one_refusal_among_ordinary(gpu_ctx, dev):
    """a hardened index at each level in turn, and a bad parent: the right status, all four outputs zero, neighbours untouched"""
    keys, ccs = keys_pool()
    rng = random.Random(0x3204)
    idx = np.array([[rng.randrange(H) for _ in range(3)] for _ in range(AMONG)], dtype=np.uint32)
    pks, cc = _brows(keys[:AMONG], 33), _brows(ccs[:AMONG], 32)
    clean = _chain(gpu_ctx, pks, cc, idx)
    assert not clean[4].any()
    cases = [("index", level) for level in range(3)] + [("parent", 0)]
    for k, (what, level) in enumerate(cases):
        for lane in (LANES[k % len(LANES)], LANES[(k + 2) % len(LANES)]):
            p, ix = pks.copy(), idx.copy()
            if what == "index":
                ix[lane, level] |= H
            else:
                p[lane, 0] = 4
            want = [a.copy() for a in clean]
            for a in want[:4]:
                a[lane] = 0
            want[4][lane] = W.BAD_INDEX if what == "index" else W.BAD_POINT
            assert _same(path(gpu_ctx, p, cc, ix, dev), want), (what, level, lane)
    gpu_ctx.check()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_path_optional_outputs(gpu_ctx, dev):
    keys, ccs = keys_pool()
    rows, by_depth = path_pool()
    for depth in (1, 3):
        for fp in (False, True):
            for h160 in (False, True):
                got = path(gpu_ctx, _brows(keys[:9], 33), _brows(ccs[:9], 32), [r[:depth] for r in rows[:9]], dev, fp, h160)
                assert _same(got, _path_want(by_depth[depth][:9], fp, h160)), (depth, fp, h160)
    gpu_ctx.check()


# ---- chunks, shards, arguments ---------------------------------------------------------------------------------------------
def test_chunks_and_shards(gpu_ctx):
    import forge_ec_amd as F
    n = 300
    keys, ccs = keys_pool()
    rng = random.Random(0x3205)
    pks = _brows([keys[i % 257] for i in range(n)], 33)
    cc = _brows([ccs[(i * 7) % 257] for i in range(n)], 32)
    idx = np.array([[rng.randrange(H) for _ in range(2)] for _ in range(n)], dtype=np.uint32)
    idx[130, 0] |= H
    pks[200, 0] = 7
    msgs = _messages(n, 3)
    want_path = _chain(gpu_ctx, pks, cc, idx)
    want_shared = _chain(gpu_ctx, pks[:1], cc[:1], idx)
    xs = np.ascontiguousarray(pks[:, 1:])
    tw = _brows([W.taptweak(bytes(x), bytes(r)) for x, r in zip(xs, cc)], 32)
    t33, tst = _secp(gpu_ctx).pubkey_tweak_add(xs, tw, 32, 33)
    want_tap = (np.ascontiguousarray(t33[:, 1:]), t33[:, 0] & 1, tst)
    want_r, want_h = _brows([W.ripemd160(m) for m in msgs], 20), _brows([W.hash160(m) for m in msgs], 20)
    want_p = _brows([W.hash160(bytes(p)) for p in pks], 20)
    assert sorted(set(want_path[4])) == [0, W.BAD_POINT, W.BAD_INDEX] and not tst.any()

    def run(ctx):
        assert _same(path(ctx, pks, cc, idx, False), want_path)
        assert _same(path(ctx, pks[:1], cc[:1], idx, False), want_shared)
        assert _same(path(ctx, pks, cc, idx, False, False, False), want_path[:2] + (None, None, want_path[4]))
        assert _same(taproot(ctx, xs, cc, 32, False), want_tap)
        assert np.array_equal(digests(ctx, "ripemd160", msgs, False)[0], want_r)
        assert np.array_equal(digests(ctx, "hash160", msgs, False)[0], want_h)
        assert np.array_equal(pubkey_hash160(ctx, pks, 33, False), want_p)

    gpu_ctx.set_chunk(128)
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
    lib, h = L.lib(), gpu_ctx._h
    p = lambda a: a.ctypes.data   # noqa: E731
    n = 4
    keys, ccs = keys_pool()
    pks, cc = _brows(keys[:n], 33), _brows(ccs[:n], 32)
    xs = np.ascontiguousarray(pks[:, 1:])
    idx = np.arange(2 * n, dtype=np.uint32).reshape(n, 2)
    msg, off = np.frombuffer(b"abcdefgh", np.uint8).copy(), np.array([0, 2, 4, 6, 8], np.uint64)
    o20, o32, o33, o4 = (np.zeros((n, w), np.uint8) for w in (20, 32, 33, 4))
    st, par = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    # the host forms: a good call, n = 0 with nulls, each null, a bad layout, the lengths, depth, n_par
    for fn in (lib.fec_canon_ripemd160, lib.fec_canon_hash160):
        assert fn(h, p(msg), p(off), 8, p(o20), n) == 0
        assert fn(h, None, p(off[:1]), 0, None, 0) == 0
        assert fn(None, p(msg), p(off), 8, p(o20), n) == ARG and fn(h, p(msg), None, 8, p(o20), n) == ARG and fn(h, p(msg), p(off), 8, None, n) == ARG
        assert fn(h, None, p(off), 8, p(o20), n) == ARG and fn(h, p(msg), p(off), 7, p(o20), n) == ARG
        assert fn(h, p(msg), p(np.array([0, 4, 2, 6, 8], np.uint64)), 8, p(o20), n) == ARG
    assert lib.fec_canon_pubkey_hash160(h, p(pks), 33, p(o20), n) == 0 and lib.fec_canon_pubkey_hash160(h, None, 33, None, 0) == 0
    for args in ((None, p(pks), 33, p(o20), n), (h, None, 33, p(o20), n), (h, p(pks), 33, None, n), (h, p(pks), 32, p(o20), n), (h, p(pks), 64, p(o20), n)):
        assert lib.fec_canon_pubkey_hash160(*args) == ARG, args
    good = [h, p(xs), 32, p(cc), p(o32), p(par), p(st), n]
    assert lib.fec_canon_taproot_output_key(*good) == 0 and lib.fec_canon_taproot_output_key(h, None, 32, None, None, None, None, 0) == 0
    assert lib.fec_canon_taproot_output_key(h, p(xs), 32, None, p(o32), p(par), p(st), n) == 0    # no roots: BIP-86
    for i in (0, 1, 4, 5, 6):
        args = list(good)
        args[i] = None
        assert lib.fec_canon_taproot_output_key(*args) == ARG, i
    for ln in (0, 31, 34, 65):
        assert lib.fec_canon_taproot_output_key(h, p(xs), ln, p(cc), p(o32), p(par), p(st), n) == ARG, ln
    good = [h, p(pks), p(cc), n, p(idx), 2, p(o33), p(o32), p(o4), p(o20), p(st), n]
    assert lib.fec_canon_bip32_derive_pub_path(*good) == 0
    assert lib.fec_canon_bip32_derive_pub_path(h, None, None, 0, None, 1, None, None, None, None, None, 0) == 0
    for i in (0, 1, 2, 4, 6, 7, 10):
        args = list(good)
        args[i] = None
        assert lib.fec_canon_bip32_derive_pub_path(*args) == ARG, i
    for depth in (0, 256, 1 << 32):
        assert lib.fec_canon_bip32_derive_pub_path(h, p(pks), p(cc), n, p(idx), depth, p(o33), p(o32), p(o4), p(o20), p(st), n) == ARG, depth
    for n_par in (0, 2, 3, 5):
        assert lib.fec_canon_bip32_derive_pub_path(h, p(pks), p(cc), n_par, p(idx), 2, p(o33), p(o32), p(o4), p(o20), p(st), n) == ARG, n_par
    # the *_dev forms: good calls at odd alignments of the unaligned records, n = 0, nulls, misalignment, a multi-device ctx
    pad = np.zeros(16, np.uint8)
    tm, tp, tc, tx = (_to_dev(np.concatenate([a.reshape(-1), pad])) for a in (msg, pks, cc, xs))
    toff, ti = _to_dev(off), _to_dev(np.concatenate([idx.reshape(-1), np.zeros(4, np.uint32)]))
    to, tc2, t20, t4 = (torch.zeros(n * w + 16, dtype=torch.uint8, device="cuda") for w in (33, 32, 20, 4))
    tst, tpar = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    M, OFF, PK, CC, X, IX, O, OC, D, FP, ST, PAR = (t.data_ptr() for t in (tm, toff, tp, tc, tx, ti, to, tc2, t20, t4, tst, tpar))
    for fn in (lib.fec_canon_ripemd160_dev, lib.fec_canon_hash160_dev):
        assert fn(h, M, OFF, 8, D, ST, n, None) == 0 and fn(h, M, OFF, 8, D + 4, None, n, None) == 0
        assert fn(h, None, None, 0, None, None, 0, None) == 0 and fn(h, M, OFF + 4, 8, D + 2, ST, 0, None) == 0
        for args in ((None, M, OFF, 8, D, ST, n, None), (h, None, OFF, 8, D, ST, n, None), (h, M, None, 8, D, ST, n, None), (h, M, OFF, 8, None, ST, n, None),
                     (h, M, OFF + 4, 8, D, ST, n, None), (h, M, OFF, 8, D + 2, ST, n, None), (h, M, OFF, 8, D + 1, ST, n, None)):
            assert fn(*args) == ARG, args
    assert lib.fec_canon_pubkey_hash160_dev(h, PK, 33, D, n, None) == 0 and lib.fec_canon_pubkey_hash160_dev(h, PK + 1, 33, D + 4, n, None) == 0
    assert lib.fec_canon_pubkey_hash160_dev(h, None, 33, None, 0, None) == 0
    for args in ((None, PK, 33, D, n, None), (h, None, 33, D, n, None), (h, PK, 33, None, n, None), (h, PK, 33, D + 2, n, None), (h, PK, 32, D, n, None)):
        assert lib.fec_canon_pubkey_hash160_dev(*args) == ARG, args
    assert lib.fec_canon_taproot_output_key_dev(h, X, 32, CC, OC, PAR, ST, n, None) == 0
    assert lib.fec_canon_taproot_output_key_dev(h, PK + 1, 33, None, OC, PAR, ST, n, None) == 0   # 33-byte records have no alignment
    assert lib.fec_canon_taproot_output_key_dev(h, None, 32, None, None, None, None, 0, None) == 0
    for args in ((None, X, 32, CC, OC, PAR, ST, n, None), (h, None, 32, CC, OC, PAR, ST, n, None), (h, X, 32, CC, None, PAR, ST, n, None),
                 (h, X, 32, CC, OC, None, ST, n, None), (h, X, 32, CC, OC, PAR, None, n, None), (h, X + 8, 32, CC, OC, PAR, ST, n, None),
                 (h, X, 32, CC + 8, OC, PAR, ST, n, None), (h, X, 32, CC, OC + 8, PAR, ST, n, None), (h, X, 34, CC, OC, PAR, ST, n, None)):
        assert lib.fec_canon_taproot_output_key_dev(*args) == ARG, args
    assert lib.fec_canon_bip32_derive_pub_path_dev(h, PK, CC, n, IX, 2, O, OC, FP, D, ST, n, None) == 0
    assert lib.fec_canon_bip32_derive_pub_path_dev(h, PK + 33, CC, 1, IX + 4, 1, O + 3, OC, FP + 4, D + 4, ST, n, None) == 0
    assert lib.fec_canon_bip32_derive_pub_path_dev(h, PK, CC, n, IX, 2, O, OC, None, None, ST, n, None) == 0
    assert lib.fec_canon_bip32_derive_pub_path_dev(h, None, None, 0, None, 1, None, None, None, None, None, 0, None) == 0
    for args in ((None, PK, CC, n, IX, 2, O, OC, FP, D, ST, n, None), (h, None, CC, n, IX, 2, O, OC, FP, D, ST, n, None),
                 (h, PK, None, n, IX, 2, O, OC, FP, D, ST, n, None), (h, PK, CC, n, None, 2, O, OC, FP, D, ST, n, None),
                 (h, PK, CC, n, IX, 2, None, OC, FP, D, ST, n, None), (h, PK, CC, n, IX, 2, O, None, FP, D, ST, n, None),
                 (h, PK, CC, n, IX, 2, O, OC, FP, D, None, n, None), (h, PK, CC + 8, n, IX, 2, O, OC, FP, D, ST, n, None),
                 (h, PK, CC, n, IX + 2, 2, O, OC, FP, D, ST, n, None), (h, PK, CC, n, IX, 2, O, OC + 8, FP, D, ST, n, None),
                 (h, PK, CC, n, IX, 2, O, OC, FP + 2, D, ST, n, None), (h, PK, CC, n, IX, 2, O, OC, FP, D + 2, ST, n, None),
                 (h, PK, CC, n, IX, 0, O, OC, FP, D, ST, n, None), (h, PK, CC, n, IX, 256, O, OC, FP, D, ST, n, None),
                 (h, PK, CC, 2, IX, 2, O, OC, FP, D, ST, n, None), (h, PK, CC, 0, IX, 2, O, OC, FP, D, ST, n, None)):
        assert lib.fec_canon_bip32_derive_pub_path_dev(*args) == ARG, args
    torch.cuda.synchronize()
    with F.Context(devices=[0, 0]) as multi:
        m = multi._h
        assert lib.fec_canon_ripemd160_dev(m, M, OFF, 8, D, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_hash160_dev(m, M, OFF, 8, D, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_pubkey_hash160_dev(m, PK, 33, D, n, None) == UNSUPPORTED
        assert lib.fec_canon_taproot_output_key_dev(m, X, 32, CC, OC, PAR, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_bip32_derive_pub_path_dev(m, PK, CC, n, IX, 2, O, OC, FP, D, ST, n, None) == UNSUPPORTED
    gpu_ctx.check()


# ---- stream order ----------------------------------------------------------------------------------------------------------
def test_taproot_and_path_alternated_on_two_streams(gpu_ctx):
    """both calls keep their work in ctx->d_verify; alternated on two streams with nothing between them but the library's own
    ordering, every round's results are still exact"""
    import torch
    n, rounds = 257, 4
    keys, ccs = keys_pool()
    xs, roots, with_root, _ = taproot_pool()
    rng = random.Random(0x3206)
    idx = np.array([[rng.randrange(H) for _ in range(3)] for _ in range(n)], dtype=np.uint32)
    pks, cc = _brows(keys, 33), _brows(ccs, 32)
    want_path = _chain(gpu_ctx, pks, cc, idx)
    want_tap = (_brows([r[0] for r in with_root], 32), np.array([r[1] for r in with_root], np.uint8), np.zeros(n, np.uint8))
    tp, tc, ti, tx, tr = _to_dev(pks), _to_dev(cc), _to_dev(idx), _to_dev(_brows(xs, 32)), _to_dev(_brows(roots, 32))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for r in range(rounds):
        a = [_dev_out(n, 32), _dev_out(n, 1), _dev_out(n, 1, 77)]
        b = [_dev_out(n, 33), _dev_out(n, 32), _dev_out(n, 4), _dev_out(n, 20), _dev_out(n, 1, 77)]
        outs.append((a, b))
    torch.cuda.synchronize()
    for a, b in outs:
        _secp(gpu_ctx).taproot_output_key_dev(tx.data_ptr(), 32, tr.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), n, stream=s1.cuda_stream)
        _hd(gpu_ctx).derive_pub_path_dev(tp.data_ptr(), tc.data_ptr(), n, ti.data_ptr(), 3, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(),
                                         b[3].data_ptr(), b[4].data_ptr(), n, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(outs):
        assert _same([t.cpu().numpy() for t in a], want_tap), r
        assert _same([t.cpu().numpy() for t in b], want_path), r
    gpu_ctx.check()
