"""
GPU tests of canonical-mode Keccak-256, ECDSA public-key recovery and recoverable signing (include/fecgpu_canon.h:
fec_canon_keccak256, fec_canon_ecdsa_recover, fec_canon_ecdsa_sign_recoverable_digest and their *_dev forms) against the
fixture tests/golden/canon_recover_vectors.json, which the model tests/canon_recover_ref.py wrote and
tests/test_canon_recover_model.py pins.  Every comparison is byte-exact, status included.  Also: the batch sizes at the edges
of the eight-element grouping and its 64-lane stride, each refused case alone among ordinary elements (a rejected r must not
poison the inversion its group shares), sign -> recover -> public key round trips, address == Keccak of the raw key, chunks,
shard workers, refused arguments.
"""
import json
import os
import random

import numpy as np
import pytest

import canon_msg_ref as R
import canon_recover_ref as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_recover_vectors.json")))
CURVES = sorted(R.WEIERSTRASS)
CASES = {cv: [c for c in FIXTURE["cases"] if c["curve"] == cv] for cv in CURVES}
COUNTS = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513]
ARG, UNSUPPORTED = -1, -5
AMONG = 64 * 3 + 5
LANES = (0, 31, 32, 63, AMONG - 1)
LOW_S = 1


def forms(curve):
    return (33, 65, 64, 20) if curve == "secp256k1" else (33, 65, 64)


def _cv(ctx, curve):
    from forge_ec_amd.canon import CANON_CURVES
    return CANON_CURVES[curve](ctx)


_POINTS = {}


def expected(case, out_len):
    """the record of one fixture case in one output form, from its key33 / address"""
    if case["status"]:
        return bytes(out_len)
    if out_len == 20:
        return bytes.fromhex(case["address"])
    if case["key33"] not in _POINTS:
        _POINTS[case["key33"]] = R.sec1_decode(R.WEIERSTRASS[case["curve"]], bytes.fromhex(case["key33"]))
    return K.encode(_POINTS[case["key33"]], out_len)


def _rows(hexes, width):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), dtype=np.uint8).reshape(len(hexes), width).copy()


def _inputs(pick):
    return (_rows([c["digest"] for c in pick], 32), _rows([c["sig"] for c in pick], 64), np.array([c["recid"] for c in pick], dtype=np.uint8),
            np.array([c["status"] for c in pick], dtype=np.uint8))


def _want(pick, out_len):
    return np.frombuffer(b"".join(expected(c, out_len) for c in pick), dtype=np.uint8).reshape(len(pick), out_len)


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _recover_dev(ctx, curve, dg, sg, rc, out_len):
    import torch
    n = dg.shape[0]
    td, ts, tr = _to_dev(dg), _to_dev(sg), _to_dev(rc)
    out = torch.full((n, out_len), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    _cv(ctx, curve).ecdsa_recover_dev(td.data_ptr(), ts.data_ptr(), tr.data_ptr(), out.data_ptr(), out_len, st.data_ptr(), n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _both(ctx, curve, dg, sg, rc, out_len):
    yield _cv(ctx, curve).ecdsa_recover(dg, sg, rc, out_len)
    yield _recover_dev(ctx, curve, dg, sg, rc, out_len)


@pytest.mark.parametrize("curve", CURVES)
def test_every_fixture_case_host_and_dev_forms(gpu_ctx, curve):
    pick = CASES[curve]
    dg, sg, rc, wst = _inputs(pick)
    assert (wst == K.NO_KEY).sum() >= 18 and (wst == 0).sum() >= 128 + 10   # sign; digest 6, doubling 2, x = n + t 2
    for out_len in forms(curve):
        want = _want(pick, out_len)
        for out, st in _both(gpu_ctx, curve, dg, sg, rc, out_len):
            bad = [i for i in range(len(pick)) if st[i] != wst[i] or bytes(out[i]) != bytes(want[i])]
            assert not bad, [(out_len, pick[i]["class"], pick[i]["name"], int(st[i])) for i in bad]
    gpu_ctx.check()


@pytest.mark.parametrize("curve", CURVES)
def test_element_counts(gpu_ctx, curve):
    """n cases at the edges of the eight-element groups and of their 64-lane stride, cycling from the refused cases on, so that
    n = 1 is not an ordinary case; the forms take turns"""
    cases = CASES[curve]
    start = next(i for i, c in enumerate(cases) if c["status"])
    fs = forms(curve)
    for j, n in enumerate(COUNTS):
        pick = [cases[(start + i) % len(cases)] for i in range(n)]
        dg, sg, rc, wst = _inputs(pick)
        out_len = fs[j % len(fs)]
        want = _want(pick, out_len)
        out, st = _cv(gpu_ctx, curve).ecdsa_recover(dg, sg, rc, out_len) if j % 2 else _recover_dev(gpu_ctx, curve, dg, sg, rc, out_len)
        assert np.array_equal(st, wst) and np.array_equal(out, want), (n, out_len)
    gpu_ctx.check()


@pytest.mark.parametrize("curve", CURVES)
def test_refused_cases_alone_among_ordinary_ones(gpu_ctx, curve):
    """each refused case alone at lanes 0, 31, 32, 63 and at the last of 197 ordinary elements, every one of which must still be
    exact: a rejected r shares its group's inversion with seven of them"""
    ordinary = [c for c in CASES[curve] if c["class"] == "sign"][:AMONG // 2] + [c for c in CASES[curve] if c["status"] == 0][-(AMONG - AMONG // 2):]
    refused = [c for c in CASES[curve] if c["status"]]
    assert len(ordinary) == AMONG and len(refused) >= 18 and not any(c["status"] for c in ordinary)
    dg0, sg0, rc0, st0 = _inputs(ordinary)
    want0 = _want(ordinary, 65)
    for j, c in enumerate(refused):
        cd, cs, cr, cst = _inputs([c])
        for lane in LANES:
            dg, sg, rc, want, wst = dg0.copy(), sg0.copy(), rc0.copy(), want0.copy(), st0.copy()
            dg[lane], sg[lane], rc[lane], want[lane], wst[lane] = cd[0], cs[0], cr[0], 0, cst[0]
            out, st = _cv(gpu_ctx, curve).ecdsa_recover(dg, sg, rc, 65) if (j + lane) % 2 else _recover_dev(gpu_ctx, curve, dg, sg, rc, 65)
            assert np.array_equal(st, wst) and np.array_equal(out, want), (c["name"], lane)
    gpu_ctx.check()


@pytest.mark.parametrize("curve", CURVES)
def test_sign_recover_round_trip(gpu_ctx, curve):
    """n = 513: sign_recoverable_digest -> recover(65) == public_key(65); the signatures are those of ecdsa_sign_digest, with
    and without LOW_S; on secp256k1 recover(20) == Keccak-256(recover(64))[12:] through fec_canon_keccak256"""
    import torch
    from forge_ec_amd.canon import CanonKeccak
    C = R.WEIERSTRASS[curve]
    rng = random.Random(0x513)
    n = 513
    keys = np.frombuffer(b"".join(rng.randrange(1, C.N).to_bytes(32, "big") for _ in range(n)), dtype=np.uint8).reshape(n, 32).copy()
    keys[5] = 0                                                         # a refused key: zero signature, recid 0, status 6
    dg = np.frombuffer(bytes(rng.randrange(256) for _ in range(32 * n)), dtype=np.uint8).reshape(n, 32).copy()
    cv = _cv(gpu_ctx, curve)
    pk, pst = cv.public_key(keys, 65)
    flipped = 0
    for flags in (0, LOW_S):
        sigs, rec, st = cv.ecdsa_sign_recoverable_digest(dg, keys, flags)
        plain, pst2 = cv.ecdsa_sign_digest(dg, keys, flags)
        assert np.array_equal(sigs, plain) and np.array_equal(st, pst2) and st[5] == 6 and rec[5] == 0 and not st[np.arange(n) != 5].any()
        assert set(rec.tolist()) == {0, 1}
        td, tk = _to_dev(dg), _to_dev(keys)
        ts = torch.full((n, 64), 0xEE, dtype=torch.uint8, device="cuda")
        tr, tst = torch.full((n,), 9, dtype=torch.uint8, device="cuda"), torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        cv.ecdsa_sign_recoverable_digest_dev(td.data_ptr(), tk.data_ptr(), flags, ts.data_ptr(), tr.data_ptr(), tst.data_ptr(), n)
        torch.cuda.synchronize()
        assert np.array_equal(ts.cpu().numpy(), sigs) and np.array_equal(tr.cpu().numpy(), rec) and np.array_equal(tst.cpu().numpy(), st)
        out, rst = cv.ecdsa_recover(dg, sigs, rec, 65)
        ok = np.arange(n) != 5
        assert np.array_equal(out[ok], pk[ok]) and not rst[ok].any() and rst[5] == K.NO_KEY and not out[5].any()
        if flags == 0:
            first = (sigs.copy(), rec.copy())
        else:
            flipped = int((sigs != first[0]).any(axis=1).sum())
            assert np.array_equal((sigs != first[0]).any(axis=1), rec != first[1])   # the id turns over exactly where s did
        for i in (0, 256, 512):
            assert (bytes(sigs[i]), int(rec[i]), 0) == K.sign_recoverable_digest(C, int.from_bytes(bytes(keys[i]), "big"), bytes(dg[i]), flags)
    assert n // 4 < flipped < 3 * n // 4
    if curve == "secp256k1":
        raw, _ = cv.ecdsa_recover(dg, sigs, rec, 64)
        addr, ast = cv.ecdsa_recover(dg, sigs, rec, 20)
        hashed = CanonKeccak(gpu_ctx).keccak256([bytes(r) for r in raw])
        assert np.array_equal(addr[ok], hashed[ok][:, 12:]) and ast[5] == K.NO_KEY and not addr[5].any()
        assert bytes(addr[0]) == K.eth_address(R.sec1_decode(C, bytes(pk[0])))
    gpu_ctx.check()


def _keccak_batch():
    """the fixture's messages in one ragged batch, each starting at its own alignment mod 8: short fillers (hashed by the model)
    in between bring the running offset there"""
    buf = bytes.fromhex(FIXTURE["keccak_buffer"])
    msgs, want = [], []
    cur = 0
    for c in FIXTURE["keccak"]:
        fill = (c["at"] - cur) % 8
        if fill:
            msgs.append(buf[100:100 + fill])
            want.append(K.keccak256(msgs[-1]))
            cur += fill
        assert cur % 8 == c["at"]
        msgs.append(buf[c["at"]:c["at"] + c["len"]])
        want.append(bytes.fromhex(c["digest"]))
        cur += c["len"]
    return msgs, np.frombuffer(b"".join(want), dtype=np.uint8).reshape(len(msgs), 32)


def test_keccak_fixture_lengths_and_alignments(gpu_ctx):
    import torch
    from forge_ec_amd.canon import CanonKeccak
    kk = CanonKeccak(gpu_ctx)
    msgs, want = _keccak_batch()
    assert len(msgs) > len(FIXTURE["keccak"]) and sum(1 for m in msgs if not m) >= 8
    assert np.array_equal(kk.keccak256(msgs), want)
    off = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    n = len(msgs)
    tm, to = _to_dev(data), _to_dev(off)
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    kk.keccak256_dev(tm.data_ptr(), to.data_ptr(), data.size, out.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and not st.cpu().numpy().any()
    # all-empty batch; no status array; a bad range: message 3 ends before it begins, message 6 ends past the buffer
    empty = kk.keccak256([b""] * 65)
    assert all(bytes(e) == K.keccak256(b"") for e in empty)
    bad = off.copy()
    bad[4] = bad[3] - 1
    bad[7] = data.size + 1
    tb = _to_dev(bad)
    out.fill_(0xEE)
    kk.keccak256_dev(tm.data_ptr(), tb.data_ptr(), data.size, out.data_ptr(), None, n)
    st.fill_(9)
    out2 = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    kk.keccak256_dev(tm.data_ptr(), tb.data_ptr(), data.size, out2.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    got, got_st = out2.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), got)
    refused = [i for i in range(n) if not (bad[i] <= bad[i + 1] <= data.size)]
    assert refused == [3, 6, 7] or refused == [3, 6]
    for i in range(n):
        if i in refused:
            assert got_st[i] == 4 and not got[i].any()
        else:
            assert got_st[i] == 0 and bytes(got[i]) == K.keccak256(data[int(bad[i]):int(bad[i + 1])].tobytes()), i
    gpu_ctx.check()


def test_chunks_and_a_multi_device_ctx(gpu_ctx):
    """n = 200 in chunks of 64; two shard workers on one GPU"""
    import forge_ec_amd as F
    from forge_ec_amd.canon import CanonKeccak
    n = 200
    cases = CASES["secp256k1"]
    pick = [cases[(60 + i) % len(cases)] for i in range(n)]      # the refused cases lie inside the second and third chunk
    dg, sg, rc, wst = _inputs(pick)
    want20, want33 = _want(pick, 20), _want(pick, 33)
    signing = [c for c in CASES["p256"] if c["class"] == "sign" and c["flags"] == LOW_S]
    sd, skeys = _rows([c["digest"] for c in signing], 32), _rows([c["key"] for c in signing], 32)
    msgs, kwant = _keccak_batch()

    def run(ctx):
        out, st = _cv(ctx, "secp256k1").ecdsa_recover(dg, sg, rc, 20)
        assert np.array_equal(out, want20) and np.array_equal(st, wst) and (wst != 0).sum() >= 18
        out, st = _cv(ctx, "secp256k1").ecdsa_recover(dg, sg, rc, 33)
        assert np.array_equal(out, want33) and np.array_equal(st, wst)
        sigs, rec, st = _cv(ctx, "p256").ecdsa_sign_recoverable_digest(sd, skeys, LOW_S)
        assert [bytes(s).hex() for s in sigs] == [c["sig"] for c in signing] and rec.tolist() == [c["recid"] for c in signing] and not st.any()
        assert np.array_equal(CanonKeccak(ctx).keccak256(msgs), kwant)

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
    assert L.CANON_NO_KEY == K.NO_KEY == 8
    lib, h = L.lib(), gpu_ctx._h
    p = lambda a: a.ctypes.data   # noqa: E731
    SECP, P256, ED = L.SECP256K1, L.P256, L.ED25519
    n = 4
    pick = CASES["secp256k1"][:n]
    dg, sg, rc, wst = _inputs(pick)
    keys = _rows([c["key"] for c in pick], 32)
    out, st = np.zeros((n, 65), np.uint8), np.zeros(n, np.uint8)
    sigs, rec = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8)
    msg = np.frombuffer(b"abcdefgh", dtype=np.uint8).copy()
    off = np.array([0, 3, 3, 8, 8], dtype=np.uint64)
    dig = np.zeros((n, 32), np.uint8)
    # the host forms: a good call, n = 0 with nulls, each null, the curves, the forms, the flags, a bad layout
    assert lib.fec_canon_ecdsa_recover(h, SECP, p(dg), p(sg), p(rc), p(out), 65, p(st), n) == 0 and np.array_equal(out, _want(pick, 65))
    assert lib.fec_canon_ecdsa_recover(h, SECP, None, None, None, None, 65, None, 0) == 0
    assert lib.fec_canon_ecdsa_sign_recoverable_digest(h, SECP, None, None, 0, None, None, None, 0) == 0
    assert lib.fec_canon_keccak256(h, None, p(off[:1]), 0, None, 0) == 0
    good = [h, SECP, p(dg), p(sg), p(rc), p(out), 65, p(st), n]
    for i in (0, 2, 3, 4, 5, 7):
        args = list(good)
        args[i] = None
        assert lib.fec_canon_ecdsa_recover(*args) == ARG, i
    for out_len in (0, 1, 21, 32, 34, 66, 128):
        assert lib.fec_canon_ecdsa_recover(h, SECP, p(dg), p(sg), p(rc), p(out), out_len, p(st), n) == ARG, out_len
    assert lib.fec_canon_ecdsa_recover(h, P256, p(dg), p(sg), p(rc), p(out), 20, p(st), n) == ARG
    assert lib.fec_canon_ecdsa_recover(h, P256, p(dg), p(sg), p(rc), p(out), 64, p(st), n) == 0
    assert lib.fec_canon_ecdsa_recover(h, ED, p(dg), p(sg), p(rc), p(out), 33, p(st), n) == UNSUPPORTED
    assert lib.fec_canon_ecdsa_recover(h, 7, p(dg), p(sg), p(rc), p(out), 33, p(st), n) == ARG
    good = [h, SECP, p(dg), p(keys), 0, p(sigs), p(rec), p(st), n]
    model = [K.sign_recoverable_digest(R.SECP, int(c["key"], 16), bytes.fromhex(c["digest"]), 0) for c in pick]
    assert lib.fec_canon_ecdsa_sign_recoverable_digest(*good) == 0
    assert [(bytes(sigs[i]), int(rec[i]), int(st[i])) for i in range(n)] == model
    for i in (0, 2, 3, 5, 6, 7):
        args = list(good)
        args[i] = None
        assert lib.fec_canon_ecdsa_sign_recoverable_digest(*args) == ARG, i
    assert lib.fec_canon_ecdsa_sign_recoverable_digest(h, SECP, p(dg), p(keys), 2, p(sigs), p(rec), p(st), n) == ARG
    assert lib.fec_canon_ecdsa_sign_recoverable_digest(h, ED, p(dg), p(keys), 0, p(sigs), p(rec), p(st), n) == UNSUPPORTED
    assert lib.fec_canon_keccak256(h, p(msg), p(off), 8, p(dig), n) == 0 and bytes(dig[0]) == K.keccak256(b"abc") and bytes(dig[1]) == K.keccak256(b"")
    for args in ((None, p(msg), p(off), 8, p(dig), n), (h, None, p(off), 8, p(dig), n), (h, p(msg), None, 8, p(dig), n), (h, p(msg), p(off), 8, None, n),
                 (h, p(msg), p(off), 7, p(dig), n), (h, p(msg), p(np.array([0, 3, 2, 8, 8], dtype=np.uint64)), 8, p(dig), n)):
        assert lib.fec_canon_keccak256(*args) == ARG, args
    # the *_dev forms: n = 0, nulls, misalignment, a multi-device ctx
    pad = np.zeros(16, np.uint8)
    td, ts, tk = (_to_dev(np.concatenate([a.reshape(-1), pad])) for a in (dg, sg, keys))
    tr = _to_dev(rc)
    to = torch.zeros(n * 65 + 16, dtype=torch.uint8, device="cuda")
    tst, trec = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    tm, toff = _to_dev(np.concatenate([msg, pad])), _to_dev(np.concatenate([off, np.zeros(2, np.uint64)]))
    D, S, KY, RC, O, ST, RE, M, OF = (t.data_ptr() for t in (td, ts, tk, tr, to, tst, trec, tm, toff))
    for out_len in (33, 65, 64, 20):
        assert lib.fec_canon_ecdsa_recover_dev(h, SECP, D, S, RC, O, out_len, ST, n, None) == 0
    assert lib.fec_canon_ecdsa_sign_recoverable_digest_dev(h, SECP, D, KY, 1, O, RE, ST, n, None) == 0
    assert lib.fec_canon_keccak256_dev(h, M, OF, 8, O, ST, n, None) == 0 and lib.fec_canon_keccak256_dev(h, M, OF, 8, O, None, n, None) == 0
    torch.cuda.synchronize()
    assert lib.fec_canon_ecdsa_recover_dev(h, SECP, None, None, None, None, 33, None, 0, None) == 0
    assert lib.fec_canon_ecdsa_sign_recoverable_digest_dev(h, SECP, None, None, 0, None, None, None, 0, None) == 0
    assert lib.fec_canon_keccak256_dev(h, None, None, 0, None, None, 0, None) == 0
    for args in ((None, SECP, D, S, RC, O, 33, ST, n, None), (h, SECP, None, S, RC, O, 33, ST, n, None), (h, SECP, D, None, RC, O, 33, ST, n, None),
                 (h, SECP, D, S, None, O, 33, ST, n, None), (h, SECP, D, S, RC, None, 33, ST, n, None), (h, SECP, D, S, RC, O, 33, None, n, None),
                 (h, SECP, D + 8, S, RC, O, 33, ST, n, None), (h, SECP, D, S + 4, RC, O, 33, ST, n, None), (h, SECP, D, S, RC, O + 8, 64, ST, n, None),
                 (h, SECP, D, S, RC, O + 4, 20, ST, n, None), (h, SECP, D, S, RC, O, 32, ST, n, None), (h, P256, D, S, RC, O, 20, ST, n, None),
                 (h, 7, D, S, RC, O, 33, ST, n, None)):
        assert lib.fec_canon_ecdsa_recover_dev(*args) == ARG, args
    assert lib.fec_canon_ecdsa_recover_dev(h, SECP, D, S, RC, O + 1, 33, ST, n, None) == 0     # a SEC 1 record array has no alignment
    assert lib.fec_canon_ecdsa_recover_dev(h, ED, D, S, RC, O, 33, ST, n, None) == UNSUPPORTED
    for args in ((None, SECP, D, KY, 0, O, RE, ST, n, None), (h, SECP, None, KY, 0, O, RE, ST, n, None), (h, SECP, D, None, 0, O, RE, ST, n, None),
                 (h, SECP, D, KY, 0, None, RE, ST, n, None), (h, SECP, D, KY, 0, O, None, ST, n, None), (h, SECP, D, KY, 0, O, RE, None, n, None),
                 (h, SECP, D, KY, 4, O, RE, ST, n, None), (h, SECP, D + 8, KY, 0, O, RE, ST, n, None), (h, SECP, D, KY + 4, 0, O, RE, ST, n, None),
                 (h, SECP, D, KY, 0, O + 8, RE, ST, n, None)):
        assert lib.fec_canon_ecdsa_sign_recoverable_digest_dev(*args) == ARG, args
    assert lib.fec_canon_ecdsa_sign_recoverable_digest_dev(h, ED, D, KY, 0, O, RE, ST, n, None) == UNSUPPORTED
    for args in ((None, M, OF, 8, O, ST, n, None), (h, None, OF, 8, O, ST, n, None), (h, M, None, 8, O, ST, n, None), (h, M, OF, 8, None, ST, n, None),
                 (h, M, OF + 4, 8, O, ST, n, None), (h, M, OF, 8, O + 8, ST, n, None)):
        assert lib.fec_canon_keccak256_dev(*args) == ARG, args
    torch.cuda.synchronize()
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_canon_ecdsa_recover_dev(multi._h, SECP, D, S, RC, O, 33, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_ecdsa_sign_recoverable_digest_dev(multi._h, SECP, D, KY, 0, O, RE, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_keccak256_dev(multi._h, M, OF, 8, O, ST, n, None) == UNSUPPORTED
