"""
GPU tests of canonical-mode verification FROM THE MESSAGE (include/fecgpu_canon.h: fec_canon_ecdsa_verify_msg,
fec_canon_bip340_verify_msg, fec_canon_ed25519_verify_msg, fec_canon_decompress and their *_dev forms) against the
fixture tests/golden/canon_msg_vectors.json, which the model tests/canon_msg_ref.py wrote and tests/test_canon_msg_model.py
pins by the published vectors: every case through the host and the *_dev forms, ragged element counts, agreement with the
after-the-hash verifiers fed by hashlib, chunk invariance, bad ranges of a *_dev caller, refused arguments.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import canon_msg_ref as R
from oracle import canon_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_msg_vectors.json")))
BATCHES = FIXTURE["batches"]
IDS = ["%s-%s-%d" % (b["scheme"], b["curve"], b["pk_len"]) for b in BATCHES]
ARG, UNSUPPORTED = -1, -5


def _arrays(cases, n=None):
    """n cases, cycling: (msgs, sigs (n,64), pks (n,pk_len), want)."""
    n = len(cases) if n is None else n
    pick = [cases[i % len(cases)] for i in range(n)]
    msgs = [bytes.fromhex(c["msg"]) for c in pick]
    sigs = np.frombuffer(b"".join(bytes.fromhex(c["sig"]) for c in pick), dtype=np.uint8).reshape(n, 64).copy()
    pk = b"".join(bytes.fromhex(c["pk"]) for c in pick)
    pks = np.frombuffer(pk, dtype=np.uint8).reshape(n, len(pk) // n).copy()
    return msgs, sigs, pks, np.array([c["want"] for c in pick], dtype=np.uint8)


def _canon(gpu_ctx, curve):
    from forge_ec_amd.canon import CANON_CURVES
    return CANON_CURVES[curve](gpu_ctx)


def _host(gpu_ctx, b, msgs, sigs, pks):
    dev = _canon(gpu_ctx, b["curve"])
    if b["scheme"] == "ecdsa":
        return dev.ecdsa_verify_msg(msgs, sigs, pks, b["pk_len"])
    return dev.bip340_verify_msg(msgs, sigs, pks) if b["scheme"] == "bip340" else dev.ed25519_verify_msg(msgs, sigs, pks)


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _layout(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy(), off, int(off[-1])


def _dev(gpu_ctx, b, d_msgs, d_off, total, d_sigs, d_pks, d_res, n, stream=None):
    dev = _canon(gpu_ctx, b["curve"])
    if b["scheme"] == "ecdsa":
        dev.ecdsa_verify_msg_dev(d_msgs, d_off, total, d_sigs, d_pks, b["pk_len"], d_res, n, stream)
    elif b["scheme"] == "bip340":
        dev.bip340_verify_msg_dev(d_msgs, d_off, total, d_sigs, d_pks, d_res, n, stream)
    else:
        dev.ed25519_verify_msg_dev(d_msgs, d_off, total, d_sigs, d_pks, d_res, n, stream)


def _run_dev(gpu_ctx, b, msgs, sigs, pks):
    import torch
    buf, off, total = _layout(msgs)
    n = len(msgs)
    # the messages end where their allocation ends (a block of its own in torch's allocator), at an odd base address
    block = torch.zeros(10 << 20, dtype=torch.uint8, device="cuda")
    at = block.numel() - total
    block[at:] = _to_dev(buf)[:total]
    to, ts, tp = _to_dev(off), _to_dev(sigs), _to_dev(pks)
    res = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    _dev(gpu_ctx, b, block.data_ptr() + at, to.data_ptr(), total, ts.data_ptr(), tp.data_ptr(), res.data_ptr(), n)
    torch.cuda.synchronize()
    return res.cpu().numpy()


def _model_points(b, pks):
    C = R.WEIERSTRASS[b["curve"]]
    pts = [R.sec1_decode(C, bytes(k)) for k in pks]
    xy = np.array([M.xy_limbs(p) for p in pts], dtype=np.uint64)
    return xy, np.array([0 if p else 2 for p in pts], dtype=np.uint8)


@pytest.mark.parametrize("b", BATCHES, ids=IDS)
def test_every_fixture_case_host_forms(gpu_ctx, b):
    msgs, sigs, pks, want = _arrays(b["cases"])
    got = _host(gpu_ctx, b, msgs, sigs, pks)
    bad = [b["cases"][i]["name"] for i in np.nonzero(got != want)[0]]
    assert not bad, bad
    assert 0 < want.sum() < len(want)
    if b["scheme"] == "ecdsa":
        xy, st = _canon(gpu_ctx, b["curve"]).decompress(pks, b["pk_len"])
        wxy, wst = _model_points(b, pks)
        assert np.array_equal(st, wst) and np.array_equal(xy, wxy) and 0 < (wst == 2).sum() < len(wst)


@pytest.mark.parametrize("b", BATCHES, ids=IDS)
def test_every_fixture_case_dev_forms(gpu_ctx, b):
    import torch
    msgs, sigs, pks, want = _arrays(b["cases"])
    got = _run_dev(gpu_ctx, b, msgs, sigs, pks)
    bad = [b["cases"][i]["name"] for i in np.nonzero(got != want)[0]]
    assert not bad, bad
    if b["scheme"] == "ecdsa":
        n = len(msgs)
        tp = _to_dev(pks)
        xy = torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
        st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        _canon(gpu_ctx, b["curve"]).decompress_dev(tp.data_ptr(), b["pk_len"], xy.data_ptr(), st.data_ptr(), n)
        torch.cuda.synchronize()
        wxy, wst = _model_points(b, pks)
        assert np.array_equal(st.cpu().numpy(), wst) and np.array_equal(xy.cpu().numpy().view(np.uint64), wxy)


def test_published_vectors(gpu_ctx):
    """RFC 6979 A.2.5 (P-256, SHA-256, "sample"), BIP-340 vector 0, RFC 8032 section 7.1 tests 1 and 2, alone and tampered"""
    pub = FIXTURE["published"]
    assert sorted(pub) == ["bip340_vector0", "rfc6979_a25_sample", "rfc8032_test1", "rfc8032_test2"]
    for name, c in pub.items():
        msg, sig, pk = bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"])
        tampered = bytes([sig[0] ^ 1]) + sig[1:]
        msgs, sigs, pks = [msg, msg, msg + b"!"], [sig, tampered, sig], [pk, pk, pk]
        assert list(_host(gpu_ctx, c, msgs, sigs, pks)) == [1, 0, 0], name
        assert list(_run_dev(gpu_ctx, c, msgs, np.frombuffer(b"".join(sigs), dtype=np.uint8), np.frombuffer(b"".join(pks), dtype=np.uint8))) == [1, 0, 0], name
    c = pub["rfc6979_a25_sample"]
    unc = R.sec1_encode(R.sec1_decode(R.P256, bytes.fromhex(c["pk"])), compressed=False)
    assert list(_canon(gpu_ctx, "p256").ecdsa_verify_msg([bytes.fromhex(c["msg"])], bytes.fromhex(c["sig"]), unc, 65)) == [1]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 511, 513])
def test_element_counts(gpu_ctx, n):
    """NORM_GROUP = 8 signatures share an inversion per lane and the grouped kernels round their stride to 64 lanes: the
    ragged group and the ragged wave.  The cycle starts inside the negative cases so that n = 1 is not always a valid one."""
    for b in BATCHES:
        cases = b["cases"][-3:] + b["cases"]
        msgs, sigs, pks, want = _arrays(cases, n)
        assert np.array_equal(_host(gpu_ctx, b, msgs, sigs, pks), want), (b["scheme"], b["curve"], b["pk_len"])
    b = BATCHES[0]
    msgs, sigs, pks, want = _arrays(b["cases"], n)
    assert np.array_equal(_run_dev(gpu_ctx, b, msgs, sigs, pks), want)


def _words(vals):
    return np.array([M.limbs(v) for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("b", BATCHES, ids=IDS)
def test_agreement_with_the_parts(gpu_ctx, b):
    """513 mixed cases: *_verify_msg_dev against the after-the-hash *_verify_dev fed with hashlib's z / e / h and, for
    ECDSA, keys decoded by the model (an undecodable key goes in as (0, 0), which no curve holds)."""
    import torch
    n = 513
    msgs, sigs, pks, want = _arrays(b["cases"], n)
    whole = _run_dev(gpu_ctx, b, msgs, sigs, pks)
    dev = _canon(gpu_ctx, b["curve"])
    raw = [(m, bytes(s), bytes(k)) for m, s, k in zip(msgs, sigs, pks)]
    big = lambda x: int.from_bytes(x, "big")         # noqa: E731
    little = lambda x: int.from_bytes(x, "little")   # noqa: E731
    res = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    if b["scheme"] == "ecdsa":
        xy, _ = _model_points(b, pks)
        a = [_words([R.ecdsa_z(m) for m, _, _ in raw]), _words([big(s[:32]) for _, s, _ in raw]), _words([big(s[32:]) for _, s, _ in raw]), xy]
        t = [_to_dev(x) for x in a]
        dev.ecdsa_verify_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), res.data_ptr(), n)
    elif b["scheme"] == "bip340":
        e = [big(R.tagged("BIP0340/challenge", s[:32] + k + m)) for m, s, k in raw]
        t = [_to_dev(x) for x in (_words([big(k) for _, _, k in raw]), _words([big(s[:32]) for _, s, _ in raw]),
                                  _words([big(s[32:]) for _, s, _ in raw]), _words(e))]
        dev.bip340_verify_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), res.data_ptr(), n)
    else:
        h = [little(hashlib.sha512(s[:32] + k + m).digest()) % R.ED.N for m, s, k in raw]
        t = [_to_dev(x) for x in (_words([little(k) for _, _, k in raw]), _words([little(s[:32]) for _, s, _ in raw]),
                                  _words([little(s[32:]) for _, s, _ in raw]), _words(h))]
        dev.eddsa_verify_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), res.data_ptr(), n)
    torch.cuda.synchronize()
    parts = res.cpu().numpy()
    assert np.array_equal(whole, parts) and np.array_equal(whole, want)


def test_chunks_and_a_multi_device_ctx(gpu_ctx):
    """n = 200 in chunks of 64 with ragged messages: the offsets are rebased per chunk; two shard workers on one GPU"""
    import forge_ec_amd as F
    n = 200
    for b in BATCHES:
        msgs, sigs, pks, want = _arrays(b["cases"], n)
        gpu_ctx.set_chunk(64)
        try:
            got = _host(gpu_ctx, b, msgs, sigs, pks)
            if b["scheme"] == "ecdsa":
                xy, st = _canon(gpu_ctx, b["curve"]).decompress(pks, b["pk_len"])
        finally:
            gpu_ctx.set_chunk(1 << 18)
        assert np.array_equal(got, want) and np.array_equal(got, _host(gpu_ctx, b, msgs, sigs, pks))
        if b["scheme"] == "ecdsa":
            wxy, wst = _model_points(b, pks)
            assert np.array_equal(st, wst) and np.array_equal(xy, wxy)
    with F.Context(devices=[0, 0]) as multi:
        for b in BATCHES:
            msgs, sigs, pks, want = _arrays(b["cases"], n)
            assert np.array_equal(_host(multi, b, msgs, sigs, pks), want)


@pytest.mark.parametrize("b", BATCHES, ids=IDS)
def test_dev_bad_ranges(gpu_ctx, b):
    """off[i] > off[i+1] for one element and off[i+1] > msg_len for another, among valid neighbours: those two get 4,
    the neighbours their own results.  The messages end where their allocation ends."""
    import torch
    msgs, sigs, pks, want = _arrays([c for c in b["cases"] if c["want"] == 1 and len(c["msg"]) >= 110], 8)
    buf, off, total = _layout(msgs)
    assert want.all() and min(len(m) for m in msgs) >= 55
    off = off.copy()
    keep = off.copy()
    off[3], off[4] = keep[4], keep[3]            # element 3 runs backwards (2 and 4 then cover other bytes than they signed)
    off[7] = keep[7]
    off[8] = total + 5                           # element 7 runs past the end
    block = torch.zeros(10 << 20, dtype=torch.uint8, device="cuda")
    at = block.numel() - total
    block[at:] = _to_dev(buf)[:total]
    to, ts, tp = _to_dev(off), _to_dev(sigs), _to_dev(pks)
    res = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    _dev(gpu_ctx, b, block.data_ptr() + at, to.data_ptr(), total, ts.data_ptr(), tp.data_ptr(), res.data_ptr(), 8)
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    assert got[3] == 4 and got[7] == 4
    for i in (0, 1, 5, 6):                        # their ranges are untouched
        assert got[i] == want[i], i
    for i in (2, 4):                              # a longer / shorter message than the one signed (unless that changes nothing)
        lo, hi = int(off[i]), int(off[i + 1])
        m = bytes(buf[lo:hi])
        assert got[i] == R.verify(b["scheme"], b["curve"], m, bytes(sigs[i]), bytes(pks[i])), i


def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib, h = L.lib(), gpu_ctx._h
    p = lambda a: a.ctypes.data   # noqa: E731
    n = 4
    for b in BATCHES:
        msgs, sigs, pks, want = _arrays(b["cases"], n)
        buf, off, total = _layout(msgs)
        res = np.zeros(n, dtype=np.uint8)
        ec = b["scheme"] == "ecdsa"
        name = {"ecdsa": "fec_canon_ecdsa_verify_msg", "bip340": "fec_canon_bip340_verify_msg", "ed25519": "fec_canon_ed25519_verify_msg"}[b["scheme"]]
        fn, fn_dev = getattr(lib, name), getattr(lib, name + "_dev")
        cid = R.CURVE_IDS[b["curve"]]

        def call(ctx=h, curve=cid, m=p(buf), o=p(off), tot=total, s=p(sigs), k=p(pks), kl=b["pk_len"], r=p(res), cnt=n, f=fn, extra=()):
            return f(ctx, *((curve,) if ec else ()), m, o, tot, s, k, *((kl,) if ec else ()), r, cnt, *extra)

        assert call() == 0 and np.array_equal(res, want)
        assert call(cnt=0, o=p(np.zeros(1, dtype=np.uint64)), tot=0) == 0
        for kw in (dict(ctx=None), dict(s=None), dict(k=None), dict(r=None), dict(o=None), dict(m=None), dict(tot=total + 1)):
            assert call(**kw) == ARG, kw
        backwards = off.copy()
        backwards[1], backwards[2] = off[2], off[1]
        if off[1] != off[2]:
            assert call(o=p(backwards)) == ARG
        if ec:
            assert call(curve=2) == UNSUPPORTED and call(curve=7) == ARG
            for kl in (0, 32, 34, 64, 66):
                assert call(kl=kl) == ARG, kl
        tm, to, ts, tp = _to_dev(buf), _to_dev(off), _to_dev(sigs), _to_dev(np.concatenate([pks.reshape(-1), np.zeros(16, dtype=np.uint8)]))
        tr = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        dv = dict(m=tm.data_ptr(), o=to.data_ptr(), s=ts.data_ptr(), k=tp.data_ptr(), r=tr.data_ptr(), f=fn_dev, extra=(None,))
        assert call(**dv) == 0
        torch.cuda.synchronize()
        assert np.array_equal(tr.cpu().numpy(), want)
        assert call(**dict(dv, cnt=0)) == 0
        for kw in (dict(s=None), dict(k=None), dict(r=None), dict(o=None), dict(m=None), dict(ctx=None),
                   dict(s=ts.data_ptr() + 8), dict(k=tp.data_ptr() + 8), dict(o=to.data_ptr() + 4)):
            assert call(**dict(dv, **kw)) == ARG, kw
        if ec:
            assert call(**dict(dv, curve=2)) == UNSUPPORTED and call(**dict(dv, kl=32)) == ARG
        with F.Context(devices=[0, 0]) as multi:
            assert call(**dict(dv, ctx=multi._h)) == UNSUPPORTED
    # decompress
    b = BATCHES[0]
    _, _, pks, _ = _arrays(b["cases"], n)
    xy, st = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    assert lib.fec_canon_decompress(h, 0, p(pks), 33, p(xy), p(st), n) == 0
    assert lib.fec_canon_decompress(h, 0, None, 33, None, None, 0) == 0
    assert lib.fec_canon_decompress(h, 2, p(pks), 33, p(xy), p(st), n) == UNSUPPORTED
    for args in ((None, 0, p(pks), 33, p(xy), p(st), n), (h, 0, None, 33, p(xy), p(st), n), (h, 0, p(pks), 33, None, p(st), n),
                 (h, 0, p(pks), 33, p(xy), None, n), (h, 0, p(pks), 32, p(xy), p(st), n), (h, 0, p(pks), 64, p(xy), p(st), n),
                 (h, 5, p(pks), 33, p(xy), p(st), n)):
        assert lib.fec_canon_decompress(*args) == ARG, args
    tp = _to_dev(np.concatenate([pks.reshape(-1), np.zeros(16, dtype=np.uint8)]))
    txy = torch.zeros((n + 1, 8), dtype=torch.int64, device="cuda")
    tst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert lib.fec_canon_decompress_dev(h, 0, tp.data_ptr(), 33, txy.data_ptr(), tst.data_ptr(), n, None) == 0
    torch.cuda.synchronize()
    assert lib.fec_canon_decompress_dev(h, 0, tp.data_ptr(), 33, txy.data_ptr(), tst.data_ptr(), 0, None) == 0
    assert lib.fec_canon_decompress_dev(h, 2, tp.data_ptr(), 33, txy.data_ptr(), tst.data_ptr(), n, None) == UNSUPPORTED
    assert lib.fec_canon_decompress_dev(h, 0, tp.data_ptr() + 8, 33, txy.data_ptr(), tst.data_ptr(), n, None) == ARG
    assert lib.fec_canon_decompress_dev(h, 0, tp.data_ptr(), 33, txy.data_ptr() + 8, tst.data_ptr(), n, None) == ARG
    assert lib.fec_canon_decompress_dev(h, 0, tp.data_ptr(), 34, txy.data_ptr(), tst.data_ptr(), n, None) == ARG
    assert lib.fec_canon_decompress_dev(h, 0, None, 33, txy.data_ptr(), tst.data_ptr(), n, None) == ARG
    with F.Context(devices=[0, 0]) as multi:
        assert lib.fec_canon_decompress_dev(multi._h, 0, tp.data_ptr(), 33, txy.data_ptr(), tst.data_ptr(), n, None) == UNSUPPORTED
