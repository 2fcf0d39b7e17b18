"""
GPU tests of the canonical-mode signing side (include/fecgpu_canon.h: fec_canon_mul_base_secret, fec_canon_public_key,
fec_canon_ecdsa_sign_digest / _msg, fec_canon_rfc6979_k, fec_canon_bip340_sign_msg, fec_canon_ed25519_sign_msg and their
*_dev forms) against the fixture tests/golden/canon_sign_vectors.json, which the model tests/canon_sign_ref.py wrote and
tests/test_canon_sign_model.py pins by published values.  Signatures are deterministic: every comparison is byte-exact.
Also: the secret comb equals the public one word for word, every signature produced verifies through the GPU verifiers and
stops verifying with one message bit flipped, chunks, shard workers, bad ranges of a *_dev caller, refused arguments.
"""
import json
import os
import random

import numpy as np
import pytest

import canon_msg_ref as R
import canon_sign_ref as S
from oracle import canon_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_sign_vectors.json")))
COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]
ARG, UNSUPPORTED = -1, -5
SCHEMES = [("ecdsa", "secp256k1"), ("ecdsa", "p256"), ("bip340", "secp256k1"), ("ed25519", "ed25519")]
IDS = ["%s-%s" % s for s in SCHEMES]


def _canon(ctx, curve):
    from forge_ec_amd.canon import CANON_CURVES
    return CANON_CURVES[curve](ctx)


def _rows(hexes, width):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), dtype=np.uint8).reshape(len(hexes), width).copy()


def _cases(scheme, curve):
    if scheme == "ecdsa":
        return FIXTURE["ecdsa"][curve]["msg_cases"]
    return FIXTURE[scheme]


def _batch(scheme, curve, n=None, flags=0):
    """n fixture cases, cycling: msgs, the secret arrays, the wanted sigs / status / public keys"""
    cases = _cases(scheme, curve)
    n = len(cases) if n is None else n
    pick = [cases[i % len(cases)] for i in range(n)]
    b = {"msgs": [bytes.fromhex(c["msg"]) for c in pick], "keys": _rows([c["key"] for c in pick], 32),
         "sigs": _rows([c["sig_low" if flags else "sig"] for c in pick], 64), "st": np.array([c["status"] for c in pick], dtype=np.uint8),
         "pks": [bytes.fromhex(c["pk"]) for c in pick]}
    if scheme == "bip340":
        b["aux"] = _rows([c["aux"] for c in pick], 32)
    return b


def _sign_host(ctx, scheme, curve, b, flags=0):
    dev = _canon(ctx, curve)
    if scheme == "ecdsa":
        return dev.ecdsa_sign_msg(b["msgs"], b["keys"], flags)
    if scheme == "bip340":
        return dev.bip340_sign_msg(b["msgs"], b["keys"], b["aux"])
    sigs, pks, st = dev.ed25519_sign_msg(b["msgs"], b["keys"])
    assert [bytes(p) for p in pks] == b["pks"]
    return sigs, st


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _layout(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy(), off, int(off[-1])


def _sign_dev(ctx, scheme, curve, b, flags=0, shift=0, off=None, with_keys=True):
    """the *_dev form; the messages end where their allocation ends, `shift` bytes off the alignment of its start"""
    import torch
    buf, off0, total = _layout(b["msgs"])
    off = off0 if off is None else off
    n = len(b["msgs"])
    block = torch.zeros((4 << 20) - shift, dtype=torch.uint8, device="cuda")
    at = block.numel() - total
    block[at:] = _to_dev(buf)[:total]
    to, tk = _to_dev(off), _to_dev(b["keys"])
    sigs = torch.full((n, 64), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    dev = _canon(ctx, curve)
    pks = None
    if scheme == "ecdsa":
        dev.ecdsa_sign_msg_dev(block.data_ptr() + at, to.data_ptr(), total, tk.data_ptr(), flags, sigs.data_ptr(), st.data_ptr(), n)
    elif scheme == "bip340":
        ta = _to_dev(b["aux"])
        dev.bip340_sign_msg_dev(block.data_ptr() + at, to.data_ptr(), total, tk.data_ptr(), ta.data_ptr(), sigs.data_ptr(), st.data_ptr(), n)
    else:
        pks = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda") if with_keys else None
        dev.ed25519_sign_msg_dev(block.data_ptr() + at, to.data_ptr(), total, tk.data_ptr(), sigs.data_ptr(),
                                 pks.data_ptr() if with_keys else None, st.data_ptr(), n)
    torch.cuda.synchronize()
    if pks is not None:
        assert [bytes(p) for p in pks.cpu().numpy()] == b["pks"]
    return sigs.cpu().numpy(), st.cpu().numpy()


def _verify(ctx, scheme, curve, msgs, sigs, pks):
    dev = _canon(ctx, curve)
    if scheme == "ecdsa":
        return dev.ecdsa_verify_msg(msgs, sigs, pks, 33)
    return dev.bip340_verify_msg(msgs, sigs, pks) if scheme == "bip340" else dev.ed25519_verify_msg(msgs, sigs, pks)


def _flip(m):
    return bytes([m[0] ^ 1]) + m[1:] if m else b"\x01"


# ---- the secret fixed-base multiplication -----------------------------------------------------------
def _scalars(name):
    n = R.ED.N if name == "ed25519" else R.WEIERSTRASS[name].N
    rng = random.Random(31)
    ks = [d << (4 * w) for w in range(64) for d in range(1, 16)]
    ks += [1, 2, n - 1, n - 2, ((1 << 256) - 1) >> 4, 0xF << 128, (1 << 128) - 1, ((1 << 64) - 1) << 190, 0x1111 << 240]
    if name == "ed25519":
        ks += [(1 << 256) - 1, 0, n, n + 1, 0x8 << 252, (1 << 255) - 19]
    ks = [k for k in ks if name == "ed25519" or 1 <= k < n]
    return ks + [rng.randrange(1, n) for _ in range(513)]


@pytest.fixture(scope="module")
def comb4_ctx():
    """a ctx whose public fixed-base call uses the 4-bit LDS comb (FEC_CANON_COMB4=1 at creation)"""
    import forge_ec_amd as F
    old = os.environ.get("FEC_CANON_COMB4")
    os.environ["FEC_CANON_COMB4"] = "1"
    try:
        ctx = F.Context(0)
    finally:
        if old is None:
            del os.environ["FEC_CANON_COMB4"]
        else:
            os.environ["FEC_CANON_COMB4"] = old
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", ["secp256k1", "p256", "ed25519"])
def test_secret_comb_equals_the_public_one(gpu_ctx, comb4_ctx, name):
    """word for word on the single-digit, edge and 513 random scalars, against the default 8-bit comb and the 4-bit one; the
    first of them against the model too; host and *_dev forms"""
    import torch
    ks = _scalars(name)
    k = np.array([M.limbs(v) for v in ks], dtype=np.uint64)
    pub8, st8 = _canon(gpu_ctx, name).mul_base(k)
    pub4, st4 = _canon(comb4_ctx, name).mul_base(k)
    for ctx in (gpu_ctx, comb4_ctx):
        xy, st = _canon(ctx, name).mul_base_secret(k)
        assert np.array_equal(xy, pub8) and np.array_equal(xy, pub4) and np.array_equal(st, st8) and np.array_equal(st, st4)
    tk = _to_dev(k)
    txy = torch.full((len(ks), 8), -1, dtype=torch.int64, device="cuda")
    tst = torch.full((len(ks),), 9, dtype=torch.uint8, device="cuda")
    _canon(gpu_ctx, name).mul_base_secret_dev(tk.data_ptr(), txy.data_ptr(), tst.data_ptr(), len(ks))
    torch.cuda.synchronize()
    assert np.array_equal(txy.cpu().numpy().view(np.uint64), pub8) and not tst.cpu().numpy().any()
    C = R.ED if name == "ed25519" else R.WEIERSTRASS[name]
    for i in (0, 14, 959 if name == "ed25519" else 950, len(ks) - 1):
        want = C.mul(ks[i] % C.N, C.G)
        assert (M.unlimbs(list(xy[i, :4])), M.unlimbs(list(xy[i, 4:]))) == tuple(want)
    gpu_ctx.check()


@pytest.mark.parametrize("name", ["secp256k1", "p256"])
@pytest.mark.parametrize("n", COUNTS)
def test_secret_comb_refuses_out_of_range_scalars(gpu_ctx, name, n):
    C = R.WEIERSTRASS[name]
    bad = [0, C.N, C.N + 1, (1 << 256) - 1]
    ks = [bad[i % 4] if i % 3 == 0 else 1 + i for i in range(n)]
    xy, st = _canon(gpu_ctx, name).mul_base_secret(np.array([M.limbs(v) for v in ks], dtype=np.uint64))
    pub, _ = _canon(gpu_ctx, name).mul_base(np.array([M.limbs(v) for v in ks], dtype=np.uint64))
    for i in range(n):
        if i % 3 == 0:
            assert st[i] == S.BAD_SCALAR and not xy[i].any(), i
        else:
            assert st[i] == 0 and np.array_equal(xy[i], pub[i]), i


# ---- the signers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,curve", SCHEMES, ids=IDS)
def test_every_fixture_case_host_forms(gpu_ctx, scheme, curve):
    for flags in ((0, 1) if scheme == "ecdsa" else (0,)):
        b = _batch(scheme, curve, flags=flags)
        sigs, st = _sign_host(gpu_ctx, scheme, curve, b, flags)
        bad = [i for i in range(len(st)) if st[i] != b["st"][i] or bytes(sigs[i]) != bytes(b["sigs"][i])]
        assert not bad, bad
    assert scheme == "ed25519" or 0 < (b["st"] == S.BAD_KEY).sum() < len(b["st"])
    gpu_ctx.check()


@pytest.mark.parametrize("scheme,curve", SCHEMES, ids=IDS)
def test_every_fixture_case_dev_forms(gpu_ctx, scheme, curve):
    """... at the four start alignments of the message bytes"""
    for shift in range(4):
        flags = shift & 1 if scheme == "ecdsa" else 0
        b = _batch(scheme, curve, flags=flags)
        sigs, st = _sign_dev(gpu_ctx, scheme, curve, b, flags, shift)
        bad = [i for i in range(len(st)) if st[i] != b["st"][i] or bytes(sigs[i]) != bytes(b["sigs"][i])]
        assert not bad, (shift, bad)
    gpu_ctx.check()


@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_ecdsa_digests_and_nonces(gpu_ctx, curve):
    """planted digests at and above the order, refused keys; fec_canon_rfc6979_k; host and *_dev forms"""
    import torch
    dc = FIXTURE["ecdsa"][curve]["digest_cases"]
    dg, keys = _rows([c["digest"] for c in dc], 32), _rows([c["key"] for c in dc], 32)
    want_st = np.array([c["status"] for c in dc], dtype=np.uint8)
    dev = _canon(gpu_ctx, curve)
    n = len(dc)
    for flags, field in ((0, "sig"), (1, "sig_low")):
        sigs, st = dev.ecdsa_sign_digest(dg, keys, flags)
        assert np.array_equal(st, want_st) and np.array_equal(sigs, _rows([c[field] for c in dc], 64))
        td, tk = _to_dev(dg), _to_dev(keys)
        ts = torch.full((n, 64), 0xEE, dtype=torch.uint8, device="cuda")
        tst = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        dev.ecdsa_sign_digest_dev(td.data_ptr(), tk.data_ptr(), flags, ts.data_ptr(), tst.data_ptr(), n)
        torch.cuda.synchronize()
        assert np.array_equal(tst.cpu().numpy(), want_st) and np.array_equal(ts.cpu().numpy(), sigs)
    ks, st = dev.rfc6979_k(dg, keys)
    assert np.array_equal(st, want_st) and np.array_equal(ks, _rows([c["k"] for c in dc], 32))
    tk_out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    dev.rfc6979_k_dev(td.data_ptr(), tk.data_ptr(), tk_out.data_ptr(), tst.data_ptr(), n)
    torch.cuda.synchronize()
    assert np.array_equal(tk_out.cpu().numpy(), ks) and np.array_equal(tst.cpu().numpy(), want_st)
    assert 0 < (want_st == S.BAD_KEY).sum() and any(int(c["digest"], 16) >= R.WEIERSTRASS[curve].N for c in dc)


def test_published_vectors(gpu_ctx):
    """RFC 6979 A.2.5 "sample" and "test": nonce and signature; BIP-340 vector 0; RFC 8032 tests 1 and 2 with their keys"""
    import hashlib
    pub = FIXTURE["published"]
    assert sorted(pub) == ["bip340_vector0", "rfc6979_a25_sample", "rfc6979_a25_test", "rfc8032_test1", "rfc8032_test2"]
    p256, secp, ed = _canon(gpu_ctx, "p256"), _canon(gpu_ctx, "secp256k1"), _canon(gpu_ctx, "ed25519")
    for name in ("rfc6979_a25_sample", "rfc6979_a25_test"):
        v = pub[name]
        msg, key = bytes.fromhex(v["msg"]), bytes.fromhex(v["key"])
        sigs, st = p256.ecdsa_sign_msg([msg], key)
        assert bytes(sigs[0]).hex() == v["sig"].lower() and st[0] == 0, name
        ks, st = p256.rfc6979_k(hashlib.sha256(msg).digest(), key)
        assert bytes(ks[0]).hex() == v["k"].lower() and st[0] == 0, name
        pk, st = p256.public_key(key, 33)
        assert bytes(pk[0]).hex() == v["pk"].lower() and st[0] == 0
    v = pub["bip340_vector0"]
    sigs, st = secp.bip340_sign_msg([bytes.fromhex(v["msg"])], bytes.fromhex(v["key"]), bytes.fromhex(v["aux"]))
    assert bytes(sigs[0]).hex() == v["sig"].lower() and st[0] == 0
    from forge_ec_amd import _lib as L
    pk, st = secp.public_key(bytes.fromhex(v["key"]), 32, scheme=L.CANON_SCHEME_BIP340)
    assert bytes(pk[0]).hex() == v["pk"].lower() and st[0] == 0
    for name in ("rfc8032_test1", "rfc8032_test2"):
        v = pub[name]
        sigs, pks, st = ed.ed25519_sign_msg([bytes.fromhex(v["msg"])], bytes.fromhex(v["key"]))
        assert bytes(sigs[0]).hex() == v["sig"] and bytes(pks[0]).hex() == v["pk"] and st[0] == 0, name
        pk, st = ed.public_key(bytes.fromhex(v["key"]))
        assert bytes(pk[0]).hex() == v["pk"] and st[0] == 0


@pytest.mark.parametrize("n", COUNTS)
def test_element_counts_sign_then_verify(gpu_ctx, n):
    """n signatures per scheme, byte-exact against the fixture; every one of them and its public key is accepted by the GPU
    verifier from the message, and rejected with one bit of the message flipped.  The cycle starts inside the refused keys so
    that n = 1 is not always a good one."""
    from forge_ec_amd import _lib as L
    for scheme, curve in SCHEMES:
        cases = _cases(scheme, curve)
        start = next((i for i, c in enumerate(cases) if c["status"]), 0)
        b = _batch(scheme, curve, n + start)
        b = {k: v[start:] for k, v in b.items()}
        sigs, st = _sign_host(gpu_ctx, scheme, curve, dict(b, pks=b["pks"]), 0)
        assert np.array_equal(st, b["st"]) and np.array_equal(sigs, b["sigs"]), (scheme, curve)
        dev = _canon(gpu_ctx, curve)
        pks, pst = dev.public_key(b["keys"], scheme=L.CANON_SCHEME_BIP340 if scheme == "bip340" else None)
        assert np.array_equal(pst, b["st"]) and [bytes(p) for p in pks] == b["pks"], (scheme, curve)
        good = np.nonzero(st == 0)[0]
        if len(good) == 0:
            continue
        msgs = [b["msgs"][i] for i in good]
        assert _verify(gpu_ctx, scheme, curve, msgs, sigs[good], pks[good]).all(), (scheme, curve)
        assert not _verify(gpu_ctx, scheme, curve, [_flip(m) for m in msgs], sigs[good], pks[good]).any(), (scheme, curve)
    sd, std = _sign_dev(gpu_ctx, "ecdsa", "secp256k1", _batch("ecdsa", "secp256k1", n))
    want = _batch("ecdsa", "secp256k1", n)
    assert np.array_equal(sd, want["sigs"]) and np.array_equal(std, want["st"])
    gpu_ctx.check()


def test_uncompressed_keys_and_no_key_output(gpu_ctx):
    for curve in ("secp256k1", "p256"):
        b = _batch("ecdsa", curve, 40)
        pks, st = _canon(gpu_ctx, curve).public_key(b["keys"], 65)
        for i in range(40):
            want, wst = S.public_key(R.CURVE_IDS[curve], bytes(b["keys"][i]), 65)
            assert bytes(pks[i]) == want and st[i] == wst, i
    b = _batch("ed25519", "ed25519", 20)
    sigs, pks, st = _canon(gpu_ctx, "ed25519").ed25519_sign_msg(b["msgs"], b["keys"], with_keys=False)
    assert pks is None and np.array_equal(sigs, b["sigs"]) and not st.any()
    sigs, st = _sign_dev(gpu_ctx, "ed25519", "ed25519", b, with_keys=False)
    assert np.array_equal(sigs, b["sigs"]) and not st.any()


def test_public_key_dev_forms(gpu_ctx):
    import torch
    from forge_ec_amd import _lib as L
    n = 65
    for scheme, curve, sid, out_len in (("ecdsa", "secp256k1", 0, 33), ("ecdsa", "p256", 1, 65), ("bip340", "secp256k1", L.CANON_SCHEME_BIP340, 32),
                                        ("ed25519", "ed25519", 2, 32)):
        b = _batch(scheme, curve, n)
        want = [S.public_key(sid, bytes(k), out_len) for k in b["keys"]]
        tk = _to_dev(b["keys"])
        out = torch.full((n, out_len), 0xEE, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        _canon(gpu_ctx, curve).public_key_dev(tk.data_ptr(), out.data_ptr(), out_len, st.data_ptr(), n, scheme=sid)
        torch.cuda.synchronize()
        assert [bytes(p) for p in out.cpu().numpy()] == [w[0] for w in want] and list(st.cpu().numpy()) == [w[1] for w in want]


def test_chunks_and_a_multi_device_ctx(gpu_ctx):
    """n = 200 in chunks of 64 with ragged messages: the offsets are rebased per chunk; two shard workers on one GPU"""
    import forge_ec_amd as F
    n = 200
    for scheme, curve in SCHEMES:
        b = _batch(scheme, curve, n)
        gpu_ctx.set_chunk(64)
        try:
            sigs, st = _sign_host(gpu_ctx, scheme, curve, b)
            if scheme == "ecdsa":
                dc = FIXTURE["ecdsa"][curve]["digest_cases"]
                pick = [dc[i % len(dc)] for i in range(n)]
                ds, dst = _canon(gpu_ctx, curve).ecdsa_sign_digest(_rows([c["digest"] for c in pick], 32), _rows([c["key"] for c in pick], 32))
                assert np.array_equal(ds, _rows([c["sig"] for c in pick], 64)) and list(dst) == [c["status"] for c in pick]
        finally:
            gpu_ctx.set_chunk(1 << 18)
        assert np.array_equal(sigs, b["sigs"]) and np.array_equal(st, b["st"]), (scheme, curve)
    with F.Context(devices=[0, 0]) as multi:
        for scheme, curve in SCHEMES:
            b = _batch(scheme, curve, n)
            sigs, st = _sign_host(multi, scheme, curve, b)
            assert np.array_equal(sigs, b["sigs"]) and np.array_equal(st, b["st"]), (scheme, curve)
        k = np.array([M.limbs(v + 1) for v in range(n)], dtype=np.uint64)
        xy, st = _canon(multi, "p256").mul_base_secret(k)
        assert np.array_equal(xy, _canon(gpu_ctx, "p256").mul_base(k)[0]) and not st.any()


@pytest.mark.parametrize("scheme,curve", SCHEMES, ids=IDS)
def test_dev_bad_ranges(gpu_ctx, scheme, curve):
    """off[i] > off[i+1] for one element and off[i+1] > msg_len for another, among valid neighbours: those two get status 4
    and a zero signature, the neighbours whose range is untouched their own signature.  The messages end where their
    allocation ends."""
    cases = [c for c in _cases(scheme, curve) if c["status"] == 0 and len(c["msg"]) >= 110]
    pick = {"msgs": [], "keys": [], "sigs": [], "aux": [], "pks": []}
    for c in cases[:8]:
        pick["msgs"].append(bytes.fromhex(c["msg"]))
    assert len(pick["msgs"]) == 8
    b = {"msgs": pick["msgs"], "keys": _rows([c["key"] for c in cases[:8]], 32), "sigs": _rows([c["sig"] for c in cases[:8]], 64),
         "pks": [bytes.fromhex(c["pk"]) for c in cases[:8]]}
    if scheme == "bip340":
        b["aux"] = _rows([c["aux"] for c in cases[:8]], 32)
    _, keep, total = _layout(b["msgs"])
    off = keep.copy()
    off[3], off[4] = keep[4], keep[3]            # element 3 runs backwards (2 and 4 then cover other bytes than the fixture's)
    off[8] = total + 5                           # element 7 runs past the end
    sigs, st = _sign_dev(gpu_ctx, scheme, curve, b, off=off, with_keys=False)
    assert st[3] == 4 and st[7] == 4 and not sigs[3].any() and not sigs[7].any()
    for i in (0, 1, 5, 6):
        assert st[i] == 0 and np.array_equal(sigs[i], b["sigs"][i]), i
    for i in (2, 4):                              # a longer / shorter message: what the model signs for those bytes
        m = b"".join(b["msgs"])[int(off[i]):int(off[i + 1])]
        key = bytes(b["keys"][i])
        if scheme == "ecdsa":
            want = S.ecdsa_sign_msg(R.WEIERSTRASS[curve], int.from_bytes(key, "big"), m)[0]
        elif scheme == "bip340":
            want = S.bip340_sign(int.from_bytes(key, "big"), m, bytes(b["aux"][i]))[0]
        else:
            want = S.ed25519_sign(key, m)[0]
        assert st[i] == 0 and bytes(sigs[i]) == want, i


def test_argument_errors(gpu_ctx):
    import torch
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib, h = L.lib(), gpu_ctx._h
    p = lambda a: a.ctypes.data   # noqa: E731
    n = 4
    b = _batch("ecdsa", "secp256k1", n)
    buf, off, total = _layout(b["msgs"])
    sigs, st = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8)
    keys, aux = b["keys"], _batch("bip340", "secp256k1", n)["aux"]
    xy, k = np.zeros((n, 8), np.uint64), np.ones((n, 4), np.uint64)
    assert lib.fec_canon_ecdsa_sign_msg(h, 0, p(buf), p(off), total, p(keys), 0, p(sigs), p(st), n) == 0
    assert lib.fec_canon_ecdsa_sign_msg(h, 0, None, p(np.zeros(1, np.uint64)), 0, None, 0, None, None, 0) == 0
    assert lib.fec_canon_ecdsa_sign_msg(h, 2, p(buf), p(off), total, p(keys), 0, p(sigs), p(st), n) == UNSUPPORTED
    assert lib.fec_canon_ecdsa_sign_digest(h, 2, p(keys), p(keys), 0, p(sigs), p(st), n) == UNSUPPORTED
    assert lib.fec_canon_rfc6979_k(h, 2, p(keys), p(keys), p(sigs), p(st), n) == UNSUPPORTED
    for args in ((None, 0, p(buf), p(off), total, p(keys), 0, p(sigs), p(st), n), (h, 7, p(buf), p(off), total, p(keys), 0, p(sigs), p(st), n),
                 (h, 0, p(buf), p(off), total, None, 0, p(sigs), p(st), n), (h, 0, p(buf), p(off), total, p(keys), 2, p(sigs), p(st), n),
                 (h, 0, p(buf), p(off), total, p(keys), 0, None, p(st), n), (h, 0, p(buf), p(off), total, p(keys), 0, p(sigs), None, n),
                 (h, 0, p(buf), p(off), total + 1, p(keys), 0, p(sigs), p(st), n), (h, 0, p(buf), None, total, p(keys), 0, p(sigs), p(st), n)):
        assert lib.fec_canon_ecdsa_sign_msg(*args) == ARG, args
    assert lib.fec_canon_bip340_sign_msg(h, p(buf), p(off), total, p(keys), None, p(sigs), p(st), n) == ARG
    assert lib.fec_canon_ed25519_sign_msg(h, p(buf), p(off), total, None, p(sigs), None, p(st), n) == ARG
    assert lib.fec_canon_ecdsa_sign_digest(h, 0, None, p(keys), 0, p(sigs), p(st), n) == ARG
    assert lib.fec_canon_ecdsa_sign_digest(h, 0, p(keys), p(keys), 4, p(sigs), p(st), n) == ARG
    assert lib.fec_canon_mul_base_secret(h, 5, p(k), p(xy), p(st), n) == ARG
    assert lib.fec_canon_mul_base_secret(h, 0, None, p(xy), p(st), n) == ARG
    assert lib.fec_canon_mul_base_secret(h, 0, None, None, None, 0) == 0
    for scheme, ln in ((0, 32), (0, 64), (1, 34), (2, 33), (3, 33), (3, 65), (4, 32), (-1, 32)):
        assert lib.fec_canon_public_key(h, scheme, p(keys), p(sigs), ln, p(st), n) == ARG, (scheme, ln)
    # the *_dev forms: misalignment, nulls, a multi-device ctx
    tm, to, tk, ta = _to_dev(buf), _to_dev(off), _to_dev(np.concatenate([keys.reshape(-1), np.zeros(16, np.uint8)])), _to_dev(aux)
    ts = torch.zeros(n * 64 + 16, dtype=torch.uint8, device="cuda")
    tst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    txy = torch.zeros((n + 1, 8), dtype=torch.int64, device="cuda")
    tkl = _to_dev(k)
    M_, O, K, A, SG, ST = tm.data_ptr(), to.data_ptr(), tk.data_ptr(), ta.data_ptr(), ts.data_ptr(), tst.data_ptr()
    assert lib.fec_canon_ecdsa_sign_msg_dev(h, 0, M_, O, total, K, 0, SG, ST, n, None) == 0
    assert lib.fec_canon_bip340_sign_msg_dev(h, M_, O, total, K, A, SG, ST, n, None) == 0
    assert lib.fec_canon_ed25519_sign_msg_dev(h, M_, O, total, K, SG, None, ST, n, None) == 0
    assert lib.fec_canon_mul_base_secret_dev(h, 0, tkl.data_ptr(), txy.data_ptr(), ST, n, None) == 0
    torch.cuda.synchronize()
    assert lib.fec_canon_ecdsa_sign_msg_dev(h, 0, M_, O, total, K, 0, SG, ST, 0, None) == 0
    assert lib.fec_canon_ecdsa_sign_msg_dev(h, 2, M_, O, total, K, 0, SG, ST, n, None) == UNSUPPORTED
    for args in ((h, 0, M_, O, total, K + 8, 0, SG, ST, n, None), (h, 0, M_, O, total, K, 0, SG + 8, ST, n, None),
                 (h, 0, M_, O + 4, total, K, 0, SG, ST, n, None), (h, 0, None, O, total, K, 0, SG, ST, n, None),
                 (h, 0, M_, None, total, K, 0, SG, ST, n, None), (h, 0, M_, O, total, None, 0, SG, ST, n, None),
                 (h, 0, M_, O, total, K, 8, SG, ST, n, None), (None, 0, M_, O, total, K, 0, SG, ST, n, None)):
        assert lib.fec_canon_ecdsa_sign_msg_dev(*args) == ARG, args
    assert lib.fec_canon_ecdsa_sign_digest_dev(h, 0, K + 8, K, 0, SG, ST, n, None) == ARG
    assert lib.fec_canon_rfc6979_k_dev(h, 0, K, K, SG + 8, ST, n, None) == ARG
    assert lib.fec_canon_bip340_sign_msg_dev(h, M_, O, total, K, A + 8, SG, ST, n, None) == ARG
    assert lib.fec_canon_ed25519_sign_msg_dev(h, M_, O, total, K, SG, SG + 8, ST, n, None) == ARG
    assert lib.fec_canon_mul_base_secret_dev(h, 0, tkl.data_ptr() + 8, txy.data_ptr(), ST, n, None) == ARG
    assert lib.fec_canon_mul_base_secret_dev(h, 0, tkl.data_ptr(), txy.data_ptr() + 8, ST, n, None) == ARG
    assert lib.fec_canon_public_key_dev(h, 3, K, SG + 8, 32, ST, n, None) == ARG
    assert lib.fec_canon_public_key_dev(h, 0, K + 8, SG, 33, ST, n, None) == ARG
    assert lib.fec_canon_public_key_dev(h, 0, K, SG + 1, 33, ST, n, None) == 0      # a 33-byte record has no alignment
    torch.cuda.synchronize()
    with F.Context(devices=[0, 0]) as multi:
        mh = multi._h
        assert lib.fec_canon_ecdsa_sign_msg_dev(mh, 0, M_, O, total, K, 0, SG, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_ecdsa_sign_digest_dev(mh, 0, K, K, 0, SG, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_rfc6979_k_dev(mh, 0, K, K, SG, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_bip340_sign_msg_dev(mh, M_, O, total, K, A, SG, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_ed25519_sign_msg_dev(mh, M_, O, total, K, SG, None, ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_mul_base_secret_dev(mh, 0, tkl.data_ptr(), txy.data_ptr(), ST, n, None) == UNSUPPORTED
        assert lib.fec_canon_public_key_dev(mh, 0, K, SG, 33, ST, n, None) == UNSUPPORTED
