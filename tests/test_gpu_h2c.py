"""
GPU tests of fec_expand_message_xmd, fec_hash_to_field, fec_map_to_curve, fec_hash_to_curve, fec_curve_hash_to_curve and
their _dev forms (kernels_h2c.hip, h2c.hpp) against the restatement of tests/h2c_ref.py.

Messages of mixed lengths inside one batch (h2c_ref.messages: an empty one, lengths that put the padding of b_0's input at
55, 56, 63 and 64 bytes modulo 64, the rest 1..150 bytes), so lanes of one wavefront run different numbers of SHA-256
blocks; dst_len in {1, 21, 22, 255}; n in {1, 63, 64, 65, 257}, host and _dev forms, unaligned `msgs` bases.

One map costs about 20 ms in the Python model, so the restatement of the maps is computed once per curve for the first
N_REF = 65 messages of the dst_len-21 batch and shared; what is compared for every element of every batch is
  * the expander and hash_to_field against the restatement (hashlib: cheap, exact), and
  * the fused calls against the composition of the small calls on the GPU -- HASH = point_op(ADD) of the two
    map_to_curve results on hash_to_field(count = 2), ENCODE = the map of hash_to_field(count = 1) with z = one, the trait
    method = to_affine of the same composition on its own field elements --
and the fixture (every dst_len, all three forms, planted limbs) goes through the host calls byte for byte.
tests/test_h2c_model.py asserts on the reference alone that sqrt is None for every fixture element, that secp256k1's HASH
is one constant and that P-256's results differ: `cand` and `legs` are what tells this implementation from a constant.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import h2c_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "h2c_vectors.json")))
GUARD = 64
DST_LENS = (1, 21, 22, 255)
NS = (1, 63, 64, 65, 257)
N_REF = 65
E_ARG, E_UNSUPPORTED = -1, -5
_MSGS, _REF = {}, {}


def _msgs(dst_len):
    if dst_len not in _MSGS:
        _MSGS[dst_len] = R.messages(257, 900 + dst_len, dst_len)
    return _MSGS[dst_len]


def _ref_hash(curve):
    """The restatement of HASH for the first N_REF messages under dst_len 21: (points, cand, legs), computed once."""
    if curve not in _REF:
        rows = [R.hash_to_curve(curve, m, R.dst_of(21)) for m in _msgs(21)[:N_REF]]
        _REF[curve] = (np.array([R.flat_proj(r[0]) for r in rows], dtype=np.uint64),
                       np.array([[list(c[0]) + list(c[1]) for c in r[1]] for r in rows], dtype=np.uint64),
                       np.array([r[2] for r in rows], dtype=np.uint8))
    return _REF[curve]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def _dev_msgs(torch, msgs, shift=0):
    """-> (keep-alive tensors, msgs address, offsets address, msg_len); the bytes start `shift` bytes into their buffer."""
    buf = b"".join(msgs)
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    tb = _dev(torch, np.frombuffer(bytes(shift) + (buf or b"\0") + bytes(16), dtype=np.uint8))
    to = _dev(torch, off)
    return (tb, to), tb.data_ptr() + shift, to.data_ptr(), len(buf)


def _field_ref(curve, msgs, dst, count):
    return np.array([[v for f in R.hash_to_field(curve, m, dst, count)[0] for v in f] for m in msgs], dtype=np.uint64).reshape(len(msgs), count, 4)


def _proj(xy):
    """from_affine of map results: z = one."""
    one = np.zeros((xy.shape[0], 4), dtype=np.uint64)
    one[:, 0] = 1
    return np.concatenate([xy, one], axis=1)


# ---- the fixture, byte for byte through the host calls ----
def test_fixture_expander(gpu_ctx):
    for msg, want in FIXTURE["k1"]:
        assert bytes(gpu_ctx.expand_message_xmd([bytes.fromhex(msg)], R.K1_DST, 32)[0]).hex() == want
    pool = bytes.fromhex(FIXTURE["pool"])
    for m, d, o, want in FIXTURE["xmd"]:
        got = gpu_ctx.expand_message_xmd([pool[:m]], R.dst_of(d) if d else None, o)
        assert got.shape == (1, o) and bytes(got[0]).hex() == want, (m, d, o)


def test_fixture_field_and_planted_maps(gpu_ctx):
    for curve, d, count, msgs, u in FIXTURE["field"]:
        got = gpu_ctx.hash_to_field(curve, [bytes.fromhex(m) for m in msgs], R.dst_of(d), count)
        assert got.reshape(len(msgs), -1).tolist() == u, (curve, d, count)
    for curve in (R.SECP, R.P256):
        cases = [c for c in FIXTURE["map"] if c[0] == curve]
        xy, cand, legs = gpu_ctx.map_to_curve(curve, [c[2] for c in cases])
        for i, c in enumerate(cases):
            assert (xy[i].tolist(), cand[i].tolist(), int(legs[i])) == (c[3], c[4], c[5]), c[1]
        # NULL is accepted for each optional output
        xy2, none_c, legs2 = gpu_ctx.map_to_curve(curve, [c[2] for c in cases], with_cand=False)
        xy3, cand3, none_l = gpu_ctx.map_to_curve(curve, [c[2] for c in cases], with_legs=False)
        assert none_c is None and none_l is None
        assert np.array_equal(xy2, xy) and np.array_equal(xy3, xy) and np.array_equal(legs2, legs) and np.array_equal(cand3, cand)


def test_fixture_curve_forms(gpu_ctx):
    for case in FIXTURE["curve"]:
        curve, d = case["curve"], case["dst_len"]
        msgs, dst = [bytes.fromhex(m) for m in case["msgs"]], (R.dst_of(case["dst_len"]) if case["dst_len"] else None)
        xy, inf = gpu_ctx.curve_hash_to_curve(curve, msgs, dst)
        assert [[xy[i].tolist(), int(inf[i])] for i in range(len(msgs))] == case["trait"], (curve, d)
        if d:
            for name, fn in (("hash", gpu_ctx.hash_to_curve), ("encode", gpu_ctx.encode_to_curve)):
                out, cand, legs = fn(curve, msgs, dst)
                got = [[out[i].tolist(), cand[i].tolist(), legs[i].tolist()] for i in range(len(msgs))]
                assert got == case[name], (curve, d, name)


# ---- the expander ----
@pytest.mark.parametrize("dst_len", DST_LENS)
def test_expander_host_and_dev(gpu_ctx, dst_len):
    import torch
    msgs, dst = _msgs(dst_len), R.dst_of(dst_len)
    n = len(msgs)
    keep, pm, po, total = _dev_msgs(torch, msgs, shift=dst_len % 4)
    for out_len in (0, 1, 32, 33, 96):
        want = np.array([list(R.expand_message_xmd(m, dst, out_len)) for m in msgs], dtype=np.uint8).reshape(n, out_len)
        assert np.array_equal(gpu_ctx.expand_message_xmd(msgs, dst, out_len), want), out_len
        d_out = torch.full((n * out_len + GUARD,), 0xA5, dtype=torch.uint8, device=keep[0].device)
        d_st = torch.full((n,), 9, dtype=torch.uint8, device=keep[0].device)
        torch.cuda.synchronize()   # the fills run on torch's stream, the call on the ctx's own (non-blocking): a late fill put the 9 back
        gpu_ctx.expand_message_xmd_dev(pm, po, total, dst, out_len, d_out.data_ptr() if out_len else None, d_st.data_ptr(), n)
        torch.cuda.synchronize()
        gpu_ctx.check()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:n * out_len].reshape(n, out_len), want), out_len
        assert (got[n * out_len:] == 0xA5).all() and not d_st.cpu().numpy().any(), out_len


def test_expander_longest_output(gpu_ctx):
    msgs, dst = _msgs(22)[:65], R.dst_of(22)
    want = np.array([list(R.expand_message_xmd(m, dst, R.MAX_OUT)) for m in msgs], dtype=np.uint8)
    buf = np.full(65 * R.MAX_OUT + GUARD, 0xA5, dtype=np.uint8)
    mb, off, total = gpu_ctx._messages(msgs)
    rc = gpu_ctx._lib.fec_expand_message_xmd(gpu_ctx._h, mb.ctypes.data, off.ctypes.data, total, ctypes.c_char_p(dst), 22, R.MAX_OUT,
                                             buf.ctypes.data, 65)
    assert rc == 0 and np.array_equal(buf[:65 * R.MAX_OUT].reshape(65, R.MAX_OUT), want) and (buf[65 * R.MAX_OUT:] == 0xA5).all()


# ---- hash_to_field ----
@pytest.mark.parametrize("curve", [0, 1])
def test_hash_to_field_host_and_dev(gpu_ctx, curve):
    import torch
    for dst_len, count in ((1, 1), (21, 2), (22, 2), (255, 3)):
        msgs, dst = _msgs(dst_len), R.dst_of(dst_len)
        want = _field_ref(curve, msgs, dst, count)
        for n in NS:
            assert np.array_equal(gpu_ctx.hash_to_field(curve, msgs[:n], dst, count), want[:n]), (dst_len, n)
        n = len(msgs)
        keep, pm, po, total = _dev_msgs(torch, msgs, shift=3)
        d_u = torch.full((n * count * 32 + GUARD,), 0xA5, dtype=torch.uint8, device=keep[0].device)
        torch.cuda.synchronize()   # (the fill, on torch's stream, ahead of the call on the ctx's own)
        gpu_ctx.hash_to_field_dev(curve, pm, po, total, dst, count, d_u.data_ptr(), None, n)
        torch.cuda.synchronize()
        got = d_u.cpu().numpy()
        assert np.array_equal(got[:n * count * 32].view(np.uint64).reshape(n, count, 4), want) and (got[n * count * 32:] == 0xA5).all()
    # count = 1 and count = 2 do not share u[0]
    a = gpu_ctx.hash_to_field(curve, _msgs(21)[:8], R.dst_of(21), 1)
    b = gpu_ctx.hash_to_field(curve, _msgs(21)[:8], R.dst_of(21), 2)
    assert not (a[:, 0] == b[:, 0]).all(axis=1).any()


# ---- the fused call against the restatement ----
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("curve", [0, 1])
def test_hash_host_form(gpu_ctx, curve, n):
    msgs, dst = _msgs(21)[:n], R.dst_of(21)
    wp, wc, wl = _ref_hash(curve)
    out, cand, legs = gpu_ctx.hash_to_curve(curve, msgs, dst)
    m = min(n, N_REF)
    assert np.array_equal(out[:m], wp[:m]) and np.array_equal(cand[:m], wc[:m]) and np.array_equal(legs[:m], wl[:m])
    # NULL for cand, for legs, for both
    for wc_, wl_ in ((False, True), (True, False), (False, False)):
        o2, c2, l2 = gpu_ctx.hash_to_curve(curve, msgs, dst, with_cand=wc_, with_legs=wl_)
        assert np.array_equal(o2, out) and (c2 is None or np.array_equal(c2, cand)) and (l2 is None or np.array_equal(l2, legs))
    # every element: the composition of the small calls
    u = gpu_ctx.hash_to_field(curve, msgs, dst, 2)
    xy0, c0, l0 = gpu_ctx.map_to_curve(curve, u[:, 0])
    xy1, c1, l1 = gpu_ctx.map_to_curve(curve, u[:, 1])
    assert np.array_equal(out, gpu_ctx.point_op(curve, 0, _proj(xy0), _proj(xy1)))
    assert np.array_equal(cand[:, 0], c0) and np.array_equal(cand[:, 1], c1)
    assert np.array_equal(legs[:, 0], l0) and np.array_equal(legs[:, 1], l1)
    assert (legs & R.LEG_SQRT_NONE).all()          # what tests/test_h2c_model.py asserts of the reference
    if curve == R.P256:
        assert len({tuple(r) for r in out.tolist()}) == n
    assert len({tuple(r) for r in cand[:, 0].tolist()}) == n      # the computation is not a constant


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("curve", [0, 1])
def test_hash_dev_form(gpu_ctx, curve, n):
    import torch
    msgs, dst = _msgs(21)[:n], R.dst_of(21)
    want = gpu_ctx.hash_to_curve(curve, msgs, dst)
    wp, wc, wl = _ref_hash(curve)
    m = min(n, N_REF)
    assert np.array_equal(want[0][:m], wp[:m])
    keep, pm, po, total = _dev_msgs(torch, msgs, shift=1)
    dev = keep[0].device
    for with_cand, with_legs in ((True, True), (False, False)):
        d_out = torch.full((n * 96 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        d_cand = torch.full((n * 128 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        d_legs = torch.full((n * 2 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()   # (the fills, on torch's stream, ahead of the call on the ctx's own)
        gpu_ctx.hash_to_curve_dev(curve, pm, po, total, dst, d_out.data_ptr(), d_cand.data_ptr() if with_cand else None,
                                  d_legs.data_ptr() if with_legs else None, d_st.data_ptr(), n)
        torch.cuda.synchronize()
        gpu_ctx.check()
        o, c, l = d_out.cpu().numpy(), d_cand.cpu().numpy(), d_legs.cpu().numpy()
        assert np.array_equal(o[:n * 96].view(np.uint64).reshape(n, 12), want[0]) and (o[n * 96:] == 0xA5).all()
        assert not d_st.cpu().numpy().any()
        if with_cand:
            assert np.array_equal(c[:n * 128].view(np.uint64).reshape(n, 2, 8), want[1]) and (c[n * 128:] == 0xA5).all()
            assert np.array_equal(l[:n * 2].reshape(n, 2), want[2]) and (l[n * 2:] == 0xA5).all()
        else:
            assert (c == 0xA5).all() and (l == 0xA5).all()


@pytest.mark.parametrize("dst_len", DST_LENS)
@pytest.mark.parametrize("curve", [0, 1])
def test_hash_equals_add_of_maps_for_every_dst_len(gpu_ctx, curve, dst_len):
    msgs, dst = _msgs(dst_len), R.dst_of(dst_len)
    out, cand, legs = gpu_ctx.hash_to_curve(curve, msgs, dst)
    u = gpu_ctx.hash_to_field(curve, msgs, dst, 2)
    assert np.array_equal(u, _field_ref(curve, msgs, dst, 2))
    xy0, c0, l0 = gpu_ctx.map_to_curve(curve, u[:, 0])
    xy1, c1, l1 = gpu_ctx.map_to_curve(curve, u[:, 1])
    assert np.array_equal(out, gpu_ctx.point_op(curve, 0, _proj(xy0), _proj(xy1)))
    assert np.array_equal(cand, np.stack([c0, c1], axis=1)) and np.array_equal(legs, np.stack([l0, l1], axis=1))


@pytest.mark.parametrize("curve", [0, 1])
def test_encode_is_the_map_of_count_one(gpu_ctx, curve):
    import torch
    msgs, dst = _msgs(22), R.dst_of(22)
    n = len(msgs)
    out, cand, legs = gpu_ctx.encode_to_curve(curve, msgs, dst)
    u1 = gpu_ctx.hash_to_field(curve, msgs, dst, 1)
    xy, c, l = gpu_ctx.map_to_curve(curve, u1[:, 0])
    assert np.array_equal(out, _proj(xy)) and np.array_equal(cand[:, 0], c) and np.array_equal(legs[:, 0], l)
    # ... and not the map of count = 2's u[0]
    u2 = gpu_ctx.hash_to_field(curve, msgs, dst, 2)
    assert not np.array_equal(cand[:, 0], gpu_ctx.map_to_curve(curve, u2[:, 0])[1])
    # against the restatement
    for i in range(0, 17):
        p, rc, rl = R.hash_to_curve(curve, msgs[i], dst, encode=True)
        assert out[i].tolist() == R.flat_proj(p) and cand[i, 0].tolist() == list(rc[0][0]) + list(rc[0][1]) and legs[i].tolist() == rl
    for k in NS:
        assert np.array_equal(gpu_ctx.encode_to_curve(curve, msgs[:k], dst)[0], out[:k])
    keep, pm, po, total = _dev_msgs(torch, msgs, shift=2)
    d_out = torch.full((n * 96 + GUARD,), 0xA5, dtype=torch.uint8, device=keep[0].device)
    d_cand = torch.zeros(n * 64, dtype=torch.uint8, device=keep[0].device)
    d_legs = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=keep[0].device)
    torch.cuda.synchronize()   # (the fills, on torch's stream, ahead of the call on the ctx's own)
    gpu_ctx.encode_to_curve_dev(curve, pm, po, total, dst, d_out.data_ptr(), d_cand.data_ptr(), d_legs.data_ptr(), None, n)
    torch.cuda.synchronize()
    o, lg = d_out.cpu().numpy(), d_legs.cpu().numpy()
    assert np.array_equal(o[:n * 96].view(np.uint64).reshape(n, 12), out) and (o[n * 96:] == 0xA5).all()
    assert np.array_equal(d_cand.cpu().numpy().view(np.uint64).reshape(n, 1, 8), cand)
    assert np.array_equal(lg[:n].reshape(n, 1), legs) and (lg[n:] == 0xA5).all()


@pytest.mark.parametrize("curve", [0, 1])
def test_trait_method(gpu_ctx, curve):
    import torch
    for dst_len in (0, 21, 255):
        msgs, dst = _msgs(dst_len if dst_len else 1), R.dst_of(dst_len)
        n = len(msgs)
        xy, inf = gpu_ctx.curve_hash_to_curve(curve, msgs, dst if dst_len else None)
        if curve == R.SECP:      # 96 uniform bytes, the first 32 of each 48-byte half, two maps, add
            ub = gpu_ctx.expand_message_xmd(msgs, dst if dst_len else None, 96)
            assert bytes(ub[5]) == R.expand_message_xmd(msgs[5], dst, 96)
            us = [[R.M.field_from_bytes(curve, bytes(row[48 * i:48 * i + 32]))[0] for row in ub] for i in range(2)]
            p0, p1 = (_proj(gpu_ctx.map_to_curve(curve, u)[0]) for u in us)
            want = gpu_ctx.batch_to_affine(curve, gpu_ctx.point_op(curve, 0, p0, p1))
        else:                    # one SHA-256 of msg || dst, one map
            u = [R.M.field_from_bytes(curve, hashlib.sha256(m + dst).digest())[0] for m in msgs]
            want = gpu_ctx.batch_to_affine(curve, _proj(gpu_ctx.map_to_curve(curve, u)[0]))
        assert np.array_equal(xy, want[0]) and np.array_equal(inf, want[1]) and not inf.any(), dst_len
        for i in range(0, 9):
            x, y, f = R.curve_hash_to_curve(curve, msgs[i], dst)
            assert xy[i].tolist() == list(x) + list(y) and int(inf[i]) == int(f), (dst_len, i)
        for k in NS:
            assert np.array_equal(gpu_ctx.curve_hash_to_curve(curve, msgs[:k], dst if dst_len else None)[0], xy[:k])
        keep, pm, po, total = _dev_msgs(torch, msgs, shift=3)
        d_xy = torch.full((n * 64 + GUARD,), 0xA5, dtype=torch.uint8, device=keep[0].device)
        d_inf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=keep[0].device)
        d_st = torch.full((n,), 9, dtype=torch.uint8, device=keep[0].device)
        torch.cuda.synchronize()   # (the fills, on torch's stream, ahead of the call on the ctx's own)
        gpu_ctx.curve_hash_to_curve_dev(curve, pm, po, total, dst if dst_len else None, d_xy.data_ptr(), d_inf.data_ptr(), d_st.data_ptr(), n)
        torch.cuda.synchronize()
        o, fl = d_xy.cpu().numpy(), d_inf.cpu().numpy()
        assert np.array_equal(o[:n * 64].view(np.uint64).reshape(n, 8), xy) and (o[n * 64:] == 0xA5).all()
        assert not fl[:n].any() and (fl[n:] == 0xA5).all() and not d_st.cpu().numpy().any()


@pytest.mark.parametrize("curve", [0, 1])
def test_map_to_curve_dev_on_planted_limbs(gpu_ctx, curve):
    import torch
    cases = [c for c in FIXTURE["map"] if c[0] == curve]
    n = len(cases)
    d_u = _dev(torch, np.array([c[2] for c in cases], dtype=np.uint64))
    d_xy = torch.full((n * 64 + GUARD,), 0xA5, dtype=torch.uint8, device=d_u.device)
    d_cand = torch.full((n * 64 + GUARD,), 0xA5, dtype=torch.uint8, device=d_u.device)
    d_legs = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=d_u.device)
    torch.cuda.synchronize()   # (the fills, on torch's stream, ahead of the call on the ctx's own)
    gpu_ctx.map_to_curve_dev(curve, d_u.data_ptr(), d_xy.data_ptr(), d_cand.data_ptr(), d_legs.data_ptr(), n)
    torch.cuda.synchronize()
    xy, cand, legs = d_xy.cpu().numpy(), d_cand.cpu().numpy(), d_legs.cpu().numpy()
    assert xy[:n * 64].view(np.uint64).reshape(n, 8).tolist() == [c[3] for c in cases] and (xy[n * 64:] == 0xA5).all()
    assert cand[:n * 64].view(np.uint64).reshape(n, 8).tolist() == [c[4] for c in cases] and (cand[n * 64:] == 0xA5).all()
    assert legs[:n].tolist() == [c[5] for c in cases] and (legs[n:] == 0xA5).all()
    gpu_ctx.map_to_curve_dev(curve, d_u.data_ptr(), d_xy.data_ptr(), None, None, n)       # NULL for both
    torch.cuda.synchronize()
    assert np.array_equal(d_xy.cpu().numpy(), xy)


# ---- bad ranges, chunks, a multi-device ctx, refused arguments ----
@pytest.mark.parametrize("curve", [0, 1])
def test_dev_bad_range_gives_status_4_and_zero_outputs(gpu_ctx, curve):
    import torch
    dev = torch.device("cuda:0")
    n, dst = 8, R.dst_of(21)
    tm = _dev(torch, np.arange(64, dtype=np.uint8))
    offs = np.array([0, 5, 10, 50, 45, 3, 1 << 62, 2, 7], dtype=np.uint64)   # elements 2..6 out of range
    to = _dev(torch, offs)
    bad = np.array([not (offs[i] <= offs[i + 1] <= 40) for i in range(n)])
    good_msgs = [bytes(range(int(offs[i]), int(offs[i + 1]))) if not bad[i] else b"" for i in range(n)]

    def run(call, widths):
        bufs = [torch.full((n * w + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for w in widths]
        st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        call([b.data_ptr() for b in bufs], st.data_ptr())
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 4).tolist() == bad.tolist() and not st.cpu().numpy()[~bad].any()
        outs = []
        for b, w in zip(bufs, widths):
            a = b.cpu().numpy()
            assert (a[n * w:] == 0xA5).all()                       # the guard is untouched
            a = a[:n * w].reshape(n, w)
            assert not a[bad].any()
            outs.append(a)
        return outs

    (xm,) = run(lambda p, s: gpu_ctx.expand_message_xmd_dev(tm.data_ptr(), to.data_ptr(), 40, dst, 33, p[0], s, n), [33])
    (fu,) = run(lambda p, s: gpu_ctx.hash_to_field_dev(curve, tm.data_ptr(), to.data_ptr(), 40, dst, 2, p[0], s, n), [64])
    hp, hc, hl = run(lambda p, s: gpu_ctx.hash_to_curve_dev(curve, tm.data_ptr(), to.data_ptr(), 40, dst, p[0], p[1], p[2], s, n), [96, 128, 2])
    ep, ec, el = run(lambda p, s: gpu_ctx.encode_to_curve_dev(curve, tm.data_ptr(), to.data_ptr(), 40, dst, p[0], p[1], p[2], s, n), [96, 64, 1])
    tx, ti = run(lambda p, s: gpu_ctx.curve_hash_to_curve_dev(curve, tm.data_ptr(), to.data_ptr(), 40, dst, p[0], p[1], s, n), [64, 1])
    good = [i for i in range(n) if not bad[i]]
    msgs = [good_msgs[i] for i in good]
    assert np.array_equal(xm[good], gpu_ctx.expand_message_xmd(msgs, dst, 33))
    assert np.array_equal(fu[good].copy().view(np.uint64).reshape(-1, 2, 4), gpu_ctx.hash_to_field(curve, msgs, dst, 2))
    wp, wc, wl = gpu_ctx.hash_to_curve(curve, msgs, dst)
    assert np.array_equal(hp[good].copy().view(np.uint64), wp) and np.array_equal(hc[good].copy().view(np.uint64).reshape(-1, 2, 8), wc)
    assert np.array_equal(hl[good], wl)
    assert np.array_equal(ep[good].copy().view(np.uint64), gpu_ctx.encode_to_curve(curve, msgs, dst)[0])
    assert np.array_equal(tx[good].copy().view(np.uint64), gpu_ctx.curve_hash_to_curve(curve, msgs, dst)[0])


@pytest.mark.parametrize("curve", [0, 1])
def test_chunked_and_multi_device(gpu_ctx, curve):
    import torch
    import forge_ec_amd as F
    msgs, dst = _msgs(22)[:200], R.dst_of(22)
    want = {"xmd": gpu_ctx.expand_message_xmd(msgs, dst, 33), "field": gpu_ctx.hash_to_field(curve, msgs, dst, 2),
            "hash": gpu_ctx.hash_to_curve(curve, msgs, dst), "encode": gpu_ctx.encode_to_curve(curve, msgs, dst),
            "trait": gpu_ctx.curve_hash_to_curve(curve, msgs, dst)}
    u = want["field"][:, 0]
    want["map"] = gpu_ctx.map_to_curve(curve, u)

    def same(ctx):
        assert np.array_equal(ctx.expand_message_xmd(msgs, dst, 33), want["xmd"])
        assert np.array_equal(ctx.hash_to_field(curve, msgs, dst, 2), want["field"])
        for name, got in (("hash", ctx.hash_to_curve(curve, msgs, dst)), ("encode", ctx.encode_to_curve(curve, msgs, dst)),
                          ("trait", ctx.curve_hash_to_curve(curve, msgs, dst)), ("map", ctx.map_to_curve(curve, u))):
            assert all(np.array_equal(a, b) for a, b in zip(got, want[name])), name

    gpu_ctx.set_chunk(64)
    try:
        same(gpu_ctx)
    finally:
        gpu_ctx.set_chunk(1 << 18)
    keep, pm, po, total = _dev_msgs(torch, msgs[:4])
    d = torch.zeros(4 * 128, dtype=torch.uint8, device=keep[0].device)
    with F.Context(devices=[0, 0]) as multi:
        same(multi)
        lib, h, c_dst = multi._lib, multi._h, ctypes.c_char_p(dst)
        assert lib.fec_expand_message_xmd_dev(h, pm, po, total, c_dst, 22, 32, d.data_ptr(), None, 4, None) == E_UNSUPPORTED
        assert lib.fec_hash_to_field_dev(h, curve, pm, po, total, c_dst, 22, 1, d.data_ptr(), None, 4, None) == E_UNSUPPORTED
        assert lib.fec_map_to_curve_dev(h, curve, d.data_ptr(), d.data_ptr(), None, None, 4, None) == E_UNSUPPORTED
        assert lib.fec_hash_to_curve_dev(h, curve, 0, 0, pm, po, total, c_dst, 22, d.data_ptr(), None, None, None, 4, None) == E_UNSUPPORTED
        assert lib.fec_curve_hash_to_curve_dev(h, curve, pm, po, total, c_dst, 22, d.data_ptr(), d.data_ptr(), None, 4, None) == E_UNSUPPORTED


def test_refused_arguments(gpu_ctx):
    import torch
    lib, h = gpu_ctx._lib, gpu_ctx._h
    msgs = [b"a", b"bc"]
    mb, off, total = gpu_ctx._messages(msgs)
    pm, po = mb.ctypes.data, off.ctypes.data
    out = np.zeros(2 * 8200, dtype=np.uint8)
    o, o2 = out.ctypes.data, out.ctypes.data + 8192
    dst = ctypes.c_char_p(bytes(300))
    keep, dm, do, dtotal = _dev_msgs(torch, msgs)
    dd = torch.zeros(2 * 8200, dtype=torch.uint8, device=keep[0].device)
    dp, dp2 = dd.data_ptr(), dd.data_ptr() + 8192
    # Ed25519 implements no HashToCurve
    assert lib.fec_hash_to_field(h, 2, pm, po, total, dst, 5, 1, o, 2) == E_UNSUPPORTED
    assert lib.fec_map_to_curve(h, 2, o, o2, None, None, 2) == E_UNSUPPORTED
    assert lib.fec_hash_to_curve(h, 2, 0, 0, pm, po, total, dst, 5, o, None, None, 2) == E_UNSUPPORTED
    assert lib.fec_curve_hash_to_curve(h, 2, pm, po, total, dst, 5, o, o2, 2) == E_UNSUPPORTED
    assert lib.fec_hash_to_curve_dev(h, 2, 0, 0, dm, do, dtotal, dst, 5, dp, None, None, None, 2, None) == E_UNSUPPORTED
    assert lib.fec_hash_to_field(h, 3, pm, po, total, dst, 5, 1, o, 2) == E_ARG
    for curve in (0, 1):
        # dst_len > 255
        assert lib.fec_expand_message_xmd(h, pm, po, total, dst, 256, 32, o, 2) == E_UNSUPPORTED
        assert lib.fec_expand_message_xmd_dev(h, dm, do, dtotal, dst, 256, 32, dp, None, 2, None) == E_UNSUPPORTED
        assert lib.fec_hash_to_field(h, curve, pm, po, total, dst, 256, 1, o, 2) == E_UNSUPPORTED
        assert lib.fec_hash_to_curve(h, curve, 0, 0, pm, po, total, dst, 256, o, None, None, 2) == E_UNSUPPORTED
        assert lib.fec_curve_hash_to_curve(h, curve, pm, po, total, dst, 256, o, o2, 2) == E_UNSUPPORTED
        assert lib.fec_curve_hash_to_curve_dev(h, curve, dm, do, dtotal, dst, 256, dp, dp2, None, 2, None) == E_UNSUPPORTED
        assert lib.fec_hash_to_field(h, curve, pm, po, total, dst, 255, 1, o, 2) == 0
        # dst_len == 0: refused by hash / encode only
        for mode in (0, 1):
            assert lib.fec_hash_to_curve(h, curve, mode, 0, pm, po, total, None, 0, o, None, None, 2) == E_ARG
            assert lib.fec_hash_to_curve_dev(h, curve, mode, 0, dm, do, dtotal, None, 0, dp, None, None, None, 2, None) == E_ARG
        assert lib.fec_expand_message_xmd(h, pm, po, total, None, 0, 32, o, 2) == 0
        assert lib.fec_hash_to_field(h, curve, pm, po, total, None, 0, 1, o, 2) == 0
        assert lib.fec_curve_hash_to_curve(h, curve, pm, po, total, None, 0, o, o2, 2) == 0
        assert lib.fec_hash_to_field(h, curve, pm, po, total, None, 5, 1, o, 2) == E_ARG      # a length without a string
        # count 0 and 256
        assert lib.fec_hash_to_field(h, curve, pm, po, total, dst, 5, 0, o, 2) == E_ARG
        assert lib.fec_hash_to_field(h, curve, pm, po, total, dst, 5, 256, o, 2) == E_UNSUPPORTED
        assert lib.fec_hash_to_field_dev(h, curve, dm, do, dtotal, dst, 5, 256, dp, None, 2, None) == E_UNSUPPORTED
        assert lib.fec_hash_to_field(h, curve, pm, po, total, dst, 5, 255, o, 2) == 0
        # an unknown mode; the methods that are not offered
        assert lib.fec_hash_to_curve(h, curve, 2, 0, pm, po, total, dst, 5, o, None, None, 2) == E_ARG
        assert lib.fec_hash_to_curve(h, curve, -1, 0, pm, po, total, dst, 5, o, None, None, 2) == E_ARG
        assert lib.fec_hash_to_curve(h, curve, 0, 1, pm, po, total, dst, 5, o, None, None, 2) == E_UNSUPPORTED
        assert lib.fec_hash_to_curve(h, curve, 1, 2, pm, po, total, dst, 5, o, None, None, 2) == E_UNSUPPORTED
        assert lib.fec_hash_to_curve(h, curve, 0, 3, pm, po, total, dst, 5, o, None, None, 2) == E_ARG
        # missing arrays, a bad layout, misaligned device arrays
        assert lib.fec_hash_to_curve(h, curve, 0, 0, pm, po, total, dst, 5, None, None, None, 2) == E_ARG
        assert lib.fec_hash_to_curve(h, curve, 0, 0, pm, None, total, dst, 5, o, None, None, 2) == E_ARG
        assert lib.fec_hash_to_curve(h, curve, 0, 0, pm, po, total + 1, dst, 5, o, None, None, 2) == E_ARG
        assert lib.fec_curve_hash_to_curve(h, curve, pm, po, total, dst, 5, o, None, 2) == E_ARG
        assert lib.fec_map_to_curve(h, curve, None, o, None, None, 2) == E_ARG
        assert lib.fec_hash_to_curve_dev(h, curve, 0, 0, dm, do, dtotal, dst, 5, dp + 8, None, None, None, 2, None) == E_ARG
        assert lib.fec_hash_to_curve_dev(h, curve, 0, 0, dm, do + 4, dtotal, dst, 5, dp, None, None, None, 2, None) == E_ARG
        assert lib.fec_map_to_curve_dev(h, curve, dp + 8, dp2, None, None, 2, None) == E_ARG
    # out_len > 8160; out_len == 0 with NULL out
    assert lib.fec_expand_message_xmd(h, pm, po, total, dst, 5, 8161, o, 2) == E_UNSUPPORTED
    assert lib.fec_expand_message_xmd_dev(h, dm, do, dtotal, dst, 5, 8161, dp, None, 2, None) == E_UNSUPPORTED
    assert lib.fec_expand_message_xmd(h, pm, po, total, dst, 5, 0, None, 2) == 0
    assert lib.fec_expand_message_xmd(h, pm, po, total, dst, 5, 32, None, 2) == E_ARG
    assert lib.fec_expand_message_xmd(None, pm, po, total, dst, 5, 32, o, 2) == E_ARG
    gpu_ctx.check()
