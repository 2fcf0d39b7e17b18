"""
GPU tests of the library's three written promises about key material in device memory, by reading the memory:

  * include/fecgpu_canon.h, the signing block: "Host forms stage keys and signatures as secrets: staging and every work-area
    region that held a key, a nonce or an un-normalised point is cleared on every way out; the *_dev forms clear their work
    area behind their last kernel."
  * csrc/host_ctx.hpp, chunked: "a call that names any secret array clears, on every way out, all the staging it used and
    the scratch of the streams it ran on."
  * include/fecgpu.h: fec_ctx_wipe "zeroes every device buffer the ctx owns that can hold copies of caller data"; the parity
    *_dev forms keep their intermediates in the stream's scratch until that wipe.

fec_debug_work_area_read (Context.debug_work_areas) reads back every buffer on the list that fec_ctx_wipe clears
(csrc/host_ctx.hpp: for_each_work_buffer), whole capacity.  hipMalloc does not zero-fill and a buffer's capacity is larger
than any request, so "all zero" is made an exact statement per case: a fresh ctx; the call once at the case's shape, which
performs every allocation; fec_ctx_wipe, after which every byte of every buffer must read zero (this pins the wipe); the
call again with other keys, whose statuses must all be 0 and whose outputs non-zero (and, at n = 1, equal to the
project's model of the call: it really did the work); then every byte of every buffer must read zero again.

Shapes: n = 1; n = 65, one lane past a wavefront; n = 300 in chunks of 128, three chunks with a ragged tail of 44, so a
two-lane call uses both lanes and a message call restages slots 2 and 3; the *_dev forms also n = 8 right after n = 300
on the same stream (a clear sized to what the small call used would leave the large call's tail).  The error ways out
are not reached here (covered by reading only).

tests/secret_residue_cases.py holds the two tables; tests/test_work_area_census.py keeps them equal to the source.
"""
import numpy as np
import pytest

import secret_residue_cases as T

pytestmark = pytest.mark.gpu

HOST_SHAPES = [(1, None), (65, None), (300, 128)]          # (n, chunk)
DEV_SHAPES = [(1,), (65,), (300,), (300, 8)]               # the calls of step 4, in order
_SIDE = {}


def _ctx(multi=False):
    import forge_ec_amd as F
    return F.Context(devices=[0, 0]) if multi else F.Context(0)


def residue(ctx):
    """[(index, name, bytes of capacity, non-zero bytes, offset of the first)] of the work buffers that are not all zero"""
    out = []
    for i, (name, buf) in enumerate(ctx.debug_work_areas()):
        nz = np.flatnonzero(buf)
        if nz.size:
            out.append((i, name, buf.size, int(nz.size), int(nz[0])))
    return out


def allocated(ctx):
    return [(name, buf.size) for name, buf in ctx.debug_work_areas() if buf.size]


def _assert_results(row, outs, sts, n):
    for s in sts:
        assert not np.asarray(s).any(), (row.id, "status", np.asarray(s).reshape(-1)[:16].tolist())
    for o in outs:
        o = np.ascontiguousarray(o).view(np.uint8).reshape(n, -1)
        assert o.any(axis=1).all(), (row.id, "an output row is all zero")


def _assert_model(row, args, outs, oracle):
    want = row.want(args, oracle)
    assert len(want) == len(outs)
    for w, o in zip(want, outs):
        w, o = np.ascontiguousarray(w).view(np.uint8).reshape(-1), np.ascontiguousarray(o).view(np.uint8).reshape(-1)
        assert np.array_equal(w, o), (row.id, "differs from the model")


# ---- (a) the host forms ---------------------------------------------------------------------------------------------------
def _host_case(row, n, chunk, multi, oracle):
    ctx = _ctx(multi)
    try:
        if chunk:
            ctx.set_chunk(chunk)
        row.call(ctx, row.make(1, n))                      # warm-up: every allocation
        assert allocated(ctx), "the call allocated no work buffer: the case would test nothing"
        ctx.wipe()
        assert residue(ctx) == [], "fec_ctx_wipe left bytes"
        before = allocated(ctx)
        args = row.make(2, n)
        outs, sts = row.call(ctx, args)
        _assert_results(row, outs, sts, n)
        if n == 1:
            _assert_model(row, args, outs, oracle)
        assert allocated(ctx) == before, "a buffer regrew: its new memory was never zero"
        assert residue(ctx) == [], "%s left bytes in the ctx's device buffers" % row.fn
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "n%d" % s[0])
@pytest.mark.parametrize("row", T.HOST_ROWS, ids=repr)
def test_host_form_leaves_nothing(oracle, row, shape):
    _host_case(row, shape[0], shape[1], False, oracle)


@pytest.mark.parametrize("row", T.HOST_ROWS, ids=repr)
def test_host_form_leaves_nothing_on_a_multi_device_ctx(oracle, row):
    """devices = [0, 0], n = 300 in chunks of 64: each shard worker runs three chunks; both children are read"""
    _host_case(row, 300, 64, True, oracle)


# ---- (b) the canonical *_dev forms --------------------------------------------------------------------------------------
def _stream(kind):
    import torch
    if kind == "null":
        return None
    if "s" not in _SIDE:
        _SIDE["s"] = torch.cuda.Stream()   # kept for the life of the module: the ctx orders its next launch behind it
    return _SIDE["s"].cuda_stream


@pytest.mark.parametrize("shape", DEV_SHAPES, ids=lambda s: "n" + "-then-".join(map(str, s)))
@pytest.mark.parametrize("stream", ["null", "side"])
@pytest.mark.parametrize("row", T.DEV_ROWS, ids=repr)
def test_dev_form_leaves_nothing(oracle, row, stream, shape):
    import torch
    s = _stream(stream)
    ctx = _ctx()
    try:
        keep = [row.call(ctx, row.make(1, shape[0]), shape[0], s)]
        torch.cuda.synchronize()
        ctx.check()
        if row.work_area:
            assert any(name == "stream_scratch" for name, _ in allocated(ctx)), "no stream scratch: the case would test nothing"
        ctx.wipe()
        assert residue(ctx) == [], "fec_ctx_wipe left bytes"
        before = allocated(ctx)
        for j, n in enumerate(shape):
            args = row.make(2 + j, n)
            k = row.call(ctx, args, n, s)
            keep.append(k)
        torch.cuda.synchronize()
        ctx.check()
        outs, sts = T.outs_of(row.id, k)                  # (of the last call: its inputs are `args`)
        _assert_results(row, outs, sts, n)
        if "rec" in k:
            assert (k["rec"].cpu().numpy() <= 3).all()
        if n == 1 and stream == "null":
            _assert_model(row, args, outs, oracle)
        assert allocated(ctx) == before, "a buffer regrew: its new memory was never zero"
        assert residue(ctx) == [], "%s left bytes in the ctx's device buffers" % row.fn
    finally:
        ctx.close()


# ---- (c) the parity *_dev forms are documented to retain ----------------------------------------------------------------------
# include/fecgpu.h, one signer per curve:
#   fec_schnorr_sign_msg_dev: "the _dev form leaves every buffer to the caller (the stream's scratch keeps k, sk, R and P until
#     the ctx is wiped, fec_ctx_wipe, or destroyed)"
#   fec_ecdsa_sign_msg_dev:   "the _dev forms leave every buffer to the caller (the stream's scratch keeps k, h1 and R until the
#     ctx is wiped, fec_ctx_wipe, or destroyed)"
#   fec_ed25519_sign_dev:     "The _dev forms leave every buffer to the caller, as fec_ecdsa_sign_dev does (the stream's scratch
#     keeps a, r, A and R until the ctx is wiped, fec_ctx_wipe, or destroyed)"
def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _up_msgs(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return _up(np.frombuffer(b"".join(msgs), dtype=np.uint8)), _up(off), int(off[-1])


@pytest.mark.parametrize("signer", ["schnorr_sign_msg_dev-secp256k1", "ecdsa_sign_msg_dev-p256", "ed25519_sign_dev"])
def test_parity_dev_signers_retain_until_the_wipe(signer):
    """the positive control: the hook reads live memory, and the documented retention is what happens"""
    import torch
    n = 65
    rng = T._rng(7)
    sk, keys, msgs = T.limbs(rng, n), T.raw_bytes(rng, n), T.messages(rng, n)
    m, off, total = _up_msgs(msgs)
    out = [torch.zeros(n * w, dtype=torch.uint8, device="cuda") for w in (64, 1, 32, 64, 1)]
    ctx = _ctx()
    try:
        if signer.startswith("schnorr"):
            d_sk = _up(sk)
            ctx.schnorr_sign_msg_dev(T.SECP, d_sk.data_ptr(), m.data_ptr(), off.data_ptr(), total, out[0].data_ptr(), out[1].data_ptr(),
                                     out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), n)
        elif signer.startswith("ecdsa"):
            d_sk = _up(sk)
            ctx.ecdsa_sign_msg_dev(T.P256, d_sk.data_ptr(), m.data_ptr(), off.data_ptr(), total, out[0].data_ptr(), out[4].data_ptr(), n)
        else:
            d_sk = _up(keys)
            ctx.ed25519_sign_dev(d_sk.data_ptr(), m.data_ptr(), off.data_ptr(), total, out[0].data_ptr(), out[4].data_ptr(), n)
        torch.cuda.synchronize()
        ctx.check()
        assert out[0].cpu().numpy().any(), "the signer wrote nothing"
        left = residue(ctx)
        assert [r for r in left if r[1] == "stream_scratch"], "the stream's scratch reads all zero after a parity *_dev signer: %r" % (left,)
        ctx.wipe()
        assert residue(ctx) == []
    finally:
        ctx.close()


# ---- (d) the wipe is complete ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_wipe_clears_every_kind_of_buffer(multi):
    """one call of each kind that touches a distinct buffer; each named buffer allocated and not all zero; then the wipe"""
    import torch
    from forge_ec_amd.canon import CanonEd25519, CanonSecp256k1
    n = 150
    rng = T._rng(11)
    ctx = _ctx(multi)
    try:
        ctx.set_chunk(32)
        g = np.array(ctx.generator(T.SECP), dtype=np.uint64).reshape(1, 12)
        pts = ctx.batch_mul(T.SECP, T.limbs(rng, n), np.repeat(g, n, axis=0))            # two lanes: slots 0, 1, 4, 5
        # a message call that names no secret (one that does would clear slots 0 .. 3 behind itself): slots 2, 3
        ctx.ecdsa_verify_msg(T.SECP, T.messages(rng, n), T.limbs(rng, n), T.limbs(rng, n), T.limbs(rng, n, 8))
        u1, u2, q = _up(T.limbs(rng, n)), _up(T.limbs(rng, n)), _up(pts)
        o1, o2 = (torch.zeros(n * 96, dtype=torch.uint8, device="cuda") for _ in range(2))
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        if multi:   # the parity *_dev forms of a multi-device ctx take one shard per worker, each on a stream of its own
            ctx.multi_batch_double_mul_dev(T.SECP, [u1.data_ptr(), u1.data_ptr()], [u2.data_ptr(), u2.data_ptr()], [q.data_ptr(), q.data_ptr()],
                                           [o1.data_ptr(), o2.data_ptr()], [n, n], streams=[s.cuda_stream for s in streams])
        else:
            ctx.batch_double_mul_dev(T.SECP, u1.data_ptr(), u2.data_ptr(), q.data_ptr(), o1.data_ptr(), n, streams[0].cuda_stream)
            ctx.batch_double_mul_dev(T.SECP, u1.data_ptr(), u2.data_ptr(), q.data_ptr(), o2.data_ptr(), n, streams[1].cuda_stream)
        # canonical mode (a multi-device ctx runs it on its first worker): d_verify, d_zbuf, d_win_scratch; then d_tbuf
        secp, ed = CanonSecp256k1(ctx), CanonEd25519(ctx)
        gxy, _ = secp.mul_base(T.limbs(rng, n))
        exy, _ = ed.mul_base(T.limbs(rng, n))
        z, r, s_, pk, res = _up(T.limbs(rng, n)), _up(T.limbs(rng, n)), _up(T.limbs(rng, n)), _up(gxy), torch.zeros(n, dtype=torch.uint8, device="cuda")
        secp.ecdsa_verify_dev(z.data_ptr(), r.data_ptr(), s_.data_ptr(), pk.data_ptr(), res.data_ptr(), n)
        e1, e2, ep = _up(T.limbs(rng, n)), _up(T.limbs(rng, n)), _up(exy)
        eo, est = torch.zeros(n * 64, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        ed.double_mul_dev(e1.data_ptr(), e2.data_ptr(), ep.data_ptr(), eo.data_ptr(), est.data_ptr(), n)
        torch.cuda.synchronize()
        ctx.check()
        areas = ctx.debug_work_areas()
        starts = [i for i, (name, _) in enumerate(areas) if name == "d_buf[0]"]   # one run of the list per shard worker
        assert len(starts) == (2 if multi else 1)
        per_child = starts[1] if multi else len(areas)
        first = areas[:per_child]
        live = {}
        for name, buf in first:
            live.setdefault(name, []).append(bool(buf.any()))
        for name in ("d_buf[0]", "d_buf[1]", "d_buf[2]", "d_buf[3]", "d_buf[4]", "d_buf[5]", "d_win_scratch", "d_zbuf", "d_tbuf", "d_verify"):
            assert live.get(name) == [True], (name, "is not allocated, or reads all zero", live)
        scratch = [bool(buf.any()) for name, buf in areas if name == "stream_scratch"]
        assert scratch.count(True) >= 2, ("two streams' scratch should hold the products", scratch)
        if multi:
            second = dict((name, buf) for name, buf in areas[per_child:] if name != "stream_scratch")
            assert second["d_buf[0]"].any() and second["d_buf[2]"].any(), "the second shard worker staged nothing"
        ctx.wipe()
        assert residue(ctx) == []
        assert [name for name, _ in ctx.debug_work_areas()] == [name for name, _ in areas]   # the hook changed nothing
    finally:
        ctx.close()
