"""
GPU tests of canonical mode's batch signature verification (fec_canon_bip340_batch_verify_msg, fec_canon_ed25519_batch_verify_msg
and their *_dev forms): every case through the host form and the *_dev form, every expected value from the model
(tests/canon_batch_ref.py on oracle/canon_model.py) or from the per-signature verifiers of the library
(fec_canon_bip340_verify_msg, fec_canon_ed25519_verify_msg), whose own tests pin them to the same model.

The signatures are the fixture's (tests/golden/canon_batch_vectors.json), tiled for the larger batches: duplicates are legal
in a batch, and the coefficients differ by index.
"""
import random

import numpy as np
import pytest

import canon_batch_ref as B
from abi_arg_table import Buffers, arr, call_args, spoils

pytestmark = pytest.mark.gpu

FX = B.load_fixture()
E_ARG, E_UNSUPPORTED = -1, -5
SEED = bytes(range(32))


@pytest.fixture(scope="module", params=B.SCHEMES)
def sv(request, gpu_ctx):
    """(scheme, device wrapper, ctx); the window and the chunk are back at their defaults afterwards"""
    from forge_ec_amd.canon import CanonEd25519, CanonSecp256k1
    scheme = request.param
    yield scheme, (CanonSecp256k1 if scheme == "bip340" else CanonEd25519)(gpu_ctx), gpu_ctx
    gpu_ctx.set_canon_msm_window(0)
    gpu_ctx.set_chunk(1 << 18)


def _fn(dev, scheme, what):
    return getattr(dev, ("bip340_" if scheme == "bip340" else "ed25519_") + what)


def _single(dev, scheme, msgs, sigs, pks):
    return [int(v) for v in _fn(dev, scheme, "verify_msg")(msgs, sigs, pks)]


def _host(dev, scheme, msgs, sigs, pks, seed=SEED):
    ok, st, verdict = _fn(dev, scheme, "batch_verify_msg")(msgs, sigs, pks, seed)
    return ok, [int(v) for v in st], verdict


def _arrays(msgs, sigs, pks):
    """the packed numpy arrays of a batch given as lists: (message bytes, offsets, sigs, pks)"""
    n = len(sigs)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return (np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy(), off, np.frombuffer(b"".join(sigs) or bytes(64), dtype=np.uint8).copy(),
            np.frombuffer(b"".join(pks) or bytes(32), dtype=np.uint8).copy())


class Resident:
    """a batch on the device, with its status and verdict buffers"""

    def __init__(self, arrays, n):
        import torch
        buf, off, sg, pk = arrays
        self.n, self.total = n, int(off[n])
        self.buf, self.sg, self.pk = (torch.from_numpy(a).cuda() for a in (buf, sg, pk))
        self.off = torch.from_numpy(off.view(np.int64)).cuda()
        self.st = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
        self.verdict = torch.full((1,), 9, dtype=torch.uint8, device="cuda")

    def enqueue(self, dev, scheme, seed=SEED, stream=None):
        _fn(dev, scheme, "batch_verify_msg_dev")(self.buf.data_ptr(), self.off.data_ptr(), self.total, self.sg.data_ptr(), self.pk.data_ptr(), seed,
                                                 self.st.data_ptr(), self.verdict.data_ptr(), self.n, stream)

    def result(self, full_status=True):
        st, verdict = self.st.cpu().numpy(), int(self.verdict.cpu()[0])
        assert st[self.n] == 9                                   # nothing written past the n statuses
        ok = bool(verdict == 1 and not st[:self.n].any())
        return ok, ([int(v) for v in st[:self.n]] if full_status else int(st[:self.n].max(initial=0))), verdict


def _dev(dev, scheme, msgs, sigs, pks, seed=SEED, stream=None):
    import torch
    r = Resident(_arrays(msgs, sigs, pks), len(sigs))
    r.enqueue(dev, scheme, seed, stream)
    torch.cuda.synchronize()
    return r.result()


def _both(dev, scheme, msgs, sigs, pks, seed=SEED):
    h, d = _host(dev, scheme, msgs, sigs, pks, seed), _dev(dev, scheme, msgs, sigs, pks, seed)
    assert h == d
    return h


def _flip(b, byte, bit=0):
    return b[:byte] + bytes([b[byte] ^ (1 << bit)]) + b[byte + 1:]


# ---- sizes, windows, slices ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 513])
def test_valid_batches_of_every_size(sv, n):
    scheme, dev, ctx = sv
    ctx.set_canon_msm_window(0)
    assert _both(dev, scheme, *FX.tiled(scheme, n)) == (True, [0] * n, 1)
    ctx.check()


@pytest.mark.parametrize("c", [2, 5, 13, 16])
def test_forced_windows(sv, c):
    scheme, dev, ctx = sv
    msgs, sigs, pks = FX.tiled(scheme, 65)
    ctx.set_canon_msm_window(c)
    assert _both(dev, scheme, msgs, sigs, pks) == (True, [0] * 65, 1)
    sigs[64] = _flip(sigs[64], 45)
    assert _both(dev, scheme, msgs, sigs, pks) == (False, [0] * 65, 0)
    ctx.set_canon_msm_window(0)
    ctx.check()


def test_host_slices_keep_the_running_sum_and_the_buckets(sv):
    """n = 513 at chunk 64 (nine slices), 4096 and the default: the same verdicts and statuses"""
    scheme, dev, ctx = sv
    msgs, sigs, pks = FX.tiled(scheme, 513)
    bad = list(sigs)
    bad[512] = _flip(bad[512], 50)          # the last slice of nine
    name, rmsg, rsig, rpk, rstatus = FX.refused(scheme)[0]
    want_status = [0] * 513
    want_status[100] = rstatus
    got = []
    for chunk in (64, 4096, 1 << 18):
        ctx.set_chunk(chunk)
        assert _host(dev, scheme, msgs, sigs, pks) == (True, [0] * 513, 1), chunk
        assert _host(dev, scheme, msgs, bad, pks) == (False, [0] * 513, 0), chunk
        got.append(_host(dev, scheme, msgs[:100] + [rmsg] + msgs[101:], sigs[:100] + [rsig] + sigs[101:], pks[:100] + [rpk] + pks[101:]))
    assert got == [(False, want_status, 1)] * 3
    ctx.set_chunk(1 << 18)
    ctx.check()


def test_two_internal_slices(sv):
    """n = 2^17 + 1: 2 n + 1 entries, more than one slice of the sum; the last element lies in the second slice"""
    import torch
    scheme, dev, ctx = sv
    n, rows = (1 << 17) + 1, FX.triples(scheme)
    idx = np.arange(n) % len(rows)
    lens = np.array([len(r[0]) for r in rows], dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens[idx], out=off[1:])
    reps = n // len(rows) + 1
    buf = np.frombuffer((b"".join(r[0] for r in rows) * reps)[:int(off[n])], dtype=np.uint8).copy()
    sg = np.frombuffer(b"".join(r[1] for r in rows), dtype=np.uint8).reshape(-1, 64)[idx].copy()
    pk = np.frombuffer(b"".join(r[2] for r in rows), dtype=np.uint8).reshape(-1, 32)[idx].copy()
    assert buf.size == int(off[n])
    r = Resident((buf, off, sg.reshape(-1), pk.reshape(-1)), n)
    r.enqueue(dev, scheme)
    torch.cuda.synchronize()
    assert r.result(full_status=False) == (True, 0, 1)
    sg[n - 1, 45] ^= 1
    r = Resident((buf, off, sg.reshape(-1), pk.reshape(-1)), n)
    r.enqueue(dev, scheme)
    torch.cuda.synchronize()
    assert r.result(full_status=False) == (False, 0, 0)
    ctx.check()


# ---- corruptions and refusals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 32, 64])
def test_one_corruption_at_a_time(sv, at):
    """a bit of s, of r, of the key, of the message -> verdict 0 with every status 0 (where the flipped r or key still decodes:
    the model says which; a bit is chosen for which it does)"""
    scheme, dev, ctx = sv
    msgs, sigs, pks = FX.tiled(scheme, 65)
    s_byte = 45
    for part in ("s", "r", "key", "msg"):
        for bit in range(8):
            m, s, p = list(msgs), list(sigs), list(pks)
            if part == "s":
                s[at] = _flip(s[at], s_byte, bit)
            elif part == "r":
                s[at] = _flip(s[at], 9, bit)
            elif part == "key":
                p[at] = _flip(p[at], 9, bit)
            else:
                m[at] = _flip(m[at], 0, bit) if m[at] else b"\0"
            if B.batch(scheme, [m[at]], [s[at]], [p[at]], SEED)[1] == [0]:
                break
        else:
            raise AssertionError("no bit found")
        assert _both(dev, scheme, m, s, p) == (False, [0] * 65, 0), (part, at)
    ctx.check()


def test_refused_elements_leave_the_verdict_to_the_rest(sv):
    scheme, dev, ctx = sv
    msgs, sigs, pks = FX.tiled(scheme, 65)
    rows = FX.refused(scheme)
    assert {r[4] for r in rows} == {B.BAD_POINT, B.BAD_SCALAR}
    for k, (name, msg, sig, pk, status) in enumerate(rows):
        at = (0, 33, 64)[k % 3]
        want = [0] * 65
        want[at] = status
        got = _both(dev, scheme, msgs[:at] + [msg] + msgs[at + 1:], sigs[:at] + [sig] + sigs[at + 1:], pks[:at] + [pk] + pks[at + 1:])
        assert got == (False, want, 1), name
    # every element refused: nothing but 0 * G in the sum
    got = _both(dev, scheme, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    assert got == (False, [r[4] for r in rows], 1)
    ctx.check()


def test_a_bad_message_range_is_status_4(sv):
    import torch
    scheme, dev, ctx = sv
    msgs, sigs, pks = FX.tiled(scheme, 5)
    buf, off, sg, pk = _arrays(msgs, sigs, pks)
    off[3] = off[5] + 1                      # elements 2 and 3
    r = Resident((buf, off, sg, pk), 5)
    r.total = int(off[5])
    r.enqueue(dev, scheme)
    torch.cuda.synchronize()
    assert r.result() == (False, [0, 0, B.BAD_RANGE, B.BAD_RANGE, 0], 1)
    ctx.check()


def test_the_cancelling_pair(sv):
    scheme, dev, ctx = sv
    msgs, sigs, pks = FX.tiled(scheme, 9)
    sigs[2], sigs[7] = B.cancelling_pair(scheme, sigs[2], sigs[7], 0x1234567)
    assert _single(dev, scheme, msgs, sigs, pks) == [1, 1, 0, 1, 1, 1, 1, 0, 1]
    assert B.batch(scheme, msgs, sigs, pks, SEED, coeff=B.ones)[2] == 1      # a sum without coefficients accepts the pair
    for k in range(8):
        assert _both(dev, scheme, msgs, sigs, pks, B.fixed_seed(k)) == (False, [0] * 9, 0), k
    ctx.check()


def test_torsion_defects_pass_here_and_not_the_per_signature_verifier(gpu_ctx):
    from forge_ec_amd.canon import CanonEd25519
    dev = CanonEd25519(gpu_ctx)
    msgs, sigs, pks = FX.tiled("ed25519", 2)
    assert len(FX.torsion()) == 6
    for name, msg, sig, pk in FX.torsion():
        seed = B.seed_with_odd(name, [1])      # a_1 odd: a cofactorless sum would refuse for certain (tests/test_canon_batch_model.py)
        m, s, p = [msgs[0], msg, msgs[1]], [sigs[0], sig, sigs[1]], [pks[0], pk, pks[1]]
        assert _both(dev, "ed25519", m, s, p, seed) == (True, [0, 0, 0], 1), name
        assert _single(dev, "ed25519", m, s, p) == [1, 0, 1], name
    gpu_ctx.check()


def test_random_batches_agree_with_the_per_signature_verifier(sv):
    """200 seeded batches of n = 33 with 0 to 3 corruptions: ok == all(per-signature verifier), the verifier run once over all
    of them; the model's verdict on every tenth"""
    scheme, dev, ctx = sv
    rng = random.Random("canon-batch/" + scheme)
    rows = FX.triples(scheme)
    batches = []
    for b in range(200):
        pick = [rows[rng.randrange(len(rows))] for _ in range(33)]
        m, s, p = [r[0] for r in pick], [r[1] for r in pick], [r[2] for r in pick]
        for _ in range(rng.randrange(4)):
            at, what = rng.randrange(33), rng.randrange(3)
            if what == 0:
                s[at] = _flip(s[at], rng.randrange(64), rng.randrange(8))
            elif what == 1:
                p[at] = _flip(p[at], rng.randrange(32), rng.randrange(8))
            else:
                m[at] = m[at] + b"x"
        batches.append((m, s, p))
    each = _single(dev, scheme, [x for b in batches for x in b[0]], [x for b in batches for x in b[1]], [x for b in batches for x in b[2]])
    seen = set()
    for b, (m, s, p) in enumerate(batches):
        seed = B.fixed_seed(1000 + b)
        got = _host(dev, scheme, m, s, p, seed) if b % 2 else _dev(dev, scheme, m, s, p, seed)
        valid = each[33 * b:33 * b + 33]
        assert got[0] == all(valid), b
        assert all(v == 0 for v, st in zip(valid, got[1]) if st), b     # a refused element is an invalid signature
        if b % 10 == 0:
            assert got == B.batch(scheme, m, s, p, seed), b
        seen.add(got[0])
    assert seen == {True, False}
    ctx.check()


def test_seeds(sv):
    scheme, dev, ctx = sv
    msgs, sigs, pks = FX.tiled(scheme, 40)
    bad = list(sigs)
    bad[7] = _flip(bad[7], 40)
    for s in (sigs, bad):
        assert _both(dev, scheme, msgs, s, pks, SEED) == _both(dev, scheme, msgs, s, pks, SEED)
    for _ in range(2):                       # seed=None: drawn by the library
        assert _host(dev, scheme, msgs, sigs, pks, None) == (True, [0] * 40, 1)
        assert _dev(dev, scheme, msgs, sigs, pks, None) == (True, [0] * 40, 1)
        assert _host(dev, scheme, msgs, bad, pks, None) == (False, [0] * 40, 0)
    ctx.check()


# ---- the shared work area ---------------------------------------------------------------------------------------------------------
def test_three_calls_on_three_streams(sv):
    """three batch calls on three streams, a per-signature verifier and an fec_canon_msm between them on the same ctx: the work
    area is the ctx's, so the calls must run in call order"""
    import torch
    import canon_msm_ref as MR
    from oracle import canon_model as CM
    from forge_ec_amd.canon import CANON_CURVES
    scheme, dev, ctx = sv
    ctx.set_canon_msm_window(0)
    curve = "secp256k1" if scheme == "bip340" else "ed25519"
    msm = CANON_CURVES[curve](ctx)
    good = FX.tiled(scheme, 300)
    bad = (good[0], list(good[1]), good[2])
    bad[1][299] = _flip(bad[1][299], 45)
    rname, rmsg, rsig, rpk, rstatus = FX.refused(scheme)[0]
    ref = (good[0][:76] + [rmsg], good[1][:76] + [rsig], good[2][:76] + [rpk])
    calls = [Resident(_arrays(*b), len(b[1])) for b in (good, bad, ref)]
    ks, refs = MR.draw(curve, 777, 12)
    pool = MR.load_fixture().pool(curve)
    pool_xy = np.array([CM.xy_limbs(pt) for _, _, pt in pool], dtype=np.uint64)
    k = np.array([CM.limbs(v) for v in ks], dtype=np.uint64).reshape(-1, 4)
    p = pool_xy[np.array(refs, dtype=np.int64)].reshape(-1, 8)
    want_msm = tuple(MR.result(curve, MR.msm_by_logs(curve, ks, [pool[r][0] for r in refs], [pool[r][1] for r in refs], MR.load_fixture().T(curve))))
    dk, dp = (torch.from_numpy(a.view(np.int64).reshape(-1)).cuda() for a in (k, p))
    out, ost = torch.full((8,), -1, dtype=torch.int64, device="cuda"), torch.full((1,), 9, dtype=torch.uint8, device="cuda")
    vmsgs, vsigs, vpks = bad
    vbuf, voff, vsg, vpk = (torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in _arrays(vmsgs, vsigs, vpks))
    vres = torch.full((300,), 9, dtype=torch.uint8, device="cuda")

    def verify(stream):
        _fn(dev, scheme, "verify_msg_dev")(vbuf.data_ptr(), voff.data_ptr(), int(voff[300]), vsg.data_ptr(), vpk.data_ptr(), vres.data_ptr(), 300, stream)

    # the work areas and the comb tables exist before the calls in flight: growing them would synchronise
    calls[0].enqueue(dev, scheme)
    verify(None)
    msm.msm_dev(dk.data_ptr(), dp.data_ptr(), 777, out.data_ptr(), ost.data_ptr(), None)
    torch.cuda.synchronize()
    for c in calls:
        c.st.fill_(9)
        c.verdict.fill_(9)
    vres.fill_(9)
    out.fill_(-1)
    streams = [torch.cuda.Stream() for _ in range(3)]
    calls[0].enqueue(dev, scheme, SEED, streams[0].cuda_stream)
    verify(streams[1].cuda_stream)
    calls[1].enqueue(dev, scheme, SEED, streams[1].cuda_stream)
    msm.msm_dev(dk.data_ptr(), dp.data_ptr(), 777, out.data_ptr(), ost.data_ptr(), streams[2].cuda_stream)
    calls[2].enqueue(dev, scheme, SEED, streams[2].cuda_stream)
    torch.cuda.synchronize()
    assert calls[0].result() == (True, [0] * 300, 1)
    assert calls[1].result() == (False, [0] * 300, 0)
    assert calls[2].result() == (False, [0] * 76 + [rstatus], 1)
    assert vres.cpu().tolist() == [1] * 299 + [0]
    assert ([int(v) for v in out.cpu().numpy().view(np.uint64)], int(ost.cpu()[0])) == want_msm
    ctx.check()


# ---- arguments ----------------------------------------------------------------------------------------------------------------
BATCH = ["ctx", "msgs", "off", "len", arr("sigs", 64), arr("pks", 32), ("val", None), arr("status", 1), arr("verdict", 1), "n"]
SPECS = {"fec_canon_%s_batch_verify_msg%s" % (s, d): (BATCH + (["stream"] if d else []), bool(d)) for s in ("bip340", "ed25519") for d in ("", "_dev")}
OFFSETS_BYTES = (8 + 1 + 2) * 8   # the table's offset arrays: the only buffers of a case that are not zero-filled


def test_argument_codes_and_nothing_launched(gpu_ctx):
    """The case set of tests/test_gpu_abi_arg_codes.py by the same machinery; the expected statuses follow from the header: a
    multi-device ctx is FEC_E_UNSUPPORTED in both forms, every other case FEC_E_ARG -- n = 0 with every array null included,
    because status and verdict are required whatever n is.  No case is a legal call, so nothing may be launched: the status and
    verdict buffers are zero-filled, and a launched call would leave verdict 1 behind in them (with status 2 on secp256k1,
    where the zero key has no square root; on Ed25519 the zero encodings are a point of order 4 and the cofactor accepts it)."""
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    lib, buf = L.lib(), Buffers()
    seen = set()
    with F.Context(devices=[0, 0]) as multi:
        for fn, (spec, dev) in SPECS.items():
            cases = spoils(spec, dev) + ([] if dev else [("ctx=multi", {"ctx": "multi"})])
            for case, spoil in cases:
                spoil = dict(spoil)
                want = E_ARG
                if spoil.get("ctx") == "multi":
                    spoil["ctx"], want = multi._h, E_UNSUPPORTED
                assert int(getattr(lib, fn)(*call_args(spec, dev, buf, gpu_ctx._h, spoil))) == want, (fn, case)
                seen.add(case.split("=")[0].split("+")[0].split(" ")[0])
    assert {"ctx", "n", "msgs", "off", "sigs", "pks", "status", "verdict"} <= seen
    buf.torch.cuda.synchronize()
    checked = 0
    for keep in buf.keep:
        a = keep.cpu().numpy() if isinstance(keep, buf.torch.Tensor) else np.asarray(keep)
        if a.nbytes == OFFSETS_BYTES or a is buf.dst:
            continue
        assert not a.any()
        checked += 1
    assert checked >= 8
    gpu_ctx.check()
