"""
GPU sweep of every *_dev entry point at the least alignment its header allows, with guarded arrays.

include/fecgpu.h and include/fecgpu_canon.h say what each array of a *_dev call must satisfy (16 bytes for records of 32 bytes
and more unless told otherwise, 8 for the message offsets, 4 for a few arrays, nothing for the rest); the argument tests show
that a pointer moved off those rules is refused.  Every passing *_dev call of the suite, though, hands the library tensors of
their own, which torch aligns to 256 bytes or more and pads behind.  A caller with slices of one resident buffer hands it the
least the header allows -- a scalar array at 16 mod 32, 33-byte keys at an odd address, digests at 4 mod 8, offsets at
8 mod 16 -- and an output of exactly n records with something else behind it.

Each case here is one call of one builder of the two call-order modules (tests/test_gpu_canon_streams.py,
tests/test_gpu_parity_streams.py: the c_* functions, with their model-computed inputs and expected outputs) in one of its
parameter forms, or of a builder below for an entry point those modules have none for, on a ctx of this module's own whose
library is the relocating proxy of tests/dev_footprint.py: every array of the call is copied into a poisoned arena -- layout
"least": at its least alignment; layout "aligned": at a multiple of 256, the control that shows the harness passes where the
suite already passes -- the call runs on the ctx's own stream, and then
  (a) the return code is 0: a refusal of an array where the header allows it is a failure;
  (b) every arena byte outside the arrays still holds the poison: no wide closing store, no lane of the ragged last
      wavefront, nothing before record 0;
  (c) every input array is byte-identical to what went in;
  (d) after the copy back, the builder's own comparison with its model (Call.bad()) is empty.
Counts: the modules' n = 197 (three full wavefronts and a ragged one) and n = 1, the smallest shape at which a wide closing
store or an unmasked lane can go wrong.  No tolerance anywhere: every comparison is bit-exact against the builders' models.

test_every_dev_entry_point_was_swept keeps the sweep from hiding a gap: what the proxy recorded must be every *_dev symbol
of forge_ec_amd._lib but the exclusions written there.
"""
import numpy as np
import pytest

import canon_sign_ref as S
import dev_footprint as D
import h2c_ref as H
import test_gpu_canon_streams as CS
import test_gpu_parity_streams as PS
from stream_gate import Call, ptr

pytestmark = pytest.mark.gpu

COUNTS = [197, 1]
ROT = CS.ROT_B
SEED = bytes(range(32))

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- builders for the entry points the call-order modules have none for (they read CS.N / PS.N like the others) ---------------
def c_canon_rfc6979_k(ctx, rot, curve):
    dev, C = CS._canon(ctx, curve), CS.MODEL[curve]
    want = cached(("canon rfc6979", curve), lambda: [S.ecdsa_nonce(C, e["d"], e["digest"]) for e in CS.recs(curve)])
    assert all(w[1] == 0 for w in want)
    at = [(i + rot) % CS.NREC for i in range(CS.N)]
    dg, k = CS.up(CS.rows(CS.cyc(curve, rot, lambda e: e["digest"]))), CS.up(CS.rows(CS.cyc(curve, rot, lambda e: e["key"])))
    out, st_ = CS.out_bytes(32), CS.out_status()
    return Call("rfc6979_k_dev " + curve, lambda st: dev.rfc6979_k_dev(dg.data_ptr(), k.data_ptr(), out[0].data_ptr(), st_[0].data_ptr(), CS.N, ptr(st)),
                [out, st_], [CS.rows([want[j][0] for j in at]), CS.ZEROS])


def c_canon_msm(ctx, rot, curve):
    """one 64-byte sum and one status byte: the drawn case of tests/test_gpu_canon_msm.py at this count, its expected sum by
    the logarithms of the fixture's pool"""
    import torch
    import test_gpu_canon_msm as TM
    dev, n = CS._canon(ctx, curve), CS.N
    k, p, (wxy, wst) = cached(("canon msm", curve, n), lambda: TM._pool_case(curve, n, 1 + rot))
    dk, dp = CS.up(k), CS.up(p)
    out, st_ = (torch.full((1, 8), -1, dtype=torch.int64, device="cuda"), -1), (torch.full((1,), 9, dtype=torch.uint8, device="cuda"), 9)
    return Call("msm_dev " + curve, lambda st: dev.msm_dev(dk.data_ptr(), dp.data_ptr(), n, out[0].data_ptr(), st_[0].data_ptr(), ptr(st)),
                [out, st_], [np.array(wxy, dtype=np.uint64).reshape(1, 8), np.array([wst], dtype=np.uint8)])


def c_canon_batch_verify(ctx, rot, scheme):
    """n status bytes and the one verdict byte: the fixture's valid signatures tiled, and from n = 8 on an element the call
    refuses (its status set, the verdict still 1: tests/test_gpu_canon_batch.py)"""
    import torch
    import test_gpu_canon_batch as TB
    from forge_ec_amd.canon import CanonEd25519, CanonSecp256k1
    dev, n = (CanonSecp256k1 if scheme == "bip340" else CanonEd25519)(ctx), CS.N
    msgs, sigs, pks = TB.FX.tiled(scheme, n)
    want = np.zeros(n, dtype=np.uint8)
    if n >= 8:
        _, rmsg, rsig, rpk, rstatus = TB.FX.refused(scheme)[0]
        msgs[5], sigs[5], pks[5], want[5] = rmsg, rsig, rpk, rstatus
    buf, off, sg, pk = TB._arrays(msgs, sigs, pks)
    m, o, s_, p_ = CS.up(buf), CS.up(off), CS.up(sg), CS.up(pk)
    verdict, st_ = (torch.full((1,), 9, dtype=torch.uint8, device="cuda"), 9), (torch.full((n,), 9, dtype=torch.uint8, device="cuda"), 9)
    fn = getattr(dev, ("bip340" if scheme == "bip340" else "ed25519") + "_batch_verify_msg_dev")
    # (the verdict first: a Call takes its count from its first output, and this call has one verdict for its n statuses)
    return Call(scheme + "_batch_verify_msg_dev",
                lambda st: fn(m.data_ptr(), o.data_ptr(), int(off[n]), s_.data_ptr(), p_.data_ptr(), SEED, st_[0].data_ptr(), verdict[0].data_ptr(), n, ptr(st)),
                [verdict, st_], [np.array([1], dtype=np.uint8), want.reshape(1, n)])


def c_curve_hash_to_curve(ctx, oracle, rot, c):
    msgs = PS.messages(3501 + c)

    def model():
        r = [H.curve_hash_to_curve(c, m, PS.DST) for m in msgs]
        return PS.u64([list(x[0]) + list(x[1]) for x in r], 8), np.array([int(x[2]) for x in r], dtype=np.uint8)
    wxy, winf = cached(("curve_h2c", c), model)
    (m, off, total), xy, inf, st_ = PS.up_msgs(msgs, rot), PS.out(64), PS.out(1), PS.status()
    return Call("curve_hash_to_curve_dev " + PS.NAMES[c],
                lambda st: ctx.curve_hash_to_curve_dev(c, m.data_ptr(), off.data_ptr(), total, PS.DST, xy[0].data_ptr(), inf[0].data_ptr(), st_[0].data_ptr(),
                                                       PS.N, ptr(st)),
                [xy, inf, st_], [PS.cyc(wxy, rot), PS.cyc(winf, rot), np.zeros(PS.N, dtype=np.uint8)])


# ---- the forms: every builder in every parameter form the call-order modules run it in ------------------------------------------
def _forms():
    canon = {}
    for name, (f, args, _) in CS.VERIFY_USERS.items():
        canon[name] = (f, args)
    canon.update(CS.PER_STREAM)
    for curve in CS.NAMES:
        canon.update({"mul_base " + curve: (CS.c_mul_base, (curve,)), "mul " + curve: (CS.c_mul, (curve,)), "double_mul " + curve: (CS.c_double_mul, (curve,)),
                      "msm " + curve: (c_canon_msm, (curve,))})
    canon.update({"rfc6979_k secp256k1": (c_canon_rfc6979_k, ("secp256k1",)), "rfc6979_k p256": (c_canon_rfc6979_k, ("p256",)),
                  "bip340_batch_verify_msg": (c_canon_batch_verify, ("bip340",)), "ed25519_batch_verify_msg": (c_canon_batch_verify, ("ed25519",))})
    parity, seen = {}, set()
    for table in (PS.TABLE_USERS, PS.FORKERS, PS.PER_STREAM):
        for name, fa in table.items():
            if fa not in seen:                                 # (batch_double_mul on Ed25519 stands in two of the tables)
                seen.add(fa)
                parity[name] = fa
    parity["batch_mul_fixed own base Y"] = (PS.c_mul_fixed, (PS.ED, "Y"))
    parity.update({"curve_hash_to_curve secp256k1": (c_curve_hash_to_curve, (PS.SECP,)), "curve_hash_to_curve p256": (c_curve_hash_to_curve, (PS.P256,))})
    return canon, parity


CANON, PARITY = _forms()
FORMS = [("canon", k) for k in CANON] + [("parity", k) for k in PARITY]

# the *_dev symbols the sweep leaves out, each with its reason
EXCLUDED = {
    "fec_multi_batch_mul_dev": "takes arrays of per-device pointers on a multi-device ctx: tests/test_gpu_multi_ctx.py is its home",
    "fec_multi_batch_mul_fixed_dev": "takes arrays of per-device pointers on a multi-device ctx: tests/test_gpu_multi_ctx.py is its home",
    "fec_multi_batch_double_mul_dev": "takes arrays of per-device pointers on a multi-device ctx: tests/test_gpu_multi_ctx.py is its home",
    "fec_generator_dev": "takes no arrays: it returns the address of the ctx's own generator",
}


@pytest.fixture(scope="module")
def rig():
    """a ctx of this module's own (the session's stays untouched) with a small prefix table, and the arena"""
    import forge_ec_amd as F
    ctx = F.Context(0)
    ctx.set_fixed_prefix_bits(13)
    state = dict(ctx=ctx, real=ctx._lib, arena=D.Arena(D.TorchMemory(D.ARENA_BYTES)), called=set(), cases=0)
    yield state
    ctx._lib = state["real"]
    ctx.close()


def sweep(rig, oracle, mp, family, form, layout, n):
    """one case: (findings, elements that differ from the model, their outputs, the entry points the proxy relocated)"""
    import torch
    from forge_ec_amd import FecError
    mod = CS if family == "canon" else PS
    mp.setattr(mod, "N", n)
    if family == "canon":
        mp.setattr(CS, "ZEROS", np.zeros(n, dtype=np.uint8))
        mp.setattr(CS, "ONES", np.ones(n, dtype=np.uint8))
    f, args = (CANON if family == "canon" else PARITY)[form]
    ctx = rig["ctx"]
    proxy = D.Proxy(rig["real"], rig["arena"], layout)
    ctx._lib = proxy
    try:
        call = f(ctx, ROT, *args) if family == "canon" else f(ctx, oracle, ROT, *args)
        torch.cuda.synchronize()
        try:
            call.run(None)
        except FecError:
            pass                                               # (the proxy holds the status as a finding)
        torch.cuda.synchronize()
    finally:
        ctx._lib = rig["real"]
    rig["called"] |= proxy.called()
    rig["cases"] += 1
    rig["ran", family, form] = True
    assert len(proxy.log) == 1, "the builder issued %d relocated calls: %s" % (len(proxy.log), proxy.log)
    return proxy.findings, call.bad(), call.bad_outputs()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("family,form", FORMS, ids=["%s: %s" % ff for ff in FORMS])
def test_dev_call_at_its_alignment_with_guarded_arrays(rig, oracle, monkeypatch, family, form, layout, n):
    findings, bad, outputs = sweep(rig, oracle, monkeypatch, family, form, layout, n)
    assert not findings, "\n".join(f["text"] for f in findings)
    assert not bad, "%d of %d elements differ from the model, the first at %s, in %s" % (len(bad), n, bad[:8], ", ".join(outputs))
    rig["ctx"].check()


def test_the_device_arena_sees_what_the_model_test_plants(rig):
    """the device backend of the arena (tests/test_dev_footprint_model.py has the host one): copies in and out by address, a
    byte planted behind an array at its least alignment and one before it are found and named"""
    import torch
    arena = rig["arena"]
    mem = arena.mem
    arena.reset()
    src = torch.arange(33 * 5, dtype=torch.uint8, device="cuda")
    at = arena.place(33 * 5, 0, "least", 33, "pks")
    other = arena.place(64, 16, "least", 32, "keys")
    assert at % 2 == 1 and other % 32 == 16
    mem.copy(at, src.data_ptr(), 33 * 5)
    mem.sync()
    assert np.array_equal(mem.read(at, 33 * 5), np.arange(33 * 5, dtype=np.uint8)) and arena.stray() == []
    assert (mem.read(mem.base, mem.size) == D.POISON).sum() == mem.size - 33 * 5               # (the ramp ends below the poison)
    mem.t[at - mem.base + 33 * 5 + 2] = 0
    mem.t[other - mem.base - 1] = 7
    mem.sync()
    got = [(f["array"], f["side"], f["bytes"], f["count"], f["record"]) for f in arena.stray()]
    assert got == [("pks", "behind", 2, 1, 5), ("keys", "before", 1, 1, 1)]
    back = torch.zeros(33 * 5, dtype=torch.uint8, device="cuda")
    mem.copy(back.data_ptr(), at, 33 * 5)
    mem.sync()
    assert torch.equal(back, src)
    arena.reset()
    assert arena.stray() == []


def test_every_dev_entry_point_was_swept(rig, oracle, monkeypatch):
    """what the proxy relocated is every *_dev symbol of the library but the exclusions above.  (Run on its own, or behind a
    part of the sweep, it first runs one case of every form whose entry point it has not seen.)"""
    from forge_ec_amd import _lib as L
    for family, form in FORMS:
        if not rig.get(("ran", family, form)):
            findings, bad, _ = sweep(rig, oracle, monkeypatch, family, form, "least", 1)
            assert not findings and not bad, (family, form, [x["text"] for x in findings], bad)
    symbols = {s for s in L.ABI_SYMBOLS + L.CANON_ABI_SYMBOLS if s.endswith("_dev")}
    assert set(EXCLUDED) <= symbols
    assert rig["called"] == symbols - set(EXCLUDED), (sorted(symbols - set(EXCLUDED) - rig["called"]), sorted(rig["called"] - symbols))
    assert not rig["called"] & set(EXCLUDED)
    print("\n%d (entry point, form, layout, count) cases over %d entry points in %d forms" % (rig["cases"], len(rig["called"]), len(FORMS)))
    rig["ctx"].check()
