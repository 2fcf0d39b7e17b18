"""
GPU tests of what the from-the-message entry points share on the host side (host_messages.hpp: message_call, with_messages):

  * an all-empty batch -- n = 5, every message empty, msg_len = 0 and a NULL message pointer, the `bytes == 0` leg of the
    staging -- through one host entry point of every caller of the engine, against the models the per-family tests use
    (hashlib for the two hashes);
  * the status every entry point, host and *_dev, returns for bad arguments: a table of cases, each rejected before
    anything is launched (or the valid n = 0 call; or Ed25519 given to the challenge, which supports it, on zeroed points),
    whose expected codes (tests/golden/msg_arg_codes.json) were recorded
    from the library as it was before the seven host scaffolds and the *_dev prologues were merged.  Every buffer of a
    case is real and large enough for n = 8, apart from the one pointer the case spoils;
  * a second table (tests/golden/msg_value_arg_codes.json): a bad value parameter of the hash-to-curve calls, or a bad
    override of fec_debug_rfc6979_k, alone and beside a pointer fault -- which of the two is reported.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from abi_arg_table import DST, arr as _arr, run_table

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "msg_arg_codes.json")


# ---- the all-empty batch ----

@pytest.fixture
def null_msgs(monkeypatch):
    """forge_ec_amd.Context hands an all-empty batch a one-byte dummy buffer; under this fixture it hands it NULL."""
    import forge_ec_amd as F
    real = F.Context._messages

    def messages(msgs):
        _, off, total = real(msgs)
        assert total == 0 and not off.any()
        return None, off, 0
    monkeypatch.setattr(F.Context, "_messages", staticmethod(messages))


EMPTY = [b""] * 5


def _scalars(seed):
    return np.random.default_rng(seed).integers(1, 1 << 62, size=(5, 4), dtype=np.uint64)


def _bytes(seed, width):
    return np.random.default_rng(seed).integers(0, 256, size=(5, width), dtype=np.uint8)


def test_empty_batch_hashes(gpu_ctx, null_msgs):
    assert gpu_ctx.sha256(EMPTY).tobytes() == hashlib.sha256(b"").digest() * 5
    assert gpu_ctx.sha512(EMPTY).tobytes() == hashlib.sha512(b"").digest() * 5


def test_empty_batch_ed25519_sign(gpu_ctx, null_msgs):
    import eddsa_sign_ref as R
    keys = _bytes(1, 32)
    keys[2, 0] = 0x9d                                   # an empty message with this key byte: the reference's fixed signature
    sig, st = gpu_ctx.ed25519_sign(keys, EMPTY)
    want = R.sign_batch(keys, EMPTY, R.CBackend())
    assert [s.tobytes() for s in sig] == [w[0] for w in want] and st.tolist() == [w[1] for w in want]


def test_empty_batch_bip340_sign(gpu_ctx, null_msgs):
    import bip340_sign_ref as R
    keys = _bytes(2, 32)
    keys[:, 31] &= 0x7F                                 # below N: computed signatures
    sig, st = gpu_ctx.bip340_sign(keys, EMPTY)
    want = R.sign_batch(keys, EMPTY, R.CBackend(4))
    assert [s.tobytes() for s in sig] == [bytes(w[0]) for w in want] and st.tolist() == [w[1] for w in want]


def test_empty_batch_ed25519_verify(gpu_ctx, null_msgs):
    import eddsa_verify_ref as R
    pk, sigs = _bytes(3, 32), _bytes(4, 64)
    want = R.verify_batch(pk, EMPTY, sigs, R.CBackend())
    assert want == [1] * 5                              # the reference accepts an empty message before it looks at anything
    assert gpu_ctx.ed25519_verify(pk, EMPTY, sigs).tolist() == want


@pytest.mark.parametrize("curve", [0, 1])
def test_empty_batch_ecdsa_verify_msg(gpu_ctx, null_msgs, oracle, curve):
    from test_gpu_ecdsa_verify_msg import _digests, _verify
    import rfc6979_ref as R
    sk = _scalars(5 + curve)
    r, s, _, _ = R.sign_msg(oracle, curve, sk, EMPTY)   # the reference's own signatures, and one spoiled
    s[3, 0] ^= np.uint64(1)
    pk, inf = oracle.batch_to_affine(curve, oracle.batch_mul_fixed(curve, sk, oracle.generator(curve)))
    pk, inf = np.ascontiguousarray(pk), np.ascontiguousarray(inf).astype(np.uint8)
    want = _verify(oracle, curve, _digests(EMPTY), r, s, pk, inf)
    assert np.array_equal(gpu_ctx.ecdsa_verify_msg(curve, EMPTY, r, s, pk, inf), want)


@pytest.mark.parametrize("curve", [0, 1])
def test_empty_batch_rfc6979_k(gpu_ctx, null_msgs, curve):
    import rfc6979_ref as R
    sk = _scalars(7 + curve)
    k, st = gpu_ctx.rfc6979_k(curve, sk, EMPTY)
    assert not st.any() and np.array_equal(k, R.nonces(curve, sk, EMPTY)[0])


@pytest.mark.parametrize("curve", [0, 1])
def test_empty_batch_schnorr_sign_msg(gpu_ctx, null_msgs, curve):
    import schnorr_sign_ref as S
    sk = _scalars(9 + curve)
    want = S.sign_many(curve, sk, EMPTY)
    r_xy, r_inf, s, sig_bytes, st = gpu_ctx.schnorr_sign_msg(curve, sk, EMPTY)
    assert np.array_equal(st, want["status"]) and np.array_equal(r_xy, want["r_xy"]) and np.array_equal(r_inf, want["r_inf"])
    assert np.array_equal(s, want["s"]) and np.array_equal(sig_bytes, want["sig_bytes"])


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_empty_batch_schnorr_challenge(gpu_ctx, null_msgs, curve):
    from test_gpu_schnorr_challenge import _points, _want
    r_xy, r_inf = _points(gpu_ctx, curve, 5, 60 + curve)
    pk_xy, pk_inf = _points(gpu_ctx, curve, 5, 70 + curve)
    assert np.array_equal(gpu_ctx.schnorr_challenge(curve, r_xy, r_inf, pk_xy, pk_inf, EMPTY), _want(curve, r_xy, r_inf, pk_xy, pk_inf, EMPTY))


def test_empty_batch_expand_message_xmd(gpu_ctx, null_msgs):
    import h2c_ref as H
    assert gpu_ctx.expand_message_xmd(EMPTY, DST, 48).tobytes() == bytes(H.expand_message_xmd(b"", DST, 48)) * 5


# ---- the return-code table ----
# (abi_arg_table.py: what an entry point's argument list says, the cases made from it, run_table)
M = ["msgs", "off", "len"]
D = ["dst", "dst_len"]
ORDER_2_255 = ("order", [0, 0, 0, 1 << 63])


HOST = {
    "fec_sha512": ["ctx"] + M + [_arr("digests", 64), "n"],
    "fec_sha256": ["ctx"] + M + [_arr("digests", 32), "n"],
    "fec_ed25519_sign": ["ctx", _arr("keys", 32)] + M + [_arr("sig", 64), _arr("status", 1), "n"],
    "fec_ed25519_derive_public_key": ["ctx", _arr("keys", 32), _arr("pk", 32), _arr("status", 1), "n"],
    "fec_eddsa_sign_ed25519": ["ctx", _arr("sk", 32)] + M + [_arr("r_xy", 64), _arr("r_inf", 1), _arr("s", 32), _arr("status", 1), "n"],
    "fec_ed25519_verify": ["ctx", _arr("pk", 32)] + M + [_arr("sigs", 64), _arr("status", 1), "n"],
    "fec_eddsa_verify_ed25519_msg": ["ctx", _arr("pk_xy", 64), _arr("pk_inf", 1, False)] + M +
                                    [_arr("r_xy", 64), _arr("r_inf", 1, False), _arr("s", 32), _arr("status", 1), "n"],
    "fec_ecdsa_verify_msg": ["ctx", "curve"] + M + [_arr("r", 32), _arr("s", 32), _arr("pk_xy", 64), _arr("pk_inf", 1, False), _arr("status", 1), "n"],
    "fec_bip340_sign": ["ctx", _arr("keys", 32)] + M + [_arr("sigs", 64), _arr("status", 1), "n"],
    "fec_ecdsa_sign_msg": ["ctx", "curve", _arr("sk", 32)] + M + [_arr("sig", 64), _arr("status", 1), "n"],
    "fec_rfc6979_k": ["ctx", "curve", _arr("sk", 32)] + M + [_arr("k", 32), _arr("status", 1), "n"],
    "fec_debug_rfc6979_k": ["ctx", "curve", ORDER_2_255, _arr("sk", 32)] + M + [_arr("k", 32), _arr("status", 1), "n"],
    "fec_schnorr_challenge": ["ctx", "curve", _arr("r_xy", 64), _arr("r_inf", 1, False), _arr("pk_xy", 64), _arr("pk_inf", 1, False)] + M +
                             [_arr("e", 32), "n"],
    "fec_schnorr_sign_msg": ["ctx", "curve", _arr("sk", 32)] + M +
                            [_arr("r_xy", 64), _arr("r_inf", 1), _arr("s", 32), _arr("sig_bytes", 64, False), _arr("status", 1), "n"],
    "fec_expand_message_xmd": ["ctx"] + M + D + [("val", 48, "out_len"), _arr("out", 48), "n"],
    "fec_hash_to_field": ["ctx", "curve"] + M + D + [("val", 2, "count"), _arr("u", 64), "n"],
    "fec_hash_to_curve": ["ctx", "curve", ("val", 0, "mode"), ("val", 0, "method")] + M + D + [_arr("out", 96), _arr("cand", 128, False), _arr("legs", 2, False), "n"],
    "fec_curve_hash_to_curve": ["ctx", "curve"] + M + D + [_arr("xy", 64), _arr("inf", 1), "n"],
}
ST, ST_OPT = _arr("status", 1), _arr("status", 1, False)
DEV = {
    "fec_sha512_dev": HOST["fec_sha512"][:-1] + [ST_OPT, "n", "stream"],
    "fec_sha256_dev": HOST["fec_sha256"][:-1] + [ST_OPT, "n", "stream"],
    "fec_schnorr_challenge_dev": HOST["fec_schnorr_challenge"][:-1] + [ST, "n", "stream"],
    "fec_expand_message_xmd_dev": HOST["fec_expand_message_xmd"][:-1] + [ST_OPT, "n", "stream"],
    "fec_hash_to_field_dev": HOST["fec_hash_to_field"][:-1] + [ST_OPT, "n", "stream"],
    "fec_hash_to_curve_dev": HOST["fec_hash_to_curve"][:-1] + [ST_OPT, "n", "stream"],
    "fec_curve_hash_to_curve_dev": HOST["fec_curve_hash_to_curve"][:-1] + [ST_OPT, "n", "stream"],
}
for _name in ("fec_ed25519_sign", "fec_ed25519_derive_public_key", "fec_eddsa_sign_ed25519", "fec_ed25519_verify", "fec_eddsa_verify_ed25519_msg",
              "fec_ecdsa_verify_msg", "fec_bip340_sign", "fec_ecdsa_sign_msg", "fec_rfc6979_k", "fec_schnorr_sign_msg"):
    DEV[_name + "_dev"] = HOST[_name] + ["stream"]


def test_return_codes_are_what_they_were(gpu_ctx):
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    want = json.load(open(GOLDEN))
    with F.Context(devices=[0, 0]) as multi:
        got = run_table(L.lib(), gpu_ctx._h, multi._h, ((HOST, False), (DEV, True)))
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if want[k] != v} == {}
    # no case but the curve-2 challenge (a supported curve there) got as far as a launch with elements in it
    assert sorted(k for k, v in want.items() if v == 0) == sorted(
        ["%s: %s" % (fn, c) for fn in ("fec_ed25519_derive_public_key", "fec_ed25519_derive_public_key_dev") for c in ("n=0,every array null",)] +
        ["%s: n=0,every array null" % fn for fn in DEV if fn != "fec_ed25519_derive_public_key_dev"] +
        ["fec_schnorr_challenge: curve=2", "fec_schnorr_challenge_dev: curve=2"])
    gpu_ctx.check()


# ---- the value parameters against the pointer checks ----
# A fault in a value parameter of the four hash-to-curve calls (h2c.hpp: MAX_DST 255, MAX_OUT 8160, MAX_COUNT 255) and in
# fec_debug_rfc6979_k's override: alone, and with a pointer fault beside it -- which of the two the call reports.
VALUE_GOLDEN = os.path.join(HERE, "golden", "msg_value_arg_codes.json")
DST_FAULTS = [("dst_len=256", {"dst_len": 256}), ("dst=null,dst_len=5", {"dst": None, "dst_len": 5})]
VALUE_FAULTS = {
    "fec_expand_message_xmd": DST_FAULTS + [("out_len=8161", {"out_len": 8161})],
    "fec_hash_to_field": DST_FAULTS + [("count=0", {"count": 0}), ("count=256", {"count": 256})],
    "fec_hash_to_curve": DST_FAULTS + [("dst_len=0", {"dst_len": 0}), ("mode=2", {"mode": 2}), ("method=1", {"method": 1}), ("method=3", {"method": 3})],
    "fec_curve_hash_to_curve": DST_FAULTS,
    "fec_debug_rfc6979_k": [("order top two bits clear", {"order": np.array([0, 0, 0, 1 << 61], dtype=np.uint64)})],
}


def _value_cases(fn, spec, dev):
    first = next(a for a in spec if isinstance(a, tuple) and len(a) == 4 and a[2])     # the first required array
    aligned = next(a for a in spec if isinstance(a, tuple) and len(a) == 4 and a[3])   # the first aligned one: 16 bytes, every one here
    beside = [("", {}), ("," + first[0] + "=null", {first[0]: None}), (",off=null", {"off": None})]
    if dev:
        beside += [(",off+4", {"off": "+4"}), (",%s+8" % aligned[0], {aligned[0]: "+8"}), (",ctx=multi", {"ctx": "multi"})]
    return [(fault + name, dict(spoil, **more)) for fault, spoil in VALUE_FAULTS[fn] for name, more in beside]


def value_fault_codes(gpu_ctx):
    """{case id: status} of the cases above (the golden file is this, recorded from the library as it was before the
    from-the-message pairs became one function each)"""
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    host = {fn: HOST[fn] for fn in VALUE_FAULTS}
    dev = {fn + "_dev": DEV[fn + "_dev"] for fn in VALUE_FAULTS if fn + "_dev" in DEV}
    extra = {fn: _value_cases(fn, spec, False) for fn, spec in host.items()}
    extra.update({fn: _value_cases(fn[:-4], spec, True) for fn, spec in dev.items()})
    with F.Context(devices=[0, 0]) as multi:
        got = run_table(L.lib(), gpu_ctx._h, multi._h, ((host, False), (dev, True)), extra)
    return {k: v for k, v in got.items() if k in {"%s: %s" % (fn, c) for fn, cases in extra.items() for c, _ in cases}}


def test_value_faults_beside_pointer_faults_return_what_they_did(gpu_ctx):
    want = json.load(open(VALUE_GOLDEN))
    got = value_fault_codes(gpu_ctx)
    assert len(got) ==3 * (3 + 4 + 6 + 2 + 1) + 6 * (3 + 4 + 6 + 2)
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if want[k] != v} == {}
    assert 0 not in want.values()                       # every case is rejected: nothing was launched
    gpu_ctx.check()
