"""
CPU checks of the test-side restatement of Rfc6979::<C, Sha256>::generate_k and of Ecdsa::<C, Sha256>::sign from the
message (tests/rfc6979_ref.py): the restatement reproduces the three nonces the reference's own test module records;
its two signing backends -- ecdsa_sign_ref.sign over the C oracle and gen_ecdsa_sign.sign over oracle/py_model.py, which
wrote tests/golden/rfc6979_vectors.json -- agree on the fixture; and the fixture covers what its generator promises.
"""
import json
import os

import numpy as np
import pytest

import rfc6979_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "rfc6979_vectors.json")))
LENGTHS = (0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 200)
KEY_CLASSES = ("0", "1", "N-1", "N", "2^256-1", "random")


def _cases(curve):
    return [c for c in FIXTURE["cases"] if c["curve"] == curve]


def test_restatement_equals_the_recorded_reference_nonces():
    assert len(FIXTURE["recorded"]) == 3
    for c in FIXTURE["recorded"]:
        assert c["sk"] == R.E._limbs(1 << 248)          # the inherent little-endian from_bytes of 00..01
        k, retries = R.generate_k(c["sk"], bytes.fromhex(c["msg"]), R.ORDER[0])
        assert R.E._limbs(k) == c["k"] and retries == 0
        assert k.to_bytes(32, "little").hex() == c["k_hex_recorded"]   # as the reference's test prints it


@pytest.mark.parametrize("curve", [0, 1])
def test_fixture_nonces_are_the_restatement(curve):
    for c in _cases(curve):
        assert R.E._limbs(R.generate_k(c["sk"], bytes.fromhex(c["msg"]), R.ORDER[curve])[0]) == c["k"]


@pytest.mark.parametrize("curve", [0, 1])
def test_sign_msg_backends_agree_on_the_fixture(oracle, curve):
    cases = _cases(curve)
    sk, msgs = [c["sk"] for c in cases], [bytes.fromhex(c["msg"]) for c in cases]
    r, s, st, k = R.sign_msg(oracle, curve, sk, msgs)
    assert st.tolist() == [c["status"] for c in cases]
    assert r.tolist() == [c["r"] for c in cases] and s.tolist() == [c["s"] for c in cases]
    for i, c in enumerate(cases):                        # a rejected key draws no nonce
        assert k[i].tolist() == (c["k"] if c["status"] != 1 else [0, 0, 0, 0])


def test_fixture_coverage():
    for curve in (0, 1):
        cases = _cases(curve)
        nv = R.ORDER[curve]
        values = {"0": 0, "1": 1, "N-1": nv - 1, "N": nv, "2^256-1": (1 << 256) - 1}
        for name in KEY_CLASSES:
            mine = [c for c in cases if c["key"] == name]
            assert sorted(len(c["msg"]) // 2 for c in mine) == sorted(LENGTHS + (12,)), (curve, name)
            assert sum(bytes.fromhex(c["msg"]) == b"test message" for c in mine) == 1
            if name in values:
                assert all(R.E._val(c["sk"]) == values[name] for c in mine)
        rejected = {c["key"] for c in cases if c["status"] == 1}
        assert rejected == ({"0", "N", "2^256-1"} if curve == 0 else {"0"})
        assert all(c["status"] == 1 for c in cases if c["key"] in rejected)
        assert any(c["status"] == 0 for c in cases)
        for c in cases:
            if c["status"] != 0:
                assert c["r"] == [1, 0, 0, 0] and c["s"] == [1, 0, 0, 0]
    assert os.path.getsize(os.path.join(HERE, "golden", "rfc6979_vectors.json")) < (1 << 20)


def test_library_exports_the_new_entry_points():
    import ctypes

    from forge_ec_amd import build
    build.build()
    lib = ctypes.CDLL(build.SO)
    for sym in ("fec_ecdsa_sign_msg", "fec_ecdsa_sign_msg_dev", "fec_rfc6979_k", "fec_rfc6979_k_dev", "fec_debug_rfc6979_k"):
        assert hasattr(lib, sym), sym
