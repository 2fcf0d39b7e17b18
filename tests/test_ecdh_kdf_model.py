"""
CPU checks of the test-side restatement of KeyExchange::derive_key, derive_shared_secret + derive_key and
KeyExchange::exchange (tests/ecdh_kdf_ref.py): the HKDF restatement gives RFC 5869's A.3 output and equals an
independent one on the `hmac` module at every grid point; both backends -- the C oracle and oracle/py_model.py, which
wrote tests/golden/ecdh_kdf_vectors.json -- reproduce the fixture; a failed exchange has zero outputs; the fixture
covers what its generator promises; and the planted batches of tests/test_gpu_ecdh_kdf.py meet their status shares on
the reference side alone.
"""
import hashlib
import hmac
import json
import os

import numpy as np
import pytest

import ecdh_kdf_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "ecdh_kdf_vectors.json")))
SECRET_POOL, INFO_POOL = bytes.fromhex(FIXTURE["secret_pool"]), bytes.fromhex(FIXTURE["info_pool"])


def _hkdf_independent(secret, info, out_len):
    """RFC 5869 with the hmac module and a zero-filled salt, written from the RFC rather than from the reference."""
    prk = hmac.new(bytes(32), secret, hashlib.sha256).digest()
    n = (out_len + 31) // 32
    t, okm = b"", b""
    for i in range(1, n + 1):
        t = hmac.new(prk, t + info + bytes([i]), hashlib.sha256).digest()
        okm += t
    return okm[:out_len]


def test_rfc5869_a3():
    assert K.hkdf_zero_salt(K.A3_IKM, b"", K.A3_L) == K.A3_OKM
    a3 = FIXTURE["a3"]
    assert bytes.fromhex(a3["ikm"]) == K.A3_IKM and a3["info"] == "" and a3["out_len"] == 42 and bytes.fromhex(a3["okm"]) == K.A3_OKM


def test_fixture_derive_key_is_the_restatement_and_an_independent_hkdf():
    seen = set()
    for curve, s, i, o, okm in FIXTURE["derive_key"]:
        secret, info = SECRET_POOL[:s], INFO_POOL[:i]
        assert K.derive_key(curve, secret, info, o).hex() == okm and len(okm) == 2 * o
        if curve == 0:
            assert _hkdf_independent(secret, info, o).hex() == okm
        else:
            assert bytes((secret[j] if j < s else 0) ^ (info[j] if j < i else 0) for j in range(o)).hex() == okm
        seen.add((curve, s, i, o))
    for curve in (0, 1):
        for s in K.SECRET_LENS:
            for i in K.INFO_LENS:
                for o in K.OUT_LENS:
                    assert (curve, s, i, o) in seen
        assert (curve, 32, 23, K.MAX_OUT) in seen
    assert K.MAX_OUT == 8128 and len(FIXTURE["derive_key"]) == len(seen)
    assert "restatement-derived" in FIXTURE["provenance"]
    assert os.path.getsize(os.path.join(HERE, "golden", "ecdh_kdf_vectors.json")) < (1 << 20)


def test_hmac_written_out_equals_the_hmac_module():
    for klen in (0, 1, 32, 64, 65, 100):
        for dlen in (0, 1, 55, 56, 64, 119, 120):
            key, data = INFO_POOL[:klen], INFO_POOL[100:100 + dlen]
            assert K.hmac_sha256(key, data) == hmac.new(key, data, hashlib.sha256).digest()


@pytest.mark.parametrize("backend", ["c_oracle", "py_model"])
def test_backends_reproduce_the_exchange_fixture(oracle, backend):
    o = oracle if backend == "c_oracle" else None
    cases = FIXTURE["exchange"]
    assert {c["status"] for c in cases} == {0, 1, 2} and {c["info"] for c in cases} == {"", b"forge-ec ecdh fixture 1".hex()}
    assert any(c["status"] == 2 and c["sk"] == [0, 0, 0, 0] for c in cases) and any(c["status"] == 2 and c["pk_inf"] for c in cases)
    assert any(c["curve"] == 1 and c["status"] == 1 and "REJECTS" in c["note"] for c in cases)
    for c in cases:
        info = bytes.fromhex(c["info"])
        keys, st = K.ecdh_derive_key(o, c["curve"], [c["sk"]], [c["pk"]], [c["pk_inf"]], info, c["out_len"])
        xy, inf, keys2, st2 = K.exchange(o, c["curve"], [c["sk"]], [c["pk"]], [c["pk_inf"]], info, c["out_len"])
        assert int(st[0]) == int(st2[0]) == c["status"]
        assert bytes(keys[0]).hex() == bytes(keys2[0]).hex() == c["key"]
        assert [int(v) for v in xy[0]] == c["public_xy"] and int(inf[0]) == c["public_inf"]
        if c["status"] != 0:                                 # an Err returns neither a public key nor a key
            assert c["public_xy"] == [0] * 8 and c["public_inf"] == 0 and set(c["key"]) <= {"0"}
        else:
            assert c["public_xy"] != [0] * 8


@pytest.mark.parametrize("curve", [0, 1])
def test_planted_batches_meet_their_status_shares(oracle, curve):
    sk, pk, inf = K.planted_batch(curve)
    _, st = oracle.batch_ecdh(curve, sk, pk, inf, nthreads=8)
    K.assert_planted_shares(curve, st)
    keys, st2 = K.ecdh_derive_key(oracle, curve, sk, pk, inf, b"abc", 33)
    assert st2.tolist() == st.tolist() and not keys[st != 0].any() and keys[st == 0].any(axis=1).all()


def test_library_exports_the_new_entry_points():
    import ctypes

    from forge_ec_amd import build
    build.build()
    lib = ctypes.CDLL(build.SO)
    for sym in ("fec_derive_key", "fec_derive_key_dev", "fec_ecdh_derive_key", "fec_ecdh_derive_key_dev", "fec_ecdh_exchange",
                "fec_ecdh_exchange_dev"):
        assert hasattr(lib, sym), sym
