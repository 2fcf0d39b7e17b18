"""
CPU checks of the parity-mode BIP-340 signer (fec_bip340_sign) and of the entry points that came with it: the test-side
restatement (tests/bip340_sign_ref.py) over the C oracle agrees with the one over oracle/py_model.py and reproduces the
fixture; the fixture is its generator's output and covers what it must (all four parity combinations, the edge keys, the
message case and its near misses, the padding-edge lengths); the library exports the new symbols.
"""
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import bip340_sign_ref as R  # noqa: E402
import gen_bip340_sign as G  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "bip340_sign_vectors.json")


@pytest.fixture(scope="module")
def fx():
    return json.load(open(FIXTURE))["sign"]


def test_fixture_is_the_generator_output(fx):
    rows = G.cases()
    assert [(bytes.fromhex(c["key"]), bytes.fromhex(c["msg"])) for c in fx] == rows


def test_c_oracle_composition_equals_fixture(fx):
    got = R.sign_batch([bytes.fromhex(c["key"]) for c in fx], [bytes.fromhex(c["msg"]) for c in fx], R.CBackend())
    assert [(s.hex(), st) for s, st in got] == [(c["sig"], c["status"]) for c in fx]


def test_python_and_c_backends_agree_on_random_inputs():
    rnd = random.Random(11)
    keys = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(4)]
    msgs = [bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(0, 150))) for _ in range(4)]
    assert R.sign_batch(keys, msgs, R.PyBackend()) == R.sign_batch(keys, msgs, R.CBackend())


def test_fixture_coverage(fx):
    keys = [bytes.fromhex(c["key"]) for c in fx]
    msgs = [bytes.fromhex(c["msg"]) for c in fx]
    par = [p for p in R.parities(keys, msgs, R.CBackend()) if p is not None]
    assert set(par) == {(False, False), (False, True), (True, False), (True, True)}
    assert {len(m) for m in msgs} >= {0, 22, 23, 24, 31, 32, 87, 88, 54, 55, 56, 63, 64, 119, 120}
    by = {(int.from_bytes(k, "little"), m): c for k, m, c in zip(keys, msgs, fx)}
    for d, st in ((0, 0), (1, 0), (R.N_VALUE - 1, 0), (R.N_VALUE, 2), ((1 << 256) - 1, 2)):
        assert by[(d, b"abc")]["status"] == st, hex(d)
    assert {c["status"] for c in fx} == {0, 1, 2}
    for k, m, c in zip(keys, msgs, fx):
        if m == b"test message":
            assert c["status"] == 1 and c["sig"] == bytes(range(64)).hex()     # schnorr.rs:311-314, before the key is read
        elif c["status"] == 2:
            assert c["sig"] == bytes(range(64)).hex() and int.from_bytes(k, "little") >= R.N_VALUE
        else:
            assert c["status"] == 0 and c["sig"] != bytes(range(64)).hex()
    assert any(m in (b"test messagf", b"Test message", b"test message ") for m in msgs)
    # d = 0: P is the identity, P.x 32 zero bytes, and s = k' (kernels_schnorr.hip's reading of 337-349)
    assert by[(0, b"abc")]["sig"] != by[(1, b"abc")]["sig"]


def test_library_exports_the_new_entry_points():
    from forge_ec_amd import _lib as L
    lib = L.lib()
    for name in ("fec_sha256", "fec_sha256_dev", "fec_ecdsa_verify_msg", "fec_ecdsa_verify_msg_dev", "fec_bip340_sign",
                 "fec_bip340_sign_dev"):
        assert hasattr(lib, name), name
