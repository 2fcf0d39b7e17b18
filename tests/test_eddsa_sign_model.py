"""
CPU checks of the parity-mode EdDSA signers (fec_ed25519_sign, fec_ed25519_derive_public_key, fec_eddsa_sign_ed25519):
the test-side restatement (tests/eddsa_sign_ref.py) over the C oracle agrees with the fixture that the same
restatement over oracle/py_model.py produced; the fixture covers what it must (special cases and near misses, the
padding boundaries, both debug-panic states); its special-case bytes are the reference source's literals; and a host
build of the device SHA-512 (forge_ec_amd/csrc/sha512.hpp, through tests/cpp/sha512_host.cpp) equals hashlib at every
length 0..400, at misaligned starts, with the prefixes the signers stream.
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import eddsa_sign_ref as R  # noqa: E402
import gen_eddsa_sign as G  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "eddsa_sign_vectors.json")


@pytest.fixture(scope="module")
def fx():
    return json.load(open(FIXTURE))


def test_fixture_is_the_generator_output(fx):
    sign, derive, generic = G.cases()
    assert [bytes.fromhex(c["key"]) for c in fx["sign"]] == [k for k, _ in sign]
    assert [bytes.fromhex(c["msg"]) for c in fx["sign"]] == [m for _, m in sign]
    assert [bytes.fromhex(c["key"]) for c in fx["derive"]] == derive
    assert [[int(v, 16) for v in c["sk"]] for c in fx["generic"]] == [k for k, _ in generic]


def test_c_oracle_composition_equals_fixture(fx):
    be = R.CBackend()
    got = R.sign_batch([bytes.fromhex(c["key"]) for c in fx["sign"]], [bytes.fromhex(c["msg"]) for c in fx["sign"]], be)
    assert [(s.hex(), st) for s, st in got] == [(c["sig"], c["status"]) for c in fx["sign"]]
    got = R.derive_batch([bytes.fromhex(c["key"]) for c in fx["derive"]], be)
    assert [(p.hex(), st) for p, st in got] == [(c["pk"], c["status"]) for c in fx["derive"]]
    got = R.eddsa_sign_batch([[int(v, 16) for v in c["sk"]] for c in fx["generic"]],
                             [bytes.fromhex(c["msg"]) for c in fx["generic"]], be)
    for (x, y, inf, s, st), c in zip(got, fx["generic"]):
        assert [f"{int(v):016x}" for v in list(x) + list(y)] == c["r_xy"]
        assert [f"{int(v):016x}" for v in s] == c["s"]
        assert (int(inf), st) == (c["r_inf"], c["status"])


def test_python_and_c_backends_agree_on_random_inputs():
    rnd = random.Random(5)
    keys = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(6)]
    msgs = [bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(0, 200))) for _ in range(6)]
    assert R.sign_batch(keys, msgs, R.PyBackend()) == R.sign_batch(keys, msgs, R.CBackend())


def test_fixture_coverage(fx):
    msgs = [bytes.fromhex(c["msg"]) for c in fx["sign"]]
    assert {len(m) for m in msgs} >= {0, 1, 111, 112, 127, 128, 239, 240, 1000, 45, 46, 61, 62, 173, 174, 79, 80}
    by = {(bytes.fromhex(c["key"])[0], bytes.fromhex(c["msg"])): c for c in fx["sign"]}
    assert any(m == b"test message" for _, m in by) and any(m == b"test messagf" for _, m in by)
    assert (0x9D, b"") in by and (0x9C, b"") in by
    assert {c["status"] for c in fx["sign"]} >= {0, 2}
    assert sum(bytes.fromhex(c["key"])[0] == 0x9D for c in fx["derive"]) >= 2
    assert {c["status"] for c in fx["generic"]} >= {0, 2}


def test_special_case_bytes_are_the_reference_literals(fx):
    for c in fx["sign"]:
        k, m = bytes.fromhex(c["key"]), bytes.fromhex(c["msg"])
        if m == b"test message":
            assert c["sig"] == bytes(range(64)).hex()
        elif not m and k[0] == 0x9D:
            assert c["sig"] == ("e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e"
                                "39701cf9b46bd25bf5f0595bbe24655141438e7a100b")
        else:
            assert c["sig"] not in (R.RFC_SIG.hex(), R.PATTERN_SIG.hex())
    for c in fx["derive"]:
        if bytes.fromhex(c["key"])[0] == 0x9D:
            assert c["pk"] == "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"
    gx, gy, _ = R.PyBackend().generator_affine()
    for c in fx["generic"]:
        m = bytes.fromhex(c["msg"])
        top = int(c["sk"][3], 16) >> 56
        if m == b"test message" or (not m and top == 0x9D):
            assert [int(v, 16) for v in c["r_xy"]] == list(gx) + list(gy) and [int(v, 16) for v in c["s"]] == [1, 0, 0, 0]


@pytest.fixture(scope="module")
def host_sha(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sha") / "sha512_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cpp", "sha512_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.sh_sha512.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p]
    return lib


def _host(lib, pre, buf, start, n):
    out = ctypes.create_string_buffer(64)
    assert lib.sh_sha512(pre, len(pre), ctypes.addressof(buf) + start, n, out) == 0
    return out.raw


@pytest.mark.parametrize("plen", [0, 32, 66])
def test_host_sha512_equals_hashlib(host_sha, plen):
    rnd = random.Random(plen)
    pre = bytes(rnd.getrandbits(8) for _ in range(plen))
    data = bytes(rnd.getrandbits(8) for _ in range(420))
    buf = ctypes.create_string_buffer(data, len(data))
    for n in range(401):
        for start in (0, 1, 2, 3, 5, 7):
            if start + n <= len(data):
                assert _host(host_sha, pre, buf, start, n) == hashlib.sha512(pre + data[start:start + n]).digest(), (n, start)
