"""
CPU checks of the device RFC 6979 chain through a host build of forge_ec_amd/csrc/rfc6979.hpp
(tests/cpp/rfc6979_host.cpp), the per-element code k_rfc6979 runs: it reproduces every nonce of
tests/golden/rfc6979_vectors.json and the reference's three recorded ones; its constant pad states of the key 0 are the
two compressions they stand for; and, with the comparison constant lowered to 2^255 -- about half of all candidates then
fail, which neither real constant ever shows -- 256 seeded (key, message) pairs equal the restatement of
tests/rfc6979_ref.py under the same constant, retries included.
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import rfc6979_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "rfc6979_vectors.json")))
U64x4 = ctypes.c_uint64 * 4
RETRY_SEED = 6979     # gives 122 / 65 of 256 pairs with >= 1 / >= 2 retries under 2^255, 11 at most (asserted below)


def retry_pairs(n=256, seed=RETRY_SEED):
    """The seeded (key limbs, message) pairs of the lowered-constant tests (tests/test_gpu_rfc6979.py uses them too):
    arbitrary 256-bit keys, message lengths 0..150."""
    rnd = random.Random(seed)
    return [(R.E._limbs(rnd.getrandbits(256)), bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(151)))) for _ in range(n)]


def assert_retry_mix(retries):
    """At least 25 % of the pairs retry once or more and at least 10 % twice or more: the test cannot pass by never
    retrying.  (Each candidate fails with probability 1/2 under 2^255: expected 50 % and 25 %.)"""
    n = len(retries)
    assert sum(r >= 1 for r in retries) * 4 >= n and sum(r >= 2 for r in retries) * 10 >= n, retries


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rfc") / "rfc6979_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cpp", "rfc6979_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.rh_generate_k.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p]
    return lib


def _k(lib, sk, msg, order, start=0):
    buf = ctypes.create_string_buffer(b"\0" * start + msg, start + len(msg) + 1)
    k, digest = U64x4(), ctypes.create_string_buffer(32)
    st = lib.rh_generate_k(U64x4(*sk), ctypes.addressof(buf) + start, len(msg), U64x4(*R.E._limbs(order)), k, digest)
    assert digest.raw == hashlib.sha256(msg).digest()
    return list(k), st


def test_zero_key_pad_states(host):
    assert host.rh_zero_key_pads_ok() == 1


def test_host_build_reproduces_the_recorded_reference_nonces(host):
    for c in FIXTURE["recorded"]:
        assert _k(host, c["sk"], bytes.fromhex(c["msg"]), R.ORDER[0]) == (c["k"], 0)


@pytest.mark.parametrize("curve", [0, 1])
def test_host_build_reproduces_every_fixture_nonce(host, curve):
    for i, c in enumerate(x for x in FIXTURE["cases"] if x["curve"] == curve):
        assert _k(host, c["sk"], bytes.fromhex(c["msg"]), R.ORDER[curve], start=i % 4) == (c["k"], 0), i


def test_retry_leg_under_a_lowered_constant(host):
    order = 1 << 255
    pairs = retry_pairs()
    want = [R.generate_k(sk, msg, order) for sk, msg in pairs]
    assert_retry_mix([r for _, r in want])
    for (sk, msg), (k, _) in zip(pairs, want):
        assert _k(host, sk, msg, order) == (R.E._limbs(k), 0)


def test_retry_cap(host):
    """A constant no candidate is below: the loop stops after 128 retries with k = 0 and status 5.  (The ABI refuses
    such a constant -- fec_debug_rfc6979_k wants at least 2^254 -- so only the host build can show the cap.)"""
    sk, msg = retry_pairs(1)[0]
    assert _k(host, sk, msg, 1) == ([0, 0, 0, 0], 5)
    assert R.generate_k(sk, msg, 1) == (0, R.MAX_RETRIES + 1)
