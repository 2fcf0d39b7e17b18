"""
CPU checks of the device code of Schnorr::<C, Sha256>::sign's hash, challenge and from_bytes_reduced through a host build
of forge_ec_amd/csrc/sha256.hpp + schnorr_sign.hpp (tests/cpp/schnorr_sign_host.cpp), the per-element code the kernels run:
hash_prefixed with the 66-byte prefix -- which runs two bytes into the second block -- equals hashlib at every fixture
message length and all four message alignments; with the 64-byte prefix it still equals hashlib at the lengths
tests/test_sha256_host.py uses; every from_bytes_reduced entry of tests/golden/schnorr_sign_vectors.json matches, with its
leg; every challenge entry matches.
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import schnorr_sign_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = S.load_fixture()
SOURCE = os.path.join(HERE, "cpp", "schnorr_sign_host.cpp")
LEGS = {0: "direct", 1: "nosub", 2: "nosub_zero", 3: "sub", 4: "sub_zero", 5: "reduce_wide"}   # schnorr_sign.hpp: LEG_*
LENGTHS = (0, 1, 2, 53, 54, 61, 62, 63, 117, 118, 126, 200, 12)                                # the fixture's, "test message" last
U64x4, U64x8 = ctypes.c_uint64 * 4, ctypes.c_uint64 * 8


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("schnorr") / "schnorr_sign_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SOURCE])
    lib = ctypes.CDLL(so)
    lib.sh_hash_prefixed.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p]
    lib.sh_hash_prefixed.restype = None
    lib.sh_from_bytes_reduced.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p]
    lib.sh_challenge.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                 ctypes.c_void_p]
    return lib


def _hash(lib, pw, pre, buf, start, n):
    out = ctypes.create_string_buffer(32)
    lib.sh_hash_prefixed(pw, pre, len(pre), ctypes.addressof(buf) + start, n, out)
    return out.raw


def test_fixture_lengths_are_the_ones_tested():
    assert sorted({len(c["msg"]) // 2 for c in FIXTURE["sign"]}) == sorted(LENGTHS)


@pytest.mark.parametrize("pw,plen,lengths", [(17, 66, LENGTHS), (17, 65, [0, 1, 54, 55, 63, 119]), (17, 68, [0, 51, 52, 60, 124]),
                                             (16, 64, [0, 54, 55, 56, 63, 64, 119, 120])])
def test_hash_prefixed_equals_hashlib(host, pw, plen, lengths):
    rnd = random.Random(plen)
    pre = bytes(rnd.getrandbits(8) for _ in range(plen))
    data = bytes(rnd.getrandbits(8) for _ in range(208))
    buf = ctypes.create_string_buffer(data, len(data))
    for n in lengths:
        for start in range(4):
            assert _hash(host, pw, pre, buf, start, n) == hashlib.sha256(pre + data[start:start + n]).digest(), (plen, n, start)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_every_from_bytes_reduced_entry_with_its_leg(host, curve):
    rows = [c for c in FIXTURE["reduced"] if c["curve"] == curve]
    seen = set()
    for c in rows:
        out = U64x4()
        leg = host.sh_from_bytes_reduced(curve, bytes.fromhex(c["bytes"]), out)
        assert (list(out), LEGS[leg]) == (c["out"], c["leg"]), c["bytes"]
        seen.add(LEGS[leg])
    assert len(rows) >= 24 and seen == {c["leg"] for c in rows}


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_every_challenge_entry(host, curve):
    rows = [c for c in FIXTURE["challenge"] if c["curve"] == curve]
    assert len(rows) == 24
    for i, c in enumerate(rows):
        msg = bytes.fromhex(c["msg"])
        start = i % 4
        buf = ctypes.create_string_buffer(b"\0" * start + msg, start + len(msg) + 1)
        e = U64x4()
        leg = host.sh_challenge(curve, U64x8(*c["r_xy"]), c["r_inf"], U64x8(*c["pk_xy"]), c["pk_inf"], ctypes.addressof(buf) + start, len(msg), e)
        assert (list(e), LEGS[leg]) == (c["e"], c["leg"]), i


@pytest.mark.parametrize("curve", [0, 1])
def test_the_signers_challenges(host, curve):
    """The challenge of every computed signature of the fixture from its R and P = multiply(G, sk): P's limbs come from the
    C oracle, R's from the fixture."""
    import numpy as np
    from oracle import c_oracle
    rows = [c for c in FIXTURE["sign"] if c["curve"] == curve and c["status"] == 0]
    pts = c_oracle.batch_mul_fixed(curve, np.array([c["sk"] for c in rows], dtype=np.uint64), c_oracle.generator(curve), nthreads=8)
    p_xy, p_inf = c_oracle.batch_to_affine(curve, pts, nthreads=8)
    for i, c in enumerate(rows):
        msg = bytes.fromhex(c["msg"])
        buf = ctypes.create_string_buffer(msg, len(msg) + 1)
        e = U64x4()
        host.sh_challenge(curve, U64x8(*c["r_xy"]), c["r_inf"], U64x8(*[int(v) for v in p_xy[i]]), int(p_inf[i]), ctypes.addressof(buf), len(msg), e)
        assert list(e) == c["e"], i
