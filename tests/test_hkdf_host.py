"""
CPU checks of the device key derivation through a host build of forge_ec_amd/csrc/hkdf.hpp (tests/cpp/hkdf_host.cpp),
the per-element code k_derive_key runs: it reproduces every derive_key case of tests/golden/ecdh_kdf_vectors.json and
RFC 5869's A.3 output, and over the same grid of lengths it equals hashlib / hmac on fresh inputs, several rows per call
so that rows of an odd length start at every byte alignment, with guard bytes behind the rows.
(The same source builds as a stand-alone program, -DHKDF_HOST_MAIN, for a sanitizer run: DESIGN.md section 17.)
"""
import ctypes
import hashlib
import hmac
import json
import os
import random
import subprocess

import pytest

import ecdh_kdf_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "ecdh_kdf_vectors.json")))
GUARD = 64


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hkdf") / "hkdf_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cpp", "hkdf_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.hh_derive_key.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                  ctypes.c_void_p, ctypes.c_size_t]
    return lib


def _derive(lib, curve, secrets, info, out_len):
    """-> the n key rows; asserts that the guard behind them is untouched.  The rows start 16-byte aligned."""
    n, sl = len(secrets), len(secrets[0])
    sec = ctypes.create_string_buffer(b"".join(secrets), max(n * sl, 1))
    raw = ctypes.create_string_buffer(b"\xA5" * (n * out_len + GUARD + 16), n * out_len + GUARD + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    shift = base - ctypes.addressof(raw)
    inf = ctypes.create_string_buffer(info, max(len(info), 1))
    assert lib.hh_derive_key(curve, ctypes.addressof(sec) if sl else None, sl, ctypes.addressof(inf) if info else None, len(info), out_len,
                             base, n) == 0
    got = raw.raw[shift:shift + n * out_len]
    assert raw.raw[shift + n * out_len:shift + n * out_len + GUARD] == b"\xA5" * GUARD
    return [got[i * out_len:(i + 1) * out_len] for i in range(n)]


def test_rfc5869_a3(host):
    assert _derive(host, 0, [K.A3_IKM], b"", K.A3_L) == [K.A3_OKM]


def test_host_build_reproduces_every_fixture_case(host):
    sp, ip = bytes.fromhex(FIXTURE["secret_pool"]), bytes.fromhex(FIXTURE["info_pool"])
    for curve, s, i, o, okm in FIXTURE["derive_key"]:
        assert _derive(host, curve, [sp[:s]], ip[:i], o) == [bytes.fromhex(okm)], (curve, s, i, o)


@pytest.mark.parametrize("curve", [0, 1])
def test_host_build_equals_hashlib_over_the_grid(host, curve):
    rnd = random.Random(5869 + curve)
    for s in K.SECRET_LENS:
        for i in K.INFO_LENS:
            for o in K.OUT_LENS + (48, 56, 60):              # and the 16-, 8- and 4-byte store classes
                secrets = [bytes(rnd.getrandbits(8) for _ in range(s)) for _ in range(5)]
                info = bytes(rnd.getrandbits(8) for _ in range(i))
                want = [K.derive_key(curve, x, info, o) for x in secrets]
                if curve == 0 and o:
                    prk = hmac.new(bytes(32), secrets[0], hashlib.sha256).digest()
                    assert want[0][:32] == hmac.new(prk, info + b"\x01", hashlib.sha256).digest()[:o]
                assert _derive(host, curve, secrets, info, o) == want, (s, i, o)


def test_lengths_the_abi_refuses(host):
    for args in ((65, 0, 32), (0, 1025, 32), (0, 0, 8129)):
        assert host.hh_derive_key(0, None, args[0], None, args[1], args[2], None, 0) == -1
