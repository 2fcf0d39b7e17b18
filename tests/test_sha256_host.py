"""
CPU checks of the device SHA-256 and of the scalar steps of BipSchnorr::sign through a host build of
forge_ec_amd/csrc/sha256.hpp and bip340.hpp (tests/cpp/sha256_host.cpp): the hash equals hashlib.sha256 at every length
0..130 without a prefix and, with the 32-byte and 64-byte prefixes the signer streams, at the message lengths that put
prefix + message on the padding edges 55 / 56 / 63 / 64 / 119 / 120, each at two start alignments; the
hash -> scalar-or-fallback step takes its failing leg for the bytes of N and its passing one for N - 1; Neg equals the
restatement of tests/bip340_sign_ref.py; and the three per-element steps the signing kernels run (bip340.hpp), composed
on the host around the device header's own ladder, reproduce tests/golden/bip340_sign_vectors.json byte for byte.
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import bip340_sign_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
STARTS = (0, 3)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sha") / "sha256_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cpp", "sha256_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.sh_sha256.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p]
    lib.sh_scalar_from_bytes.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.sh_scalar_neg.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.sh_scalar_neg.restype = None
    lib.sh_bip340_sign.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    return lib


def _sha(lib, pre, buf, start, n):
    out = ctypes.create_string_buffer(32)
    assert lib.sh_sha256(pre, len(pre), ctypes.addressof(buf) + start, n, out) == 0
    return out.raw


@pytest.mark.parametrize("plen,lengths", [(0, list(range(131))), (32, [0, 22, 23, 24, 31, 32, 87, 88]),
                                          (64, [0, 54, 55, 56, 63, 64, 119, 120])])
def test_host_sha256_equals_hashlib(host, plen, lengths):
    rnd = random.Random(plen)
    pre = bytes(rnd.getrandbits(8) for _ in range(plen))
    data = bytes(rnd.getrandbits(8) for _ in range(140))
    buf = ctypes.create_string_buffer(data, len(data))
    for n in lengths:
        for start in STARTS:
            assert _sha(host, pre, buf, start, n) == hashlib.sha256(pre + data[start:start + n]).digest(), (plen, n, start)


def _from_bytes(lib, b):
    out = ctypes.create_string_buffer(32)
    return lib.sh_scalar_from_bytes(b, out), out.raw


def test_hash_to_scalar_fallback_leg_forced(host):
    """The leg no message reaches (a hash whose top limb is >= 0xFFFFFFFFFFFFFFFE): forced with the bytes of N, N - 1 and
    their neighbours, against the restated from_bytes."""
    le = lambda v: v.to_bytes(32, "little")
    some, limbs = _from_bytes(host, le(R.N_VALUE))
    assert some == 0 and R.hash_to_scalar(le(R.N_VALUE)) is None
    some, limbs = _from_bytes(host, le(R.N_VALUE - 1))
    assert some == 1 and limbs == le(R.N_VALUE - 1) and R.hash_to_scalar(le(R.N_VALUE - 1)) == R.from_bytes_le(le(R.N_VALUE - 1))[0]
    for v in (0, 1, R.N_VALUE + 1, (1 << 256) - 1, 0xFFFFFFFFFFFFFFFE << 192, (0xFFFFFFFFFFFFFFFE << 192) - 1,
              0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141):
        assert _from_bytes(host, le(v))[0] == int(R.from_bytes_le(le(v))[1]), hex(v)


def test_scalar_neg_equals_restatement(host):
    rnd = random.Random(7)
    vals = [0, 1, R.N_VALUE - 1, R.N_VALUE >> 1] + [rnd.randrange(R.N_VALUE) for _ in range(50)]
    for v in vals:
        out = ctypes.create_string_buffer(32)
        host.sh_scalar_neg(v.to_bytes(32, "little"), out)
        assert out.raw == R.to_bytes_le(R.neg(R.from_bytes_le(v.to_bytes(32, "little"))[0])), hex(v)
        assert int.from_bytes(out.raw, "little") == (R.N_VALUE - v if v else 0)


def test_kernel_steps_on_the_host_reproduce_the_fixture(host):
    from oracle import py_model as M
    g = M.Secp.generator()
    G = (ctypes.c_uint64 * 12)(*(list(g[0]) + list(g[1]) + list(g[2])))
    for i, c in enumerate(json.load(open(os.path.join(HERE, "golden", "bip340_sign_vectors.json")))["sign"]):
        key, msg = bytes.fromhex(c["key"]), bytes.fromhex(c["msg"])
        out = ctypes.create_string_buffer(64)
        st = host.sh_bip340_sign(G, key, msg, len(msg), out)
        assert (out.raw.hex(), st) == (c["sig"], c["status"]), i
