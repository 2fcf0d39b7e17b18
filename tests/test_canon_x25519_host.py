"""
CPU checks of the canonical-mode X25519 device code through a host build of forge_ec_amd/csrc/canon_x25519.hpp
(tests/cpp/canon_x25519_host.cpp), the per-element code the kernels run: the ladder over the whole fixture
tests/golden/canon_x25519_vectors.json and the RFC's 1000-step chain, mul_small against a * 121665 mod p on edge values
(0, 1, p - 1, values whose fold lands in [p, 2^255), where the field's finishing leg must run) and random ones, and the
public key through the Ed25519 scanned comb and the birational map against the ladder at u = 9.  The same source builds as a
stand-alone program (-DCANON_X25519_HOST_MAIN), which is run once here; built with -fsanitize=address,undefined it is the
sanitizer run of this code (not run by this file):
    g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DCANON_X25519_HOST_MAIN \
        -o canon_x25519_host_san tests/cpp/canon_x25519_host.cpp && ./canon_x25519_host_san
"""
import ctypes
import json
import os
import random
import subprocess

import pytest

import canon_x25519_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_x25519_vectors.json")))
SRC = os.path.join(HERE, "cpp", "canon_x25519_host.cpp")
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_x25519") / "canon_x25519_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.cx_ced_finish_count.restype = ctypes.c_ulong
    return lib


def _x25519(host, k, u):
    out = (ctypes.c_uint8 * 32)()
    st = host.cx_x25519(k, u, out)
    return bytes(out), st


def _base(host, k):
    out = (ctypes.c_uint8 * 32)()
    host.cx_x25519_base(k, out)
    return bytes(out)


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "canon_x25519_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DCANON_X25519_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


def test_every_fixture_case(host):
    cases = FIXTURE["cases"]
    n = len(cases)
    ks = b"".join(bytes.fromhex(c["k"]) for c in cases)
    us = b"".join(bytes.fromhex(c["u"]) for c in cases)
    out, st = (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * n)()
    host.cx_x25519_batch.restype = SZ
    assert host.cx_x25519_batch(SZ(n), ks, us, out, st) == n
    out = bytes(out)
    for i, c in enumerate(cases):
        assert (out[32 * i:32 * i + 32].hex(), st[i]) == (c["out"], c["status"]), (c["class"], c["name"])
    assert sum(s == X.ZERO_SHARED for s in st) == 14 + 2      # the low-order class, and p, p + 1 among the non-canonical


def test_chain_of_1000(host):
    out = (ctypes.c_uint8 * 32)()
    host.cx_chain(SZ(1), out)
    assert bytes(out).hex() == X.ITERATED_1
    host.cx_chain(SZ(1000), out)
    assert bytes(out).hex() == X.ITERATED_1000 == FIXTURE["iterated_1000"]


def test_mul_small(host):
    """a * 121665 mod p.  a = v / 121665 mod p for v = 1 .. 18 has a * 121665 = v + m p with m >= 1, which the fold with
    2^255 = 19 brings to p + v -- inside [p, 2^255), so the finishing leg has to run; the counter says that it did."""
    rng = random.Random(22)
    inv = pow(X.A24, X.P - 2, X.P)
    folds = [v * inv % X.P for v in range(1, 19)]
    edge = [0, 1, 2, X.P - 1, X.P - 2, (1 << 255) // X.A24, (1 << 255) // X.A24 + 1, (1 << 254), (1 << 224) - 1]
    before = host.cx_ced_finish_count()
    for a in folds:
        out = (ctypes.c_uint8 * 32)()
        host.cx_mul_small(a.to_bytes(32, "little"), X.A24, out)
        assert int.from_bytes(bytes(out), "little") == a * X.A24 % X.P < 19
    assert host.cx_ced_finish_count() - before == len(folds)
    for a in edge + [rng.randrange(X.P) for _ in range(200)]:
        for k in (X.A24, 1, 0, 0xFFFFFFFF):
            out = (ctypes.c_uint8 * 32)()
            host.cx_mul_small(a.to_bytes(32, "little"), k, out)
            assert int.from_bytes(bytes(out), "little") == a * k % X.P, (hex(a), k)


def test_public_key_by_comb_and_map(host):
    """clamp -> scanned Ed25519 comb -> (Z + Y) / (Z - Y) against the ladder at u = 9 and the model: the edge scalars of the
    fixture's clamp class, single bits, and 200 random scalars"""
    rng = random.Random(23)
    ks = [bytes.fromhex(c["k"]) for c in FIXTURE["cases"] if c["class"] in ("clamp", "published")]
    ks += [bytes(32), b"\xff" * 32, (X.P).to_bytes(32, "little")]
    ks += [(1 << b).to_bytes(32, "little") for b in (0, 2, 3, 4, 127, 128, 253, 254, 255)]
    ks += [bytes(rng.randrange(256) for _ in range(32)) for _ in range(200)]
    for i, k in enumerate(ks):
        got = _base(host, k)
        assert got == _x25519(host, k, X.BASE_U)[0], k.hex()
        if i % 8 == 0 or i < 40:
            assert got == X.x25519_base(k), k.hex()
    d = X.DH
    assert _base(host, bytes.fromhex(d["a"])).hex() == d["A"] and _base(host, bytes.fromhex(d["b"])).hex() == d["B"]


def test_clamp_and_decoding(host):
    """bits the clamp overrides and bit 255 of u change nothing; a non-canonical u is its reduction"""
    rng = random.Random(24)
    for _ in range(8):
        k, u = bytearray(rng.randrange(256) for _ in range(32)), bytearray(rng.randrange(256) for _ in range(32))
        want = _x25519(host, bytes(k), bytes(u))
        assert want == X.x25519_status(bytes(k), bytes(u))
        k2, u2 = bytearray(k), bytearray(u)
        k2[0] ^= 7
        k2[31] ^= 0xC0
        u2[31] ^= 0x80
        assert _x25519(host, bytes(k2), bytes(u2)) == want
    k = bytes(rng.randrange(256) for _ in range(32))
    for v in range(2, 19):
        assert _x25519(host, k, (X.P + v).to_bytes(32, "little")) == _x25519(host, k, v.to_bytes(32, "little"))
