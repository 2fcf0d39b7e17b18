"""
CPU checks of the canonical-mode Keccak-256, recovery and recovery-id device code through a host build of
forge_ec_amd/csrc/keccak.hpp and canon_recover.hpp (tests/cpp/canon_recover_host.cpp), the per-element code the kernels run:
the whole fixture tests/golden/canon_recover_vectors.json -- every Keccak message at its alignment, every recovery case in
every output form through the prepare group and the finish step, every signing case's recovery id -- the sponge against
hashlib.sha3_256 at the domain byte 0x06, and the recovery id fed x >= n directly, which no real signature reaches.
The same source builds as a stand-alone program (-DCANON_RECOVER_HOST_MAIN), which is run once here; built with
-fsanitize=address,undefined it is the sanitizer run of this code (not run by this file):
    g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DCANON_RECOVER_HOST_MAIN \
        -o canon_recover_host_san tests/cpp/canon_recover_host.cpp && ./canon_recover_host_san
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import canon_msg_ref as R
import canon_recover_ref as K
import canon_sign_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_recover_vectors.json")))
SRC = os.path.join(HERE, "cpp", "canon_recover_host.cpp")
SZ = ctypes.c_size_t
CURVES = sorted(R.WEIERSTRASS)


def expected(case, out_len):
    """the record of one fixture case in one output form, from its key33 / address"""
    if case["status"]:
        return bytes(out_len)
    if out_len == 20:
        return bytes.fromhex(case["address"])
    pt = R.sec1_decode(R.WEIERSTRASS[case["curve"]], bytes.fromhex(case["key33"]))
    return K.encode(pt, out_len)


def forms(curve):
    return (33, 65, 64, 20) if curve == "secp256k1" else (33, 65, 64)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_recover") / "canon_recover_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.cr_recid.restype = ctypes.c_uint
    lib.cr_rs_flags.restype = ctypes.c_uint
    return lib


def _keccak(host, msg, al, domain=1):
    out = (ctypes.c_uint8 * 32)()
    host.cr_keccak(msg, SZ(len(msg)), SZ(al), ctypes.c_uint(domain), out)
    return bytes(out)


def _recover(host, curve, cases, out_len):
    n = len(cases)
    dg = b"".join(bytes.fromhex(c["digest"]) for c in cases)
    sg = b"".join(bytes.fromhex(c["sig"]) for c in cases)
    rc = bytes(c["recid"] for c in cases)
    out, st = (ctypes.c_uint8 * (out_len * n))(), (ctypes.c_uint8 * n)()
    host.cr_recover(R.CURVE_IDS[curve], SZ(n), dg, sg, rc, out_len, out, st)
    out = bytes(out)
    return [out[out_len * i:out_len * (i + 1)] for i in range(n)], list(st)


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "canon_recover_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DCANON_RECOVER_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


def test_keccak_fixture(host):
    buf = bytes.fromhex(FIXTURE["keccak_buffer"])
    assert {c["len"] for c in FIXTURE["keccak"]} >= set(K.KECCAK_LENGTHS)
    for c in FIXTURE["keccak"]:
        msg = buf[c["at"]:c["at"] + c["len"]]
        assert _keccak(host, msg, c["at"]).hex() == c["digest"], (c["len"], c["at"])


def test_sponge_is_sha3_256_at_domain_6(host):
    rng = random.Random(0x5A4)
    for n in K.KECCAK_LENGTHS + [rng.randrange(0, 700) for _ in range(64)]:
        msg = bytes(rng.randrange(256) for _ in range(n))
        assert _keccak(host, msg, rng.randrange(4), 6) == hashlib.sha3_256(msg).digest(), n
        assert _keccak(host, msg, rng.randrange(4), 1) == K.keccak256(msg), n


def test_keccak_of_64_bytes_in_registers(host):
    rng = random.Random(0x5A5)
    for _ in range(8):
        msg = bytes(rng.randrange(256) for _ in range(64))
        out = (ctypes.c_uint8 * 32)()
        host.cr_keccak64(msg, out)
        assert bytes(out) == K.keccak256(msg)


@pytest.mark.parametrize("curve", CURVES)
def test_every_recovery_case(host, curve):
    """the whole fixture as one batch per output form: the refused cases sit among the ordinary ones and share their groups"""
    cases = [c for c in FIXTURE["cases"] if c["curve"] == curve]
    assert len(cases) >= 150 and {c["class"] for c in cases} == {"sign", "recid", "range", "digest", "infinity", "doubling", "bit1", "off-curve"}
    for out_len in forms(curve):
        out, st = _recover(host, curve, cases, out_len)
        for c, o, s in zip(cases, out, st):
            assert (o, s) == (expected(c, out_len), c["status"]), (c["class"], c["name"], out_len)


@pytest.mark.parametrize("curve", CURVES)
def test_signing_cases_recids(host, curve):
    """the finish pass of the recoverable signer on the model's nonces: the fixture's signatures and ids"""
    C = R.WEIERSTRASS[curve]
    cases = [c for c in FIXTURE["cases"] if c["curve"] == curve and c["class"] == "sign"][:40]
    n = len(cases)
    for flags in (0, S.LOW_S):
        sel = [c for c in cases if c["flags"] == flags]
        dg = b"".join(bytes.fromhex(c["digest"]) for c in sel)
        keys = b"".join(bytes.fromhex(c["key"]) for c in sel)
        ks = b"".join(S.rfc6979_k(C.N, int(c["key"], 16), bytes.fromhex(c["digest"])).to_bytes(32, "big") for c in sel)
        m = len(sel)
        sigs, rec, st = (ctypes.c_uint8 * (64 * m))(), (ctypes.c_uint8 * m)(), (ctypes.c_uint8 * m)()
        host.cr_sign(R.CURVE_IDS[curve], SZ(m), dg, keys, ks, flags, sigs, rec, st)
        assert bytes(sigs).hex() == "".join(c["sig"] for c in sel) and list(rec) == [c["recid"] for c in sel] and not any(st)
    assert n == 40 and {c["recid"] for c in cases} == {0, 1}


def test_recid_bit_1(host):
    """x(kG) >= n: bit 1 of the id, and r = x - n"""
    assert [host.cr_recid(y, f, x) for x in (0, 1) for f in (0, 1) for y in (6, 7)] == [K.recid_of(y, f, x) for x in (0, 1) for f in (0, 1) for y in (0, 1)]
    for curve, C in R.WEIERSTRASS.items():
        for x in (C.N - 1, C.N, C.N + 1, C.P - 1, 1):
            r = (ctypes.c_uint8 * 32)()
            fl = host.cr_rs_flags(R.CURVE_IDS[curve], x.to_bytes(32, "little"), r)
            assert (fl & 1, int.from_bytes(bytes(r), "little")) == (int(x >= C.N), x % C.N), (curve, hex(x))
