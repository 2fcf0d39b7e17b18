"""
CPU checks of the canonical-mode from-the-message device code through a host build of forge_ec_amd/csrc/canon_msg.hpp
(tests/cpp/canon_msg_host.cpp), the per-element code the k_canon_*_prepare_msg kernels and k_canon_decompress run:
the constant state after the BIP-340 tag block, the BIP-340 and Ed25519 challenges of every fixture case, reduce512
against Python integers, SEC 1 decoding of every fixture key at every byte alignment, and what the three prepare steps
hand the verifier (the point, u2, the flag) against the model tests/canon_msg_ref.py.  The same source builds as a
stand-alone program (-DCANON_MSG_HOST_MAIN), which is run once here.
"""
import ctypes
import hashlib
import json
import os
import random
import struct
import subprocess

import pytest

import canon_msg_ref as R
from oracle import canon_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_msg_vectors.json")))
SRC = os.path.join(HERE, "cpp", "canon_msg_host.cpp")
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_msg") / "canon_msg_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    return ctypes.CDLL(so)


def _cases(scheme, curve=None, pk_len=None):
    for b in FIXTURE["batches"]:
        if b["scheme"] == scheme and curve in (None, b["curve"]) and pk_len in (None, b["pk_len"]):
            for c in b["cases"]:
                yield bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"]), c["want"], c["name"]
    for name, c in FIXTURE["published"].items():
        if c["scheme"] == scheme and curve in (None, c["curve"]) and pk_len in (None, c["pk_len"]):
            yield bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"]), c["want"], name


def _limbs(n=4):
    return (ctypes.c_uint64 * n)()


def _int(l, at=0):
    return M.unlimbs(list(l)[at:at + 4])


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "canon_msg_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DCANON_MSG_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


# FIPS 180-4 compression in Python, pinned by hashlib below: hashlib shows no state between blocks
_K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
      0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
      0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
      0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
      0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def _compress(h, blk):
    m32 = 0xFFFFFFFF
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & m32  # noqa: E731
    w = list(struct.unpack(">16I", blk))
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & m32)
    a, b, c, d, e, f, g, hh = h
    for t in range(64):
        t1 = (hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & m32)) + _K[t] + w[t]) & m32
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & m32
        hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & m32, c, b, a, (t1 + t2) & m32
    return [(x + y) & m32 for x, y in zip(h, [a, b, c, d, e, f, g, hh])]


def test_tag_block_state(host):
    """after_bip340_challenge_tag() is compress(init, T || T): finishing the hash from it by hand gives hashlib's digest."""
    T = hashlib.sha256(b"BIP0340/challenge").digest()
    data = bytes(range(70))
    padded = T + T + data + b"\x80" + bytes((55 - len(data)) % 64) + struct.pack(">Q", (64 + len(data)) * 8)
    st = list(_IV)
    for o in range(0, len(padded), 64):
        st = _compress(st, padded[o:o + 64])
    assert struct.pack(">8I", *st) == hashlib.sha256(T + T + data).digest()      # the Python compression is SHA-256's
    got = (ctypes.c_uint32 * 8)()
    host.cm_bip340_tag_state(got)
    assert list(got) == _compress(list(_IV), T + T)


def test_challenges_of_every_fixture_case(host):
    out = _limbs()
    for i, (msg, sig, pk, _, name) in enumerate(_cases("bip340")):
        for al in ((i % 4,) if len(msg) > 1 else range(4)):
            host.cm_bip340_challenge(sig, pk, msg, SZ(len(msg)), SZ(al), out)
            assert _int(out) == int.from_bytes(R.tagged("BIP0340/challenge", sig[:32] + pk + msg), "big"), name
    for i, (msg, sig, pk, _, name) in enumerate(_cases("ed25519")):
        for al in ((i % 4,) if len(msg) > 1 else range(4)):
            host.cm_ed25519_challenge(sig, pk, msg, SZ(len(msg)), SZ(al), out)
            assert _int(out) == R.ed25519_challenge(sig[:32], pk, msg), name
    for i, (msg, _, _, _, name) in enumerate(_cases("ecdsa", "p256", 33)):
        host.cm_ecdsa_z(msg, SZ(len(msg)), SZ(i % 4), out)
        assert _int(out) == R.ecdsa_z(msg), name


def test_challenges_at_every_length_and_alignment(host):
    """every boundary length of the fixture at all four alignments, whatever order the fixture has them in"""
    rng = random.Random(16)
    out = _limbs()
    for n in sorted(set(FIXTURE["sha256_lengths"] + FIXTURE["sha512_lengths"] + [2, 3, 4, 127, 128, 129, 300])):
        msg, sig, pk = rng.randbytes(n), rng.randbytes(64), rng.randbytes(32)
        for al in range(4):
            host.cm_bip340_challenge(sig, pk, msg, SZ(n), SZ(al), out)
            assert _int(out) == int.from_bytes(R.tagged("BIP0340/challenge", sig[:32] + pk + msg), "big"), (n, al)
            host.cm_ed25519_challenge(sig, pk, msg, SZ(n), SZ(al), out)
            assert _int(out) == R.ed25519_challenge(sig[:32], pk, msg), (n, al)
            host.cm_ecdsa_z(msg, SZ(n), SZ(al), out)
            assert _int(out) == R.ecdsa_z(msg), (n, al)


@pytest.mark.parametrize("name", ["secp256k1", "p256", "ed25519"])
def test_reduce512(host, name):
    order = R.ED.N if name == "ed25519" else R.WEIERSTRASS[name].N
    rng = random.Random(512)
    vals = [0, 1, order - 1, order, order + 1, 2 * order, 2**252, 2**255, 2**256 - 1, 2**256, 2**256 + 1, order << 256,
            (order << 256) - 1, 2**511, 2**512 - 1, (2**256 - 1) << 256] + [rng.randrange(2**512) for _ in range(300)]
    vals += [rng.randrange(2**256) for _ in range(100)]       # the 256-bit case
    out = _limbs()
    for v in vals:
        host.cm_reduce512(R.CURVE_IDS[name], v.to_bytes(64, "little"), out)
        assert _int(out) == v % order, hex(v)


@pytest.mark.parametrize("name", ["secp256k1", "p256"])
@pytest.mark.parametrize("pk_len", [33, 65])
def test_sec1_decoding_of_every_fixture_key(host, name, pk_len):
    C = R.WEIERSTRASS[name]
    keys = [pk for _, _, pk, _, _ in _cases("ecdsa", name, pk_len)]
    keys += [R.sec1_encode(C.mul(k, C.G), pk_len == 33) for k in (1, 2, 3, C.N - 1)]
    xy = _limbs(8)
    n_ok = 0
    for j, pk in enumerate(keys):
        want = R.sec1_decode(C, pk)
        for al in range(4):
            assert host.cm_sec1_decode(R.CURVE_IDS[name], pk, SZ(pk_len), SZ(1), SZ(0), SZ(al), xy) == (want is not None), pk.hex()
            if want:
                assert (_int(xy), _int(xy, 4)) == want
        n_ok += want is not None
    assert n_ok > 20 and n_ok < len(keys)
    # records in an array: element i of several, the array at any alignment (33 and 65 are odd: every offset mod 4 occurs)
    block = b"".join(keys[:9])
    for i in range(9):
        want = R.sec1_decode(C, keys[i])
        assert host.cm_sec1_decode(R.CURVE_IDS[name], block, SZ(pk_len), SZ(9), SZ(i), SZ(i % 4), xy) == (want is not None)
        if want:
            assert (_int(xy), _int(xy, 4)) == want


def test_bip340_prepare_step(host):
    pxy, u2, r, s = _limbs(8), _limbs(), _limbs(), _limbs()
    n_ok = 0
    for i, (msg, sig, pk, _, name) in enumerate(_cases("bip340")):
        ok = host.cm_bip340_prepare_msg(sig, pk, msg, SZ(len(msg)), SZ(i % 4), pxy, u2, r, s)
        P = R.lift_x(int.from_bytes(pk, "big"))
        rr, ss = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        assert ok == (1 if P is not None and rr < R.SECP.P and ss < R.SECP.N else 0), name
        assert (_int(r), _int(s)) == (rr, ss)
        assert _int(u2) == (-R.bip340_challenge(sig[:32], pk, msg)) % R.SECP.N, name
        if P is not None:
            assert (_int(pxy), _int(pxy, 4)) == P, name
        n_ok += ok
    assert 40 < n_ok < i


def test_ed25519_prepare_step(host):
    axy, rxy, u2, s = _limbs(8), _limbs(8), _limbs(), _limbs()
    n_ok = 0
    for i, (msg, sig, pk, _, name) in enumerate(_cases("ed25519")):
        ok = host.cm_eddsa_prepare_msg(sig, pk, msg, SZ(len(msg)), SZ(i % 4), axy, rxy, u2, s)
        A, Rp, S = R.ed_decode(pk), R.ed_decode(sig[:32]), int.from_bytes(sig[32:], "little")
        assert ok == (1 if A is not None and Rp is not None and S < R.ED.N else 0), name
        assert _int(s) == S
        assert _int(u2) == R.ed25519_challenge(sig[:32], pk, msg), name
        if ok:   # the key comes out negated: the verifier adds h (-A)
            assert (_int(axy), _int(axy, 4)) == R.ED.neg(A) and (_int(rxy), _int(rxy, 4)) == Rp, name
        n_ok += ok
    assert 40 < n_ok < i


@pytest.mark.parametrize("name", ["secp256k1", "p256"])
@pytest.mark.parametrize("pk_len", [33, 65])
def test_ecdsa_prepare_step(host, name, pk_len):
    C = R.WEIERSTRASS[name]
    z, r, s, q = _limbs(), _limbs(), _limbs(), _limbs(8)
    n_ok = 0
    for i, (msg, sig, pk, _, cname) in enumerate(_cases("ecdsa", name, pk_len)):
        ok = host.cm_ecdsa_prepare_msg(R.CURVE_IDS[name], sig, pk, SZ(pk_len), msg, SZ(len(msg)), SZ(i % 4), z, r, s, q)
        Q = R.sec1_decode(C, pk)
        assert ok == (Q is not None), cname
        assert (_int(z), _int(r), _int(s)) == (R.ecdsa_z(msg), int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")), cname
        if Q:
            assert (_int(q), _int(q, 4)) == Q, cname
        n_ok += ok
    assert 40 < n_ok < i
