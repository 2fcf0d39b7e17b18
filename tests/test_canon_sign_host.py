"""
CPU checks of the canonical-mode signing device code through a host build of forge_ec_amd/csrc/canon_sign.hpp
(tests/cpp/canon_sign_host.cpp), the per-element code the signing kernels run: the scanned table lookup and the branch-free
addition against the big-integer model on every single-digit scalar and the edge scalars, the RFC 6979 nonce wrapper with the
curve's order and with small order constants (rejected candidates, the retry bound), and the three signers over the whole
fixture tests/golden/canon_sign_vectors.json at every message alignment.  The same source builds as a stand-alone program
(-DCANON_SIGN_HOST_MAIN), which is run once here; built with -fsanitize=address,undefined it is the sanitizer run of this
code (not run by this file):
    g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DCANON_SIGN_HOST_MAIN \
        -o canon_sign_host_san tests/cpp/canon_sign_host.cpp && ./canon_sign_host_san
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import canon_msg_ref as R
import canon_sign_ref as S
from oracle import canon_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_sign_vectors.json")))
SRC = os.path.join(HERE, "cpp", "canon_sign_host.cpp")
SZ = ctypes.c_size_t
CURVES = {"secp256k1": (0, R.SECP), "p256": (1, R.P256)}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_sign") / "canon_sign_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    return ctypes.CDLL(so)


def _limbs(v):
    return (ctypes.c_uint64 * 4)(*M.limbs(v))


def _mul_base(host, curve, k, fn="cs_mul_base_secret"):
    xy = (ctypes.c_uint64 * 8)()
    rc = getattr(host, fn)(curve, _limbs(k), xy)
    return (M.unlimbs(list(xy)[:4]), M.unlimbs(list(xy)[4:])), rc


def test_stand_alone_program(tmp_path):
    exe = str(tmp_path / "canon_sign_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DCANON_SIGN_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


def test_tag_block_states(host):
    """the constants after the "BIP0340/aux" and "BIP0340/nonce" tag blocks, through the signer: see test_bip340 below; here
    they differ from each other and from the challenge's"""
    a, b = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)()
    host.cs_bip340_tag_state(0, a)
    host.cs_bip340_tag_state(1, b)
    assert list(a) != list(b) and list(a)[0] == 0x24dd3219 and list(b)[0] == 0x46615b35


def _edge_scalars(n, rng):
    f = (1 << 256) - 1
    out = [1, 2, 15, 16, n - 1, n - 2, f >> 4, 0x1111 << 240, 0xF, 0xF << 128, (1 << 128) - 1, ((1 << 64) - 1) << 190]
    out += [rng.randrange(1, n) for _ in range(24)]
    return [k for k in out if 1 <= k < n]


def _single_digit_points(C, G):
    """{d * 16^w: d * 16^w * G} for d = 1..15, w = 0..63, by the model's own group law: 16^w * G by doublings, its
    multiples by repeated addition (the model's double-and-add from scratch takes 12 ms per scalar)."""
    out, base = {}, G
    for w in range(64):
        acc = base
        for d in range(1, 16):
            out[d << (4 * w)] = acc
            acc = C.add(acc, base)
        for _ in range(4):
            base = C.add(base, base)
    return out


@pytest.mark.parametrize("name", ["secp256k1", "p256"])
def test_scanned_comb_weierstrass(host, name):
    """all 960 single-digit scalars d * 16^w (those below n), the edge scalars and random ones against the model; the refused
    scalars"""
    cid, C = CURVES[name]
    want = _single_digit_points(C, C.G)
    assert len(want) == 960 and want[15 << 40] == C.mul(15 << 40, C.G)
    want = {k: v for k, v in want.items() if k < C.N}
    assert len(want) >= 955
    want.update((k, C.mul(k, C.G)) for k in _edge_scalars(C.N, random.Random(17)))
    for k, pt in want.items():
        got, rc = _mul_base(host, cid, k)
        assert rc == 0 and got == pt, hex(k)
        assert _mul_base(host, cid, k, "cs_mul_base_public")[0] == pt, hex(k)
    for k in (0, C.N, C.N + 1, (1 << 256) - 1):
        got, rc = _mul_base(host, cid, k)
        assert rc == S.BAD_SCALAR and got == (0, 0), hex(k)


def test_scanned_comb_ed25519(host):
    """every single-digit scalar d * 16^w, d = 1..15 (the signed recoding turns d > 8 into d - 16 and a carry: the whole
    signed-digit set, the carry out of the top window included), all-F nibbles, long zero runs, random"""
    E = R.ED
    rng = random.Random(18)
    want = {k: tuple(v) for k, v in _single_digit_points(E, E.G).items()}
    assert want[9 << 252] == tuple(E.mul((9 << 252) % E.N, E.G))
    ks = [(1 << 256) - 1, 1, E.N - 1, E.N + 1, 0x8 << 252, (1 << 255) - 19, ((1 << 64) - 1) << 100, (1 << 128) - 1]
    ks += [rng.randrange(1 << 256) for _ in range(24)]
    want.update((k, tuple(E.mul(k % E.N, E.G))) for k in ks)
    want[0] = want[E.N] = (0, 1)
    for k, pt in want.items():
        got, rc = _mul_base(host, 2, k)
        assert rc == 0 and got == pt, hex(k)


def _ecdsa(host, cid, digests, keys, flags=0, order=None):
    n = len(digests)
    sigs, kb, st = (ctypes.c_uint8 * (64 * n))(), (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * n)()
    host.cs_ecdsa_sign(cid, SZ(n), b"".join(digests), b"".join(keys), _limbs(order) if order is not None else None, flags, sigs, kb, st)
    sigs, kb = bytes(sigs), bytes(kb)
    return [sigs[64 * i:64 * i + 64] for i in range(n)], [kb[32 * i:32 * i + 32] for i in range(n)], list(st)


@pytest.mark.parametrize("name", ["secp256k1", "p256"])
def test_ecdsa_every_fixture_case(host, name):
    cid, C = CURVES[name]
    b = FIXTURE["ecdsa"][name]
    dc = b["digest_cases"]
    digests, keys = [bytes.fromhex(c["digest"]) for c in dc], [bytes.fromhex(c["key"]) for c in dc]
    for flags, field in ((0, "sig"), (1, "sig_low")):
        sigs, ks, st = _ecdsa(host, cid, digests, keys, flags)
        assert st == [c["status"] for c in dc]
        assert [s.hex() for s in sigs] == [c[field] for c in dc]
        assert [k.hex() for k in ks] == [c["k"] for c in dc]
    mc = b["msg_cases"]
    msgs = [bytes.fromhex(c["msg"]) for c in mc]
    h1 = []
    for i, m in enumerate(msgs):
        out = (ctypes.c_uint8 * 32)()
        host.cs_sha256(m, SZ(len(m)), SZ(i % 4), out)
        h1.append(bytes(out))
        assert h1[-1] == hashlib.sha256(m).digest()
    keys = [bytes.fromhex(c["key"]) for c in mc]
    for flags, field in ((0, "sig"), (1, "sig_low")):
        for n in (len(mc), 9, 1):                 # a ragged group, and one element alone
            sigs, _, st = _ecdsa(host, cid, h1[:n], keys[:n], flags)
            assert st == [c["status"] for c in mc[:n]] and [s.hex() for s in sigs] == [c[field] for c in mc[:n]]


def test_published_nonces_and_signatures(host):
    for name in ("rfc6979_a25_sample", "rfc6979_a25_test"):
        v = S.published()[name]
        sigs, ks, st = _ecdsa(host, 1, [hashlib.sha256(v["msg"]).digest()], [v["key"]])
        assert (sigs[0], ks[0], st[0]) == (v["sig"], v["k"], 0), name


def test_nonce_chain_with_small_orders(host):
    """an order constant of 2^253 rejects seven candidates in eight: the retry leg; 1 rejects them all: the bound.  The model
    runs the same chain on the same octets with the same constant."""
    rng = random.Random(19)
    C = R.SECP
    for order in (1 << 253, (1 << 250) + 12345, 1):
        digests = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(6)] + [b"\xff" * 32]
        keys = [rng.randrange(1, C.N).to_bytes(32, "big") for _ in digests]
        _, ks, st = _ecdsa(host, 0, digests, keys, order=order)
        for h1, key, k, s in zip(digests, keys, ks, st):
            want = S.rfc6979_chain(key, (int.from_bytes(h1, "big") % C.N).to_bytes(32, "big"), order)
            assert (k, s) == ((bytes(32), S.RETRY) if want is None else (want.to_bytes(32, "big"), S.OK))
        assert (order == 1) == all(s == S.RETRY for s in st)
    assert S.RETRIED["count"] > 0


def test_bip340_every_fixture_case(host):
    cases = FIXTURE["bip340"] + [dict(FIXTURE["published"]["bip340_vector0"], status=0)]
    for i, c in enumerate(cases):
        m = bytes.fromhex(c["msg"])
        sig, pk = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 32)()
        for al in range(4) if i % 5 == 0 else (i % 4,):
            st = host.cs_bip340_sign(bytes.fromhex(c["key"]), bytes.fromhex(c["aux"]), m, SZ(len(m)), SZ(al), sig, pk)
            assert st == c["status"] and bytes(sig).hex() == c["sig"].lower() and bytes(pk).hex() == c["pk"].lower(), (i, al)


def test_ed25519_every_fixture_case(host):
    cases = FIXTURE["ed25519"] + [FIXTURE["published"]["rfc8032_test1"], FIXTURE["published"]["rfc8032_test2"]]
    for i, c in enumerate(cases):
        m = bytes.fromhex(c["msg"])
        sig, pk = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 32)()
        for al in range(4):
            host.cs_ed25519_sign(bytes.fromhex(c["key"]), m, SZ(len(m)), SZ(al), sig, pk)
            assert bytes(sig).hex() == c["sig"].lower() and bytes(pk).hex() == c["pk"].lower(), (i, al)
