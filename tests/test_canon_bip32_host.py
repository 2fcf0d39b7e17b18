"""
CPU checks of the canonical-mode tweak-add and BIP-32 device code through a host build of forge_ec_amd/csrc/canon_bip32.hpp
(tests/cpp/canon_bip32_host.cpp), the per-element code the kernels run: hmac_sha512_37 and its midstate form against hmac for
200 random inputs, the whole fixture tests/golden/canon_bip32_vectors.json through the lane functions (a double-and-add stands
in for the comb), the shared-parent path against the replicated one, the add-affine step fed its three exceptional cases, and
the functions behind the HMAC fed IL >= n, IL + k = 0 and a child at infinity, which no HMAC output reaches.
The same source builds as a stand-alone program (-DCANON_BIP32_HOST_MAIN); test_stand_alone_program_under_sanitizers builds it
with -fsanitize=address,undefined -fno-sanitize-recover=undefined and runs it directly.
"""
import ctypes
import os
import random
import subprocess

import pytest

import canon_bip32_ref as B

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = B.load_fixture(os.path.join(HERE, "golden", "canon_bip32_vectors.json"))
SRC = os.path.join(HERE, "cpp", "canon_bip32_host.cpp")
SZ = ctypes.c_size_t
SECP = B.SECP256K1


def forms(curve):
    return (33, 65, 32) if curve == "secp256k1" else (33, 65)


def expected(case, out_len):
    """the record of one tweak case in one output form, from its out33"""
    if case["status"]:
        return bytes(out_len)
    return B.encode(B.decode(B.CURVES[case["curve"]], bytes.fromhex(case["out33"])), out_len)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_bip32") / "canon_bip32_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.cb_pub_from_il.restype = ctypes.c_uint
    lib.cb_priv_from_il.restype = ctypes.c_uint
    return lib


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "canon_bip32_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DCANON_BIP32_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


def test_hmac_sha512_37_both_forms(host):
    rng = random.Random(0x512)
    for i in range(200):
        key = bytes(rng.randrange(256) for _ in range(32))
        msg = bytes(rng.randrange(256) for _ in range(37))
        if i == 0:
            key, msg = bytes(32), bytes(37)
        if i == 1:
            key, msg = b"\xff" * 32, b"\xff" * 37
        want = B.hmac512(key, msg)
        for mid in (0, 1):
            out = (ctypes.c_uint8 * 64)()
            host.cb_hmac(key, msg, mid, out)
            assert bytes(out) == want, (i, mid)


def test_ser37(host):
    rng = random.Random(0x513)
    for first in (0, 2, 3):
        for index in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, rng.randrange(2**32)):
            v = bytes(rng.randrange(256) for _ in range(32))
            out = (ctypes.c_uint8 * 37)()
            host.cb_ser37(first, v, ctypes.c_uint(index), out)
            assert bytes(out) == bytes([first]) + v + index.to_bytes(4, "big")


@pytest.mark.parametrize("curve", sorted(B.CURVES))
def test_every_tweak_case(host, curve):
    """the fixture's cases of one input form as one batch, in every output form"""
    cases = [c for c in FIXTURE["tweak"] if c["curve"] == curve]
    assert {c["class"] for c in cases} == {"random", "tweak", "doubling", "infinity", "off-curve", "range", "tag", "wrong-y"}
    for pk_len in forms(curve):
        sel = [c for c in cases if len(c["key"]) == 2 * pk_len]
        assert len(sel) >= 70
        n = len(sel)
        pks = b"".join(bytes.fromhex(c["key"]) for c in sel)
        tw = b"".join(bytes.fromhex(c["tweak"]) for c in sel)
        for out_len in forms(curve):
            out, st = (ctypes.c_uint8 * (out_len * n))(), (ctypes.c_uint8 * n)()
            host.cb_pubkey_tweak_add(B.CURVE_IDS[curve], SZ(n), pks, pk_len, tw, out_len, out, st)
            out = bytes(out)
            for i, c in enumerate(sel):
                assert (out[out_len * i:out_len * (i + 1)], st[i]) == (expected(c, out_len), c["status"]), (c["class"], c["name"], out_len)


@pytest.mark.parametrize("curve", sorted(B.CURVES))
def test_every_seckey_case(host, curve):
    cases = [c for c in FIXTURE["seckey"] if c["curve"] == curve]
    assert {c["class"] for c in cases} == {"random", "tweak", "key", "zero"}
    n = len(cases)
    out, st = (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * n)()
    host.cb_seckey_tweak_add(B.CURVE_IDS[curve], SZ(n), b"".join(bytes.fromhex(c["key"]) for c in cases),
                             b"".join(bytes.fromhex(c["tweak"]) for c in cases), out, st)
    assert bytes(out).hex() == "".join(c["out"] for c in cases) and list(st) == [c["status"] for c in cases]


def _derive_pub(host, pks, ccs, n_par, idx):
    n = len(idx)
    out, occ, st = (ctypes.c_uint8 * (33 * n))(), (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * n)()
    host.cb_derive_pub(SZ(n), pks, ccs, SZ(n_par), (ctypes.c_uint32 * n)(*idx), out, occ, st)
    return bytes(out), bytes(occ), list(st)


def _derive_priv(host, keys, ccs, n_par, idx, flags):
    n = len(idx)
    out, occ, st = (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * n)()
    host.cb_derive_priv(SZ(n), keys, ccs, SZ(n_par), (ctypes.c_uint32 * n)(*idx), flags, out, occ, st)
    return bytes(out), bytes(occ), list(st)


def test_every_ckd_pub_case(host):
    cases = FIXTURE["bip32_pub"]
    assert {c["class"] for c in cases} == {"vector1", "random", "index", "key"}
    out, occ, st = _derive_pub(host, b"".join(bytes.fromhex(c["pk"]) for c in cases), b"".join(bytes.fromhex(c["cc"]) for c in cases),
                               len(cases), [c["index"] for c in cases])
    assert out.hex() == "".join(c["child"] for c in cases) and occ.hex() == "".join(c["child_cc"] for c in cases)
    assert st == [c["status"] for c in cases] and {2, 9} <= set(st)


def test_every_ckd_priv_case(host):
    cases = FIXTURE["bip32_priv"]
    assert {c["class"] for c in cases} == {"vector1", "random", "index", "key", "no-comb"}
    for flags in (0, B.NO_COMB):
        sel = [c for c in cases if c["flags"] == flags]
        out, occ, st = _derive_priv(host, b"".join(bytes.fromhex(c["key"]) for c in sel), b"".join(bytes.fromhex(c["cc"]) for c in sel),
                                    len(sel), [c["index"] for c in sel], flags)
        assert out.hex() == "".join(c["child"] for c in sel) and occ.hex() == "".join(c["child_cc"] for c in sel)
        assert st == [c["status"] for c in sel]


def test_shared_parent_is_the_replicated_parent(host):
    rng = random.Random(0x514)
    key, cc = B.b32(rng.randrange(1, SECP.N)), bytes(rng.randrange(256) for _ in range(32))
    pk = B.public_key(SECP, key)
    idx = [rng.randrange(2**31) for _ in range(20)] + [2**31, 0, 2**31 - 1]
    n = len(idx)
    assert _derive_pub(host, pk, cc, 1, idx) == _derive_pub(host, pk * n, cc * n, n, idx)
    want = [B.ckd_pub(pk, cc, i) for i in idx]
    got = _derive_pub(host, pk, cc, 1, idx)
    assert got[0] == b"".join(w[0] for w in want) and got[1] == b"".join(w[1] for w in want) and got[2] == [w[2] for w in want]
    idx += [2**31 + 5, 2**32 - 1]
    n = len(idx)
    assert _derive_priv(host, key, cc, 1, idx, 0) == _derive_priv(host, key * n, cc * n, n, idx, 0)
    want = [B.ckd_priv(key, cc, i) for i in idx]
    got = _derive_priv(host, key, cc, 1, idx, 0)
    assert got[0] == b"".join(w[0] for w in want) and got[1] == b"".join(w[1] for w in want) and got[2] == [w[2] for w in want]
    bad = b"\x05" + pk[1:]
    assert _derive_pub(host, bad, cc, 1, idx[:3]) == (bytes(99), bytes(96), [2, 2, 2])


def _le(v):
    return v.to_bytes(32, "little")


@pytest.mark.parametrize("curve", sorted(B.CURVES))
def test_add_affine_exceptional_cases(host, curve):
    """the accumulator at infinity, P == Q, P == -Q, and an ordinary sum, each with Z = 1 and with a Z of its own"""
    C = B.CURVES[curve]
    rng = random.Random(0x515)
    cid = B.CURVE_IDS[curve]

    def run(acc, q):
        out = (ctypes.c_uint8 * 64)()
        inf = host.cb_add_affine(cid, b"".join(_le(v) for v in acc), _le(q[0]) + _le(q[1]), out)
        out = bytes(out)
        return None if inf else (int.from_bytes(out[:32], "little"), int.from_bytes(out[32:], "little")), out

    for _ in range(4):
        P, Q = C.mul(rng.randrange(1, C.N), C.G), C.mul(rng.randrange(1, C.N), C.G)
        for z in (1, rng.randrange(2, C.P)):
            jac = lambda pt: (pt[0] * z * z % C.P, pt[1] * z * z * z % C.P, z)  # noqa: E731
            assert run((rng.randrange(C.P), rng.randrange(C.P), 0), Q)[0] == Q
            assert run((1, 1, 0), Q)[0] == Q
            assert run(jac(Q), Q)[0] == C.add(Q, Q)
            got, raw = run(jac(C.neg(Q)), Q)
            assert got is None and raw == bytes(64)
            assert run(jac(P), Q)[0] == C.add(P, Q)


def test_behind_the_hmac(host):
    """IL >= n, IL + k = 0 (mod n) and a child at infinity: status 10 and zeros; their neighbours in range are keys"""
    n = SECP.N
    k = 0x1F00D
    key, pk = B.b32(k), B.public_key(SECP, B.b32(k))

    def priv(il, index=0, flags=0, key=key):
        ok, occ = (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)()
        st = host.cb_priv_from_il(key, B.b32(il), ctypes.c_uint(index), flags, ok, occ)
        return bytes(ok), bytes(occ), st

    def pub(il, index=0, pk=pk):
        o = (ctypes.c_uint8 * 33)()
        st = host.cb_pub_from_il(pk, B.b32(il), ctypes.c_uint(index), o)
        return bytes(o), st

    kept = b"\xa5" * 32
    for il in (n, n + 1, 2**256 - 1, n - k):
        assert priv(il) == (bytes(32), bytes(32), B.BIP32_INVALID), hex(il)
        assert priv(il, 2**31) == (bytes(32), bytes(32), B.BIP32_INVALID), hex(il)
        assert pub(il) == (bytes(33), B.BIP32_INVALID), hex(il)
    for il in (0, 1, n - 1, n - k - 1, n - k + 1, k):
        assert priv(il) == (B.b32(B.ckd_priv_from_il(k, il)), kept, 0), hex(il)
        assert pub(il) == (B.encode(B.ckd_pub_from_il(B.decode(SECP, pk), il), 33), 0), hex(il)
    # the order of the statuses: key, index, invalid
    assert priv(n, 5, B.NO_COMB)[2] == B.BAD_INDEX and priv(n, 5, B.NO_COMB, bytes(32))[2] == B.BAD_KEY
    assert priv(3, 2**31 + 5, B.NO_COMB) == (B.b32(k + 3), kept, 0)
    assert pub(n, 2**31)[1] == B.BAD_INDEX and pub(n, 2**31, b"\x05" + pk[1:])[1] == B.BAD_POINT
