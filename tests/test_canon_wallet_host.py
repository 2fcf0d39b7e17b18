"""
CPU checks of the canonical-mode RIPEMD-160 / HASH160, Taproot and CKDpub-along-a-path device code through a host build of
forge_ec_amd/csrc/ripemd160.hpp and canon_wallet.hpp (tests/cpp/canon_wallet_host.cpp), the per-element code the kernels run:
the hashes against the model at every length where the padding or the block count changes and at every byte alignment, the
TapTweak midstate against hashlib, the whole fixture tests/golden/canon_wallet_vectors.json through the lane functions (a
double-and-add stands in for the comb), the shared parent against the replicated one, and the functions behind the hashes fed
what no hash output reaches: IL >= n at level 1 of 3, a child at infinity at a middle level, t >= n, P + t G at infinity.
The same source builds as a stand-alone program (-DCANON_WALLET_HOST_MAIN); test_stand_alone_program_under_sanitizers builds it
with -fsanitize=address,undefined -fno-sanitize-recover=undefined and runs it directly.
"""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

import canon_bip32_ref as B
import canon_wallet_ref as W

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = W.load_fixture(os.path.join(HERE, "golden", "canon_wallet_vectors.json"))
SRC = os.path.join(HERE, "cpp", "canon_wallet_host.cpp")
SZ = ctypes.c_size_t
SECP = B.SECP256K1
LENGTHS = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 200)
FILL = 0xEE


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_wallet") / "canon_wallet_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.cw_taproot_from_t.restype = ctypes.c_uint
    return lib


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "canon_wallet_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DCANON_WALLET_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


def _hash(host, sha_first, msg, shift):
    out = (ctypes.c_uint8 * 20)()
    host.cw_hash(sha_first, msg, SZ(len(msg)), SZ(shift), out)
    return bytes(out)


def test_hashes_at_every_length_and_alignment(host):
    rng = random.Random(0x161)
    msgs = [bytes.fromhex(c["msg"]) for c in FIXTURE["hashes"]] + [bytes(rng.randrange(256) for _ in range(n)) for n in LENGTHS]
    assert sorted({len(m) for m in msgs}) == list(LENGTHS)
    for m in msgs:
        for shift in range(4):
            assert _hash(host, 0, m, shift) == W.ripemd160(m), (len(m), shift)
            assert _hash(host, 1, m, shift) == W.hash160(m), (len(m), shift)


def test_hash160_from_the_coordinates(host):
    rng = random.Random(0x162)
    for _ in range(20):
        pk = B.encode(SECP.mul(rng.randrange(1, SECP.N), SECP.G), 33)
        out = (ctypes.c_uint8 * 20)()
        assert host.cw_hash160_compressed(pk, out) == 1
        assert bytes(out) == W.hash160(pk)


def test_taptweak_midstate(host):
    const, comp = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)()
    host.cw_taptweak_midstate(hashlib.sha256(b"TapTweak").digest(), const, comp)
    assert list(const) == list(comp)
    host.cw_taptweak_midstate(hashlib.sha256(b"TapLeaf").digest(), const, comp)   # the comparison can fail
    assert list(const) != list(comp)


def _taproot(host, pks, pk_len, roots):
    n = len(pks)
    out, par, st = (ctypes.c_uint8 * (32 * n))(*([FILL] * (32 * n))), (ctypes.c_uint8 * n)(*([FILL] * n)), (ctypes.c_uint8 * n)(*([FILL] * n))
    host.cw_taproot(SZ(n), b"".join(pks), pk_len, None if roots is None else b"".join(roots), out, par, st)
    return [(bytes(out[32 * i:32 * i + 32]).hex(), par[i], st[i]) for i in range(n)]


def test_every_taproot_case(host):
    cases = FIXTURE["taproot"]
    assert {c["class"] for c in cases} == {"bip86", "random", "range", "off-curve", "tag"}
    seen = 0
    for pk_len in (32, 33):
        for rooted in (False, True):
            sel = [c for c in cases if len(c["pk"]) == 2 * pk_len and (c["root"] is not None) == rooted]
            if not sel:
                continue
            got = _taproot(host, [bytes.fromhex(c["pk"]) for c in sel], pk_len, [bytes.fromhex(c["root"]) for c in sel] if rooted else None)
            assert got == [(c["out"], c["parity"], c["status"]) for c in sel], (pk_len, rooted)
            seen += len(sel)
    assert seen == len(cases)


def _path(host, pks, ccs, rows, fp=True, h160=True, force_level=-1, force_il=None):
    n, depth = len(rows), len(rows[0])
    idx = (ctypes.c_uint32 * (n * depth))(*[v for r in rows for v in r])
    bufs = [(ctypes.c_uint8 * (w * n))(*([FILL] * (w * n))) for w in (33, 32, 4, 20, 1)]
    host.cw_derive_pub_path(SZ(n), b"".join(pks), b"".join(ccs), SZ(len(pks)), idx, SZ(depth), bufs[0], bufs[1], bufs[2] if fp else None,
                            bufs[3] if h160 else None, bufs[4], force_level, force_il)
    return [tuple(bytes(b[w * i:w * i + w]).hex() for b, w in zip(bufs[:4], (33, 32, 4, 20))) + (bufs[4][i],) for i in range(n)]


def _want(c):
    return (c["child"], c["child_cc"], c["fingerprint"], c["hash160"], c["status"])


def test_every_path_case(host):
    cases = FIXTURE["path"]
    for depth in sorted({len(c["indices"]) for c in cases}):
        sel = [c for c in cases if len(c["indices"]) == depth]
        got = _path(host, [bytes.fromhex(c["pk"]) for c in sel], [bytes.fromhex(c["cc"]) for c in sel], [c["indices"] for c in sel])
        assert got == [_want(c) for c in sel], depth
        for fp, h160 in ((False, True), (True, False), (False, False)):   # an output not asked for is not written
            part = _path(host, [bytes.fromhex(c["pk"]) for c in sel], [bytes.fromhex(c["cc"]) for c in sel], [c["indices"] for c in sel], fp, h160)
            fill4, fill20 = bytes([FILL] * 4).hex(), bytes([FILL] * 20).hex()
            assert part == [(w[0], w[1], w[2] if fp else fill4, w[3] if h160 else fill20, w[4]) for w in map(_want, sel)]


def test_shared_parent_equals_the_replicated_one(host):
    rng = random.Random(0x163)
    pk, cc = B.encode(SECP.mul(rng.randrange(1, SECP.N), SECP.G), 33), bytes(rng.randrange(256) for _ in range(32))
    rows = [[rng.randrange(B.HARDENED) for _ in range(3)] for _ in range(6)]
    rows[2][1] |= B.HARDENED
    shared = _path(host, [pk], [cc], rows)
    assert shared == _path(host, [pk] * 6, [cc] * 6, rows)
    assert shared == [tuple(x.hex() for x in W.derive_pub_path(pk, cc, r)[:4]) + (W.derive_pub_path(pk, cc, r)[4],) for r in rows]
    assert shared[2][4] == W.BAD_INDEX and shared[1][4] == 0 and shared[3][4] == 0
    bad = _path(host, [b"\x05" + pk[1:]], [cc], rows)   # a shared parent that does not decode refuses every element
    assert bad == [(bytes(33).hex(), bytes(32).hex(), bytes(4).hex(), bytes(20).hex(), W.BAD_POINT)] * 6


ZEROS = (bytes(33).hex(), bytes(32).hex(), bytes(4).hex(), bytes(20).hex())


def test_behind_the_hmac_il_not_below_n_at_level_1_of_3(host):
    rng = random.Random(0x164)
    pk, cc = B.encode(SECP.mul(rng.randrange(1, SECP.N), SECP.G), 33), bytes(32)
    for il in (SECP.N, SECP.N + 1, 2**256 - 1):
        # the later levels run on G and would succeed or, with the hardened index, fail with another status: the first sticks
        for row in ([1, 2, 3], [1, 2 | B.HARDENED, 3]):
            assert _path(host, [pk], [cc], [row], force_level=0, force_il=B.b32(il)) == [ZEROS + (W.BIP32_INVALID,)]
    ok = _path(host, [pk], [cc], [[1, 2, 3]], force_level=0, force_il=B.b32(SECP.N - 1))   # the largest IL is accepted
    assert ok[0][4] == 0 and ok[0][0] != ZEROS[0]


def test_behind_the_hmac_child_at_infinity_at_a_middle_level(host):
    """parent k G; level 1 gives (k + IL0) G with IL0 the HMAC's; level 2 of 3 is forced to IL = n - (k + IL0)"""
    rng = random.Random(0x165)
    for _ in range(3):
        k, cc = rng.randrange(1, SECP.N), bytes(rng.randrange(256) for _ in range(32))
        pk = B.encode(SECP.mul(k, SECP.G), 33)
        il0 = int.from_bytes(B.hmac512(cc, pk + (7).to_bytes(4, "big"))[:32], "big")
        assert il0 < SECP.N
        il1 = (SECP.N - (k + il0)) % SECP.N
        for row in ([7, 8, 9], [7, 8, 9 | B.HARDENED]):
            assert _path(host, [pk], [cc], [row], force_level=1, force_il=B.b32(il1)) == [ZEROS + (W.BIP32_INVALID,)]
        # an earlier status is not replaced: a hardened index at level 1 and the forced infinity at level 2
        assert _path(host, [pk], [cc], [[7 | B.HARDENED, 8, 9]], force_level=1, force_il=B.b32(il1)) == [ZEROS + (W.BAD_INDEX,)]
        # one off: the child is G or -G, a point, and the walk goes on
        near = _path(host, [pk], [cc], [[7, 8, 9]], force_level=1, force_il=B.b32((il1 + 1) % SECP.N))
        assert near[0][4] == 0


def _from_t(host, pk, t):
    out, par = (ctypes.c_uint8 * 32)(*([FILL] * 32)), (ctypes.c_uint8 * 1)(FILL)
    st = host.cw_taproot_from_t(pk, len(pk), B.b32(t), out, par)
    return bytes(out).hex(), par[0], st


def test_behind_the_tagged_hash(host):
    rng = random.Random(0x166)
    z = bytes(32).hex()
    for _ in range(3):
        k = rng.randrange(1, SECP.N)
        P = SECP.mul(k, SECP.G)
        if P[1] & 1:   # lift_x takes the even y: that point is (n - k) G
            k = SECP.N - k
        x = B.b32(P[0])
        for t in (SECP.N, 2**256 - 1):
            assert _from_t(host, x, t) == (z, 0, W.BAD_SCALAR)
            assert _from_t(host, b"\x04" + x, t) == (z, 0, W.BAD_POINT)     # the order: the key first
        assert _from_t(host, x, SECP.N - k) == (z, 0, W.NO_KEY)
        assert _from_t(host, b"\x03" + x, SECP.N - k) == (z, 0, W.NO_KEY)
        want, st = B.pubkey_tweak_add(SECP, x, B.b32(SECP.N - k + 1), 33)   # one off: G
        assert st == 0 and _from_t(host, x, (SECP.N - k + 1) % SECP.N) == (want[1:].hex(), want[0] & 1, 0)
