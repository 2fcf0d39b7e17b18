"""
CPU checks of the model tests/canon_wallet_ref.py, which the fixture and every device test of the RIPEMD-160 / HASH160, Taproot
and path calls rest on: RIPEMD-160 by the paper's digests and, where the OpenSSL command line loads its legacy provider, by
random messages; HASH160 and CKDpub along a path by BIP-32 test vector 1; the Taproot output key by BIP-86's first receive key
and by the existing tweak-add model; every status; and the committed fixture agrees with it row by row.
"""
import hashlib
import os
import random
import subprocess

import pytest

import canon_bip32_ref as B
import canon_wallet_ref as W

HERE = os.path.dirname(os.path.abspath(__file__))
SECP = B.SECP256K1

PAPER = [
    (b"", "9c1185a5c5e9fc54612808977ee8f548b2258d31"),
    (b"a", "0bdc9d2d256b3ee9daae347be6f4dc835a467ffe"),
    (b"abc", "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"),
    (b"message digest", "5d0689ef49d2fae572b881b123a85ffa21595f36"),
    (b"abcdefghijklmnopqrstuvwxyz", "f71c27109c692c1b56bbdceb5b9d2865b3708dbc"),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "12a053384a9c0c88e405a06c27dcf49ada62eb2b"),
    (b"1234567890" * 8, "9b752e45573d4b39f4dbd3323cab82bf63326bfb"),
]
V1_MASTER_PK = "0339a36013301597daef41fbe593a02cc513d0b55527ec2df1050e2e8ff49c85c2"
V1_PK = "0357bfe1e341d01c69fe5654309956cbea516822fba8a601743a012a7896ee8dc2"          # m/0'/1/2'
V1_CC = "04466b9cc8e161e966409ca52986c584f07e9dc81f735db683c3ff6ec7b1503f"
BIP86_INTERNAL = "cc8a4bc64d897bddc5fbc2f670f7a8ba0b386779106cf1223c6fc5d7cd6fc115"
BIP86_OUTPUT = "a60869f0dbcf1dc659c9cecbaf8050135ea9e8cdc487053f1dc6880949dc684c"


def test_ripemd160_published_digests():
    for msg, want in PAPER:
        assert W.ripemd160(msg).hex() == want, msg


def test_ripemd160_against_openssl(tmp_path):
    probe = subprocess.run(["openssl", "dgst", "-provider", "legacy", "-ripemd160", os.devnull], capture_output=True, text=True)
    if probe.returncode != 0 or PAPER[0][1] not in probe.stdout:
        pytest.skip("the OpenSSL command line has no RIPEMD-160 here")
    rng = random.Random(0x160)
    for n in (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 200, 1000):
        msg = bytes(rng.randrange(256) for _ in range(n))
        p = tmp_path / ("m%d" % n)
        p.write_bytes(msg)
        out = subprocess.run(["openssl", "dgst", "-provider", "legacy", "-ripemd160", str(p)], capture_output=True, text=True, check=True)
        assert out.stdout.strip().split("= ")[-1] == W.ripemd160(msg).hex(), n


def test_hash160_of_vector_1_master_key():
    assert W.hash160(bytes.fromhex(V1_MASTER_PK)).hex() == "3442193e1bb70916e914552172cd4e2dbc9df811"


def test_path_from_vector_1():
    child, cc, fp, h160, st = W.derive_pub_path(bytes.fromhex(V1_PK), bytes.fromhex(V1_CC), [2, 1000000000])
    assert st == 0
    assert child.hex() == "022a471424da5e657499d1ff51cb43c47481a03b1e77f951fe64cec9f5a48f7011"
    assert cc.hex() == "c783e67b921d2beb8f6b389cc646d7263b4145701dadd2161548a8b078e65e9e"
    assert fp.hex() == "d880d7d8"
    assert h160.hex() == "d69aa102255fed74378278c7812701ea641fdf32"
    # the fingerprint is that of m/0'/1/2'/2, the last level's parent
    mid, _, st = B.ckd_pub(bytes.fromhex(V1_PK), bytes.fromhex(V1_CC), 2)
    assert st == 0 and W.hash160(mid)[:4] == fp
    assert W.derive_pub_path(bytes.fromhex(V1_PK), bytes.fromhex(V1_CC), [2])[2] == W.hash160(bytes.fromhex(V1_PK))[:4]


def test_path_statuses():
    pk, cc = bytes.fromhex(V1_PK), bytes.fromhex(V1_CC)
    zeros = (bytes(33), bytes(32), bytes(4), bytes(20))
    for level in range(3):
        idx = [1, 2, 3]
        idx[level] |= B.HARDENED
        assert W.derive_pub_path(pk, cc, idx) == zeros + (W.BAD_INDEX,)
    assert W.derive_pub_path(b"\x04" + pk[1:], cc, [B.HARDENED, 1]) == zeros + (W.BAD_POINT,)


def test_taproot_bip86_first_receive_key():
    assert W.taproot_output_key(bytes.fromhex(BIP86_INTERNAL)) == (bytes.fromhex(BIP86_OUTPUT), 1, 0)
    for tag in (2, 3):
        assert W.taproot_output_key(bytes([tag]) + bytes.fromhex(BIP86_INTERNAL)) == (bytes.fromhex(BIP86_OUTPUT), 1, 0)


def test_taproot_is_the_tweak_add_of_the_tagged_hash():
    rng = random.Random(0x341)
    tag = hashlib.sha256(b"TapTweak").digest()
    for i in range(12):
        x = B.encode(SECP.mul(rng.randrange(1, SECP.N), SECP.G), 32)
        root = bytes(rng.randrange(256) for _ in range(32)) if i & 1 else None
        t = hashlib.sha256(tag + tag + x + (root or b"")).digest()
        assert W.taptweak(x, root) == t
        want33, st = B.pubkey_tweak_add(SECP, x, t, 33)
        assert st == 0
        assert W.taproot_output_key(x, root) == (want33[1:], want33[0] & 1, 0)


def test_taproot_statuses():
    z = (bytes(32), 0, W.BAD_POINT)
    assert W.taproot_output_key(B.b32(SECP.P)) == z
    assert W.taproot_output_key(b"\x04" + bytes.fromhex(BIP86_INTERNAL)) == z
    assert W.taproot_output_key(b"\x00" + bytes.fromhex(BIP86_INTERNAL)) == z
    x = next(v for v in range(1, 50) if B.sqrt_mod(SECP, (v ** 3 + 7) % SECP.P) is None)
    assert W.taproot_output_key(B.b32(x), bytes(32)) == z


def test_the_fixture_agrees_with_the_model_and_is_small():
    path = os.path.join(HERE, "golden", "canon_wallet_vectors.json")
    assert os.path.getsize(path) < 40000   # well under canon_bip32_vectors.json (127 KB)
    fx = W.load_fixture(path)
    assert [c["len"] for c in fx["hashes"]] == [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 200]
    for c in fx["hashes"]:
        m = bytes.fromhex(c["msg"])
        assert len(m) == c["len"] and W.ripemd160(m).hex() == c["ripemd160"] and W.hash160(m).hex() == c["hash160"]
    assert {c["class"] for c in fx["taproot"]} == {"bip86", "random", "range", "off-curve", "tag"}
    for c in fx["taproot"]:
        out, par, st = W.taproot_output_key(bytes.fromhex(c["pk"]), bytes.fromhex(c["root"]) if c["root"] else None)
        assert (out.hex(), par, st) == (c["out"], c["parity"], c["status"]), c["name"]
    assert {c["class"] for c in fx["path"]} == {"vector1", "random", "index", "key"}
    assert {len(c["indices"]) for c in fx["path"]} >= {1, 2, 3, 8}
    for c in fx["path"]:
        got = W.derive_pub_path(bytes.fromhex(c["pk"]), bytes.fromhex(c["cc"]), c["indices"])
        assert tuple(g.hex() for g in got[:4]) + (got[4],) == (c["child"], c["child_cc"], c["fingerprint"], c["hash160"], c["status"]), c["name"]
