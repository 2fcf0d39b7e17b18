"""
CPU checks of the model tests/canon_bip32_ref.py, which the fixture and every device test of the tweak-add and BIP-32 calls
rest on: BIP-32 test vector 1 (seed 000102...0f) -- m, m/0', m/0'/1 as published -- by CKDpriv, and m/0'/1 again by CKDpub from
m/0''s public key; CKDpriv and CKDpub commute with the public key on random non-hardened cases; the public tweak-add is the
secret one under the public key on both curves; and every status.
"""
import random

import pytest

import canon_bip32_ref as B

SECP = B.SECP256K1

# BIP-32 test vector 1: (path, key, chain code, public key)
VECTOR1 = [
    ("m", "e8f32e723decf4051aefac8e2c93c9c5b214313817cdb01a1494b917c8436b35",
     "873dff81c02f525623fd1fe5167eac3a55a049de3d314bb42ee227ffed37d508",
     "0339a36013301597daef41fbe593a02cc513d0b55527ec2df1050e2e8ff49c85c2"),
    ("m/0'", "edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea",
     "47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141",
     "035a784662a4a20a65bf6aab9ae98a6c068a81c52e4b032c0fb5400c706cfccc56"),
    ("m/0'/1", "3c6cb8d0f6a264c91ea8b5030fadaa8e538b020f0a387421a12de9319dc93368",
     "2a7857631386ba23dacac34180dd1983734e444fdbf774041578e9b6adb37c19",
     "03501e454bf00751f24b1b489aa925215d66af2234e3891c3b21a52bedb3cd711c"),
]
VECTOR1_INDICES = [B.HARDENED, 1]


def test_vector_1_by_ckd_priv():
    key, cc = B.master(bytes(range(16)))
    assert (key.hex(), cc.hex(), B.public_key(SECP, key).hex()) == VECTOR1[0][1:]
    for index, row in zip(VECTOR1_INDICES, VECTOR1[1:]):
        key, cc, st = B.ckd_priv(key, cc, index)
        assert st == 0 and (key.hex(), cc.hex(), B.public_key(SECP, key).hex()) == row[1:], row[0]


def test_vector_1_last_level_by_ckd_pub():
    _, _, cc, pk = VECTOR1[1]
    child, ccc, st = B.ckd_pub(bytes.fromhex(pk), bytes.fromhex(cc), 1)
    assert st == 0 and (ccc.hex(), child.hex()) == VECTOR1[2][2:]
    assert B.ckd_pub(bytes.fromhex(pk), bytes.fromhex(cc), B.HARDENED) == (bytes(33), bytes(32), B.BAD_INDEX)


def test_hardened_with_and_without_the_comb_agree():
    key, cc = bytes.fromhex(VECTOR1[0][1]), bytes.fromhex(VECTOR1[0][2])
    assert B.ckd_priv(key, cc, B.HARDENED, B.NO_COMB) == B.ckd_priv(key, cc, B.HARDENED)
    assert B.ckd_priv(key, cc, 1, B.NO_COMB) == (bytes(32), bytes(32), B.BAD_INDEX)


def test_ckd_priv_and_ckd_pub_commute():
    rng = random.Random(0xB1932)
    for _ in range(64):
        key, cc = B.b32(rng.randrange(1, SECP.N)), bytes(rng.randrange(256) for _ in range(32))
        index = rng.randrange(B.HARDENED)
        ck, cc1, st1 = B.ckd_priv(key, cc, index)
        cp, cc2, st2 = B.ckd_pub(B.public_key(SECP, key), cc, index)
        assert st1 == st2 == 0 and cc1 == cc2 and B.public_key(SECP, ck) == cp


@pytest.mark.parametrize("curve", sorted(B.CURVES))
def test_pubkey_tweak_add_is_the_secret_one_under_the_public_key(curve):
    C = B.CURVES[curve]
    rng = random.Random(0xB1933)
    for i in range(24):
        d, t = rng.randrange(1, C.N), rng.randrange(C.N)
        if i == 0:
            t = 0
        want = C.mul((d + t) % C.N, C.G)
        forms = (33, 65, 32) if curve == "secp256k1" else (33, 65)
        for fin in forms:
            pk = B.encode(C.mul(d, C.G), fin)
            for fout in forms:
                out, st = B.pubkey_tweak_add(C, pk, B.b32(t), fout)
                if fin == 32 and (C.mul(d, C.G)[1] & 1):   # x-only means the even y: the key is -d G
                    want2 = C.mul((t - d) % C.N, C.G)
                    assert (out, st) == (B.encode(want2, fout), 0)
                else:
                    assert (out, st) == (B.encode(want, fout), 0)
        sk, st = B.seckey_tweak_add(C, B.b32(d), B.b32(t))
        assert st == 0 and B.public_key(C, sk) == B.encode(want, 33)


@pytest.mark.parametrize("curve", sorted(B.CURVES))
def test_statuses(curve):
    C = B.CURVES[curve]
    d = 0x1234567
    pk = B.public_key(C, B.b32(d))
    assert B.pubkey_tweak_add(C, pk, B.b32(C.N - d), 33) == (bytes(33), B.NO_KEY)
    assert B.pubkey_tweak_add(C, pk, B.b32(d), 33) == (B.encode(C.mul(2 * d, C.G), 33), 0)
    assert B.pubkey_tweak_add(C, pk, B.b32(C.N), 65) == (bytes(65), B.BAD_SCALAR)
    assert B.pubkey_tweak_add(C, pk, B.b32(C.N - 1), 33)[1] == 0
    for tag in (0, 4, 5, 6, 7):
        assert B.pubkey_tweak_add(C, bytes([tag]) + pk[1:], B.b32(1), 33) == (bytes(33), B.BAD_POINT)
    assert B.pubkey_tweak_add(C, b"\x02" + B.b32(C.P), B.b32(1), 33)[1] == B.BAD_POINT
    full = B.public_key(C, B.b32(d), 65)
    wrong_y = full[:64] + bytes([full[64] ^ 1])
    assert B.pubkey_tweak_add(C, wrong_y, B.b32(1), 33)[1] == B.BAD_POINT
    assert B.seckey_tweak_add(C, bytes(32), B.b32(1)) == (bytes(32), B.BAD_KEY)
    assert B.seckey_tweak_add(C, B.b32(C.N), B.b32(1)) == (bytes(32), B.BAD_KEY)
    assert B.seckey_tweak_add(C, B.b32(d), B.b32(C.N)) == (bytes(32), B.BAD_SCALAR)
    assert B.seckey_tweak_add(C, B.b32(d), B.b32(C.N - d)) == (bytes(32), B.NO_KEY)
    assert B.seckey_tweak_add(C, B.b32(d), bytes(32)) == (B.b32(d), 0)


def test_invalid_il_is_status_10():
    n = SECP.N
    assert B.ckd_priv_from_il(5, n) is None and B.ckd_priv_from_il(5, n - 5) is None and B.ckd_priv_from_il(5, n - 6) == n - 1
    K = SECP.mul(5, SECP.G)
    assert B.ckd_pub_from_il(K, n) is None and B.ckd_pub_from_il(K, n - 5) is None
    assert B.ckd_pub_from_il(K, 5) == SECP.mul(10, SECP.G)
    assert B.ckd_priv(bytes(32), bytes(32), 0)[2] == B.BAD_KEY and B.ckd_pub(b"\x05" + bytes(32), bytes(32), 0)[2] == B.BAD_POINT
