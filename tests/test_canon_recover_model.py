"""
Pins tests/canon_recover_ref.py, the model behind the recovery fixture and the GPU tests.
Keccak: the permutation and the sponge are compared with hashlib.sha3_256 at the domain byte 0x06, which differs from
Keccak-256 in that byte alone; the 0x01 variant is pinned by published digests and by the best-known Ethereum address.
Recovery: no published vector is needed -- for signatures the signing model makes, the model's recovery id recovers d G, and
every id that returns a key returns one under which the verifier accepts; where there is an `openssl` program, it accepts
too.
"""
import hashlib
import random

import pytest

import canon_msg_ref as R
import canon_recover_ref as K
import canon_sign_ref as S
import openssl_cli as O

CURVES = sorted(R.WEIERSTRASS)


def test_round_constants_and_permutation_of_zero():
    assert K.RC[0] == 1 and K.RC[1] == 0x8082 and K.RC[23] == 0x8000000080008008 and len(K.RC) == 24
    # Keccak-f[1600] of the all-zero state: the first lane of the team's KeccakF-1600-IntermediateValues.txt
    assert K.keccak_f([0] * 25)[0] == 0xF1258F7940E1DDE7


def test_sponge_is_sha3_256_at_domain_6():
    rng = random.Random(0x5A3)
    lengths = K.KECCAK_LENGTHS + [rng.randrange(0, 700) for _ in range(64)]
    for n in lengths:
        msg = bytes(rng.randrange(256) for _ in range(n))
        assert K.sponge256(msg, 0x06) == hashlib.sha3_256(msg).digest(), n


def test_keccak256_published():
    assert K.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert K.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert K.keccak256(b"") != hashlib.sha3_256(b"").digest()
    assert K.eth_address(R.SECP.G).hex() == "7e5f4552091a69125d5dfcb7b8c2659029395bdf"   # secret key 1


def _signed(curve, count, seed):
    C = R.WEIERSTRASS[curve]
    rng = random.Random(seed)
    for i in range(count):
        d = rng.randrange(1, C.N)
        msg = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 80)))
        yield C, d, msg, hashlib.sha256(msg).digest(), (i & 1) * S.LOW_S


@pytest.mark.parametrize("curve", CURVES)
def test_models_recid_recovers_the_signers_key(curve):
    flipped = 0
    for C, d, _, h1, flags in _signed(curve, 24, 0x41):
        sig, recid, st = K.sign_recoverable_digest(C, d, h1, flags)
        assert st == 0 and (sig, st) == S.ecdsa_sign_digest(C, d, h1, flags) and recid in (0, 1)
        assert K.recover_point(C, h1, sig, recid) == C.mul(d, C.G)
        assert K.recover_point(C, h1, sig, recid ^ 1) != C.mul(d, C.G)
        flipped += sig != S.ecdsa_sign_digest(C, d, h1, 0)[0]
        for out_len in (33, 65, 64):
            assert K.recover(C, h1, sig, recid, out_len) == (K.encode(C.mul(d, C.G), out_len), K.OK)
    assert flipped >= 1             # the leg where LOW_S turned s over, and the parity with it, ran


@pytest.mark.parametrize("curve", CURVES)
def test_every_recovered_key_verifies(curve):
    keys = 0
    for C, d, _, h1, flags in _signed(curve, 12, 0x42):
        sig, _, _ = K.sign_recoverable_digest(C, d, h1, flags)
        for recid in range(4):
            Q = K.recover_point(C, h1, sig, recid)
            if Q is not None:
                keys += 1
                assert K.verify_digest(C, h1, sig, Q)
        for recid in (4, 5, 255):
            assert K.recover(C, h1, sig, recid, 33) == (bytes(33), K.NO_KEY)
    assert keys >= 24               # ids 0 and 1 always lift for a real signature; 2 and 3 need r + n < p


def test_recid_of():
    assert [K.recid_of(y, f, x) for x in (0, 1) for f in (0, 1) for y in (0, 1)] == [0, 1, 1, 0, 2, 3, 3, 2]


@pytest.mark.skipif(O.OPENSSL is None, reason="no openssl program on PATH")
@pytest.mark.parametrize("curve", CURVES)
def test_openssl_accepts_the_recovered_keys(curve):
    cli = O.Cli()
    try:
        n = 0
        for C, d, msg, h1, flags in _signed(curve, 6, 0x43):
            sig, recid, _ = K.sign_recoverable_digest(C, d, h1, flags)
            for rid in (recid, recid ^ 1):
                out, st = K.recover(C, h1, sig, rid, 33 if n & 1 else 65)
                assert st == 0 and cli.ecdsa_verify(curve, msg, sig, out) == 1
                n += 1
    finally:
        cli.close()
