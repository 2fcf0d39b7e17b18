"""
An outside opinion on the model that decides what canonical mode must answer (oracle/canon_model.py, tests/canon_msg_ref.py):
the `openssl` program, driven through tests/openssl_cli.py.  Skipped where there is none.  It verifies every ECDSA and
Ed25519 case from the message of both verification fixtures, signs the Ed25519 cases of the signing fixture again from
their seeds, derives the public keys of its secret keys, accepts its ECDSA signatures (secp256k1 has no published vector
in the tree: this is its independent pin) and derives ECDH secrets.  BIP-340 is left out: OpenSSL has none.
"""
import json
import os
import random

import pytest

import canon_msg_ref as R
import openssl_cli as O

pytestmark = pytest.mark.skipif(O.OPENSSL is None, reason="no openssl program on PATH")

HERE = os.path.dirname(os.path.abspath(__file__))
ADVERSARIAL = json.load(open(os.path.join(HERE, "golden", "canon_adversarial_vectors.json")))
MSG = json.load(open(os.path.join(HERE, "golden", "canon_msg_vectors.json")))
SIGN = json.load(open(os.path.join(HERE, "golden", "canon_sign_vectors.json")))

# Where OpenSSL follows a documented policy of its own, by class of the adversarial fixture and by case name of
# canon_msg_vectors.json (which has no classes).  Everything else is compared.
OWN_POLICY_CLASSES = {
    "non-canonical A": "OpenSSL decodes y >= p and x = 0 with the sign bit; RFC 8032 5.1.3 and the model refuse both",
}
OWN_POLICY_NAMES = {   # of the 65-byte ECDSA batches
    "key tag 6": "OpenSSL takes the hybrid SEC 1 form (tag 6 or 7, then x and y); the model takes tags 2, 3 and 4 only",
    "key tag 7": "the hybrid form again: OpenSSL accepts the one of the two whose parity bit agrees with y",
}
# A third condition is the program's, not the library's: `openssl pkeyutl -rawin` of OpenSSL 3.0 cannot read an empty
# message ("Could not allocate 0 bytes"), so an Ed25519 case with an empty message has no answer there (O.EMPTY_INPUT).


@pytest.fixture(scope="module")
def cli():
    c = O.Cli()
    yield c
    c.close()


def _from_the_message():
    """(label, class or name that an exclusion may list, scheme, curve, msg, sig, pk, want) of every ECDSA and Ed25519 case"""
    for c in ADVERSARIAL["msg"]:
        if c["scheme"] != "bip340":
            yield "adversarial %s %d: %s / %s" % (c["curve"], c["pk_len"], c["class"], c["name"]), c["class"], c
    for b in MSG["batches"]:
        if b["scheme"] != "bip340":
            for c in b["cases"]:
                yield "msg %s %d: %s" % (b["curve"], b["pk_len"], c["name"]), c["name"], dict(c, scheme=b["scheme"], curve=b["curve"], pk_len=b["pk_len"])
    for name, c in MSG["published"].items():
        if c["scheme"] != "bip340":
            yield "published " + name, name, c


def test_verdicts_of_both_verification_fixtures(cli):
    bad, compared, listed, unanswered, total = [], 0, 0, 0, 0
    for label, key, c in _from_the_message():
        total += 1
        msg, sig, pk = bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"])
        assert R.verify(c["scheme"], c["curve"], msg, sig, pk) == c["want"], label      # the fixture is the model's
        got = cli.verify(c["scheme"], c["curve"], msg, sig, pk)
        if got is None:
            assert c["scheme"] == "ed25519" and not msg, label
            unanswered += 1
            continue
        if "ossl" in c:
            assert c["ossl"] == got, label                                               # and records this program's answer
        if key in OWN_POLICY_CLASSES or (key in OWN_POLICY_NAMES and c["pk_len"] == 65):
            listed += 1
            continue
        compared += 1
        if got != c["want"]:
            bad.append("%s: model %d, openssl %d" % (label, c["want"], got))
    assert not bad, "\n".join(bad)
    n_listed = sum(c["class"] in OWN_POLICY_CLASSES for c in ADVERSARIAL["msg"]) + sum(
        c["name"] in OWN_POLICY_NAMES for b in MSG["batches"] if b["scheme"] == "ecdsa" and b["pk_len"] == 65 for c in b["cases"])
    n_empty = sum(1 for _, _, c in _from_the_message() if c["scheme"] == "ed25519" and not c["msg"])
    assert listed == n_listed == 6 and unanswered in (0, n_empty) and n_empty <= 5
    assert compared == total - n_listed - unanswered and total > 400


def test_ed25519_signatures_byte_for_byte(cli):
    """Ed25519 signing is deterministic: OpenSSL signing from the seed gives the fixture's bytes"""
    cases = [c for c in SIGN["ed25519"] if c["status"] == 0] + [c for c in SIGN["published"].values() if c["scheme"] == "ed25519"]
    signed = 0
    for c in cases:
        sig = cli.ed25519_sign(bytes.fromhex(c["key"]), bytes.fromhex(c["msg"]))
        if sig is not None:   # None: an empty message, which this openssl program cannot read
            assert sig == bytes.fromhex(c["sig"]), c["msg"]
            signed += 1
    assert signed >= len(cases) - sum(not c["msg"] for c in cases) >= 20


def _ec_keys(curve):
    """distinct (secret key, SEC 1 public key) pairs of the signing fixture"""
    seen = {}
    for c in SIGN["ecdsa"][curve]["msg_cases"]:
        if c["status"] == 0:
            seen[c["key"]] = bytes.fromhex(c["pk"])
    return sorted(seen.items())


def test_public_keys_of_the_signing_fixture(cli):
    n = 0
    for curve, C in R.WEIERSTRASS.items():
        for key, pk in _ec_keys(curve):
            Q = R.sec1_decode(C, pk)
            assert Q == C.mul(int(key, 16), C.G)
            assert cli.public_key(O.ec_private_key(curve, bytes.fromhex(key))) == O.ec_spki(curve, R.sec1_encode(Q, compressed=False)), key
            n += 1
    for c in SIGN["bip340"]:
        if c["status"] == 0:   # x-only keys: OpenSSL's point has this x
            spki = cli.public_key(O.ec_private_key("secp256k1", bytes.fromhex(c["key"])))
            assert spki[-64:-32] == bytes.fromhex(c["pk"]) and spki[:-64] == O.ec_spki("secp256k1", b"\x04" + bytes(64))[:-64], c["key"]
            n += 1
    for c in SIGN["ed25519"]:
        if c["status"] == 0:
            assert cli.public_key(O.ed25519_pkcs8(bytes.fromhex(c["key"]))) == O.ed25519_spki(bytes.fromhex(c["pk"])), c["key"]
            n += 1
    assert n > 30


@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_ecdsa_signatures_of_the_signing_fixture(cli, curve):
    """both forms of every signature from the message, and the signatures over given digests (verified without hashing)"""
    C = R.WEIERSTRASS[curve]
    n = 0
    for c in SIGN["ecdsa"][curve]["msg_cases"]:
        if c["status"] == 0:
            for sig in {c["sig"], c["sig_low"]}:
                assert cli.ecdsa_verify(curve, bytes.fromhex(c["msg"]), bytes.fromhex(sig), bytes.fromhex(c["pk"])) == 1, c["msg"]
                n += 1
    for c in SIGN["ecdsa"][curve]["digest_cases"]:
        if c["status"] == 0:
            pk = O.ec_spki(curve, R.sec1_encode(C.mul(int(c["key"], 16), C.G)))
            out = cli.run("pkeyutl", "-verify", "-pubin", "-inkey", cli.path("pk", pk), "-keyform", "DER", "-in",
                          cli.path("digest", bytes.fromhex(c["digest"])), "-sigfile", cli.path("sig", O.ecdsa_sig(bytes.fromhex(c["sig"]))))
            assert out.returncode == 0 and b"Signature Verified Successfully" in out.stdout, c["digest"]
            n += 1
    assert n > 80


@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_ecdh_shared_x(cli, curve):
    """16 pairs per curve (a dozen milliseconds each): the x coordinate of d1 (d2 G)"""
    C = R.WEIERSTRASS[curve]
    rng = random.Random(0xECD4)
    for _ in range(16):
        d1, d2 = rng.randrange(1, C.N), rng.randrange(1, C.N)
        want = C.mul(d1, C.mul(d2, C.G))[0].to_bytes(32, "big")
        assert cli.ecdh_x(curve, d1.to_bytes(32, "big"), R.sec1_encode(C.mul(d2, C.G), compressed=False)) == want
