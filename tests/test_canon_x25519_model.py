"""
Pins of the model tests/canon_x25519_ref.py, which decides what fec_canon_x25519 / fec_canon_x25519_base must answer:
the published vectors of RFC 7748 (section 5.2: both single vectors and the chain from k = u = 9 after 1 and after 1000
steps; section 6.1: the Diffie-Hellman example), the committed fixture against a fresh run of its generator's model, and
-- where there is an `openssl` program -- its X25519 on 32 random pairs and on the low-order points.
"""
import json
import os
import random
import shutil
import subprocess

import pytest

import canon_x25519_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_x25519_vectors.json")))
OPENSSL = shutil.which("openssl")


def test_rfc7748_section_5_2_vectors():
    for name, v in X.PUBLISHED.items():
        assert X.x25519(bytes.fromhex(v["k"]), bytes.fromhex(v["u"])).hex() == v["out"], name


def test_rfc7748_section_5_2_chain():
    ks = X.iterate(1000)
    assert ks[0].hex() == "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
    assert ks[999].hex() == "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"
    assert FIXTURE["iterated_1000"] == ks[999].hex()


def test_rfc7748_section_6_1_diffie_hellman():
    a = bytes.fromhex("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
    b = bytes.fromhex("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb")
    pa, pb = X.x25519_base(a), X.x25519_base(b)
    assert pa.hex() == "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
    assert pb.hex() == "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"
    shared = "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
    assert X.x25519(a, pb).hex() == shared and X.x25519(b, pa).hex() == shared


def test_base_point_is_the_image_of_the_ed25519_base_point():
    """u = (1 + y) / (1 - y) with y = 4/5: what fec_canon_x25519_base's map relies on"""
    y = 4 * pow(5, X.P - 2, X.P) % X.P
    assert (1 + y) * pow(1 - y, X.P - 2, X.P) % X.P == 9


def test_fixture_is_the_model():
    cases = FIXTURE["cases"]
    classes = {c["class"] for c in cases}
    assert classes == {"low-order", "non-canonical", "bit255", "clamp", "published", "random"}
    assert sum(c["class"] == "random" for c in cases) == 256 and sum(c["class"] == "non-canonical" for c in cases) == 19
    for c in cases:
        out, st = X.x25519_status(bytes.fromhex(c["k"]), bytes.fromhex(c["u"]))
        assert (out.hex(), st) == (c["out"], c["status"]), c["name"]
        if c["class"] == "low-order":
            assert st == X.ZERO_SHARED and out == bytes(32)
    low = {int.from_bytes(bytes.fromhex(c["u"]), "little") for c in cases if c["class"] == "low-order"}
    assert low == {v | t << 255 for v in X.LOW_ORDER for t in (0, 1)}


def test_decoding_rules():
    k = bytes(range(7, 39))
    nine_top = (9 | 1 << 255).to_bytes(32, "little")
    assert X.x25519(k, nine_top) == X.x25519_base(k)                      # bit 255 of u is ignored
    u = 1234567                                                           # p + u reaches bit 255, which is dropped: u - 19 is left
    assert X.x25519(k, (X.P + u).to_bytes(32, "little")) == X.x25519(k, (u - 19).to_bytes(32, "little"))
    for v in range(2, 19):                                                # non-canonical p + v, v < 19, is v
        assert X.x25519(k, (X.P + v).to_bytes(32, "little")) == X.x25519(k, v.to_bytes(32, "little"))
    assert X.decode_scalar(bytes(32)) == 1 << 254 and X.decode_scalar(b"\xff" * 32) == (1 << 255) - 8


# ---- the openssl program ------------------------------------------------------------------------------------------------
PKCS8 = bytes.fromhex("302e020100300506032b656e04220420")   # PrivateKeyInfo, X25519, then the 32 key bytes
SPKI = bytes.fromhex("302a300506032b656e032100")            # SubjectPublicKeyInfo, X25519, then the 32 bytes of u


def _openssl_public(tmp, k):
    key = os.path.join(tmp, "k.der")
    open(key, "wb").write(PKCS8 + k)
    r = subprocess.run([OPENSSL, "pkey", "-inform", "DER", "-in", key, "-pubout", "-outform", "DER"], capture_output=True)
    assert r.returncode == 0 and r.stdout[:len(SPKI)] == SPKI, r.stderr
    return r.stdout[len(SPKI):]


def _openssl_derive(tmp, k, u):
    """the 32 shared bytes, or None where the program refuses"""
    key, peer = os.path.join(tmp, "k.der"), os.path.join(tmp, "p.der")
    open(key, "wb").write(PKCS8 + k)
    open(peer, "wb").write(SPKI + u)
    r = subprocess.run([OPENSSL, "pkeyutl", "-derive", "-keyform", "DER", "-inkey", key, "-peerform", "DER", "-peerkey", peer],
                       capture_output=True)
    return r.stdout if r.returncode == 0 and len(r.stdout) == 32 else None


@pytest.mark.skipif(OPENSSL is None, reason="no openssl program on PATH")
def test_openssl_agrees(tmp_path):
    tmp = str(tmp_path)
    rng = random.Random(0x0551)
    for _ in range(32):
        k, peer = bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(32))
        u = _openssl_public(tmp, peer)
        assert u == X.x25519_base(peer)
        assert _openssl_derive(tmp, k, u) == X.x25519(k, u)
    # an all-zero result: the program refuses exactly where the model reports status 7
    k = bytes(rng.randrange(256) for _ in range(32))
    for c in FIXTURE["cases"]:
        if c["class"] in ("low-order", "non-canonical", "bit255"):
            u = bytes.fromhex(c["u"])
            out, st = X.x25519_status(k, u)
            got = _openssl_derive(tmp, k, u)
            assert (got is None) == (st == X.ZERO_SHARED), c["name"]
            if got is not None:
                assert got == out, c["name"]
