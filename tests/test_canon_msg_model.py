"""
The model of the canonical-mode from-the-message verifiers (tests/canon_msg_ref.py: hashlib + oracle/canon_model.py) is
pinned by the published from-the-message vectors in the tree -- RFC 6979 A.2.5 (P-256, SHA-256, "sample"; the key is
compressed here), BIP-340 vector 0, RFC 8032 section 7.1 tests 1 and 2 -- and the fixture it wrote
(tests/golden/canon_msg_vectors.json) is checked against it: every recorded result, the message lengths at all four
start alignments, and the negative cases each scheme must hold.  secp256k1 ECDSA has no published vector in the tree:
its cases are model-signed, and the fixture says so.  No GPU.
"""
import json
import os

import pytest

import canon_msg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_msg_vectors.json")))


def _flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def test_published_vectors_verify_and_tampered_ones_do_not():
    pub = R.published()
    assert sorted(pub) == ["bip340_vector0", "rfc6979_a25_sample", "rfc8032_test1", "rfc8032_test2"]
    for name, (scheme, curve, msg, sig, pk) in pub.items():
        assert R.verify(scheme, curve, msg, sig, pk) == 1, name
        assert R.verify(scheme, curve, msg + b"x", sig, pk) == 0, name
        assert R.verify(scheme, curve, msg, _flip(sig, 5), pk) == 0, name
        assert R.verify(scheme, curve, msg, _flip(sig, 300), pk) == 0, name
        f = FIXTURE["published"][name]
        assert (f["scheme"], f["curve"], f["msg"], f["sig"], f["pk"], f["want"]) == (scheme, curve, msg.hex(), sig.hex(), pk.hex(), 1)
    # the RFC 6979 key in both SEC 1 forms
    C = R.P256
    _, _, msg, sig, pk = pub["rfc6979_a25_sample"]
    pt = R.sec1_decode(C, pk)
    assert pt == (0x60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6,
                  0x7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299)
    assert R.ecdsa_verify(C, msg, sig, R.sec1_encode(pt, compressed=False)) == 1


def test_the_signers_reproduce_the_published_signatures():
    """BIP-340 vector 0 (secret key 3, aux 0^32) and RFC 8032 tests 1 and 2 are deterministic: sign() gives their bytes."""
    from oracle import canon_model as M
    pub = R.published()
    assert R.bip340_sign(3, bytes(32), bytes(32)) == pub["bip340_vector0"][3]
    assert R.bip340_pubkey(3) == pub["bip340_vector0"][4]
    assert R.ed25519_sign(M.ED25519_RFC8032_TEST1[0], b"") == pub["rfc8032_test1"][3]
    assert R.ed25519_sign(M.ED25519_RFC8032_TEST2[0], b"\x72") == pub["rfc8032_test2"][3]
    d = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
    k = 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60   # RFC 6979 A.2.5, SHA-256, "sample"
    assert R.ecdsa_sign(R.P256, d, b"sample", k) == pub["rfc6979_a25_sample"][3]


def test_sec1_round_trip_and_refusals():
    for C in R.WEIERSTRASS.values():
        for k in (1, 2, 3, 0xDEADBEEF):
            pt = C.mul(k, C.G)
            for comp in (True, False):
                assert R.sec1_decode(C, R.sec1_encode(pt, comp)) == pt
            enc = R.sec1_encode(pt)
            assert R.sec1_decode(C, bytes([enc[0] ^ 1]) + enc[1:]) == C.neg(pt)
            for tag in (0, 1, 4, 5, 6, 7):
                assert R.sec1_decode(C, bytes([tag]) + enc[1:]) is None
            unc = R.sec1_encode(pt, False)
            for tag in (0, 2, 3, 6, 7):
                assert R.sec1_decode(C, bytes([tag]) + unc[1:]) is None
        assert R.sec1_decode(C, b"\x02" + C.P.to_bytes(32, "big")) is None


@pytest.mark.parametrize("index", range(len(FIXTURE["batches"])))
def test_fixture_agrees_with_the_model(index):
    b = FIXTURE["batches"][index]
    for c in b["cases"]:
        msg, sig, pk = bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"])
        assert len(sig) == 64 and len(pk) == b["pk_len"]
        assert R.verify(b["scheme"], b["curve"], msg, sig, pk) == c["want"], c["name"]


def test_fixture_covers_what_it_must():
    assert "model-signed" in FIXTURE["note"] and "no published vector" in FIXTURE["note"]
    assert FIXTURE["sha256_lengths"] == [0, 1, 55, 56, 63, 64, 65, 119, 120]
    assert FIXTURE["sha512_lengths"] == [0, 1, 47, 48, 63, 64, 65, 175, 176, 192]
    seen = set()
    for b in FIXTURE["batches"]:
        seen.add((b["scheme"], b["curve"], b["pk_len"]))
        lengths = FIXTURE["sha512_lengths" if b["scheme"] == "ed25519" else "sha256_lengths"]
        at, off = set(), 0
        for c in b["cases"]:
            n = len(c["msg"]) // 2
            if c["want"] == 1 and c["name"].startswith("valid"):
                at.add((n, off % 4))
            off += n
        assert at >= {(n, a) for n in lengths for a in range(4)}, (b["scheme"], b["curve"])
        names = " | ".join(c["name"] for c in b["cases"])
        must = ["message byte changed", "bit of s changed", "bit of the key changed"]
        if b["scheme"] == "ecdsa":
            must += ["bit of r changed", "r = 0", "s = 0", "r = n", "s = n", "malleable twin", "key x >= p"]
            must += ["no root", "tag 0", "tag 4", "tag 5", "tag 6"] if b["pk_len"] == 33 else ["tag 2", "tag 6", "y >= p", "off the curve"]
            twin = next(c for c in b["cases"] if c["name"].startswith("malleable twin"))
            assert twin["want"] == 1
        elif b["scheme"] == "bip340":
            must += ["bit of r changed", "r = p", "s = n", "key x >= p", "no root"]
        else:
            must = ["message byte changed", "bit of R changed", "bit of S changed", "bit of the key changed", "S >= l", "S = l",
                    "key y >= p", "x = 0 with the sign bit", "R undecodable"]
        for m in must:
            assert m in names, (b["scheme"], b["curve"], b["pk_len"], m)
        assert all(c["want"] == 0 for c in b["cases"] if not c["name"].startswith(("valid", "malleable twin")))
    assert seen == {("ecdsa", "secp256k1", 33), ("ecdsa", "secp256k1", 65), ("ecdsa", "p256", 33), ("ecdsa", "p256", 65),
                    ("bip340", "secp256k1", 32), ("ed25519", "ed25519", 32)}
    assert sum(len(b["cases"]) for b in FIXTURE["batches"]) < 500
