"""The signing model tests/canon_sign_ref.py, pinned by published values, and the fixture it wrote
(tests/golden/canon_sign_vectors.json) re-derived.  CPU only."""
import hashlib
import json
import os

import canon_msg_ref as R
import canon_sign_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_sign_vectors.json")))


def test_rfc6979_a25_nonces_and_signatures():
    for name in ("rfc6979_a25_sample", "rfc6979_a25_test"):
        v = S.published()[name]
        d, h1 = int.from_bytes(v["key"], "big"), hashlib.sha256(v["msg"]).digest()
        assert S.ecdsa_nonce(R.P256, d, h1) == (v["k"], S.OK), name
        assert S.ecdsa_sign_msg(R.P256, d, v["msg"]) == (v["sig"], S.OK), name
        assert S.public_key(1, v["key"], 33) == (v["pk"], S.OK)
        assert R.ecdsa_verify(R.P256, v["msg"], v["sig"], v["pk"]) == 1


def test_bip340_vector0_and_rfc8032():
    pub = S.published()
    v = pub["bip340_vector0"]
    assert S.bip340_sign(3, v["msg"], v["aux"]) == (v["sig"], S.OK)
    assert S.public_key(S.SCHEME_BIP340, v["key"], 32) == (v["pk"], S.OK)
    for name in ("rfc8032_test1", "rfc8032_test2"):
        v = pub[name]
        assert S.ed25519_sign(v["key"], v["msg"]) == (v["sig"], v["pk"]), name


def test_refused_keys_and_the_retry_bound():
    for C in (R.SECP, R.P256):
        for d in (0, C.N, 2**256 - 1):
            assert S.ecdsa_sign_digest(C, d, bytes(32)) == (bytes(64), S.BAD_KEY)
            assert S.ecdsa_nonce(C, d, bytes(32)) == (bytes(32), S.BAD_KEY)
    assert S.bip340_sign(0, b"", bytes(32)) == (bytes(64), S.BAD_KEY)
    # a small order constant: candidates are rejected and drawn again; 1 rejects them all and the chain gives up
    x, hz = (5).to_bytes(32, "big"), hashlib.sha256(b"x").digest()
    before = S.RETRIED["count"]
    k = S.rfc6979_chain(x, hz, 1 << 250)
    assert k is not None and 1 <= k < 1 << 250 and S.RETRIED["count"] > before
    before = S.RETRIED["count"]
    assert S.rfc6979_chain(x, hz, 1) is None and S.RETRIED["count"] == before + 1 + S.MAX_RETRIES


def test_fixture_is_what_the_model_signs():
    """every tenth case re-signed (the generator signed them all); the coverage the generator asserts is present"""
    for curve, b in FIXTURE["ecdsa"].items():
        C = R.WEIERSTRASS[curve]
        cases = b["msg_cases"]
        for c in cases[::10]:
            d = int(c["key"], 16)
            assert S.ecdsa_sign_msg(C, d, bytes.fromhex(c["msg"]), 0) == (bytes.fromhex(c["sig"]), c["status"])
            assert S.ecdsa_sign_msg(C, d, bytes.fromhex(c["msg"]), S.LOW_S)[0] == bytes.fromhex(c["sig_low"])
        diff = sum(c["sig"] != c["sig_low"] for c in cases if c["status"] == 0)
        assert 0 < diff < sum(c["status"] == 0 for c in cases)
        assert {c["status"] for c in cases} == {S.OK, S.BAD_KEY}
        assert any(int(c["digest"], 16) >= C.N for c in b["digest_cases"])
        for c in b["digest_cases"][::5]:
            assert S.ecdsa_sign_digest(C, int(c["key"], 16), bytes.fromhex(c["digest"]), 0) == (bytes.fromhex(c["sig"]), c["status"])
    legs = {tuple(c["parity"]) for c in FIXTURE["bip340"] if c["status"] == 0}
    assert legs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for c in FIXTURE["bip340"][::10]:
        assert S.bip340_sign(int(c["key"], 16), bytes.fromhex(c["msg"]), bytes.fromhex(c["aux"])) == (bytes.fromhex(c["sig"]), c["status"])
    for c in FIXTURE["ed25519"][::10]:
        assert S.ed25519_sign(bytes.fromhex(c["key"]), bytes.fromhex(c["msg"])) == (bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"]))
    for name, v in S.published().items():
        assert {k: (x.hex() if isinstance(x, bytes) else x) for k, x in v.items()} == FIXTURE["published"][name], name
