"""
GPU tests of the canonical-mode verifiers against tests/golden/canon_adversarial_vectors.json (built by
tests/canon_adversarial.py from the model, its Ed25519 and ECDSA verdicts confirmed by OpenSSL in
tests/test_canon_model_vs_openssl.py): points with a torsion component, R.x in [n, p), final additions that are a
doubling or infinity, prescribed u1 / u2 / Q through the GLV ladder and the windowed ladders.

Every case goes through every entry point that takes it -- the *_verify_msg calls in their host and *_dev forms, the
after-the-hash verifiers fed by hashlib, double_mul against the recorded point -- in two placements, because the
exceptional legs are wave-uniform branches: 64 copies of the case filling a wavefront, and the case alone at lanes 0,
31, 32, 63 and at the last element of 64 * 3 + 5 honest valid signatures of tests/golden/canon_msg_vectors.json.
"""
import json
import os
import random

import numpy as np
import pytest

import canon_msg_ref as R
import test_gpu_canon_msg as G
from oracle import canon_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_adversarial_vectors.json")))
WAVE, AMONG = 64, 64 * 3 + 5
LANES = (0, 31, 32, 63, AMONG - 1)
KEYS = sorted({(c["scheme"], c["curve"], c["pk_len"]) for c in FIXTURE["msg"]})
KEY_IDS = ["%s-%s-%d" % k for k in KEYS]
CURVES = ["secp256k1", "p256", "ed25519"]


def _cases(key):
    return [c for c in FIXTURE["msg"] if (c["scheme"], c["curve"], c["pk_len"]) == key]


def _row(c):
    return bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"])


def _limbs(h):
    """the fixture's hex (one 256-bit integer, or a point's x then y; None for infinity) -> 64-bit limbs"""
    return None if h is None else [l for i in range(0, len(h), 64) for l in M.limbs(int(h[i:i + 64], 16))]


def _label(c):
    return "%s / %s" % (c["class"], c["name"])


_honest = {}


def honest_rows(key):
    """AMONG valid signatures of the batch of canon_msg_vectors.json with this scheme, curve and key form, and their parts"""
    if key not in _honest:
        b = next(b for b in G.BATCHES if (b["scheme"], b["curve"], b["pk_len"]) == key)
        valid = [c for c in b["cases"] if c["want"] == 1]
        rows = [_row(valid[i % len(valid)]) for i in range(AMONG)]
        _honest[key] = (rows, [parts_of(key, r) for r in rows])
    return _honest[key]


def parts_of(key, row):
    """what the after-the-hash verifier takes, four limb lists: ECDSA z, r, s, key xy (zeros for an undecodable key);
    BIP-340 key x, r, s, e; Ed25519 A, R, S as little-endian integers and h"""
    msg, sig, pk = row
    big = lambda x: M.limbs(int.from_bytes(x, "big"))         # noqa: E731
    little = lambda x: M.limbs(int.from_bytes(x, "little"))   # noqa: E731
    if key[0] == "ecdsa":
        Q = R.sec1_decode(R.WEIERSTRASS[key[1]], pk)
        return M.limbs(R.ecdsa_z(msg)), big(sig[:32]), big(sig[32:]), M.xy_limbs(Q) if Q else [0] * 8
    if key[0] == "bip340":
        return big(pk), big(sig[:32]), big(sig[32:]), big(R.tagged("BIP0340/challenge", sig[:32] + pk + msg))
    return little(pk), little(sig[:32]), little(sig[32:]), M.limbs(R.ed25519_challenge(sig[:32], pk, msg))


def verify_parts(gpu_ctx, key, parts):
    dev = G._canon(gpu_ctx, key[1])
    a = [np.array([p[k] for p in parts], dtype=np.uint64) for k in range(4)]
    return {"ecdsa": dev.ecdsa_verify, "bip340": getattr(dev, "bip340_verify", None), "ed25519": getattr(dev, "eddsa_verify", None)}[key[0]](*a)


def every_form(gpu_ctx, key, rows, parts):
    """name -> verdicts: from the message through the host and the *_dev form, and after the hash"""
    b = {"scheme": key[0], "curve": key[1], "pk_len": key[2]}
    msgs = [r[0] for r in rows]
    sigs = np.frombuffer(b"".join(r[1] for r in rows), dtype=np.uint8).reshape(len(rows), 64).copy()
    pks = np.frombuffer(b"".join(r[2] for r in rows), dtype=np.uint8).reshape(len(rows), key[2]).copy()
    return {"from the message": G._host(gpu_ctx, b, msgs, sigs, pks), "from the message, dev": G._run_dev(gpu_ctx, b, msgs, sigs, pks),
            "after the hash": verify_parts(gpu_ctx, key, parts)}


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_a_wavefront_per_case(gpu_ctx, key):
    """64 copies of each case: every lane of the wavefront takes the exceptional leg"""
    cases = _cases(key)
    rows = [_row(c) for c in cases for _ in range(WAVE)]
    parts = [p for c in cases for p in [parts_of(key, _row(c))] * WAVE]
    want = np.repeat(np.array([c["want"] for c in cases], dtype=np.uint8), WAVE)
    for form, got in every_form(gpu_ctx, key, rows, parts).items():
        bad = sorted({_label(cases[i // WAVE]) for i in np.nonzero(got != want)[0]})
        assert not bad, "%s:\n%s" % (form, "\n".join(bad))
    assert 0 < want.sum() < len(want)


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_one_lane_among_honest_signatures(gpu_ctx, key):
    """the case at lanes 0, 31, 32, 63 and at the last element of 197 valid signatures: the whole verdict vector"""
    base_rows, base_parts = honest_rows(key)
    bad = []
    for c in _cases(key):
        rows, parts, want = list(base_rows), list(base_parts), np.ones(AMONG, dtype=np.uint8)
        for i in LANES:
            rows[i], parts[i], want[i] = _row(c), parts_of(key, _row(c)), c["want"]
        for form, got in every_form(gpu_ctx, key, rows, parts).items():
            if not np.array_equal(got, want):
                bad.append("%s: %s at %s" % (form, _label(c), np.nonzero(got != want)[0].tolist()))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_ecdsa_after_the_hash_with_z_free(gpu_ctx, curve):
    """prescribed (u2, Q = q G) pairs, z in {0, n, n + 1, 2^256 - 1}, the P-256 key with x = 0: both placements"""
    key = ("ecdsa", curve, 33)
    cases = [c for c in FIXTURE["hash"] if c["curve"] == curve]
    parts_c = [tuple(_limbs(c[k]) for k in "zrsq") for c in cases]
    want = np.repeat(np.array([c["want"] for c in cases], dtype=np.uint8), WAVE)
    got = verify_parts(gpu_ctx, key, [p for p in parts_c for _ in range(WAVE)])
    bad = sorted({_label(cases[i // WAVE]) for i in np.nonzero(got != want)[0]})
    assert not bad and want.all(), "\n".join(bad)
    _, base_parts = honest_rows(key)
    for c, p in zip(cases, parts_c):
        parts = list(base_parts)
        for i in LANES:
            parts[i] = p
        assert verify_parts(gpu_ctx, key, parts).all(), _label(c)
    # and refused when anything moves: r + 1 under the same z, s and key
    moved = [(z, M.limbs((M.unlimbs(r) + 1) % R.WEIERSTRASS[curve].N or 1), s, q) for z, r, s, q in parts_c]
    assert not verify_parts(gpu_ctx, key, moved).any()


# ---- double_mul against the recorded point ---------------------------------------------------------
def _dm_cases(curve):
    """(label, u1, u2, q, point) of every double multiplication recorded for this curve"""
    out = [(_label(c), c["dm"]) for c in FIXTURE["msg"] if c["curve"] == curve and c["pk_len"] != 65 and "dm" in c]
    out += [(_label(c), c) for c in FIXTURE["double_mul"] if c["curve"] == curve]
    out = [(name,) + tuple(_limbs(d[k]) for k in ("u1", "u2", "q", "point")) for name, d in out]
    for c in FIXTURE["hash"]:   # after the hash: u1 = z / s, u2 = r / s
        if c["curve"] == curve:
            n = R.WEIERSTRASS[curve].N
            w = pow(int(c["s"], 16), -1, n)
            out.append((_label(c), M.limbs(int(c["z"], 16) * w % n), M.limbs(int(c["r"], 16) * w % n), _limbs(c["q"]), _limbs(c["point"])))
    return out


_filler = {}


def dm_filler(curve):
    """8 ordinary double multiplications by the model, cycled to fill a batch"""
    if curve not in _filler:
        C = R.ED if curve == "ed25519" else R.WEIERSTRASS[curve]
        rng = random.Random(0xF111E5)
        f = []
        for _ in range(8):
            u1, u2, Q = rng.randrange(1, C.N), rng.randrange(1, C.N), C.mul(rng.randrange(1, C.N), C.G)
            f.append((M.limbs(u1), M.limbs(u2), M.xy_limbs(Q), M.xy_limbs(C.add(C.mul(u1, C.G), C.mul(u2, Q)))))
        _filler[curve] = f
    return _filler[curve]


def run_double_mul(gpu_ctx, curve, items):
    """items of (u1, u2, q, point or None) -> indices where the GPU's point or status differs"""
    arr = lambda k: np.array([it[k] for it in items], dtype=np.uint64)   # noqa: E731
    xy, st = G._canon(gpu_ctx, curve).double_mul(arr(0), arr(1), arr(2))
    want_xy = np.array([it[3] or [0] * 8 for it in items], dtype=np.uint64)
    want_st = np.array([1 if it[3] is None else 0 for it in items], dtype=np.uint8)
    return np.nonzero((xy != want_xy).any(axis=1) | (st != want_st))[0]


@pytest.mark.parametrize("curve", CURVES)
def test_double_mul_points(gpu_ctx, curve):
    cases = _dm_cases(curve)
    assert len(cases) > 40
    bad = run_double_mul(gpu_ctx, curve, [c[1:] for c in cases for _ in range(WAVE)])
    assert not len(bad), "\n".join(sorted({cases[i // WAVE][0] for i in bad}))
    if curve != "ed25519":
        assert any(c[4] is None for c in cases)      # sums that are infinity
    base = [dm_filler(curve)[i % 8] for i in range(AMONG)]
    wrong = []
    for c in cases:
        items = list(base)
        for i in LANES:
            items[i] = c[1:]
        bad = run_double_mul(gpu_ctx, curve, items)
        if len(bad):
            wrong.append("%s at %s" % (c[0], bad.tolist()))
    assert not wrong, "\n".join(wrong)
