"""
CPU checks of the restatement of Schnorr::<C, Sha256>::sign (tests/schnorr_sign_ref.py) and of its fixture
(tests/golden/schnorr_sign_vectors.json, generated over oracle/py_model.py): the C oracle backend reproduces every entry,
so the two backends agree; every leg of from_bytes_reduced that the restatement's docstring calls reachable is taken by a
fixture entry and no entry takes another; sk = 0 gives s = k; the "test message" entries are (to_affine(G), 1); and the
legs the docstring calls unreachable stay untaken under a seeded search over the inputs that could reach them.
"""
import json
import os
import random

import pytest

import schnorr_sign_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = S.load_fixture()


@pytest.fixture(scope="module")
def cbe():
    return S.CBackend()


@pytest.fixture(scope="module")
def pybe():
    return S.PyBackend()


@pytest.mark.parametrize("curve", [0, 1])
def test_c_oracle_backend_reproduces_every_sign_entry(cbe, curve):
    rows = [c for c in FIXTURE["sign"] if c["curve"] == curve]
    assert len(rows) == 78
    for c in rows:
        r = S.sign(cbe, curve, c["sk"], bytes.fromhex(c["msg"]))
        got = {"status": r["status"], "r_xy": r["r_xy"], "r_inf": int(r["r_inf"]), "s": r["s"], "sig_bytes": r["sig_bytes"].hex(),
               "k": r["k"], "e": r["e"], "leg": r["leg"]}
        assert got == {k: c[k] for k in got}, (c["key"], c["msg"])


def test_python_model_backend_reproduces_a_sample_of_sign_entries(pybe):
    """The fixture was generated over this backend; three entries per curve are recomputed (a multiplication in the
    Python model takes a tenth of a second)."""
    for curve in (0, 1):
        rows = [c for c in FIXTURE["sign"] if c["curve"] == curve]
        for c in (rows[0], rows[40], rows[77]):
            r = S.sign(pybe, curve, c["sk"], bytes.fromhex(c["msg"]))
            assert (r["status"], r["r_xy"], r["s"], r["sig_bytes"].hex()) == (c["status"], c["r_xy"], c["s"], c["sig_bytes"])


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_both_backends_reproduce_every_reduced_and_challenge_entry(cbe, pybe, curve):
    for c in (x for x in FIXTURE["reduced"] if x["curve"] == curve):
        for be in (cbe, pybe):
            assert S.from_bytes_reduced(curve, bytes.fromhex(c["bytes"]), be.reduce_wide) == (c["out"], c["leg"]), c["bytes"]
    rows = [x for x in FIXTURE["challenge"] if x["curve"] == curve]
    assert sorted({(c["r_inf"], c["pk_inf"]) for c in rows}) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for c in rows:
        for be in (cbe, pybe):
            assert S.challenge(be, curve, c["r_xy"], c["r_inf"], c["pk_xy"], c["pk_inf"], bytes.fromhex(c["msg"])) == (c["e"], c["leg"])


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_every_reachable_leg_is_in_the_fixture_and_no_other(curve):
    legs = [c["leg"] for c in FIXTURE["reduced"] if c["curve"] == curve]
    assert set(legs) == set(S.REACHABLE[curve])
    for leg in S.REACHABLE[curve]:
        assert legs.count(leg) >= 8, leg
    assert len(legs) >= 8 * len(S.REACHABLE[curve]) + 16


def test_unreachable_legs_stay_untaken():
    """secp256k1: only inputs with b[0..7] = FF x 7 and b[7] in {FE, FF} pass the first branch; 4096 seeded ones of that
    shape, biased towards the edges of every later comparison, take the four reachable legs and nothing else."""
    rnd = random.Random(1601)
    edge = [b"\xff" * 8, b"\xff" * 7 + b"\xfe", b"\xfe" + b"\xff" * 7, bytes(8), S.N[0][0].to_bytes(8, "big"), S.N[0][1].to_bytes(8, "big"),
            S.N[0][0].to_bytes(8, "little"), S.N[0][1].to_bytes(8, "little")]
    seen = set()
    for _ in range(4096):
        b = b"\xff" * 7 + bytes([0xFE + rnd.randrange(2)])
        for _ in range(3):
            b += rnd.choice(edge) if rnd.randrange(2) else bytes(rnd.randrange(256) for _ in range(8))
        seen.add(S.from_bytes_reduced(0, b)[1])
    assert seen == set(S.REACHABLE[0]), seen


def test_zero_key_signs_with_s_equal_to_k():
    for curve in (0, 1):
        rows = [c for c in FIXTURE["sign"] if c["curve"] == curve and c["key"] == "0" and c["status"] == 0]
        assert len(rows) == 12
        for c in rows:
            assert c["s"] == c["k"] and c["sk"] == [0, 0, 0, 0]


def test_test_message_entries_are_the_generator_and_one(cbe, pybe):
    for curve in (0, 1):
        g_c, g_py = cbe.generator_affine(curve), pybe.generator_affine(curve)
        assert g_c == g_py and g_c[1] is False
        rows = [c for c in FIXTURE["sign"] if c["curve"] == curve and c["msg"] == b"test message".hex()]
        assert len(rows) == 6
        for c in rows:
            assert (c["status"], c["r_xy"], c["r_inf"], c["s"]) == (1, g_c[0], 0, [1, 0, 0, 0])
            assert c["sig_bytes"] == (cbe.compress(curve, g_c[0], False)[:32] + bytes(31) + b"\x01").hex()


def planted_batch(n, seed):
    """The seeded inputs of the chunked GPU test (tests/test_gpu_schnorr_sign.py): random 256-bit keys, messages of mixed
    length (0..200 bytes) with b"test message" planted at 5 % of the positions."""
    import numpy as np
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    msgs = [rng.integers(0, 256, size=int(rng.integers(0, 201)), dtype=np.uint8).tobytes() for _ in range(n)]
    plant = rng.random(n) < 0.05
    return sk, [b"test message" if p else m for p, m in zip(plant, msgs)]


@pytest.mark.parametrize("curve", [0, 1])
def test_planted_batch_meets_both_status_shares_on_the_reference(curve):
    """What the GPU test asserts of the device's statuses -- at least 90 % computed, at least 2 % the message case -- holds
    for the reference on the same seeded inputs."""
    sk, msgs = planted_batch(200, 12 + curve)
    st = S.sign_many(curve, sk, msgs)["status"]
    assert (st == 0).sum() >= 180 and (st == 1).sum() >= 4 and set(st.tolist()) == {0, 1}
