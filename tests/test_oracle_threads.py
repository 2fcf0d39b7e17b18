"""
The batch verifiers of the C oracle with nthreads > 1 (oracle/forge_ec_oracle.c: the per-element products on
threads, the checks, folds and early returns in index order) give bit for bit what the single-threaded call gives:
the verdict, both affine sides and their infinity flags, the Ed25519 debug-build flag, ECDSA's folded sums.  These
are the references the large-batch GPU tests compare against, so a threaded oracle that differed would hide a
kernel bug or invent one.
"""
import json
import os

import numpy as np
import pytest

import vectors as V

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = (2, 7)


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def _schnorr_inputs(n, curve, seed):
    pk = V.field_elements(2 * n, curve, seed).reshape(n, 8)
    r = V.field_elements(2 * n, curve, seed + 1).reshape(n, 8)
    return pk, r, V.scalars(n, curve, seed + 2), V.scalars(n, curve, seed + 3), V.scalars(n, curve, seed + 4)


def _schnorr_call(oracle, curve, pk, pinf, r, rinf, s, a, e, nthreads):
    if curve == 2:
        res, sides, sinf, dbg = oracle.ed25519_schnorr_batch_verify(pk, pinf, r, rinf, s, a, e, nthreads=nthreads)
        return res, sides, sinf, dbg
    res, sides, sinf = oracle.schnorr_batch_verify(curve, pk, pinf, r, rinf, s, a, e, nthreads=nthreads)
    return res, sides, sinf, None


def _assert_schnorr_threads_agree(oracle, curve, pk, pinf, r, rinf, s, a, e, what):
    one = _schnorr_call(oracle, curve, pk, pinf, r, rinf, s, a, e, 1)
    for t in THREADS:
        many = _schnorr_call(oracle, curve, pk, pinf, r, rinf, s, a, e, t)
        assert many[0] == one[0], (what, t)
        assert np.array_equal(many[1], one[1]) and np.array_equal(many[2], one[2]), (what, t)
        assert many[3] == one[3], (what, t)
    return one


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_schnorr_batch_verify_threads_match_single_thread(oracle, curve):
    n = 300
    pk, r, s, a, e = _schnorr_inputs(n, curve, 4100 + 10 * curve)
    # zero scalars, all-ones scalars (every Ed25519 column sum wraps), zero weights, at both ends of the batch
    s[0] = 0
    e[1] = 0
    a[2] = 0
    s[n - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    a[n - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    a[n - 2] = 0
    res, sides, _, dbg = _assert_schnorr_threads_agree(oracle, curve, pk, None, r, None, s, a, e, "random")
    assert sides.any()
    if curve == 2:
        assert dbg == 1
    # all weights zero: true through (infinity, infinity)
    res, sides, sinf, _ = _assert_schnorr_threads_agree(oracle, curve, pk, None, r, None, s, np.zeros_like(a), e, "a = 0")
    assert res == 1 and list(sinf) == [1, 1]
    # an identity input anywhere rejects before any product
    inf = np.zeros(n, dtype=np.uint8)
    inf[n - 1] = 1
    assert _assert_schnorr_threads_agree(oracle, curve, pk, inf, r, None, s, a, e, "pk_inf")[0] == 0
    assert _assert_schnorr_threads_agree(oracle, curve, pk, None, r, inf, s, a, e, "r_inf")[0] == 0
    # fewer elements than threads
    _assert_schnorr_threads_agree(oracle, curve, pk[:3], None, r[:3], None, s[:3], a[:3], e[:3], "n = 3")


def test_schnorr_batch_verify_fixture_batches_threads_match(oracle):
    t = _load("schnorr_vectors.json")
    for key, curve in (("batch_p256", 1), ("batch_ed25519", 2)):
        for b in t[key]:
            res = _assert_schnorr_threads_agree(oracle, curve, b["pk"], None, b["r"], None, b["s"], b["a"], b["e"],
                                                b.get("kind", key))[0]
            assert res == b["result"]


def _ecdsa_inputs(n, curve, seed):
    rng = np.random.default_rng(seed)
    dg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    dg[:, 0] &= 0x7F
    r, s, a = V.scalars(n, curve, seed + 1), V.scalars(n, curve, seed + 2), V.scalars(n, curve, seed + 3)
    pk = np.ascontiguousarray(np.concatenate([V.field_elements(n, curve, seed + 4), V.field_elements(n, curve, seed + 5)], axis=1))
    return dg, r, s, pk, a


def _assert_ecdsa_threads_agree(oracle, curve, dg, r, s, pk, inf, a, what):
    st, detail = oracle.ecdsa_batch_verify(curve, dg, r, s, pk, inf, a)
    for t in THREADS:
        st_t, detail_t = oracle.ecdsa_batch_verify(curve, dg, r, s, pk, inf, a, nthreads=t)
        assert st_t == st and np.array_equal(detail_t, detail), (what, t)
    return st, detail


@pytest.mark.parametrize("curve", [0, 1])
def test_ecdsa_batch_verify_threads_match_single_thread(oracle, curve):
    n = 300
    dg, r, s, pk, a = _ecdsa_inputs(n, curve, 4200 + 10 * curve)
    inf = np.zeros(n, dtype=np.uint8)
    inf[::37] = 1
    a[5] = 0
    st, detail = _assert_ecdsa_threads_agree(oracle, curve, dg, r, s, pk, inf, a, "random")
    assert st == 0 and detail.any()                 # every product computed, the final comparison fails
    # early exits: the first failing signature in index order decides, however the products were split
    r3 = r.copy(); r3[200] = 0
    assert _assert_ecdsa_threads_agree(oracle, curve, dg, r3, s, pk, None, a, "r = 0 at 200")[0] == 0
    dg4 = dg.copy(); dg4[17] = 0xFF
    assert _assert_ecdsa_threads_agree(oracle, curve, dg4, r3, s, pk, None, a, "panic at 17")[0] == 2
    s5 = s.copy(); s5[3] = 0
    assert _assert_ecdsa_threads_agree(oracle, curve, dg4, r, s5, pk, None, a, "s = 0 at 3")[0] == 0
    dg6 = dg.copy(); dg6[n - 1] = 0xFF
    assert _assert_ecdsa_threads_agree(oracle, curve, dg6, r, s, pk, None, a, "panic at the last")[0] == 2
    _assert_ecdsa_threads_agree(oracle, curve, dg[:3], r[:3], s[:3], pk[:3], None, a[:3], "n = 3")


def test_ecdsa_batch_verify_fixture_batches_threads_match(oracle):
    for c in _load("ecdsa_batch_vectors.json")["cases"]:
        dg = np.frombuffer(bytes.fromhex("".join(c["digests"])), dtype=np.uint8).reshape(-1, 32)
        st, _ = _assert_ecdsa_threads_agree(oracle, c["curve"], dg, c["r"], c["s"], c["pk"], c["pk_inf"], c["a"], c["note"])
        assert st == c["status"], c["note"]
