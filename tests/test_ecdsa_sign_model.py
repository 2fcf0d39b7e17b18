"""
CPU checks of batched Ecdsa::<C, D>::sign (fec_ecdsa_sign): the two test-side compositions of the reference's
sign_internal + sign -- tests/golden/gen_ecdsa_sign.py over oracle/py_model.py and tests/ecdsa_sign_ref.py over the C
oracle -- agree with each other; the `half` constants committed in the device headers are the reference's
get_order() / Scalar::from(2); and the built library exports the two entry points.
"""
import ctypes
import json
import os
import random
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import ecdsa_sign_ref as R  # noqa: E402
import gen_ecdsa_sign as G  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "ecdsa_sign_vectors.json")
CSRC = os.path.join(ROOT, "forge_ec_amd", "csrc")


def _cases(curve):
    return [c for c in json.load(open(FIXTURE))["cases"] if c["curve"] == curve]


def _arrays(cases):
    sk = np.array([c["sk"] for c in cases], dtype=np.uint64)
    d = np.array([list(bytes.fromhex(c["digest"])) for c in cases], dtype=np.uint8)
    k = np.array([c["k"] for c in cases], dtype=np.uint64)
    return sk, d, k


@pytest.mark.parametrize("curve", [0, 1])
def test_c_oracle_composition_matches_fixture(oracle, curve):
    cases = _cases(curve)
    r, s, st = R.sign(oracle, curve, *_arrays(cases))
    assert st.tolist() == [c["status"] for c in cases]
    assert r.tolist() == [c["r"] for c in cases]
    assert s.tolist() == [c["s"] for c in cases]


@pytest.mark.parametrize("curve", [0, 1])
def test_compositions_agree_on_random_elements(oracle, curve):
    """256 random elements per curve: sk and k mostly below n, some arbitrary 256-bit; random digests, some >= n."""
    rng = random.Random(0x51C0 + curve)
    nv = R._val(R.N[curve])
    rows = []
    for i in range(256):
        sk = rng.randrange(1, nv) if i % 8 else rng.randrange(R.W)
        k = rng.randrange(1, nv) if i % 16 else rng.randrange(R.W)
        rows.append((G.limbs(sk), bytes(rng.randrange(256) for _ in range(32)), G.limbs(k)))
    r, s, st = R.sign(oracle, curve, [x[0] for x in rows], [list(x[1]) for x in rows], [x[2] for x in rows])
    for i, (sk, d, k) in enumerate(rows):
        want = G.sign(curve, sk, d, k)
        assert (int(st[i]), [int(v) for v in r[i]], [int(v) for v in s[i]]) == want, i


def test_fixture_reaches_every_status():
    """secp256k1: 0-3 all reachable.  P-256: 1 only for sk = 0 (its ct_lt against n holds for every other value)."""
    for curve in (0, 1):
        cases = _cases(curve)
        assert {c["status"] for c in cases} == {0, 1, 2, 3}
        rejected = [c["sk"] for c in cases if c["status"] == 1]
        if curve == 1:
            assert rejected == [[0, 0, 0, 0]]
        else:
            assert len(rejected) == 3                   # 0, n, 2^256 - 1
    for c in json.load(open(FIXTURE))["cases"]:
        if c["status"] != 0:
            assert c["r"] == [1, 0, 0, 0] and c["s"] == [1, 0, 0, 0]


def _header_half(path):
    src = open(os.path.join(CSRC, path)).read()
    body = re.search(r"FEC_DEV fe SC_HALF_\(\) \{(.*?)\n\}", src, flags=re.S).group(1)
    if "return fe_zero();" in body:
        return 0
    words = {int(i): int(v, 16) for i, v in re.findall(r"h\.w\[(\d)\] = 0x([0-9A-Fa-f]+)u;", body)}
    assert sorted(words) == list(range(8))
    return sum(words[i] << (32 * i) for i in range(8))


@pytest.mark.parametrize("curve,header", [(0, "secp256k1.hpp"), (1, "p256.hpp")])
def test_half_constants_in_device_headers(oracle, curve, header):
    """normalize's half = get_order() / Scalar::from(2) = Mul(n, invert(2)) under the reference's scalar arithmetic."""
    op = oracle.secp256k1_scalar_op if curve == 0 else oracle.p256_scalar_op
    inv2, ok = op("inv", [2, 0, 0, 0])
    assert ok                                            # Div's unwrap sees Some
    want, _ = op("mul", R.N[curve], inv2)
    assert _header_half(header) == R._val([int(v) for v in want])
    assert R._val(G.half(curve)) == R._val([int(v) for v in want])


def test_library_exports_ecdsa_sign():
    from forge_ec_amd import build
    build.build()
    lib = ctypes.CDLL(build.SO)
    for sym in ("fec_ecdsa_sign", "fec_ecdsa_sign_dev"):
        assert hasattr(lib, sym), sym
