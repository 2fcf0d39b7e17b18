"""
CPU checks of the reference module of fec_canon_msm (tests/canon_msm_ref.py) against published values -- SEC 2's 3 G, the
RFC 6979 A.2.5 P-256 public key, the RFC 8032 test 1 public key -- and of its logarithm shortcut against the direct sum of
model multiplications; the fixture's recorded sums are re-derived as well.
"""
import random

import pytest

import canon_msm_ref as R
from oracle import canon_model as CM

FX = R.load_fixture()
NAMES = sorted(R.MODELS)


def test_one_plus_two_g_is_sec2_3g():
    C = CM.SECP256K1
    assert R.msm_direct("secp256k1", [1, 1], [C.G, C.KNOWN_MULTIPLES[2]]) == C.KNOWN_MULTIPLES[3]


def test_rfc6979_p256_public_key():
    C = CM.P256
    x = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
    assert R.msm_direct("p256", [x], [C.G]) == C.KNOWN_MULTIPLES[x]
    assert R.msm_by_logs("p256", [x], [1]) == C.KNOWN_MULTIPLES[x]


def test_rfc8032_test1_public_key():
    E = CM.ED25519
    seed, pk = CM.ED25519_RFC8032_TEST1
    a = E.secret_scalar(seed)
    assert E.encode(R.msm_direct("ed25519", [a], [E.G])) == pk
    assert E.encode(R.msm_by_logs("ed25519", [a], [1], [0], FX.T("ed25519"))) == pk


def test_the_torsion_generator_has_order_8():
    E, T = CM.ED25519, FX.T("ed25519")
    assert E.on_curve(T) and E.mul(8, T) == E.IDENTITY and E.mul(4, T) != E.IDENTITY
    assert len({E.mul(j, T) for j in range(8)}) == 8


@pytest.mark.parametrize("name", NAMES)
def test_pool_points_are_their_logarithms(name):
    C, pool = R.MODELS[name], FX.pool(name)
    assert len(pool) == 64 and len({p for _, _, p in pool}) == 64
    for a, j, p in pool[::7]:
        want = C.mul(a, C.G)
        if R.is_ed(name):
            want = C.add(want, C.mul(j, FX.T(name)))
        assert p == want and C.on_curve(p)


@pytest.mark.parametrize("name", NAMES)
def test_shortcut_equals_direct_sum(name):
    rng = random.Random("msm-model/" + name)
    C = R.MODELS[name]
    for case in range(50):
        n = rng.randrange(0, 5)
        ks = [rng.choice([rng.getrandbits(256), rng.randrange(C.N), R.TOP, 0, C.N, C.N + 1]) for _ in range(n)]
        refs = [rng.choice([rng.randrange(64), -rng.randrange(1, 65)] + (["t%d" % rng.randrange(8), "id"] if R.is_ed(name) else []))
                for _ in range(n)]
        assert FX.expected(name, ks, refs) == R.msm_direct(name, ks, FX.points(name, refs)), case


def test_scalars_are_not_reduced_on_ed25519_torsion():
    """k and k mod l differ on a torsion point, and the reference says so (it is what the GPU test relies on)"""
    E, name = CM.ED25519, "ed25519"
    assert FX.expected(name, [E.N + 1], ["t1"]) == E.mul((E.N + 1) % 8, FX.T(name)) != E.mul(1, FX.T(name))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_hold_the_models_sums(name):
    names = [c["name"] for c in FX.cases(name)]
    assert {"empty", "single", "equal-scalars-64", "one-point-50", "k-P-and-k-minus-P", "k-P-and-N-minus-k-P", "zeros-20", "all-ones-20",
            "top-bucket-2^255", "steering"} <= set(names)
    for c in FX.cases(name):
        ks = [int(v, 16) for v in c["k"]]
        xy, st = R.result(name, FX.expected(name, ks, c["p"]))
        assert (CM.unlimbs(xy[:4]), CM.unlimbs(xy[4:]), st) == (int(c["x"], 16), int(c["y"], 16), c["status"]), c["name"]
    inf = {c["name"]: c["status"] for c in FX.cases(name)}
    want = R.FINITE if R.is_ed(name) else R.INFINITY
    assert inf["empty"] == inf["k-P-and-k-minus-P"] == inf["k-P-and-N-minus-k-P"] == inf["zeros-20"] == want
