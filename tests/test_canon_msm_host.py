"""
CPU checks of the per-lane code of fec_canon_msm through a host build of forge_ec_amd/csrc/canon_msm.hpp
(tests/cpp/canon_msm_host.cpp): the signed-digit recoding for every window width on the scalars that steer it and 10^4 random
ones per width; the segment reduction against the model's sum b * B_b with empty buckets, a bucket holding infinity and neighbouring
buckets holding P and -P; and the whole pipeline -- the kernels' lane functions run serially in the kernels' order -- over
every case of tests/golden/canon_msm_vectors.json.  The same source builds as a stand-alone program
(-DCANON_MSM_HOST_MAIN); test_stand_alone_program_under_sanitizers builds it with -fsanitize=address,undefined
-fno-sanitize-recover=undefined and runs it directly.
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import canon_msm_ref as R
from oracle import canon_model as CM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "canon_msm_host.cpp")
FX = R.load_fixture()
NAMES = sorted(R.MODELS)
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_msm") / "canon_msm_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    return ctypes.CDLL(so)


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "canon_msm_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DCANON_MSM_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


def _digits(host, k, c):
    kw = (ctypes.c_uint32 * 8)(*[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    d = (ctypes.c_int32 * 129)()
    W = host.cm_recode(kw, c, d)
    return list(d[:W])


@pytest.mark.parametrize("c", range(2, 17))
def test_recoding(host, c):
    rng = random.Random(0x2800 + c)
    ks = set()
    for N in (CM.SECP256K1.N, CM.P256.N, CM.ED25519.N):
        ks |= {0, 1, 2**(c - 1) - 1, 2**(c - 1), 2**(c - 1) + 1, 2**c - 1, 2**c, N - 1, N, N + 1, 2**255, 2**256 - 1}
    ks = sorted(ks) + [rng.getrandbits(256) for _ in range(10**4)]
    for k in ks:
        d = _digits(host, k, c)
        assert len(d) == (257 + c - 1) // c
        assert sum(v << (c * w) for w, v in enumerate(d)) == k, (c, hex(k))
        assert max(abs(v) for v in d) <= 2**(c - 1), (c, hex(k))


def test_the_run_splits_a_513_element_bucket_at_least_twice(host):
    assert 513 // host.cm_run() >= 3


def _reduce(host, name, buckets):
    """buckets: B entries, None (empty), "inf" (infinity as an addition leaves it) or a point"""
    B = len(buckets)
    state = (ctypes.c_ubyte * B)(*[0 if b is None else (2 if b == "inf" else 1) for b in buckets])
    xy = np.zeros((B, 16), dtype=np.uint32)
    for i, b in enumerate(buckets):
        if isinstance(b, tuple):
            xy[i] = np.array(CM.limbs(b[0]) + CM.limbs(b[1]), dtype=np.uint64).view(np.uint32)
    out = np.zeros(16, dtype=np.uint32)
    st = host.cm_reduce(R.CURVE_ID[name], B, state, xy.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    o = [int(v) for v in out.view(np.uint64)]
    return o, st


@pytest.mark.parametrize("name", NAMES)
def test_segment_reduction(host, name):
    C, rng = R.MODELS[name], random.Random("msm-reduce/" + name)
    seg = host.cm_seg()
    pool = [p for _, _, p in FX.pool(name)]
    for B in (1, 2, 16, seg, seg + 1, 4 * seg, 4 * seg + 5):
        buckets = [rng.choice([None, None, "inf", rng.choice(pool)]) for _ in range(B)]
        if B >= 16:
            buckets[5], buckets[6] = pool[0], C.neg(pool[0])      # neighbours P, -P
            buckets[B - 1], buckets[B - 2] = pool[1], pool[1]     # neighbours P, P: the running sums meet a doubling
        want = R.identity(name)
        for b, v in enumerate(buckets, 1):
            if isinstance(v, tuple):
                want = C.add(want, C.mul(b, v))
        assert _reduce(host, name, buckets) == R.result(name, want), B
    assert _reduce(host, name, [None] * (2 * seg)) == R.result(name, R.identity(name))


def _msm(host, name, c, cap, ks, pts):
    k, p = R.pack(ks, pts)
    out, st = np.zeros(8, dtype=np.uint64), (ctypes.c_ubyte * 1)(9)
    host.cm_msm(R.CURVE_ID[name], c, SZ(cap), SZ(len(ks)), k.ctypes.data_as(ctypes.c_void_p), p.ctypes.data_as(ctypes.c_void_p),
                out.ctypes.data_as(ctypes.c_void_p), st)
    return [int(v) for v in out], st[0]


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_over_the_fixture(host, name):
    for case in FX.cases(name):
        ks, pts = [int(v, 16) for v in case["k"]], FX.points(name, case["p"])
        want = (CM.limbs(int(case["x"], 16)) + CM.limbs(int(case["y"], 16)), case["status"])
        for c, cap in ((2, 7), (4, 200), (5, 33), (8, 16), (8, 200)):
            assert _msm(host, name, c, cap, ks, pts) == want, (case["name"], c, cap)


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_at_the_wide_windows(host, name):
    """13 and 16 bits: many reduce segments per window, non-zero segment bases; one case each (the reduce dominates on a CPU)"""
    case = next(c for c in FX.cases(name) if c["name"] == "random-40")
    ks, pts = [int(v, 16) for v in case["k"]], FX.points(name, case["p"])
    want = (CM.limbs(int(case["x"], 16)) + CM.limbs(int(case["y"], 16)), case["status"])
    assert _msm(host, name, 13, 17, ks, pts) == want
    if name == "secp256k1":
        assert _msm(host, name, 16, 40, ks, pts) == want


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_refuses_a_bad_point(host, name):
    C = R.MODELS[name]
    case = next(c for c in FX.cases(name) if c["name"] == "random-40")
    ks, pts = [int(v, 16) for v in case["k"]], FX.points(name, case["p"])
    for at in (0, 20, 39):
        for bad in ((C.P, pts[at][1]), (pts[at][0], C.P), (pts[at][0], (pts[at][1] + 1) % C.P)):
            spoiled = list(pts)
            spoiled[at] = bad
            assert _msm(host, name, 4, 16, ks, spoiled) == ([0] * 8, R.BAD_POINT)
