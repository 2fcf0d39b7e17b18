"""
CPU checks of the Curve25519 parity restatements and of the device header, without a GPU:
  * the reference's own KATs (curve25519.rs:2010-2034, 2128-2155) on all three forms;
  * tests/cpp/x25519_ref.cpp (written from the Rust) against tests/x25519_ref.py on >= 2000 random and crafted inputs
    per function;
  * Mul against exact a * b mod p where no quirk can fire (products below 2^255);
  * the host build of forge_ec_amd/csrc/curve25519.hpp (tests/cpp/x25519_host.cpp) against the restatements: field ops,
    one ladder step, invert and full x25519;
  * the rare-leg census tests/x25519_rare_legs.json, each forced leg confirmed reached;
  * the fixture tests/golden/x25519_vectors.json is what tests/golden/gen_x25519.py's restatement computes.
"""
import ctypes
import json
import multiprocessing
import os
import random
import re
import subprocess

import numpy as np
import pytest

import x25519_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "forge_ec_amd", "csrc")
FIX = json.load(open(os.path.join(HERE, "golden", "x25519_vectors.json")))
CENSUS = json.load(open(os.path.join(HERE, "x25519_rare_legs.json")))
M = X.M64
P = sum(v << (64 * i) for i, v in enumerate(X.P))
G = ([9, 0, 0, 0], [1, 0, 0, 0])
PATTERNS = [0, 1, 2, 19, M, M - 1, M - 18, 1 << 63, (1 << 63) - 1, 0xFFFFFFFF, 0xFFFFFFFF00000000]


def _build(tmp, name, extra=()):
    so = str(tmp / (name + ".so"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", *extra, "-o", so,
                           os.path.join(HERE, "cpp", name + ".cpp")])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    lib = _build(tmp_path_factory.mktemp("xr"), "x25519_ref")
    lib.xr_field_op.restype = ctypes.c_uint
    lib.xr_x25519.restype = ctypes.c_uint
    lib.xr_multiply.restype = ctypes.c_uint
    lib.xr_x25519_batch.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = _build(tmp_path_factory.mktemp("xh"), "x25519_host")
    lib.xh_rare_leg_name.restype = ctypes.c_char_p
    return lib


def arr(v):
    return (ctypes.c_uint64 * len(v))(*[int(x) for x in v])


def c_field(lib, fn, op, a, b):
    o = arr([0] * 4)
    getattr(lib, fn)(op, arr(a), arr(b if b is not None else [0] * 4), o)
    return list(o)


def c_x25519(lib, fn, s, u):
    o = ctypes.create_string_buffer(32)
    getattr(lib, fn)(bytes(s), bytes(u), o)
    return o.raw


def c_multiply(lib, x, z, k):
    o = arr([0] * 8)
    lib.xr_multiply(arr(k), arr(list(x) + list(z)), o)
    return list(o)


def counters(host):
    names = [host.xh_rare_leg_name(i).decode() for i in range(host.xh_rare_leg_count())]
    buf = (ctypes.c_ulong * len(names))()
    host.xh_rare_legs(buf)
    return dict(zip(names, buf[:]))


def rand_limbs(rng):
    return [rng.choice(PATTERNS) if rng.random() < 0.3 else rng.getrandbits(64) for _ in range(4)]


def leg_cases():
    return [c for c in FIX["field"] if c["legs"]]


def rand_bytes(rng):
    return bytes(rng.getrandbits(8) for _ in range(32))


def x25519_inputs(n, seed):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        s, u = rand_bytes(rng), rand_bytes(rng)
        if i % 50 == 0:
            s = bytes([2] + [0] * 31)
        elif i % 50 == 1:
            u = bytes(32)
        elif i % 50 == 2:
            u = X.to_bytes([rng.getrandbits(64), M, M, M])           # >= p before reduce, top bit set
        elif i % 50 == 3:
            u = X.to_bytes([rng.choice(PATTERNS) for _ in range(4)])
        out.append((s, u))
    return out


def multiply_inputs(n, seed):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        k = [rng.getrandbits(64) for _ in range(4)]
        x, z = rand_limbs(rng), rand_limbs(rng)
        sel = i % 16
        if sel < 4:
            k = [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 2 << 56]][sel]
        elif sel == 4:
            z = [0, 0, 0, 0]
        out.append((x, z, k))
    return out


def _py_x25519(args):
    return X.x25519(*args)


def _py_multiply(args):
    x, z, k = args
    ox, oz = X.multiply(x, z, k)
    return ox + oz


def _pool_map(fn, items):
    with multiprocessing.get_context("fork").Pool(min(16, os.cpu_count() or 1)) as pool:
        return pool.map(fn, items, chunksize=16)


# ---- the reference's KATs ---------------------------------------------------------------------------------------

def test_reference_kats(cref, host):
    one, two = [1, 0, 0, 0], [2, 0, 0, 0]
    for lib, fn in ((cref, "xr_field_op"), (host, "xh_field_op"), (None, None)):
        f = (lambda op, a, b=None: X.FIELD_OPS[op](a, b)) if lib is None else (lambda op, a, b=None: c_field(lib, fn, op, a, b))
        c = f(0, one, two)
        assert c[0] == 3
        assert f(1, c, one)[0] == 2
        assert f(2, one, two)[0] == 2
        assert f(0, one, f(4, one)) == [0, 0, 0, 0]
    assert X.mul(one, X.invert(one)) == one
    out = arr([0] * 4)
    assert cref.xr_invert(arr(one), out) == 1 and list(out) == one
    assert cref.xr_invert(arr([0] * 4), out) == 0                                # invert(0) is None
    host.xh_invert_or_zero(arr(one), out)
    assert list(out) == one
    # the scalar-2 constant (1626-1632) and multiply by 0, 1, 2 (2128-2145)
    s2 = bytes([2] + [0] * 31)
    for fn in (lambda s, u: X.x25519(s, u), lambda s, u: c_x25519(cref, "xr_x25519", s, u),
               lambda s, u: c_x25519(host, "xh_x25519", s, u)):
        assert fn(s2, bytes(range(32))) == X.SCALAR2_RESULT
    assert X.multiply(*G, [1, 0, 0, 0]) == G
    assert X.multiply(*G, [2, 0, 0, 0]) == X.double(*G)
    ox, oz = X.multiply(*G, [0, 0, 0, 0])
    assert X.is_zero(oz)
    for k in ([0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 2 << 56]):
        ox, oz = X.multiply(*G, k)
        assert c_multiply(cref, *G, k) == ox + oz
    # raw [0, 0, 0, 2 << 56] reaches x25519's special case through the big-endian Scalar::to_bytes
    assert X.multiply(*G, [0, 0, 0, 2 << 56])[0] == X.from_bytes(X.SCALAR2_RESULT)[0]
    pd = arr([0] * 8)
    host.xh_pdouble(arr(G[0] + G[1]), pd)
    assert list(pd) == sum(X.double(*G), [])


# ---- C++ restatement against Python -----------------------------------------------------------------------------

def test_cpp_field_ops_match_python(cref):
    rng = random.Random(1)
    cases = [(c["a"], c["b"]) for c in FIX["field"]]
    while len(cases) < 2000:
        cases.append((rand_limbs(rng), rand_limbs(rng)))
    for op in range(5):
        for a, b in cases:
            assert c_field(cref, "xr_field_op", op, a, b) == X.FIELD_OPS[op](a, b), (op, a, b)


def test_cpp_invert_and_ladder_step_match_python(cref):
    rng = random.Random(2)
    out = arr([0] * 4)
    for i in range(2000):
        a = rand_limbs(rng) if i % 4 else [rng.getrandbits(64) for _ in range(3)] + [rng.getrandbits(63)]
        if i < 300:
            ok = cref.xr_invert(arr(a), out)
            want = X.invert(a)
            assert bool(ok) == (want is not None) and (want is None or list(out) == want), a
        st = [rand_limbs(rng) for _ in range(5)]
        o = arr([0] * 16)
        cref.xr_ladder_step(arr(sum(st, [])), o)
        assert list(o) == sum(X.ladder_step(*st), []), st


def test_cpp_x25519_matches_python(cref):
    items = x25519_inputs(2000, 3)
    want = _pool_map(_py_x25519, items)
    for (s, u), w in zip(items, want):
        assert c_x25519(cref, "xr_x25519", s, u) == w, (s.hex(), u.hex())
    s = np.frombuffer(b"".join(a for a, _ in items), dtype=np.uint8).reshape(-1, 32).copy()
    u = np.frombuffer(b"".join(b for _, b in items), dtype=np.uint8).reshape(-1, 32).copy()
    o = np.zeros_like(s)
    cref.xr_x25519_batch(s.ctypes.data, u.ctypes.data, o.ctypes.data, s.shape[0], 4)
    assert [bytes(r) for r in o] == want


def test_cpp_multiply_matches_python(cref):
    items = multiply_inputs(2000, 4)
    want = _pool_map(_py_multiply, items)
    for (x, z, k), w in zip(items, want):
        assert c_multiply(cref, x, z, k) == w, (x, z, k)


def test_mul_is_exact_below_2p255(cref, host):
    """no quirk can fire when a * b < 2^255: Mul is then the exact product (which is below p or reduced once)"""
    rng = random.Random(5)
    for _ in range(3000):
        la = rng.randrange(1, 254)
        a = rng.getrandbits(la)
        b = rng.getrandbits(254 - la)
        al = [(a >> (64 * i)) & M for i in range(4)]
        bl = [(b >> (64 * i)) & M for i in range(4)]
        want = (a * b) % P
        wl = [(want >> (64 * i)) & M for i in range(4)]
        assert X.mul(al, bl) == wl
        assert c_field(cref, "xr_field_op", 2, al, bl) == wl
        assert c_field(host, "xh_field_op", 2, al, bl) == wl


# ---- host build of the device header ------------------------------------------------------------------------------

def test_host_header_field_ops(host):
    rng = random.Random(6)
    cases = [(c["a"], c["b"]) for c in FIX["field"]]
    while len(cases) < 2000:
        cases.append((rand_limbs(rng), rand_limbs(rng)))
    for op in range(5):
        for a, b in cases:
            assert c_field(host, "xh_field_op", op, a, b) == X.FIELD_OPS[op](a, b), (op, a, b)
    for _ in range(2000):
        e = rand_limbs(rng)
        assert c_field(host, "xh_field_op", 5, e, None) == X.mul(X.A, e), e


def test_host_header_ladder_step_invert_x25519(host):
    rng = random.Random(7)
    for _ in range(500):
        st = [rand_limbs(rng) for _ in range(5)]
        o = arr([0] * 16)
        host.xh_ladder_step(arr(sum(st, [])), o)
        assert list(o) == sum(X.ladder_step(*st), []), st
    out = arr([0] * 4)
    for i in range(256):
        a = rand_limbs(rng) if i else [0, 0, 0, 0]
        host.xh_invert_or_zero(arr(a), out)
        want = X.invert(a)
        assert list(out) == (want if want is not None else [0, 0, 0, 0]), a
    items = x25519_inputs(256, 8)
    want = _pool_map(_py_x25519, items)
    for (s, u), w in zip(items, want):
        assert c_x25519(host, "xh_x25519", s, u) == w, (s.hex(), u.hex())


# ---- rare-leg census ---------------------------------------------------------------------------------------------------

def rare_sites():
    out = []
    for f in ("curve25519.hpp", "kernels_x25519.hip"):
        fn, seen = None, {}
        for line in open(os.path.join(CSRC, f)):
            if re.match(r"(FEC_DEV|__global__)\b", line):
                fn = re.search(r"(\w+)\s*\(", re.sub(r"__launch_bounds__\([^)]*\)", "", line)).group(1)
            for _ in re.finditer(r"__builtin_expect\(", line.split("//")[0]):
                k = seen.get(fn, 0)
                seen[fn] = k + 1
                out.append("%s::%s#%d" % (f, fn, k))
    return out


def test_census_names_every_rare_leg(host):
    found = rare_sites()
    assert sorted(found) == sorted(CENSUS["legs"]), (sorted(found), sorted(CENSUS["legs"]))
    names = set(counters(host))
    assert names == {leg["counter"] for leg in CENSUS["legs"].values() if leg["counter"]}
    for key, leg in CENSUS["legs"].items():
        assert leg["status"] in ("forced", "routine") and leg["how"], key
    old = json.load(open(os.path.join(HERE, "rare_legs.json")))
    assert not set(found) & (set(old["legs"]) | set(old.get("excluded", {})))


def test_forced_legs_are_reached(cref, host):
    # Mul: every fixture leg case fires its leg in the C++ restatement (bit set 1 c1, 2 c3, 4 f2), the literal leg of
    # the header's mul, and gives the restatement's value
    bits = {"c1": 1, "c3": 2, "f2": 4}
    for c in leg_cases():
        before = counters(host)["X25519_MUL_LITERAL"]
        assert c_field(host, "xh_field_op", 2, c["a"], c["b"]) == c["expect"]
        assert counters(host)["X25519_MUL_LITERAL"] > before, c["legs"]
        o = arr([0] * 4)
        assert cref.xr_field_op(2, arr(c["a"]), arr(c["b"]), o) & bits[c["legs"][0]], c["legs"]
        X.LEGS.clear()
        X.mul(c["a"], c["b"])
        assert X.LEGS == set(c["legs"])
    # Mul(A, e): e = ceil((2^64 - 1) * 2^128 / A)
    e = -(-(M << 128) // 486662)
    el = [(e >> (64 * i)) & M for i in range(4)]
    before = counters(host)["X25519_MULA_LITERAL"]
    assert c_field(host, "xh_field_op", 5, el, None) == X.mul(X.A, el)
    assert counters(host)["X25519_MULA_LITERAL"] > before
    # invert(0): the fixture's u = 0 cases; reduce's top leg: any x25519
    for c in FIX["x25519"]:
        if c["family"] in ("u_zero", "z2_zero"):
            before = counters(host)
            assert c_x25519(host, "xh_x25519", bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"])).hex() == c["expect"]
            after = counters(host)
            assert after["X25519_INVERT_ZERO"] > before["X25519_INVERT_ZERO"]
            assert after["X25519_REDUCE_TOP"] > before["X25519_REDUCE_TOP"]
    assert {c["family"] for c in FIX["multiply"]} >= {"k_two", "k_two_unreduced"}


def test_random_operands_reach_no_mul_leg(host):
    """the forcing is needed: random operands take neither literal Mul leg"""
    rng = random.Random(9)
    before = counters(host)
    for _ in range(3000):
        a = [rng.getrandbits(64) for _ in range(4)]
        b = [rng.getrandbits(64) for _ in range(4)]
        c_field(host, "xh_field_op", 2, a, b)
        c_field(host, "xh_field_op", 5, a, None)
    after = counters(host)
    assert after["X25519_MUL_LITERAL"] == before["X25519_MUL_LITERAL"]
    assert after["X25519_MULA_LITERAL"] == before["X25519_MULA_LITERAL"]


def test_fixture_matches_restatement():
    for c in FIX["field"]:
        assert X.FIELD_OPS[c["op"]](c["a"], c["b"]) == c["expect"]
    for c in FIX["x25519"][:12]:
        assert X.x25519(bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"])).hex() == c["expect"], c["family"]
    for c in FIX["multiply"][:10]:
        ox, oz = X.multiply(c["point"][:4], c["point"][4:], c["scalar"])
        assert ox + oz == c["expect"], c["family"]
    assert {c["family"] for c in FIX["x25519"]} >= {"scalar_two", "u_zero", "u_top_bit", "u_is_p", "z2_zero"}
    assert FIX["searches"][0]["hits"] >= 1
