"""
CPU checks of the device hash-to-curve code through a host build of forge_ec_amd/csrc/h2c.hpp (tests/cpp/h2c_host.cpp),
the per-element code kernels_h2c.hip runs: it reproduces tests/golden/h2c_vectors.json, and it forces the legs no message
reaches -- the os2ip fallbacks (bytes not below p on each curve, the i + 1 and zero variants of the trait method) and
secp256k1's valid_point and w == 0 legs, by calling the finishing step with chosen flags.
(The same source builds as a stand-alone program, -DH2C_HOST_MAIN, for a sanitizer run: DESIGN.md section 18.)
"""
import ctypes
import json
import os
import subprocess

import pytest

import h2c_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "h2c_vectors.json")))
U64x4 = ctypes.c_uint64 * 4
P_BYTES = {R.SECP: (2**256 - 2**32 - 977).to_bytes(32, "big"), R.P256: (2**256 - 2**224 + 2**192 + 2**96 - 1).to_bytes(32, "big")}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("h2c") / "h2c_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cpp", "h2c_host.cpp")])
    return ctypes.CDLL(so)


def _buf(b):
    return ctypes.create_string_buffer(bytes(b), max(len(b), 4))   # (the hash loads whole aligned dwords)


def _xmd(lib, msg, dst, out_len):
    out = ctypes.create_string_buffer(max(out_len, 1) + 8)
    out.raw = b"\xA5" * (max(out_len, 1) + 8)
    assert lib.h2c_xmd(_buf(msg), ctypes.c_size_t(len(msg)), _buf(dst), ctypes.c_size_t(len(dst)), ctypes.c_size_t(out_len), out) == 0
    assert out.raw[out_len:out_len + 8] == b"\xA5" * 8
    return out.raw[:out_len]


def _hash(lib, curve, form, msg, dst):
    out, cand, legs, inf = (ctypes.c_uint64 * 12)(), (ctypes.c_uint64 * 16)(), (ctypes.c_uint8 * 2)(), ctypes.c_uint8(0)
    assert lib.h2c_hash(curve, form, _buf(msg), ctypes.c_size_t(len(msg)), _buf(dst), ctypes.c_size_t(len(dst)), out, ctypes.byref(inf),
                        cand, legs) == 0
    return list(out), list(cand), list(legs), inf.value


def test_expander_fixture(host):
    for msg, want in FIXTURE["k1"]:
        assert _xmd(host, bytes.fromhex(msg), R.K1_DST, 32).hex() == want
    pool = bytes.fromhex(FIXTURE["pool"])
    for m, d, o, want in FIXTURE["xmd"]:
        assert _xmd(host, pool[:m], R.dst_of(d), o).hex() == want, (m, d, o)
    assert host.h2c_xmd(None, ctypes.c_size_t(0), None, ctypes.c_size_t(256), ctypes.c_size_t(32), None) == -1
    assert host.h2c_xmd(None, ctypes.c_size_t(0), None, ctypes.c_size_t(0), ctypes.c_size_t(8161), None) == -1


def test_hash_to_field_fixture(host):
    for curve, d, count, msgs, u in FIXTURE["field"]:
        for m, want in zip(msgs, u):
            m = bytes.fromhex(m)
            out, fell = (ctypes.c_uint64 * (4 * count))(), (ctypes.c_uint8 * count)()
            assert host.h2c_hash_to_field(curve, _buf(m), ctypes.c_size_t(len(m)), _buf(R.dst_of(d)), ctypes.c_size_t(d),
                                          ctypes.c_size_t(count), out, fell) == 0
            assert list(out) == want and not any(fell)


@pytest.mark.parametrize("paired", [0, 1])
def test_map_fixture(host, paired):
    for curve in (R.SECP, R.P256):
        cases = [c for c in FIXTURE["map"] if c[0] == curve]
        n = len(cases)
        u = (ctypes.c_uint64 * (4 * n))(*[v for c in cases for v in c[2]])
        xy, cand, legs = (ctypes.c_uint64 * (8 * n))(), (ctypes.c_uint64 * (8 * n))(), (ctypes.c_uint8 * n)()
        host.h2c_map(curve, u, xy, cand, legs, ctypes.c_size_t(n), paired)
        for i, c in enumerate(cases):
            assert (list(xy[8 * i:8 * i + 8]), list(cand[8 * i:8 * i + 8]), legs[i]) == (c[3], c[4], c[5]), c[1]


def test_fused_forms_fixture(host):
    for case in FIXTURE["curve"]:
        curve, dst = case["curve"], R.dst_of(case["dst_len"])
        for i, m in enumerate(case["msgs"]):
            m = bytes.fromhex(m)
            out, _, _, inf = _hash(host, curve, 2, m, dst)
            assert [out[:8], inf] == case["trait"][i]
            if case["dst_len"]:
                for form, name, maps in ((0, "hash", 2), (1, "encode", 1)):
                    out, cand, legs, _ = _hash(host, curve, form, m, dst)
                    want = case[name][i]
                    assert out == want[0] and cand[:8 * maps] == [v for c in want[1] for v in c] and legs[:maps] == want[2]


@pytest.mark.parametrize("curve", [R.SECP, R.P256])
def test_os2ip_fallback_is_forced(host, curve):
    p = P_BYTES[curve]
    below = (int.from_bytes(p, "big") - 1).to_bytes(32, "big")
    for b, fell in ((p, 1), (b"\xff" * 32, 1), (below, 0)):
        u, f = U64x4(), ctypes.c_uint8(7)
        host.h2c_os2ip(curve, b, u, ctypes.byref(f))
        want, wf = R.os2ip_mod_p(curve, b)
        assert (list(u), f.value) == (want, int(wf)) and f.value == fell
        if fell:
            assert list(u) == [1, 0, 0, 0]


def test_trait_method_fallbacks_are_forced(host):
    # secp256k1 (1739-1747): element i falls back to from_raw([i + 1, 0, 0, 0]); bytes [32, 48) and [80, 96) are unused
    p = P_BYTES[R.SECP]
    good = bytes(range(1, 33))
    for b0, b1 in ((p, good), (good, p), (p, b"\xff" * 32)):
        ub = b0 + b"\xEE" * 16 + b1 + b"\xEE" * 16
        u, fell = (ctypes.c_uint64 * 8)(), (ctypes.c_uint8 * 2)()
        host.h2c_trait_elements(R.SECP, ub, u, fell)
        for i, b in enumerate((b0, b1)):
            v, ok = R.M.field_from_bytes(R.SECP, b)
            assert list(u[4 * i:4 * i + 4]) == (list(v) if ok else [i + 1, 0, 0, 0]) and fell[i] == (0 if ok else 1)
    # P-256 (core lib.rs:1569-1570): unwrap_or(zero)
    u, fell = (ctypes.c_uint64 * 8)(), (ctypes.c_uint8 * 2)()
    host.h2c_trait_elements(R.P256, P_BYTES[R.P256], u, fell)
    assert list(u[:4]) == [0, 0, 0, 0] and fell[0] == 1
    host.h2c_trait_elements(R.P256, good, u, fell)
    assert list(u[:4]) == R.M.field_from_bytes(R.P256, good)[0] and fell[0] == 0


def test_secp256k1_valid_point_and_zero_w_are_forced(host):
    u = [3, 0, 0, 0]
    eu, legs0, w, x, y2 = R.secp_map_parts(u)
    for s in ([5, 0, 0, 0], [6, 0, 0, 0], [0x1234, 7, 8, 9]):
        for dz in (0, 1):
            for some in (0, 1):
                xy, cand, legs = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), ctypes.c_uint8(0)
                host.h2c_finish(R.SECP, U64x4(*u), dz, U64x4(*s), some, xy, cand, ctypes.byref(legs))
                # with w forced to zero the reference's w_inv is zero, and with it x
                xx, yy2 = (x, y2) if not dz else ([0, 0, 0, 0], R.M.Secp.mul([7, 0, 0, 0], R.SECP_R2))
                pt, want_legs = R.secp_map_finish(eu, legs0 | (R.LEG_INV_ZERO if dz else 0), xx, yy2, s, bool(some))
                assert (list(xy[:4]), list(xy[4:]), legs.value) == (pt[0], pt[1], want_legs)
                assert list(cand) == list(xx) + list(yy2)
                if some and not dz:
                    assert list(xy[:4]) == x and list(xy[4:]) in (s, R.M.Secp.neg(s))       # the valid_point leg
                else:
                    assert list(xy[:4]) == list(R.SECP_DEFAULT[0])


def test_p256_finishing_step_with_a_root(host):
    u = [2, 0, 0, 0]
    legs0, x, y2 = R.p256_map_parts(u)
    for s in ([4, 0, 0, 0], [5, 0, 0, 0]):
        xy, cand, legs = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), ctypes.c_uint8(0)
        host.h2c_finish(R.P256, U64x4(*u), 0, U64x4(*s), 1, xy, cand, ctypes.byref(legs))
        pt, want = R.p256_map_finish(u, legs0, x, s, True)
        assert (list(xy[:4]), list(xy[4:]), legs.value) == (pt[0], pt[1], want)
