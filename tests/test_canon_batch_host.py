"""
CPU checks of the per-lane code of fec_canon_bip340_batch_verify_msg / fec_canon_ed25519_batch_verify_msg through a host build
of forge_ec_amd/csrc/canon_batch.hpp (tests/cpp/canon_batch_host.cpp): the coefficient against hashlib, and the whole call --
the kernels' lane functions run serially in the kernels' order on the kernels' buffer layout, fed to canon_msm.hpp's host
pipeline, the verdict function run on the result -- against the model (tests/canon_batch_ref.py) over every case of
tests/golden/canon_batch_vectors.json.  The same source builds as a stand-alone program (-DCANON_BATCH_HOST_MAIN);
test_stand_alone_program_under_sanitizers builds it with -fsanitize=address,undefined -fno-sanitize-recover=undefined and runs
it directly.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import canon_batch_ref as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "canon_batch_host.cpp")
FX = B.load_fixture()
SZ, U64, U32 = ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("canon_batch") / "canon_batch_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    return ctypes.CDLL(so)


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "canon_batch_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DCANON_BATCH_HOST_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout + out.stderr


def _words(a):
    return sum(int(v) << (32 * i) for i, v in enumerate(a))


def test_coefficient_is_the_models(host):
    mid = (U32 * 8)()
    host.cb_midstate(mid)
    assert list(mid) == B.tag_midstate()
    out = (U32 * 8)()
    for seed in (SEED, bytes(32), b"\xff" * 32):
        for i in (0, 1, 255, 256, 2**32 - 1, 2**32, 2**32 + 1, 2**64 - 1):
            host.cb_coefficient(seed, U64(i), out)
            assert _words(out) == B.coefficient(seed, i), (seed.hex(), i)


def test_a_zero_coefficient_becomes_one(host):
    out = (U32 * 8)()
    host.cb_coefficient_from_digest(U32(0), U32(0), U32(0), U32(0), out)
    assert _words(out) == 1 == B.coefficient_from_digest(bytes(32))
    host.cb_coefficient_from_digest(U32(0), U32(0), U32(0), U32(2), out)
    assert _words(out) == 2
    host.cb_coefficient_from_digest(U32(0x80000000), U32(0), U32(0), U32(0), out)
    assert _words(out) == 2**127 == B.coefficient_from_digest(b"\x80" + bytes(31))


def _batch(host, scheme, msgs, sigs, pks, seed, c=5, slice_=300, off=None):
    n = len(sigs)
    buf = np.frombuffer(b"".join(msgs) + bytes(8), dtype=np.uint8).copy()   # (the hashes read whole aligned dwords)
    if off is None:
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in msgs], out=off[1:])
    sg = np.frombuffer(b"".join(sigs) + bytes(8), dtype=np.uint8).copy()
    pk = np.frombuffer(b"".join(pks) + bytes(8), dtype=np.uint8).copy()
    st, verdict = np.full(n + 1, 9, dtype=np.uint8), np.full(1, 9, dtype=np.uint8)
    vp = ctypes.c_void_p
    host.cb_batch(int(scheme == "ed25519"), c, SZ(slice_), SZ(n), buf.ctypes.data_as(vp), off.ctypes.data_as(vp), U64(len(buf) - 8),
                  sg.ctypes.data_as(vp), pk.ctypes.data_as(vp), seed, st.ctypes.data_as(vp), verdict.ctypes.data_as(vp))
    assert st[n] == 9
    status = [int(v) for v in st[:n]]
    return bool(verdict[0] == 1 and not any(status)), status, int(verdict[0])


@pytest.mark.parametrize("scheme", B.SCHEMES)
def test_the_valid_triples(host, scheme):
    msgs, sigs, pks = FX.tiled(scheme, 80)
    assert _batch(host, scheme, msgs, sigs, pks, SEED) == (True, [0] * 80, 1)
    assert _batch(host, scheme, msgs[:65], sigs[:65], pks[:65], SEED, c=2, slice_=33) == (True, [0] * 65, 1)   # two slices, the second short
    assert _batch(host, scheme, msgs[:9], sigs[:9], pks[:9], SEED, c=8, slice_=1) == (True, [0] * 9, 1)
    assert _batch(host, scheme, [], [], [], SEED) == (True, [], 1)
    assert _batch(host, scheme, msgs[:1], sigs[:1], pks[:1], SEED) == (True, [0], 1)


@pytest.mark.parametrize("scheme", B.SCHEMES)
def test_one_corruption_at_a_time(host, scheme):
    msgs, sigs, pks = FX.tiled(scheme, 17)
    for at in (0, 8, 16):
        for part in ("s", "r", "msg"):
            m, s = list(msgs), list(sigs)
            if part == "msg":
                m[at] = m[at] + b"?"
            else:
                k = 40 if part == "s" else 8
                s[at] = s[at][:k] + bytes([s[at][k] ^ 1]) + s[at][k + 1:]
            want = B.batch(scheme, m, s, pks, SEED)
            assert want[2] == 0 or any(want[1]), (at, part)     # (a flipped r may not decode: then the status names it)
            assert _batch(host, scheme, m, s, pks, SEED, slice_=7) == want, (at, part)


@pytest.mark.parametrize("scheme", B.SCHEMES)
def test_refused_elements(host, scheme):
    msgs, sigs, pks = FX.tiled(scheme, 4)
    for name, msg, sig, pk, status in FX.refused(scheme):
        got = _batch(host, scheme, msgs[:2] + [msg] + msgs[2:], sigs[:2] + [sig] + sigs[2:], pks[:2] + [pk] + pks[2:], SEED, slice_=2)
        assert got == (False, [0, 0, status, 0, 0], 1), name
    # every element refused: the sum is the generator times zero
    rows = FX.refused(scheme)
    got = _batch(host, scheme, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], SEED)
    assert got == (False, [r[4] for r in rows], 1)


@pytest.mark.parametrize("scheme", B.SCHEMES)
def test_a_bad_message_range_is_status_4(host, scheme):
    msgs, sigs, pks = FX.tiled(scheme, 3)
    off = np.zeros(4, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    total = int(off[3])
    bad = off.copy()
    bad[2] = total + 1          # elements 1 and 2 see an end / a start past the buffer
    assert _batch(host, scheme, msgs, sigs, pks, SEED, off=bad) == (False, [0, B.BAD_RANGE, B.BAD_RANGE], 1)


@pytest.mark.parametrize("scheme", B.SCHEMES)
def test_the_cancelling_pair(host, scheme):
    msgs, sigs, pks = FX.tiled(scheme, 5)
    sigs[1], sigs[3] = B.cancelling_pair(scheme, sigs[1], sigs[3], 0x1234567)
    for k in range(8):
        assert _batch(host, scheme, msgs, sigs, pks, B.fixed_seed(k), slice_=3) == (False, [0] * 5, 0), k


def test_torsion_defects_are_accepted(host):
    msgs, sigs, pks = FX.tiled("ed25519", 2)
    for name, msg, sig, pk in FX.torsion():
        seed = B.seed_with_odd(name, [1])
        got = _batch(host, "ed25519", [msgs[0], msg, msgs[1]], [sigs[0], sig, sigs[1]], [pks[0], pk, pks[1]], seed)
        assert got == (True, [0, 0, 0], 1), name
