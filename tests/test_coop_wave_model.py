"""The cooperative additions of the ordered folds (secp::, p256::, ed::padd_coop) on the host, as a wavefront of threads
(tests/cpp/coop_wave.cpp): the plain host build replaces them by padd(), so this program is the only CPU run of their slot
tables, level schedules and early-outs.  Eight threads are lanes 0..7; every case of tests/fold_cases.py, 10 000 random
operand pairs and random chains of 65 per curve; every lane's sum must be padd's bit for bit, and a case's last sum the
oracle's.  Built a second time with -fsanitize=thread: a reported race would be a level reading a slot that another lane
writes before the next sync().  A stand-alone host program: nothing here touches a GPU or runs inside this process."""
import os
import subprocess

import pytest

import fold_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "coop_wave.cpp")
CSRC = os.path.join(ROOT, "forge_ec_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("limbs.hpp", "point_io.hpp", "coop.hpp", "secp256k1.hpp", "p256.hpp", "ed25519.hpp")]
FLAGS = ["-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]


def _build(exe, extra):
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++"] + extra + FLAGS + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def case_file(oracle, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fold_cases") / "fold_cases.txt")
    FC.write_case_file(oracle, path)
    return path


def _check(out, oracle):
    for curve in (FC.SECP, FC.P256, FC.ED):
        assert "%s: %d cases, 10000 random pairs, 3 chains of 65 on 8 lanes" % (FC.NAMES[curve], len(FC.cases(oracle, curve))) in out, out
    assert "every lane's sum is padd's: 0 mismatches" in out, out


def test_the_wave_macro_is_the_programs_alone():
    """FEC_HOST_EMUL_WAVE is defined by coop_wave.cpp and nowhere else: without it the headers are what they were"""
    hits = []
    for top in ("forge_ec_amd", "tools", "tests", "include", "oracle"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".cpp", ".hip", ".hpp", ".h", ".c", ".inc")):
                    text = open(os.path.join(dirpath, f), errors="replace").read()
                    if "#define FEC_HOST_EMUL_WAVE" in text:
                        hits.append(f)
    assert hits == ["coop_wave.cpp"]
    for hdr in ("secp256k1.hpp", "p256.hpp", "ed25519.hpp"):
        text = open(os.path.join(CSRC, hdr)).read()
        assert text.count("#if defined(FEC_HOST_EMUL) && !defined(FEC_HOST_EMUL_WAVE)") == 1, hdr


def test_every_lane_of_the_host_wavefront_agrees_with_padd(oracle, case_file):
    exe = _build(os.path.join(ROOT, "tests", "cpp", "coop_wave"), ["-O2"])
    r = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    _check(r.stdout, oracle)


def test_host_wavefront_is_race_free_under_thread_sanitizer(oracle, case_file):
    exe = _build(os.path.join(ROOT, "tests", "cpp", "coop_wave_tsan"), ["-O1", "-g", "-fsanitize=thread"])
    r = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66"))
    assert "ThreadSanitizer" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-6000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    _check(r.stdout, oracle)
