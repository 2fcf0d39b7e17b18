"""
CPU checks of the parity-mode Ed25519 EdDSA verifiers from the message (fec_ed25519_verify,
fec_eddsa_verify_ed25519_msg): the test-side restatement (tests/eddsa_verify_ref.py) over the C oracle agrees with the
fixture that the same restatement over oracle/py_model.py produced, and with the Python backend on random inputs; the
fixture is its generator's output and covers what it must; the header declares the four entry points and the built
library exports them.
"""
import json
import os
import random
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import eddsa_verify_ref as R  # noqa: E402
import gen_eddsa_verify as G  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "eddsa_verify_vectors.json")
NEW = ["fec_ed25519_verify", "fec_ed25519_verify_dev", "fec_eddsa_verify_ed25519_msg", "fec_eddsa_verify_ed25519_msg_dev"]


@pytest.fixture(scope="module")
def fx():
    return json.load(open(FIXTURE))


def _byte_inputs(fx):
    c = fx["bytes"]
    return [bytes.fromhex(x["pk"]) for x in c], [bytes.fromhex(x["msg"]) for x in c], [bytes.fromhex(x["sig"]) for x in c]


def _generic_inputs(fx):
    c = fx["generic"]
    h = lambda l: [int(v, 16) for v in l]
    return ([h(x["pk"]) for x in c], [x["pk_inf"] for x in c], [bytes.fromhex(x["msg"]) for x in c], [h(x["r"]) for x in c],
            [x["r_inf"] for x in c], [h(x["s"]) for x in c])


def test_fixture_inputs_are_the_generator_output(fx):
    pk, msg, sig = _byte_inputs(fx)
    want = G.byte_cases()
    assert [(p, m, s) for p, m, s, _ in want] == list(zip(pk, msg, sig))[:len(want)]
    assert len(pk) - len(want) == (1 if "found after" in fx["provenance"] else 0)


def test_c_backend_equals_fixture(fx):
    be = R.CBackend()
    assert R.verify_batch(*_byte_inputs(fx), be) == [c["status"] for c in fx["bytes"]]
    assert R.eddsa_verify_batch(*_generic_inputs(fx), be) == [c["status"] for c in fx["generic"]]


def test_fixture_coverage(fx):
    b = {c["note"]: c for c in fx["bytes"]}
    msgs = {bytes.fromhex(c["msg"]): c["status"] for c in fx["bytes"]}
    assert msgs[b"test message"] == 1 and msgs[b""] == 1 and msgs[b"different message"] == 0
    assert b"test messagf" in msgs and b"different messagE" in msgs and any(len(m) == 1 for m in msgs)
    for note in ("R None, A Some", "R Some, A None", "both Some", "R limb 0 above p's", "A limb 0 above p's", "s all 0xff"):
        assert note in b, note
    assert b["s all 0xff"]["sig"][64:] == "ff" * 32
    assert "found after" in fx["provenance"] or "none among" in fx["provenance"]
    g = fx["generic"]
    assert any(c["r_inf"] and bytes.fromhex(c["msg"]) not in (b"", b"test message") and c["status"] == 0 for c in g)
    ok = [c for c in g if c["note"].startswith("verifies")]
    assert {len(c["msg"]) // 2 for c in ok} >= {45, 46, 173, 174} and all(c["status"] == 1 and c["pk_inf"] for c in ok)
    assert {c["status"] for c in g} == {0, 1, 2}


def test_python_and_c_backends_agree_on_random_inputs():
    rnd = random.Random(7)
    n = 500
    rb = lambda k: bytes(rnd.getrandbits(8) for _ in range(k))
    msgs = [rb(rnd.randrange(0, 200)) for _ in range(n)]
    msgs[3], msgs[4], msgs[5] = b"test message", b"different message", b""
    # byte form: a random x does not decode under the reference's sqrt, so half of the keys and signatures carry x = 0
    pk = [bytes(32) if rnd.getrandbits(1) else rb(32) for _ in range(n)]
    sig = [(bytes(32) if rnd.getrandbits(1) else rb(32)) + (bytes(32) if rnd.getrandbits(2) == 0 else rb(32)) for _ in range(n)]
    got_c = R.verify_batch(pk, msgs, sig, R.CBackend())
    assert got_c == R.verify_batch(pk, msgs, sig, R.PyBackend())
    assert {0, 1} <= set(got_c[6:])
    # generic form: random coordinates, some identity flags, some verifying constructions (pk at infinity)
    from oracle import py_model as M
    m = 500
    rxy = lambda: G.limbs(rnd.randrange(G.P)) + G.limbs(rnd.randrange(G.P))
    pkx, pinf, rx, rinf, s = [], [], [], [], []
    for i in range(m):
        sc = G.limbs(rnd.randrange(1, G.ORDER))
        if i % 3 == 0:
            x, y, _ = M.Ed.to_affine(M.Ed.multiply(M.Ed.generator(), sc))
            rx.append(list(x) + list(y))
            pinf.append(1)
        else:
            rx.append(rxy())
            pinf.append(0)
        pkx.append(rxy())
        rinf.append(1 if i % 7 == 6 else 0)
        s.append(sc)
    gm = [rb(rnd.randrange(1, 200)) for _ in range(m)]
    got_c = R.eddsa_verify_batch(pkx, pinf, gm, rx, rinf, s, R.CBackend())
    assert got_c == R.eddsa_verify_batch(pkx, pinf, gm, rx, rinf, s, R.PyBackend())
    assert {0, 1} <= set(got_c)


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "fecgpu.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    from forge_ec_amd import build
    so = build.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, exported), name
