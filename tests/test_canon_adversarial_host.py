"""
The adversarial fixture (tests/golden/canon_adversarial_vectors.json, built by tests/canon_adversarial.py) through the
device headers compiled for the host (tools/host_emul.cpp), composed the way the verification kernels compose them:
u1 G from the 8-bit comb, u2 Q from the GLV ladder (secp256k1) or the windowed ladders (P-256, Ed25519), the sum from
the general addition, then the scheme's final test.  No GPU needed; tests/test_gpu_canon_adversarial.py runs the same
cases through the kernels.
"""
import json
import os

import numpy as np

import canon_msg_ref as R
from oracle import canon_model as M
from test_canon_host_emulation import CURVE_IDS, _arr, _ext, _jac, _p, _pt_of, emu  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "canon_adversarial_vectors.json")))
E = M.ED25519
REFUSED = "refused before any point arithmetic"   # M.INF is None, so None cannot say this


# the double multiplication of a case from the message; the 65-byte twin of an ECDSA case shares its 33-byte case's
DM = {(c["scheme"], c["curve"], c["class"], c["name"]): c["dm"] for c in FIXTURE["msg"] if "dm" in c}


def _dm(c):
    return DM.get((c["scheme"], c["curve"], c["class"], c["name"]))


def _np(h):
    """the fixture's hex (one 256-bit integer, or a point's x then y) or a list of limbs -> uint64 limbs"""
    if isinstance(h, str):
        h = [l for i in range(0, len(h), 64) for l in M.limbs(int(h[i:i + 64], 16))]
    return np.array(h, dtype=np.uint64)


def _pt(h):
    return M.INF if h is None else (int(h[:64], 16), int(h[64:], 16))


def weierstrass_sum(emu, name, u1, u2, q):
    """u1 G + u2 q as k_canon_mul_base8 and k_canon_mul<W, ACCUM> compute it; limbs in, a model point out"""
    C, cid = M.CURVES[name], CURVE_IDS[name]
    a, b, out = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    sa = emu.he_canon_mul_base8(cid, _p(_np(u1)), _p(a))
    sb = emu.he_glv_mul(_p(_np(u2)), _p(_np(q)), _p(b)) if name == "secp256k1" else emu.he_canon_mul(cid, _p(_np(u2)), _p(_np(q)), _p(b))
    assert sa in (0, 1) and sb in (0, 1)
    inf = emu.he_canon_point_op(cid, 1, _p(_jac(C, _pt_of(a, sa == 1), 1)), _p(_jac(C, _pt_of(b, sb == 1), 1)), _p(out))
    return _pt_of(out, inf)


def edwards_sum(emu, u1, u2, q):
    a, b, out = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    assert emu.he_ced_mul_base8(_p(_np(u1)), _p(a)) == 0 and emu.he_ced_mul(_p(_np(u2)), _p(_np(q)), _p(b)) == 0
    assert emu.he_ced_point_op(1, _p(_ext(_pt_of(b, False), 1)), _p(_ext(_pt_of(a, False), 1)), _p(out)) == 0
    return _pt_of(out, False)


def ecdsa_verdict(emu, name, z, r, s, q, dm):
    """(verdict, point or REFUSED): the scalar half, the double multiplication, x(R) mod n == r"""
    cid = CURVE_IDS[name]
    u1, u2 = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    if not emu.he_canon_ecdsa_scalars(cid, _p(_np(z)), _p(_np(r)), _p(_np(s)), _p(u1), _p(u2)):
        return 0, REFUSED
    if dm is not None:
        assert M.unlimbs(u1) == int(dm["u1"], 16) and M.unlimbs(u2) == int(dm["u2"], 16)
    pt = weierstrass_sum(emu, name, list(u1), list(u2), q)
    if pt is M.INF:
        return 0, pt
    return emu.he_canon_ecdsa_x_matches(cid, _p(_arr(pt[0])), _p(_np(r))), pt


def msg_verdict(emu, c):
    msg, sig, pk = bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"])
    if c["scheme"] == "ecdsa":
        Q = R.sec1_decode(R.WEIERSTRASS[c["curve"]], pk)
        assert Q is not None
        return ecdsa_verdict(emu, c["curve"], M.limbs(R.ecdsa_z(msg)), M.limbs(int.from_bytes(sig[:32], "big")),
                             M.limbs(int.from_bytes(sig[32:], "big")), M.xy_limbs(Q), _dm(c))
    if c["scheme"] == "bip340":
        pxy, u2 = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        e = int.from_bytes(R.tagged("BIP0340/challenge", sig[:32] + pk + msg), "big")
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        if not emu.he_bip340_prepare(_p(_arr(int.from_bytes(pk, "big"))), _p(_arr(r)), _p(_arr(s)), _p(_arr(e)), _p(pxy), _p(u2)):
            return 0, REFUSED
        pt = weierstrass_sum(emu, "secp256k1", M.limbs(s), list(u2), list(pxy))
        return (1 if pt is not M.INF and pt[0] == r and pt[1] % 2 == 0 else 0), pt
    axy, rxy, u2 = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    little = lambda b: _arr(int.from_bytes(b, "little"))   # noqa: E731
    h = R.ed25519_challenge(sig[:32], pk, msg)
    if not emu.he_eddsa_prepare(_p(little(pk)), _p(little(sig[:32])), _p(little(sig[32:])), _p(_arr(h)), _p(axy), _p(rxy), _p(u2)):
        return 0, REFUSED
    pt = edwards_sum(emu, M.limbs(int.from_bytes(sig[32:], "little")), list(u2), list(axy))
    return (1 if pt == _pt_of(rxy, False) else 0), pt


def test_every_case_from_the_message(emu):
    """the verdict of every case and the point of its double multiplication; an Ed25519 key with a torsion component
    shows whether -h A is computed as h (-A)"""
    bad = []
    for c in FIXTURE["msg"]:
        got, pt = msg_verdict(emu, c)
        dm = _dm(c)
        if got != c["want"] or (dm is not None and pt != _pt(dm["point"])):
            bad.append("%s %s: %s / %s" % (c["scheme"], c["curve"], c["class"], c["name"]))
        assert (dm is not None) == (pt is not REFUSED), c["name"]
    assert not bad, "\n".join(bad)
    assert {c["want"] for c in FIXTURE["msg"]} == {0, 1}


def test_every_case_after_the_hash(emu):
    for c in FIXTURE["hash"]:
        got, pt = ecdsa_verdict(emu, c["curve"], c["z"], c["r"], c["s"], c["q"], None)
        assert got == c["want"] and pt == _pt(c["point"]), (c["curve"], c["class"], c["name"])


def test_double_multiplications(emu):
    """prescribed (u2, Q) pairs through the GLV ladder and the windowed ladder, sums that are a doubling or infinity"""
    seen = set()
    for c in FIXTURE["double_mul"] + FIXTURE["hash"]:
        want = _pt(c["point"])
        if "u1" in c:
            u1, u2 = c["u1"], c["u2"]
        else:   # after the hash: u1 = z / s, u2 = r / s
            n = M.CURVES[c["curve"]].N
            w = pow(int(c["s"], 16), -1, n)
            u1, u2 = M.limbs(int(c["z"], 16) * w % n), M.limbs(int(c["r"], 16) * w % n)
        assert weierstrass_sum(emu, c["curve"], u1, u2, c["q"]) == want, (c["curve"], c["class"], c["name"])
        seen.add(want is M.INF)
    assert seen == {True, False}
