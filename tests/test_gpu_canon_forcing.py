"""
GPU tests of canonical mode's rare legs: the operands and points of tests/golden/canon_forcing_vectors.json
(gen_canon_forcing.py; each confirmed by the host emulation's reach counters, tests/test_canon_rare_legs.py) through the
kernels, every output element compared with oracle/canon_model.py.

The legs are wave-uniform branches (`if (lanes_where(...) != 0)`): one lane that needs the leg takes its 63 neighbours
through it, and a lane that needs it may share a wavefront with lanes that need another one.  So every case runs in two
placements, those of test_gpu_canon_adversarial.py: 64 copies of the case filling a wavefront, and the case alone at lanes
0, 31, 32, 63 and at the last element of 64 * 3 + 5 ordinary elements, whose results must be right as well.  Field cases go
through fec_canon_field_op with all six opcodes (a sqr case takes its operand twice); points through fec_canon_mul,
fec_canon_double_mul, fec_canon_decompress (33 and 65 bytes, host and _dev form), fec_canon_ecdsa_verify,
fec_canon_bip340_verify and fec_canon_eddsa_verify, each kernel with its own inlined copy of on_curve, mul and sqr.
"""
import json
import os
import random

import numpy as np
import pytest

import canon_msg_ref as R
from oracle import canon_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "canon_forcing_vectors.json")))
WAVE, AMONG = 64, 64 * 3 + 5
LANES = (0, 31, 32, 63, AMONG - 1)
NAMES = ["secp256k1", "p256", "ed25519"]
MODEL = dict(zip(NAMES, [M.SECP256K1, M.P256, M.ED25519]))
OPS = ["add", "sub", "mul", "sqr", "neg", "inv"]
FINITE, INFINITE, BAD = 0, 1, 2


def _canon(gpu_ctx, curve):
    from forge_ec_amd.canon import CANON_CURVES
    return CANON_CURVES[curve](gpu_ctx)


def _op_codes():
    from forge_ec_amd import _lib as L
    return dict(zip(OPS, (L.F_ADD, L.F_SUB, L.F_MUL, L.F_SQR, L.F_NEG, L.F_INV)))


def _int(h):
    return int(h, 16)


def _pt(h):
    return M.INF if h is None else (_int(h[:64]), _int(h[64:]))


def _words(vals):
    return np.array([M.limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def _xy(pts):
    return np.array([M.xy_limbs(p) for p in pts], dtype=np.uint64).reshape(len(pts), 8)


def _placed(base, item):
    out = list(base)
    for i in LANES:
        out[i] = item
    return out


def _points(curve):
    return [c for c in FIX["points"] if NAMES[c["curve"]] == curve]


def _twin(curve, pt):
    """one bit of y (Ed25519: of x) flipped: in range and off the curve"""
    return (pt[0] ^ 1, pt[1]) if curve == "ed25519" else (pt[0], pt[1] ^ 1)


# ---- ordinary elements, computed once per curve by the model -----------------------------------------------------------
_ordinary = {}


def forge(C, Q, rng):
    """signatures that verify under the key Q, built from the model without Q's secret key: ECDSA (z, r, s), BIP-340
    (r, s, e) for an even-y key, EdDSA (R, S, h)"""
    n = C.N
    if C is M.ED25519:
        S, h = rng.randrange(n), rng.randrange(n)
        return dict(eddsa=(int.from_bytes(C.encode(C.add(C.mul(S, C.G), C.mul(h, C.neg(Q)))), "little"), S, h))
    u1, u2 = rng.randrange(1, n), rng.randrange(1, n)
    r = C.add(C.mul(u1, C.G), C.mul(u2, Q))[0] % n
    s = r * pow(u2, -1, n) % n
    out = dict(ecdsa=(u1 * s % n, r, s))
    if C is M.SECP256K1 and Q[1] % 2 == 0:
        while True:
            s, e = rng.randrange(n), rng.randrange(n)
            Rp = C.add(C.mul(s, C.G), C.mul((n - e) % n, Q))
            if Rp is not M.INF and Rp[1] % 2 == 0:
                out["bip340"] = (Rp[0], s, e)
                break
    return out


def ordinary(curve):
    """8 ordinary points of the curve (even y on secp256k1) with a scalar multiple, a double multiplication and valid
    signatures each, and AMONG random field operand pairs with the six results: what fills the lanes around a case"""
    if curve not in _ordinary:
        C = MODEL[curve]
        rng = random.Random(0x0D1 + NAMES.index(curve))
        pts = []
        for _ in range(8):
            Q = C.mul(rng.randrange(1, C.N), C.G)
            if curve == "secp256k1" and Q[1] % 2:
                Q = C.neg(Q)
            k, u1, u2 = rng.randrange(2**256), rng.randrange(1, C.N), rng.randrange(1, C.N)
            pts.append(dict(pt=Q, k=k, kp=C.mul(k if curve == "ed25519" else k % C.N, Q), u1=u1, u2=u2, dm=C.add(C.mul(u1, C.G), C.mul(u2, Q)), **forge(C, Q, rng)))
        a, b = [rng.randrange(C.P) for _ in range(AMONG)], [rng.randrange(C.P) for _ in range(AMONG)]
        _ordinary[curve] = dict(points=pts, a=a, b=b, results={op: [C.field_op(op, x, y) for x, y in zip(a, b)] for op in OPS})
    return _ordinary[curve]


def among(curve, key):
    """AMONG ordinary elements: key(point record) for the 8 points, cycled"""
    pts = ordinary(curve)["points"]
    return [key(pts[i % len(pts)]) for i in range(AMONG)]


# ---- the field layer ---------------------------------------------------------------------------------------------------
def _field_cases(curve):
    C = MODEL[curve]
    out = []
    for c in FIX["field"]:
        if NAMES[c["curve"]] == curve:
            a = _int(c["a"])
            b = a if c["b"] is None else _int(c["b"])
            assert C.field_op(c["op"], a, b) == _int(c["expect"])
            out.append((c["family"], a, b, {op: C.field_op(op, a, b) for op in OPS}))
    return out


def _field_op(dev, op, code, a, b):
    return [M.unlimbs(r) for r in dev.field_op(code, _words(a), _words(b) if op in ("add", "sub", "mul") else None)]


@pytest.mark.parametrize("curve", NAMES)
def test_field_a_wavefront_per_case(gpu_ctx, curve):
    """64 copies of each operand pair: every lane of the wavefront needs the leg"""
    dev, codes, cases = _canon(gpu_ctx, curve), _op_codes(), _field_cases(curve)
    assert len(cases) >= 40
    a = [c[1] for c in cases for _ in range(WAVE)]
    b = [c[2] for c in cases for _ in range(WAVE)]
    for op in OPS:
        got = _field_op(dev, op, codes[op], a, b)
        want = [c[3][op] for c in cases for _ in range(WAVE)]
        bad = sorted({cases[i // WAVE][0] for i in range(len(got)) if got[i] != want[i]})
        assert not bad, "%s: %s" % (op, bad)


@pytest.mark.parametrize("curve", NAMES)
def test_field_one_lane_among_ordinary_operands(gpu_ctx, curve):
    """the pair at lanes 0, 31, 32, 63 and at the last of 197 random pairs, which are dragged through the leg: the whole vector"""
    dev, codes, o = _canon(gpu_ctx, curve), _op_codes(), ordinary(curve)
    bad = []
    for family, x, y, res in _field_cases(curve):
        a, b = _placed(o["a"], x), _placed(o["b"], y)
        for op in OPS:
            got = _field_op(dev, op, codes[op], a, b)
            want = _placed(o["results"][op], res[op])
            if got != want:
                bad.append("%s %s at %s" % (family, op, [i for i in range(AMONG) if got[i] != want[i]]))
    assert not bad, "\n".join(bad)


# ---- points: k * P and u1 G + u2 P -------------------------------------------------------------------------------------
def _check_points(got, want, labels):
    """(xy, status) of a call against model points (None = infinity, "bad" = rejected): labels of the elements that differ"""
    xy, st = got
    want_xy = _xy([M.INF if w == "bad" else w for w in want])
    want_st = np.array([BAD if w == "bad" else INFINITE if w is M.INF else FINITE for w in want], dtype=np.uint8)
    return sorted({"%s at %d" % (labels[i], i) for i in np.nonzero((xy != want_xy).any(axis=1) | (st != want_st))[0]})


@pytest.mark.parametrize("curve", NAMES)
def test_mul(gpu_ctx, curve):
    """k * P for k in {1, 2, n - 1, a random 256-bit k}: k_canon_mul / k_ced_mul test the point with their own on_curve"""
    dev, C = _canon(gpu_ctx, curve), MODEL[curve]
    items = [(c["family"], _int(m["k"]), _pt(c["x"] + c["y"]), _pt(m["out"])) for c in _points(curve) for m in c["mul"]]
    assert {1, C.N - 1} <= {it[1] for it in items}
    items += [(f + " twin", k, _twin(curve, p), "bad") for f, k, p, _ in items if k == 1]
    wave = [it for it in items for _ in range(WAVE)]
    bad = _check_points(dev.mul(_words([it[1] for it in wave]), _xy([it[2] for it in wave])), [it[3] for it in wave], [it[0] for it in wave])
    assert not bad, "\n".join(bad)
    base = among(curve, lambda r: ("ordinary", r["k"], r["pt"], r["kp"]))
    for it in items:
        batch = _placed(base, it)
        bad = _check_points(dev.mul(_words([e[1] for e in batch]), _xy([e[2] for e in batch])), [e[3] for e in batch], [e[0] for e in batch])
        assert not bad, "%s, k = %#x:\n%s" % (it[0], it[1], "\n".join(bad))


@pytest.mark.parametrize("curve", NAMES)
def test_double_mul(gpu_ctx, curve):
    dev = _canon(gpu_ctx, curve)
    items = [(c["family"], _int(c["dm"]["u1"]), _int(c["dm"]["u2"]), _pt(c["x"] + c["y"]), _pt(c["dm"]["out"])) for c in _points(curve)]
    items += [(f + " twin", u1, u2, _twin(curve, p), "bad") for f, u1, u2, p, _ in items]

    def run(batch):
        got = dev.double_mul(_words([e[1] for e in batch]), _words([e[2] for e in batch]), _xy([e[3] for e in batch]))
        return _check_points(got, [e[4] for e in batch], [e[0] for e in batch])

    bad = run([it for it in items for _ in range(WAVE)])
    assert not bad, "\n".join(bad)
    base = among(curve, lambda r: ("ordinary", r["u1"], r["u2"], r["pt"], r["dm"]))
    for it in items:
        bad = run(_placed(base, it))
        assert not bad, "%s:\n%s" % (it[0], "\n".join(bad))


@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_edge_scalars(gpu_ctx, curve):
    """k * P and k * G with k in {0, 1, n - 1, n, ...}: the additions meet infinity and, for k = n, P + (-P)"""
    dev, C = _canon(gpu_ctx, curve), MODEL[curve]
    cases = [c for c in FIX["edge_scalars"] if NAMES[c["curve"]] == curve]
    mul = [("k = %s" % c["k"], _int(c["k"]), _pt(c["point"]), _pt(c["out"])) for c in cases if c["fn"] == "mul"]
    base = among(curve, lambda r: ("ordinary", r["k"], r["pt"], r["kp"]))
    for batch in [[it for it in mul for _ in range(WAVE)]] + [_placed(base, it) for it in mul]:
        bad = _check_points(dev.mul(_words([e[1] for e in batch]), _xy([e[2] for e in batch])), [e[3] for e in batch], [e[0] for e in batch])
        assert not bad, "\n".join(bad)
    fixed = [("k = %s" % c["k"], _int(c["k"]), _pt(c["out"])) for c in cases if c["fn"] == "mul_base"]
    fill = [("ordinary", r["k"], C.mul(r["k"] % C.N, C.G)) for r in ordinary(curve)["points"]]
    base = [fill[i % len(fill)] for i in range(AMONG)]
    for batch in [[it for it in fixed for _ in range(WAVE)]] + [_placed(base, it) for it in fixed]:
        bad = _check_points(dev.mul_base(_words([e[1] for e in batch])), [e[2] for e in batch], [e[0] for e in batch])
        assert not bad, "\n".join(bad)
    assert any(it[3] is M.INF for it in mul) and any(it[2] is M.INF for it in fixed)


# ---- SEC 1 decoding ----------------------------------------------------------------------------------------------------
def _decompress(gpu_ctx, dev, keys, pk_len, form):
    raw = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), pk_len).copy()
    if form == "host":
        return dev.decompress(raw, pk_len)
    import torch
    n = len(keys)
    d_in = torch.from_numpy(raw.reshape(-1)).cuda()
    xy = torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    dev.decompress_dev(d_in.data_ptr(), pk_len, xy.data_ptr(), st.data_ptr(), n)
    torch.cuda.synchronize()
    return xy.cpu().numpy().view(np.uint64), st.cpu().numpy()


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("pk_len", [33, 65])
@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_decompress(gpu_ctx, curve, pk_len, form):
    """33 bytes: sqr and mul of x, then the square root chain; 65 bytes: on_curve.  The other tag decodes to the negative,
    a 65-byte key with a bit of y flipped is rejected."""
    dev, C = _canon(gpu_ctx, curve), MODEL[curve]
    items = []
    for c in _points(curve):
        pt = _pt(c["x"] + c["y"])
        items.append((c["family"], bytes.fromhex(c["sec1_%d" % pk_len]), pt))
        assert R.sec1_decode(C, items[-1][1]) == pt
        if pk_len == 33:
            items.append((c["family"] + " other tag", R.sec1_encode(C.neg(pt)), C.neg(pt)))
        else:
            items.append((c["family"] + " twin", R.sec1_encode(_twin(curve, pt), compressed=False), "bad"))
    wave = [it for it in items for _ in range(WAVE)]
    bad = _check_points(_decompress(gpu_ctx, dev, [it[1] for it in wave], pk_len, form), [it[2] for it in wave], [it[0] for it in wave])
    assert not bad, "\n".join(bad)
    base = among(curve, lambda r: ("ordinary", R.sec1_encode(r["pt"], compressed=pk_len == 33), r["pt"]))
    for it in items:
        batch = _placed(base, it)
        bad = _check_points(_decompress(gpu_ctx, dev, [e[1] for e in batch], pk_len, form), [e[2] for e in batch], [e[0] for e in batch])
        assert not bad, "%s:\n%s" % (it[0], "\n".join(bad))


# ---- the verifiers, with the point as the public key -------------------------------------------------------------------
def _verdicts(call, items, base):
    """items of (label, four integers or point, verdict): both placements through call(four arrays); labels that differ"""
    def run(batch):
        cols = [_xy([e[1][k] for e in batch]) if isinstance(batch[0][1][k], tuple) else _words([e[1][k] for e in batch]) for k in range(4)]
        got = call(*cols)
        return sorted({"%s at %d" % (batch[i][0], i) for i in range(len(batch)) if got[i] != batch[i][2]})

    bad = run([it for it in items for _ in range(WAVE)])
    for it in items:
        bad += run(_placed(base, it))
    return bad


@pytest.mark.parametrize("curve", ["secp256k1", "p256"])
def test_ecdsa_verify(gpu_ctx, curve):
    """a signature that the model built to verify under the point: accepted; refused under the point with a bit of y flipped
    (the verifier's own on_curve), under the negated point, and for z + 1"""
    dev, C = _canon(gpu_ctx, curve), MODEL[curve]
    items = []
    for c in _points(curve):
        pt, (z, r, s) = _pt(c["x"] + c["y"]), (_int(c["ecdsa"][k]) for k in "zrs")
        items += [(c["family"], (z, r, s, pt), 1), (c["family"] + " twin", (z, r, s, _twin(curve, pt)), 0),
                  (c["family"] + " negated", (z, r, s, C.neg(pt)), 0), (c["family"] + " z + 1", ((z + 1) % 2**256, r, s, pt), 0)]
    base = among(curve, lambda r: ("ordinary", r["ecdsa"] + (r["pt"],), 1))
    bad = _verdicts(dev.ecdsa_verify, items, base)
    assert not bad, "\n".join(bad)


def test_bip340_verify(gpu_ctx):
    """the x-only keys: lift_x squares and cubes x in k_canon_bip340_prepare"""
    dev = _canon(gpu_ctx, "secp256k1")
    items = []
    for c in _points("secp256k1"):
        if "bip340" in c:
            x, (r, s, e) = _int(c["x_only"]), (_int(c["bip340"][k]) for k in "rse")
            items += [(c["family"], (x, r, s, e), 1), (c["family"] + " e + 1", (x, r, s, (e + 1) % 2**256), 0), (c["family"] + " r ^ 1", (x, r ^ 1, s, e), 0)]
    assert len(items) >= 12
    base = among("secp256k1", lambda r: ("ordinary", (r["pt"][0],) + r["bip340"], 1))
    bad = _verdicts(dev.bip340_verify, items, base)
    assert not bad, "\n".join(bad)


def test_eddsa_verify(gpu_ctx):
    """the encodings as A: ed_decode squares y in k_ced_eddsa_prepare; the other sign bit is -A, h + 1 another equation"""
    dev = _canon(gpu_ctx, "ed25519")
    items = []
    for c in _points("ed25519"):
        a, (r, s, h) = int.from_bytes(bytes.fromhex(c["ed"]), "little"), (_int(c["eddsa"][k]) for k in "rsh")
        items += [(c["family"], (a, r, s, h), 1), (c["family"] + " negated", (a ^ (1 << 255), r, s, h), 0), (c["family"] + " h + 1", (a, r, s, (h + 1) % M.ED25519.N), 0)]
    enc = lambda p: int.from_bytes(M.ED25519.encode(p), "little")   # noqa: E731
    base = among("ed25519", lambda r: ("ordinary", (enc(r["pt"]),) + r["eddsa"], 1))
    bad = _verdicts(dev.eddsa_verify, items, base)
    assert not bad, "\n".join(bad)
