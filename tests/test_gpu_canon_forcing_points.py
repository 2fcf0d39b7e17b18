"""
GPU tests of canonical mode's rare field legs in the kernels that came after tests/test_gpu_canon_forcing.py: the points of
tests/golden/canon_forcing_vectors.json (whose x^2 -- y^2 on Ed25519 -- fires a leg inside on_curve / decompression; each
decoding function confirmed by the host emulation's reach counters, tests/test_canon_rare_legs.py) through
fec_canon_msm, fec_canon_ecdsa_recover, fec_canon_pubkey_tweak_add, BIP-32 derive_pub / derive_pub_path,
fec_canon_taproot_output_key, the two batch verifiers and the from-the-message verifiers, host form and *_dev form.  Every
kernel carries its own inlined copy of on_curve, mul and sqr, so no kernel stands for another: DRIVES names, per kernel of
the census (tests/rare_legs.json), the tests here that reach it.

The legs are wave-uniform, so every case runs in the two placements of test_gpu_canon_forcing.py: 64 copies filling a
wavefront, and the case alone at lanes 0, 31, 32, 63 and at the last of 64 * 3 + 5 ordinary elements, whose outputs are
checked as well.  Every expected value is the model's: oracle/canon_model.py and the canon_*_ref.py models of tests/.

tests/golden/canon_forcing_keyed_vectors.json (gen_canon_forcing_keyed.py) holds multiples of secp256k1's generator WITH their
logarithms that fire CSECP_GENERAL: only with those can a valid signature have a forcing point as its key and another as its
nonce (test_keyed_*).  P-256 and Ed25519 have no keyed points.
"""
import functools
import hashlib
import json
import os
import random

import numpy as np
import pytest

import canon_batch_ref as BR
import canon_bip32_ref as B32
import canon_msg_ref as R
import canon_msm_ref as MS
import canon_recover_ref as K
import canon_wallet_ref as W
from oracle import canon_model as M
from test_gpu_canon_forcing import AMONG, LANES, MODEL, NAMES, WAVE, _canon, _int, _placed, _points, _pt, _twin, ordinary

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYED = json.load(open(os.path.join(HERE, "golden", "canon_forcing_keyed_vectors.json")))
SECP = M.SECP256K1
WEIERSTRASS = ["secp256k1", "p256"]
BAD_POINT, BAD_SCALAR = 2, 3
SEED = hashlib.sha256(b"canon-forcing-points/batch-seed").digest()
MSG_LENGTHS = (0, 55, 56, 119)
MSM_FX = MS.load_fixture()
BATCH_FX = BR.load_fixture()

# kernel of the census -> the tests of this file that reach it with a forcing point (tests/test_canon_rare_legs.py holds the
# census against this map)
DRIVES = {
    "k_canon_msm_recode": ["test_msm", "test_msm_dev_over_two_slices", "test_batch_verifiers_on_the_unkeyed_points", "test_keyed_bip340"],
    "k_canon_batch_prepare": ["test_batch_verifiers_on_the_unkeyed_points", "test_keyed_bip340"],
    "k_canon_recover_prepare": ["test_ecdsa_recover", "test_keyed_ecdsa"],
    "k_canon_tweak_prepare": ["test_pubkey_tweak_add"],
    "k_canon_bip32_parent": ["test_derive_pub", "test_derive_pub_path"],
    "k_canon_bip32_pub_prepare": ["test_derive_pub", "test_derive_pub_path"],
    "k_canon_taproot_prepare": ["test_taproot_output_key"],
    "k_canon_bip340_prepare_msg": ["test_batch_verifiers_on_the_unkeyed_points", "test_keyed_bip340"],
    "k_ced_eddsa_prepare_msg": ["test_batch_verifiers_on_the_unkeyed_points"],
    "k_canon_ecdsa_prepare_msg": ["test_keyed_ecdsa"],
}

# (fixture, function) pairings in which a point does NOT light its leg, by the reach counters: test_canon_rare_legs.py
# test_every_decoding_function_lights_the_points_legs finds none among canon_forcing_vectors.json's points (each fires its
# leg through x^2, Ed25519 through y^2, which every decoding function forms); the keyed fixture records its own per point
# ("lit"), and the x-only roles below take only the points it marks through_x.
NOT_LIT = {}


def _b32(v):
    return v.to_bytes(32, "big")


def _rows(items, width):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), width).copy()


def _placements(items, base):
    """the batches of both placements: 64 copies of every item in one batch, then every item at LANES among `base`"""
    yield [it for it in items for _ in range(WAVE)]
    for it in items:
        yield _placed(base, it)


def _cycle(records):
    return [records[i % len(records)] for i in range(AMONG)]


def _differing(batch, got, want):
    """labels (item[0]) of the elements whose got and want rows differ; rows are tuples of comparable values"""
    return sorted({"%s at %d" % (batch[i][0], i) for i in range(len(batch)) if got[i] != want[i]})


def _forcing(curve):
    """(label, point) of the fixture's points on `curve`"""
    return [("%s #%d" % (c["family"], i), _pt(c["x"] + c["y"]), c) for i, c in enumerate(_points(curve))]


def _keyed(through_x=True):
    """(k, point, record) of the keyed fixture, by default those whose leg fires through x"""
    return [(_int(p["k"]), (_int(p["x"]), _int(p["y"])), p) for p in KEYED["points"] if p["through_x"] or not through_x]


def _keyed_pairs():
    """(key record, nonce record, message) of consecutive through-x points: both the public key and R are forcing points"""
    pts = _keyed()
    rng = random.Random(0x4B31)
    return [(pts[2 * j], pts[2 * j + 1], bytes(rng.randrange(256) for _ in range(MSG_LENGTHS[j % 4]))) for j in range(len(pts) // 2)]


# ---- 4a. fec_canon_msm --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _msm_pool(curve):
    """AMONG pool elements (scalars, points) and the sum of those outside LANES, by the logarithms"""
    ks, refs = MS.draw(curve, AMONG, 21)
    pool = MSM_FX.pool(curve)
    rest = [0 if i in LANES else k for i, k in enumerate(ks)]
    part = MS.msm_by_logs(curve, rest, [pool[r][0] for r in refs], [pool[r][1] for r in refs], MSM_FX.T(curve))
    return ks, MSM_FX.points(curve, refs), part


@functools.lru_cache(maxsize=None)
def _msm_cases(curve):
    """(label, k, point, 64 k P, pool part + 5 k P): the model's arithmetic on the integer 64 k -- Ed25519 scalars are not
    reduced modulo l, the points may carry torsion -- and the fixture's `out` five times on top of the pool's sum"""
    C, part = MODEL[curve], _msm_pool(curve)[2]
    out = []
    for label, pt, c in _forcing(curve):
        for m in c["mul"]:
            k, kp = _int(m["k"]), _pt(m["out"])
            wave = C.mul(64 * k if curve == "ed25519" else 64 * k % C.N, pt)
            out.append(("%s k = %#x" % (label, k), k, pt, tuple(MS.result(curve, wave)), tuple(MS.result(curve, C.add(part, C.mul(5, kp))))))
    return out


@pytest.mark.parametrize("window", [4, 13])
@pytest.mark.parametrize("curve", NAMES)
def test_msm(gpu_ctx, curve, window):
    """every forcing point with each of its fixture scalars: k_canon_msm_recode runs on_curve on all three curves.  The twin
    (one bit flipped: in range, off the curve) in the same placements is BAD_POINT and 64 zero bytes, and the same call on
    the untouched batch afterwards is right."""
    from test_gpu_canon_msm import _both
    dev = _canon(gpu_ctx, curve)
    ks, pts, _ = _msm_pool(curve)
    bad = ([0] * 8, MS.BAD_POINT)
    gpu_ctx.set_canon_msm_window(window)
    try:
        for label, k, pt, want_wave, want_among in _msm_cases(curve):
            runs = [([k] * WAVE, [pt] * WAVE, want_wave), (_placed(ks, k), _placed(pts, pt), want_among)]
            for kk, pp, want in runs:
                assert tuple(_both(dev, *MS.pack(kk, pp))) == want, (label, len(kk))
            if k == 1:
                twin = _twin(curve, pt)
                for kk, pp, want in runs:
                    spoilt = [twin if q == pt else q for q in pp]
                    assert _both(dev, *MS.pack(kk, spoilt)) == bad, (label, "twin", len(kk))
                    assert tuple(_both(dev, *MS.pack(kk, pp))) == want, (label, "after the twin", len(kk))
    finally:
        gpu_ctx.set_canon_msm_window(0)
    gpu_ctx.check()


# ---- 4h. fec_canon_msm_dev over two slices --------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["secp256k1", "ed25519"])
def test_msm_dev_over_two_slices(gpu_ctx, curve):
    """n = 2^18 + 65, kMsmSlice elements and a second slice: ds + lo * 4, dp + lo * 8 and buckets that persist.  A forcing
    point is element 2^18 -- the first of slice two -- and the last element; the automatic window, one call."""
    from test_gpu_canon_msm import _dev
    C, n, first = MODEL[curve], (1 << 18) + 65, 1 << 18
    ks, refs = MS.draw(curve, n, 31)
    pool = MSM_FX.pool(curve)
    cases = _forcing(curve)
    placed = {first: cases[len(cases) // 2], n - 1: cases[-1]}
    want = MS.msm_by_logs(curve, [0 if i in placed else k for i, k in enumerate(ks)], [pool[r][0] for r in refs], [pool[r][1] for r in refs],
                          MSM_FX.T(curve))
    k = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ks), dtype="<u8").reshape(n, 4).copy()
    p = np.array([M.xy_limbs(pt) for _, _, pt in pool], dtype=np.uint64)[np.array(refs, dtype=np.int64)].reshape(n, 8)
    for at, (_, pt, c) in placed.items():
        m = c["mul"][3]
        k[at], p[at] = np.array(M.limbs(_int(m["k"])), dtype=np.uint64), np.array(M.xy_limbs(pt), dtype=np.uint64)
        want = C.add(want, _pt(m["out"]))
    gpu_ctx.set_canon_msm_window(0)
    assert tuple(_dev(_canon(gpu_ctx, curve), k, p)) == tuple(MS.result(curve, want))
    gpu_ctx.check()


# ---- 4b. fec_canon_ecdsa_recover --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _recover_want(curve, digest, sig, recid, out_len):
    out, st = K.recover(MODEL[curve], digest, sig, recid, out_len)
    return out, st


def _recover_item(curve, label, pt, parity, rng):
    """R = pt lifted from r = x mod n (the id's high bit where x >= n) with the id's low bit = parity: (label, digest, sig, recid)"""
    C = MODEL[curve]
    digest, s = bytes(rng.randrange(256) for _ in range(32)), rng.randrange(1, C.N)
    return (label, digest, _b32(pt[0] % C.N) + _b32(s), (2 if pt[0] >= C.N else 0) | parity)


@pytest.mark.parametrize("out_len", [33, 65])
@pytest.mark.parametrize("curve", WEIERSTRASS)
def test_ecdsa_recover(gpu_ctx, curve, out_len):
    """R is the forcing point (k_canon_recover_prepare lifts it from r, then k_canon_mul tests it); the other parity of the id
    lifts -R and gives the model's other key.  secp256k1's point with x above n takes the r + n branch and the general-wrap
    leg in one element."""
    from test_gpu_canon_recover import _both
    rng = random.Random(0x4B32 + NAMES.index(curve))
    items = []
    for label, pt, _ in _forcing(curve):
        items += [_recover_item(curve, label, pt, pt[1] & 1, rng), _recover_item(curve, label + " other parity", pt, (pt[1] & 1) ^ 1, rng)]
    if curve == "secp256k1":
        above = [it for it in items if it[3] & 2]
        assert above and all(_recover_want(curve, it[1], it[2], it[3], out_len)[1] == K.OK for it in above)
    base = _cycle([_recover_item(curve, "ordinary", r["pt"], r["pt"][1] & 1, rng) for r in ordinary(curve)["points"]])
    for batch in _placements(items, base):
        want = [_recover_want(curve, e[1], e[2], e[3], out_len) for e in batch]
        assert all(st == K.OK for _, st in want)
        dg, sg, rc = _rows([e[1] for e in batch], 32), _rows([e[2] for e in batch], 64), np.array([e[3] for e in batch], dtype=np.uint8)
        for out, st in _both(gpu_ctx, curve, dg, sg, rc, out_len):
            bad = _differing(batch, [(bytes(o), int(s)) for o, s in zip(out, st)], want)
            assert not bad, "\n".join(bad)
    keys = {it[0]: _recover_want(curve, it[1], it[2], it[3], out_len)[0] for it in items}
    assert all(keys[l] != keys[l + " other parity"] for l in keys if not l.endswith("parity"))
    gpu_ctx.check()


# ---- 4c. fec_canon_pubkey_tweak_add --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tweak_want(curve, pk, tweak, out_len):
    return B32.pubkey_tweak_add(MODEL[curve], pk, tweak, out_len)


@pytest.mark.parametrize("pk_len", [33, 65])
@pytest.mark.parametrize("curve", WEIERSTRASS)
def test_pubkey_tweak_add(gpu_ctx, curve, pk_len):
    """the forcing point as the key, tweaks 1 and random: k_canon_tweak_prepare decodes it (33 bytes: the root of x; 65: on_curve,
    which refuses the twin)"""
    from test_gpu_canon_bip32 import tweak
    C = MODEL[curve]
    rng = random.Random(0x4B33 + NAMES.index(curve))
    items = []
    for label, pt, _ in _forcing(curve):
        items += [("%s tweak %s" % (label, w), B32.encode(pt, pk_len), _b32(t)) for w, t in (("1", 1), ("random", rng.randrange(C.N)))]
        if pk_len == 65:
            items.append((label + " twin", B32.encode(_twin(curve, pt), 65), _b32(1)))
    base = _cycle([("ordinary", B32.encode(r["pt"], pk_len), _b32(rng.randrange(C.N))) for r in ordinary(curve)["points"]])
    for batch in _placements(items, base):
        pks, tw = _rows([e[1] for e in batch], pk_len), _rows([e[2] for e in batch], 32)
        for out_len in (33, 65):
            want = [_tweak_want(curve, e[1], e[2], out_len) for e in batch]
            assert all(st == (BAD_POINT if e[0].endswith("twin") else 0) for e, (_, st) in zip(batch, want))
            for dev in (False, True):
                out, st = tweak(gpu_ctx, curve, pks, tw, pk_len, out_len, dev)
                bad = _differing(batch, [(bytes(o), int(s)) for o, s in zip(out, st)], want)
                assert not bad, "out_len %d dev %s:\n%s" % (out_len, dev, "\n".join(bad))
    gpu_ctx.check()


# ---- 4d. BIP-32 derive_pub and derive_pub_path --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ckd_want(pk33, cc, index):
    return B32.ckd_pub(pk33, cc, index)


@functools.lru_cache(maxsize=None)
def _path_want(pk33, cc, path):
    return W.derive_pub_path(pk33, cc, list(path))


def _parents(rng, depth):
    """(label, parent key 33 bytes, chain code, non-hardened indices) with the forcing points as parents, and the ordinary base"""
    draw = lambda: (bytes(rng.randrange(256) for _ in range(32)), tuple(rng.randrange(B32.HARDENED) for _ in range(depth)))   # noqa: E731
    items = [(label, R.sec1_encode(pt)) + draw() for label, pt, _ in _forcing("secp256k1")]
    base = _cycle([("ordinary", R.sec1_encode(r["pt"])) + draw() for r in ordinary("secp256k1")["points"]])
    return items, base


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_derive_pub(gpu_ctx, dev):
    """the forcing point as the 33-byte parent key: parent i per element (k_canon_bip32_pub_prepare decodes it), and one
    shared parent for eight indices (k_canon_bip32_parent decodes it once, in one lane)"""
    from test_gpu_canon_bip32 import derive_pub
    rng = random.Random(0x4B34)
    items, base = _parents(rng, 1)
    for batch in _placements(items, base):
        want = [_ckd_want(e[1], e[2], e[3][0]) for e in batch]
        assert all(st == 0 for _, _, st in want)
        out, occ, st = derive_pub(gpu_ctx, _rows([e[1] for e in batch], 33), _rows([e[2] for e in batch], 32), [e[3][0] for e in batch], dev)
        bad = _differing(batch, [(bytes(o), bytes(c), int(s)) for o, c, s in zip(out, occ, st)], want)
        assert not bad, "\n".join(bad)
    for label, pk, cc, _ in items:
        idx = [rng.randrange(B32.HARDENED) for _ in range(8)]
        out, occ, st = derive_pub(gpu_ctx, _rows([pk], 33), _rows([cc], 32), idx, dev)
        assert [(bytes(o), bytes(c), int(s)) for o, c, s in zip(out, occ, st)] == [_ckd_want(pk, cc, i) for i in idx], label
    gpu_ctx.check()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_derive_pub_path(gpu_ctx, dev):
    """depth 2 with fingerprints and HASH160: the forcing point is the first level's parent, per element and shared"""
    from test_gpu_canon_wallet import path
    rng = random.Random(0x4B35)
    items, base = _parents(rng, 2)
    rows = lambda got: [(bytes(o), bytes(c), bytes(f), bytes(h), int(s)) for o, c, f, h, s in zip(*got)]   # noqa: E731
    for batch in _placements(items, base):
        want = [_path_want(e[1], e[2], e[3]) for e in batch]
        assert all(w[4] == 0 for w in want)
        got = path(gpu_ctx, _rows([e[1] for e in batch], 33), _rows([e[2] for e in batch], 32), [list(e[3]) for e in batch], dev)
        bad = _differing(batch, rows(got), want)
        assert not bad, "\n".join(bad)
    for label, pk, cc, _ in items:
        paths = [tuple(rng.randrange(B32.HARDENED) for _ in range(2)) for _ in range(4)]
        got = path(gpu_ctx, _rows([pk], 33), _rows([cc], 32), [list(q) for q in paths], dev)
        assert rows(got) == [_path_want(pk, cc, q) for q in paths], label
    gpu_ctx.check()


# ---- 4e. fec_canon_taproot_output_key ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _taproot_want(pk, root):
    return W.taproot_output_key(pk, root)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("with_root", [False, True], ids=["no-root", "root"])
@pytest.mark.parametrize("form", [32, 33])
def test_taproot_output_key(gpu_ctx, form, with_root, dev):
    """the points that carry x_only as the internal key: k_canon_taproot_prepare lifts x (form 33: either tag, ignored)"""
    from test_gpu_canon_wallet import taproot
    rng = random.Random(0x4B36)
    root = lambda: bytes(rng.randrange(256) for _ in range(32)) if with_root else None   # noqa: E731
    keys = lambda x: [_b32(x)] if form == 32 else [b"\x02" + _b32(x), b"\x03" + _b32(x)]   # noqa: E731
    items = [(label, pk, root()) for label, _, c in _forcing("secp256k1") if "x_only" in c for pk in keys(_int(c["x_only"]))]
    assert len(items) >= 6
    base = _cycle([("ordinary", keys(r["pt"][0])[0], root()) for r in ordinary("secp256k1")["points"]])
    for batch in _placements(items, base):
        want = [_taproot_want(e[1], e[2]) for e in batch]
        assert all(st == 0 for _, _, st in want)
        out, par, st = taproot(gpu_ctx, _rows([e[1] for e in batch], form), _rows([e[2] for e in batch], 32) if with_root else None, form, dev)
        bad = _differing(batch, [(bytes(o), int(q), int(s)) for o, q, s in zip(out, par, st)], want)
        assert not bad, "\n".join(bad)
    gpu_ctx.check()


# ---- 4f. the batch and from-the-message verifiers on the unkeyed points ---------------------------------------------------------------
def _batch_model(scheme, msgs, sigs, pks, seed):
    """tests/canon_batch_ref.py's verdict on a batch with many equal elements, at the cost of its distinct ones: equal
    (message, signature, key) triples share one term T of the sum, and sum a_i T = (sum a_i) T, so the model is given each
    distinct triple once with the sum of its coefficients (its own `coeff` argument).  On Ed25519 the reduction of a h modulo l
    differs from the sum of the reduced products by a multiple of l, which the model's cofactor 8 removes as it does in the call."""
    first, total, order = {}, [], []
    for i, t in enumerate(zip(msgs, sigs, pks)):
        if t not in first:
            first[t] = len(order)
            order.append(t)
            total.append(0)
        total[first[t]] += BR.coefficient(seed, i)
    ok, st, verdict = BR.batch(scheme, [t[0] for t in order], [t[1] for t in order], [t[2] for t in order], seed, coeff=lambda _, j: total[j])
    status = [st[first[t]] for t in zip(msgs, sigs, pks)]
    return bool(verdict and not any(status)), status, verdict


@functools.lru_cache(maxsize=None)
def _single(scheme, msg, sig, pk):
    return BR.single(scheme, msg, sig, pk)


def _valid(scheme, lengths=MSG_LENGTHS):
    """some of the batch fixture's valid triples, with messages of the given lengths"""
    t = BATCH_FX.triples(scheme)
    pick = [next(q for q in t if len(q[0]) == n) for n in lengths]
    assert all(_single(scheme, *q) == 1 for q in pick)
    return pick


def _out_of_range(scheme, sig):
    return BR.with_s(scheme, sig, BR.order(scheme))


@pytest.mark.parametrize("scheme", BR.SCHEMES)
def test_batch_verifiers_on_the_unkeyed_points(gpu_ctx, scheme):
    """Each forcing point once as the key and once as R of an element that cannot verify (nobody knows the point's logarithm):
    k_canon_batch_prepare decodes it -- bip340_lift_x(r) and both Ed25519 decodings are the batch's own -- and
    k_canon_msm_recode tests it again.  The element is admitted (status 0: it decoded) and the model's verdict is 0; with its s
    pushed out of range its status is 3 and the verdict is 1 over the valid rest.  The per-signature from-the-message
    verifiers (k_canon_bip340_prepare_msg, k_ced_eddsa_prepare_msg) answer 0 for the same elements.

    VERDICT 0 CANNOT TELL A WRONGLY DECODED y FROM A RIGHT ONE: an element that cannot verify fails whatever point the kernel
    decoded, so this test shows only that the leg's lanes run, admit the element and leave their neighbours right.  The
    check that can tell is test_keyed_bip340, on valid signatures whose key and R are forcing points with known logarithms
    (secp256k1 only: Ed25519 has no keyed points)."""
    import test_gpu_canon_batch as TB
    import test_gpu_canon_msg as TM
    from forge_ec_amd.canon import CanonEd25519, CanonSecp256k1
    ed = scheme == "ed25519"
    dev = (CanonEd25519 if ed else CanonSecp256k1)(gpu_ctx)
    valid = _valid(scheme, (55, 119))   # two ordinary triples: the model's cost goes by the distinct elements of a batch
    msg, sig, pk = valid[0]
    items = []
    for label, pt, c in _forcing("ed25519" if ed else "secp256k1"):
        enc = bytes.fromhex(c["ed"]) if ed else _b32(pt[0])
        items += [(label + " as the key", b"forcing", sig, enc), (label + " as R", b"forcing", enc + sig[32:], pk)]
    base = _cycle([("ordinary",) + q for q in valid])
    b = dict(curve="ed25519" if ed else "secp256k1", scheme=scheme, pk_len=32)
    for batch in _placements(items, base):
        forcing = [i for i, e in enumerate(batch) if e[0] != "ordinary"]
        for refused in (False, True):
            msgs, pks = [e[1] for e in batch], [e[3] for e in batch]
            sigs = [_out_of_range(scheme, e[2]) if refused and e[0] != "ordinary" else e[2] for e in batch]
            want = _batch_model(scheme, msgs, sigs, pks, SEED)
            assert all(want[1][i] == (BAD_SCALAR if refused else 0) for i in forcing) and sum(want[1]) == (BAD_SCALAR * len(forcing) if refused else 0)
            assert want[2] == (1 if refused else 0), batch[forcing[0]][0]
            assert TB._both(dev, scheme, msgs, sigs, pks, SEED) == want, (batch[forcing[0]][0], refused)
        want = np.array([_single(scheme, e[1], e[2], e[3]) for e in batch], dtype=np.uint8)
        assert all(want[i] == 0 for i in forcing) and want.sum() == len(batch) - len(forcing)
        msgs, sg, pk_rows = [e[1] for e in batch], _rows([e[2] for e in batch], 64), _rows([e[3] for e in batch], 32)
        assert np.array_equal(TM._host(gpu_ctx, b, msgs, sg, pk_rows), want), batch[forcing[0]][0]
        assert np.array_equal(TM._run_dev(gpu_ctx, b, msgs, sg, pk_rows), want), batch[forcing[0]][0]
    gpu_ctx.check()


# ---- 4g. the keyed points, on valid signatures --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ordinary_ecdsa():
    """four ordinary (message, signature, 33-byte key, 65-byte key) of secp256k1, signed by the model"""
    rng = random.Random(0x4B37)
    out = []
    for n in MSG_LENGTHS:
        d, msg = rng.randrange(1, SECP.N), bytes(rng.randrange(256) for _ in range(n))
        Q = SECP.mul(d, SECP.G)
        out.append((msg, R.ecdsa_sign(SECP, d, msg, rng.randrange(1, SECP.N)), R.sec1_encode(Q), R.sec1_encode(Q, compressed=False)))
    return out


@functools.lru_cache(maxsize=None)
def _ecdsa_verdict(msg, sig, pk):
    return R.ecdsa_verify(SECP, msg, sig, pk)


@pytest.mark.parametrize("pk_len", [33, 65])
def test_keyed_ecdsa(gpu_ctx, pk_len):
    """A valid ECDSA signature whose public key AND nonce point are forcing points: ecdsa_verify_msg decodes the key
    (k_canon_ecdsa_prepare_msg) and must answer 1 -- a wrongly decoded y answers 0 -- and ecdsa_recover lifts R from r
    (k_canon_recover_prepare) and must return the key.  One bit of s flipped: 0, and another key."""
    import test_gpu_canon_msg as TM
    from test_gpu_canon_recover import _both
    pairs = _keyed_pairs()
    assert len(pairs) >= 2
    items = []
    for (d, Q, _), (kn, Rp, _), msg in pairs:
        sig = R.ecdsa_sign(SECP, d, msg, kn)
        pk = R.sec1_encode(Q, compressed=pk_len == 33)
        assert sig[:32] == _b32(Rp[0] % SECP.N) and R.ecdsa_verify(SECP, msg, sig, pk) == 1
        recid = (Rp[1] & 1) | (2 if Rp[0] >= SECP.N else 0)
        items += [("keyed %d bytes" % len(msg), msg, sig, pk, recid), ("keyed %d bytes, s ^ 1" % len(msg), msg, sig[:63] + bytes([sig[63] ^ 1]), pk, recid)]
    base = _cycle([("ordinary", o[0], o[1], o[2 if pk_len == 33 else 3], 0) for o in _ordinary_ecdsa()])
    b = dict(curve="secp256k1", scheme="ecdsa", pk_len=pk_len)
    for batch in _placements(items, base):
        want = np.array([_ecdsa_verdict(e[1], e[2], e[3]) for e in batch], dtype=np.uint8)
        assert all(want[i] == (0 if e[0].endswith("s ^ 1") else 1) for i, e in enumerate(batch))
        msgs, sg, pks = [e[1] for e in batch], _rows([e[2] for e in batch], 64), _rows([e[3] for e in batch], pk_len)
        assert np.array_equal(TM._host(gpu_ctx, b, msgs, sg, pks), want)
        assert np.array_equal(TM._run_dev(gpu_ctx, b, msgs, sg, pks), want)
        keyed = [e for e in batch if e[0] != "ordinary"]   # recovery: the keyed elements alone keep their places' lanes
        rec = [_recover_want("secp256k1", hashlib.sha256(e[1]).digest(), e[2], e[4], pk_len) for e in keyed]
        assert all((out == e[3]) == (not e[0].endswith("s ^ 1")) and st == K.OK for e, (out, st) in zip(keyed, rec))
        dg = _rows([hashlib.sha256(e[1]).digest() for e in keyed], 32)
        for out, st in _both(gpu_ctx, "secp256k1", dg, _rows([e[2] for e in keyed], 64), np.array([e[4] for e in keyed], dtype=np.uint8), pk_len):
            bad = _differing(keyed, [(bytes(o), int(s)) for o, s in zip(out, st)], rec)
            assert not bad, "\n".join(bad)
    gpu_ctx.check()


def test_keyed_bip340(gpu_ctx):
    """A valid BIP-340 signature whose x-only key and R are forcing points (the logarithms after BIP-340's even-y negation,
    the fixture's bip340_d): bip340_verify_msg answers 1, the batch verifier with a fixed seed verdict 1 with no status set --
    k_canon_batch_prepare lifts both, a wrongly decoded y of either breaks the equation -- and with one bit of the forcing
    element's s flipped verdict 0."""
    import test_gpu_canon_batch as TB
    import test_gpu_canon_msg as TM
    from forge_ec_amd.canon import CanonSecp256k1
    dev = CanonSecp256k1(gpu_ctx)
    pairs = _keyed_pairs()
    assert len(_keyed()) >= 4 or "SHORTFALL" in KEYED["note"]
    items = []
    for (_, Q, key), (_, Rp, nonce), msg in pairs:
        d, kn = _int(key["bip340_d"]), _int(nonce["bip340_d"])
        r32, pk32 = _b32(Rp[0]), _b32(Q[0])
        sig = r32 + _b32((kn + R.bip340_challenge(r32, pk32, msg) * d) % SECP.N)
        assert R.bip340_verify(msg, sig, pk32) == 1
        items.append(("keyed %d bytes" % len(msg), msg, sig, pk32))
    base = _cycle([("ordinary",) + q for q in _valid("bip340")])
    b = dict(curve="secp256k1", scheme="bip340", pk_len=32)
    for batch in _placements(items, base):
        msgs, sigs, pks = [e[1] for e in batch], [e[2] for e in batch], [e[3] for e in batch]
        each = np.ones(len(batch), dtype=np.uint8)   # (every distinct element is valid by the model: asserted above and in _valid)
        assert np.array_equal(TM._host(gpu_ctx, b, msgs, _rows(sigs, 64), _rows(pks, 32)), each)
        assert np.array_equal(TM._run_dev(gpu_ctx, b, msgs, _rows(sigs, 64), _rows(pks, 32)), each)
        want = _batch_model("bip340", msgs, sigs, pks, SEED)
        assert want == (True, [0] * len(batch), 1)
        assert TB._both(dev, "bip340", msgs, sigs, pks, SEED) == want
        flipped = [s[:63] + bytes([s[63] ^ 1]) if e[0] != "ordinary" else s for e, s in zip(batch, sigs)]
        want = _batch_model("bip340", msgs, flipped, pks, SEED)
        assert want[2] == 0 and not any(want[1])
        assert TB._both(dev, "bip340", msgs, flipped, pks, SEED) == want
    gpu_ctx.check()
