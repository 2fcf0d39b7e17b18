"""
The carries that the secp256k1 ladder's fast step does not compute, inside the ladder kernel (k_secp_mul).

FEC_SECP_MUL_ACC_ASM drops the carry count behind the first product of columns 2..13 and FEC_SECP_SQR_ACC_ASM the
ripple of a cross term's +1 inside the limb it enters; the fast step flags a lane whose a.w[0], b.w[7] (Mul) or
W[6], W[10], W[14] (square) is >= RARE_WORD, and a flagged wavefront recomputes the point operation with the exact
code (secp_step.hpp, tools/gen_field_asm.py).  tests/golden/secp256k1_rare_carry_operands.json holds operands on which
each of these carries fires, and near misses on either side of the threshold (tests/test_secp_rare_carry_model.py
checks every row against the model).

As in tests/test_gpu_secp_sqr_exception_lanes.py the first ladder bit is set on every lane, so step 0 doubles P on the
fast path -- squares of X and Y, mul(Y, Z) with a = Y, b = Z -- and step 1 squares Z and multiplies X and Y by powers
of Z.  The Mul rows go into (Y, Z), the square rows into X, Y and Z, in three placements: alone among 63 random lanes,
on half the lanes of a wavefront, and in the first and last wavefront of the batch.  Whole batches are compared with
the C oracle, for batch_mul and for batch_mul_fixed with a crafted base.
"""
import json
import os

import numpy as np
import pytest

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "secp256k1_rare_carry_operands.json")))
WAVE = 64
THREADS = 16


def _items():
    """(first limb column, limbs) to write into a point row: Mul rows as (Y, Z), square rows as X, as Y and as Z"""
    items = [(4, row["a"] + row["b"]) for row in FIXTURE["mul"]]
    for coord in range(3):
        items += [(4 * coord, row["a"]) for row in FIXTURE["sqr"]]
    return items


ITEMS = _items()


def _put(p, pos, item):
    col, limbs = item
    p[pos, col:col + len(limbs)] = np.array(limbs, dtype=np.uint64)


def _sparse():
    """item j alone among the 63 random lanes of wavefront j; two wavefronts of random points at the end"""
    p = V.points(WAVE * (len(ITEMS) + 2), 0, 1400)
    where = [j * WAVE + (7 * j) % WAVE for j in range(len(ITEMS))]
    for pos, item in zip(where, ITEMS):
        _put(p, pos, item)
    return p, where


def _dense():
    """items on every even lane of a wavefront, random points on the odd lanes and in every other wavefront"""
    nw = (len(ITEMS) + WAVE // 2 - 1) // (WAVE // 2)
    p = V.points(2 * nw * WAVE, 0, 1401)
    where = [2 * (j // (WAVE // 2)) * WAVE + 2 * (j % (WAVE // 2)) for j in range(len(ITEMS))]
    for pos, item in zip(where, ITEMS):
        _put(p, pos, item)
    return p, where


def _edges():
    """items in the first and in the last wavefront of the batch (their first, middle and last lanes), 22 wavefronts of
    random points between; every item is in one of the two"""
    nw = 24
    p = V.points(nw * WAVE, 0, 1402)
    lanes = [0, 63, 1, 62, 31, 32] + list(range(2, 31)) + list(range(33, 62))
    half = (len(ITEMS) + 1) // 2
    assert half <= WAVE // 2 + 6
    where = [lanes[j] for j in range(half)] + [(nw - 1) * WAVE + lanes[j] for j in range(len(ITEMS) - half)]
    for pos, item in zip(where, ITEMS):
        _put(p, pos, item)
    return p, where


BATCHES = [("alone among 63 random lanes", _sparse), ("half of the lanes", _dense), ("first and last wavefront", _edges)]


def _scalars(n, stream):
    k = V.scalars(n, 0, stream)
    k[:, 0] |= np.uint64(0x80)  # the first ladder bit: step 0 keeps double(P), on the fast path
    return k


def _bases():
    """crafted bases for batch_mul_fixed: every Mul row as (Y, Z) under a square row as X, then square rows as Y and Z"""
    mul, sqr = FIXTURE["mul"], FIXTURE["sqr"]
    fires = [r for r in mul if r["kind"] == "fires"]
    pick = [fires[0], fires[-1]] + [r for r in mul if r["kind"] != "fires"][:2]
    bases = [sqr[i % len(sqr)]["a"] + r["a"] + r["b"] for i, r in enumerate(pick)]
    bases += [sqr[(i + 1) % len(sqr)]["a"] + sqr[i]["a"] + sqr[(i + 2) % len(sqr)]["a"] for i in (0, 3, 8)]
    return np.array(bases, dtype=np.uint64)


def test_every_fixture_row_is_in_every_batch():
    assert len(FIXTURE["mul"]) >= 6 and len(FIXTURE["sqr"]) >= 8
    for what, make in BATCHES:
        p, where = make()
        assert p.shape[0] % WAVE == 0 and p.shape[0] // WAVE >= 4 and len(set(where)) == len(ITEMS), what
        for pos, (col, limbs) in zip(where, ITEMS):
            assert list(p[pos, col:col + len(limbs)]) == limbs, what
        per_wave = np.bincount(np.array(where) // WAVE, minlength=p.shape[0] // WAVE)
        assert per_wave.max() <= WAVE // 2 + 6, what
    assert sorted(set(np.array(_edges()[1]) // WAVE)) == [0, 23]
    assert _bases().shape[1] == 12


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(BATCHES)), ids=[b[0].replace(" ", "_") for b in BATCHES])
def test_ladder_meets_fixture_rows_on_some_lanes(gpu_ctx, oracle, which):
    what, make = BATCHES[which]
    p, _ = make()
    k = _scalars(p.shape[0], 1410 + which)
    got = gpu_ctx.batch_mul(0, k, p)
    want = oracle.batch_mul(0, k, p, nthreads=THREADS)
    bad = np.nonzero(~(got == want).all(axis=-1))[0]
    assert len(bad) == 0, "secp256k1 batch_mul, rare-carry rows %s: %d rows differ, first at %s" % (what, len(bad), list(bad[:8]))


@pytest.mark.gpu
def test_fixed_base_ladder_on_crafted_bases(gpu_ctx, oracle):
    n = 5 * WAVE  # two blocks, the second one partial
    for i, base in enumerate(_bases()):
        k = _scalars(n, 1420 + i)
        got = gpu_ctx.batch_mul_fixed(0, k, base)
        want = oracle.batch_mul_fixed(0, k, base, nthreads=THREADS)
        bad = np.nonzero(~(got == want).all(axis=-1))[0]
        assert len(bad) == 0, "secp256k1 batch_mul_fixed, crafted base %d: %d rows differ, first at %s" % (i, len(bad), list(bad[:8]))
