"""
The exception lanes of the secp256k1 square inside the ladder kernel (k_secp_mul), not only in k_field_op.

FEC_SECP_SQR_ACC_ASM (tools/gen_field_asm.py, secp_sqr) no longer collects the carry of every +1 chain: it flags a lane
from five words of the square (the high words of the limbs that receive a +1, as the limb squares left them, and of
limb 1 before the folds), folded into the fast step's running maximum of top words.  Every operand of
tests/golden/secp256k1_sqr_ripple_operands.json makes a cross-term or fold ripple travel, so each must be flagged and
its wavefront must recompute the point operation with the exact code.

The ladder squares its input's coordinates in its first two steps when the first ladder bit (bit 7 of the scalar's
byte 0) is set on every lane of the wavefront: step 0 doubles P on the fast path (squares of X and Y; with a clear bit
on any lane the wavefront doubles the identity and takes the exact code up front), and step 1 adds P and 2P (square of
P's Z).  The batches below put the fixture's values into X, Y or Z of a few lanes of a wavefront whose other lanes hold
random points -- a ripple on some lanes and not on others -- and into half the lanes of a wavefront.  Whole batches are
compared with the C oracle.
"""
import json
import os

import numpy as np
import pytest

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPERANDS = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "secp256k1_sqr_ripple_operands.json")))["operands"],
                    dtype=np.uint64)
WAVE = 64
THREADS = 16


def _sparse(coord):
    """fixture value j alone among 63 random lanes of wavefront j, and with two others in wavefront m + j // 3"""
    m = len(OPERANDS)
    n = WAVE * (m + (m + 2) // 3 + 2)  # two wavefronts of random points alone at the end
    p = V.points(n, 0, 1300 + coord)
    used = []
    for j in range(m):
        for pos in (j * WAVE + (7 * j) % WAVE, (m + j // 3) * WAVE + (21 * (j % 3) + j // 3) % WAVE):
            p[pos, 4 * coord:4 * coord + 4] = OPERANDS[j]
            used.append(j)
    return p, used


def _dense():
    """fixture values on every even lane of a wavefront, as X, then as Y, then as Z; random points on the odd lanes"""
    m = len(OPERANDS)
    per = WAVE // 2
    nw = (m + per - 1) // per
    p = V.points(3 * nw * WAVE, 0, 1310)
    used = []
    for coord in range(3):
        for j in range(m):
            pos = (coord * nw + j // per) * WAVE + 2 * (j % per)
            p[pos, 4 * coord:4 * coord + 4] = OPERANDS[j]
            used.append(j)
    return p, used


BATCHES = [("X of a few lanes", lambda: _sparse(0)), ("Y of a few lanes", lambda: _sparse(1)),
           ("Z of a few lanes", lambda: _sparse(2)), ("half of the lanes", _dense)]


def _scalars(n, stream):
    k = V.scalars(n, 0, stream)
    k[:, 0] |= np.uint64(0x80)  # the first ladder bit: step 0 keeps double(P), on the fast path
    return k


def test_every_fixture_value_is_in_every_batch():
    for what, make in BATCHES:
        p, used = make()
        assert set(used) == set(range(len(OPERANDS))), what
        assert p.shape[0] % WAVE == 0
        crafted = np.zeros(p.shape[0], dtype=bool)
        for c in range(3):
            crafted |= (p[:, None, 4 * c:4 * c + 4] == OPERANDS[None, :, :]).all(axis=-1).any(axis=-1)
        per_wave = crafted.reshape(-1, WAVE).sum(axis=1)
        assert per_wave.max() <= WAVE // 2 and (per_wave > 0).sum() >= len(OPERANDS) // (WAVE // 2), what


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(BATCHES)), ids=[b[0].replace(" ", "_") for b in BATCHES])
def test_ladder_squares_fixture_values_on_some_lanes(gpu_ctx, oracle, which):
    what, make = BATCHES[which]
    p, _ = make()
    k = _scalars(p.shape[0], 1320 + which)
    got = gpu_ctx.batch_mul(0, k, p)
    want = oracle.batch_mul(0, k, p, nthreads=THREADS)
    bad = np.nonzero(~(got == want).all(axis=-1))[0]
    assert len(bad) == 0, "secp256k1 batch_mul, ripple operands as %s: %d rows differ, first at %s" % (what, len(bad), list(bad[:8]))
