"""
The secp256k1 ladder's fast step (forge_ec_amd/csrc/secp_step.hpp) and its way out: a point operation that meets a rare
condition on any lane is recomputed by the whole wavefront with the exact code.  Every secp256k1 family of
tests/golden/kernel_forcing_vectors.json goes through variable-base, fixed-base (prefix tables on and off) and double
multiplication at 2^20, each crafted element alone among 63 random lanes of its wavefront, in the first and the last
wavefronts of the batch.  The oracle checks every element of every wavefront that holds a crafted one (those are the
wavefronts that take the exact code), and a sample of the others.

The families exercise these exits of the fast step: identity operands (secp_x_zero), u1 == u2, Mul's borrow, square's
exception mask, mul-by-3's exc, Add's carry and the top word of a reduced result.  No vectors are known for Sub's
borrow, for double's carry or top word, or for mul-by-k's borrow, so the accumulation of those conditions
(FEC_SECP_SUB_ACC_ASM, FEC_SECP_DBL_ACC_ASM, the second s_or_b64 of FEC_SECP_MUL3/MUL8_ACC_ASM) is not exercised on
the GPU here: it rests on review of the generated statements against the exact ones.
"""
import json
import os

import numpy as np
import pytest

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCING = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_forcing_vectors.json")))
THREADS = 16
N = 1 << 20
WAVE = 64
CASES = [c for c in FORCING["cases"] if c["curve"] == 0]
BASES = [b for b in FORCING["bases"] if b["curve"] == 0]


def _place(m, n):
    """positions of m crafted elements: element j alone in wavefront j and in wavefront n/64 - 1 - j, at a lane that
    moves with j; returns (element index into the m, position) pairs and the rows the oracle checks"""
    nw = n // WAVE
    assert 2 * m <= nw
    pos, src = [], []
    for j in range(m):
        lane = (7 * j) % WAVE
        for w in (j, nw - 1 - j):
            pos.append(w * WAVE + lane)
            src.append(j)
    waves = sorted({p // WAVE for p in pos})
    rows = np.concatenate([np.arange(w * WAVE, (w + 1) * WAVE) for w in waves] + [np.arange(0, n, 4099)])
    return np.array(src), np.array(pos), np.unique(rows)


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(~(got == want).all(axis=-1))[0]
        raise AssertionError("%s: %d rows differ, first at %s" % (what, len(bad), list(bad[:8])))


def test_placement_covers_first_and_last_wavefronts():
    src, pos, rows = _place(len(CASES), N)
    assert set(src) == set(range(len(CASES)))
    assert {p // WAVE for p in pos} >= {0, N // WAVE - 1}
    assert len({p // WAVE for p in pos}) == len(pos)  # one crafted element per wavefront
    assert {c["family"] for c in CASES} == {CASES[j]["family"] for j in src}


@pytest.mark.gpu
def test_batch_mul_var_crafted_in_random_wavefronts(gpu_ctx, oracle):
    k = np.array([c["scalar"] for c in CASES], dtype=np.uint64)
    p = np.array([c["point"] for c in CASES], dtype=np.uint64)
    e = np.array([c["expect"] for c in CASES], dtype=np.uint64)
    src, pos, rows = _place(len(CASES), N)
    ks, ps = V.scalars(N, 0, 1200), V.points(N, 0, 1201)
    ks[pos], ps[pos] = k[src], p[src]
    got = gpu_ctx.batch_mul(0, ks, ps)
    _same(got[pos], e[src], "secp256k1 batch_mul 2^20 crafted elements vs fixture")
    _same(got[rows], oracle.batch_mul(0, ks[rows], ps[rows], nthreads=THREADS), "secp256k1 batch_mul 2^20 vs oracle")


@pytest.mark.gpu
def test_batch_mul_fixed_crafted_bases_in_random_wavefronts(gpu_ctx, oracle):
    """k_secp_mul<1> (prefix tables off) and k_secp_mul<3>/<2> (the table built from the base, then the ladder from it)"""
    import forge_ec_amd as F
    off = F.Context(0)
    try:
        off.set_fixed_prefix_bits(0)
        for i, b in enumerate(BASES):
            base = np.array(b["point"], dtype=np.uint64)
            kb, eb = np.array(b["scalars"], dtype=np.uint64), np.array(b["expect"], dtype=np.uint64)
            src, pos, rows = _place(kb.shape[0], N)
            ks = V.scalars(N, 0, 1210 + i)
            ks[pos] = kb[src]
            want = oracle.batch_mul_fixed(0, ks[rows], base, nthreads=THREADS)
            for ctx, how in ((gpu_ctx, "prefix tables on"), (off, "prefix tables off")):
                got = ctx.batch_mul_fixed(0, ks, base)
                what = "secp256k1 batch_mul_fixed(%s base) 2^20, %s" % (b["family"], how)
                _same(got[pos], eb[src], what + " vs fixture")
                _same(got[rows], want, what + " vs oracle")
    finally:
        off.close()


@pytest.mark.gpu
def test_batch_double_mul_crafted_in_random_wavefronts(gpu_ctx, oracle):
    k = np.array([c["scalar"] for c in CASES], dtype=np.uint64)
    p = np.array([c["point"] for c in CASES], dtype=np.uint64)
    src, pos, rows = _place(len(CASES), N)
    u1, u2, q = V.scalars(N, 0, 1220), V.scalars(N, 0, 1221), V.points(N, 0, 1222)
    u2[pos], q[pos] = k[src], p[src]
    got = gpu_ctx.batch_double_mul(0, u1, u2, q)
    _same(got[rows], oracle.batch_double_mul(0, u1[rows], u2[rows], q[rows], nthreads=THREADS),
          "secp256k1 batch_double_mul 2^20 crafted Q vs oracle")
